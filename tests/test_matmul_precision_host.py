"""CPU: the matmul precision level — C ABI, Python API, the two queries, the code objects of the two-term kernels, and the
error bound of the three-product form derived in csrc/common.h (evaluated with torch's bf16 cast, no GPU)."""
import os
import re
import subprocess
import sys

import pytest
import torch

import dsgcn_amd as D
from dsgcn_amd import native
from matmul_precision_emul import HIGH_BOUND, PAIRS, split_terms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('dsgcn_set_matmul_precision', 'dsgcn_get_matmul_precision', 'dsgcn_pwconv_terms', 'dsgcn_tconv_terms')

# the shapes of tests/test_matmul_precision_gpu.py, n = 2
PW_SHAPES = [(64, 128, 8, 25), (128, 256, 8, 25), (96, 160, 8, 25), (256, 96, 8, 25), (128, 128, 8, 25), (256, 256, 8, 25),
             (256, 128, 8, 25), (128, 128, 9, 17)]
TC_SHAPES = [(2, 128, 128, 32, 25, 9, 1), (2, 256, 256, 16, 25, 9, 1), (2, 48, 80, 12, 17, 9, 1), (1, 32, 40, 20, 18, 5, 1),
             (2, 16, 24, 8, 25, 3, 1), (2, 64, 128, 32, 25, 9, 2), (3, 32, 48, 15, 17, 5, 2)]


@pytest.fixture(autouse=True)
def _level_restored():
    before = native.lib().dsgcn_get_matmul_precision()
    yield
    assert native.lib().dsgcn_set_matmul_precision(before) == 0


def test_abi_symbols_exported_declared_and_bound():
    with open(os.path.join(ROOT, 'include', 'dsgcn.h')) as f:
        header = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    out = subprocess.run(['nm', '-D', '--defined-only', native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), f'{name} is not declared in include/dsgcn.h'
        assert re.search(r' T ' + name + r'$', out, flags=re.M), f'{name} is not exported'
        assert name in native.SIGNATURES
    assert 'PROCESS-WIDE' in open(os.path.join(ROOT, 'include', 'dsgcn.h')).read()      # stated beside the thread-safety paragraph


def test_abi_set_get_and_rejection_without_gpu():
    lib = native.lib()                       # loads without a GPU (test_argument_rejection_without_gpu relies on the same)
    assert lib.dsgcn_get_matmul_precision() == 0, 'highest is the default'
    assert lib.dsgcn_set_matmul_precision(1) == 0 and lib.dsgcn_get_matmul_precision() == 1
    for bad in (2, -1):
        assert lib.dsgcn_set_matmul_precision(bad) == -1          # DSGCN_EINVAL
        assert lib.dsgcn_get_matmul_precision() == 1, 'a rejected level must leave the level unchanged'
    assert lib.dsgcn_set_matmul_precision(0) == 0 and lib.dsgcn_get_matmul_precision() == 0


def test_python_api():
    assert D.get_matmul_precision() == 'highest'
    for bad in ('medium', 'bogus'):
        with pytest.raises(ValueError):
            D.set_matmul_precision(bad)
        with pytest.raises(ValueError):
            D.matmul_precision(bad)
    assert D.get_matmul_precision() == 'highest'
    D.set_matmul_precision('high')
    assert D.get_matmul_precision() == 'high' and native.lib().dsgcn_get_matmul_precision() == 1
    with D.matmul_precision('highest'):
        assert D.get_matmul_precision() == 'highest'
    assert D.get_matmul_precision() == 'high', 'restored on normal exit'
    D.set_matmul_precision('highest')
    with pytest.raises(RuntimeError, match='boom'):
        with D.matmul_precision('high'):
            assert D.get_matmul_precision() == 'high'
            raise RuntimeError('boom')
    assert D.get_matmul_precision() == 'highest', 'restored when the block raises'
    with D.matmul_precision('high'):
        with D.matmul_precision('high'):
            pass
        assert D.get_matmul_precision() == 'high', 'nested blocks restore what THEY found'


def _child(code, value):
    env = dict(os.environ)
    env.pop('DSGCN_MATMUL_PRECISION', None)
    if value is not None:
        env['DSGCN_MATMUL_PRECISION'] = value
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    return subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, cwd=ROOT)


def test_environment_variable_in_a_fresh_process():
    code = 'import dsgcn_amd as D; print(D.get_matmul_precision())'
    for value, want in ((None, 'highest'), ('highest', 'highest'), ('high', 'high')):
        r = _child(code, value)
        assert r.returncode == 0, r.stderr
        assert r.stdout.split()[-1] == want, (value, r.stdout)
    r = _child('import dsgcn_amd', 'medium')
    assert r.returncode != 0 and 'ValueError' in r.stderr and 'DSGCN_MATMUL_PRECISION' in r.stderr, r.stderr


def test_engines_reject_an_unknown_level():
    m = torch.nn.Linear(2, 2)
    with pytest.raises(ValueError):
        D.TrainEngine(m, matmul_precision='medium')
    with pytest.raises(ValueError):
        D.InferEngine(m, matmul_precision='bogus')


def test_train_engine_fixes_its_level_at_construction(monkeypatch):
    """None = the process level at construction; every step runs under the engine's level and puts the process level back,
    whatever it was set to in between (the GPU file checks the same on results)."""
    D.set_matmul_precision('high')
    eng = D.TrainEngine(torch.nn.Linear(2, 2), use_graph=False)
    D.set_matmul_precision('highest')
    assert eng.matmul_precision == 'high'
    seen = []
    monkeypatch.setattr(eng, '_step', lambda *a: seen.append(D.get_matmul_precision()) or {})
    eng.step(None, None)
    assert seen == ['high'] and D.get_matmul_precision() == 'highest'
    assert D.TrainEngine(torch.nn.Linear(2, 2), use_graph=False).matmul_precision == 'highest'
    assert D.TrainEngine(torch.nn.Linear(2, 2), use_graph=False, matmul_precision='high').matmul_precision == 'high'


def test_term_queries():
    lib = native.lib()
    n = 2
    for level, want in ((0, 6), (1, 3)):
        assert lib.dsgcn_set_matmul_precision(level) == 0
        for Ci, Co, T, V in PW_SHAPES:
            # forward of every shape is the GEMM form on the weight image
            assert lib.dsgcn_pwconv_terms(0, n, Ci, Co, T, V, 1) == want, (level, Ci, Co, T, V)
        # both sides wide: the data gradient (k_pwg3) and the weight gradient (k_wg2<..B3> / k_wg3) too
        for Ci, Co, T, V in [(128, 256, 8, 25), (96, 160, 8, 25), (256, 96, 8, 25), (128, 128, 8, 25), (256, 256, 8, 25),
                             (256, 128, 8, 25), (128, 128, 9, 17)]:
            assert lib.dsgcn_pwconv_terms(1, n, Ci, Co, T, V, 1) == want, (level, Ci, Co, T, V)
            assert lib.dsgcn_pwconv_terms(2, n, Ci, Co, T, V, 1) == want, (level, Ci, Co, T, V)
        # 64 -> 128: the data gradient has 64 output rows and the weight gradient a 128 x 64 tile: fp32 MFMA forms
        assert lib.dsgcn_pwconv_terms(1, n, 64, 128, 8, 25, 1) == 0 and lib.dsgcn_pwconv_terms(2, n, 64, 128, 8, 25, 1) == 0
        for nn, Ci, Co, T, V, KT, st in TC_SHAPES:
            for d in range(3):
                assert lib.dsgcn_tconv_terms(d, nn, Ci, Co, T, V, KT, st) == want, (level, d, nn, Ci, Co, T, V, KT, st)
        # narrow (CTR-GCN's conv4, 8 -> 64): no bf16 terms at all
        for d in range(3):
            assert lib.dsgcn_pwconv_terms(d, n, 8, 64, 8, 25, 1) == 0
        # the one-pass backward of 64 -> 64 (k_bwd64b) stays on six terms at both levels; its forward is an fp32 MFMA form
        assert lib.dsgcn_pwconv_terms(1, n, 64, 64, 8, 25, 1) == 6 and lib.dsgcn_pwconv_terms(2, n, 64, 64, 8, 25, 1) == 6
        assert lib.dsgcn_pwconv_terms(0, n, 64, 64, 8, 25, 1) == 0
        # not a direction / strided 1x1 conv / a temporal kernel the GEMM form does not take
        assert lib.dsgcn_pwconv_terms(3, n, 128, 128, 8, 25, 1) == 0 and lib.dsgcn_pwconv_terms(0, n, 128, 128, 8, 25, 2) == 0
        assert lib.dsgcn_tconv_terms(0, n, 128, 128, 32, 25, 4, 1) == 0 and lib.dsgcn_tconv_terms(3, n, 128, 128, 32, 25, 9, 1) == 0


# six-term instantiations of the library the two-term kernels were derived from (k_pwg3 10, k_wg2<128, 128, 32, .., true> 4,
# k_wg3 8, k_tcg 24, k_tcw 6), counted on a build of the parent commit
PARENT_SIX_TERM = 52


def test_code_objects_of_the_two_term_kernels():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import codeobj_report
    ks = codeobj_report.kernels(native.LIB_PATH)
    six = [k for k in ks if re.match(r'k_(pwg3|wg3|tcg|tcw)<', k) or re.match(r'k_wg2<128, 128, 32, \w+, \w+, true>', k)]
    assert len(six) == PARENT_SIX_TERM, sorted(six)
    want = ([f'k_pwg3h<{m}, {e}, {mt}>' for m, e in ((0, 0), (1, 0), (2, 0), (0, 1), (2, 1)) for mt in (1, 2)] +
            [f'k_wg2h<128, 128, 32, {a}, {b}>' for a in ('false', 'true') for b in ('false', 'true')] +
            [f'k_wg3h<{tm}, {tn}, {a}, {b}>' for tm, tn in ((256, 128), (128, 256)) for a in ('false', 'true')
             for b in ('false', 'true')] +
            [f'k_tcgh<{m}, {e}, {wm}, {q}>' for m in (0, 1, 2) for e in (0, 1) for wm in (2, 4) for q in ('false', 'true')] +
            [f'k_tcwh<{kt}, {st}>' for kt in (3, 5, 9) for st in (1, 2)])
    two = sorted(k for k in ks if re.match(r'k_(pwg3h|wg2h|wg3h|tcgh|tcwh)<', k))
    assert two == sorted(want), set(two) ^ set(want)
    assert len(two) == PARENT_SIX_TERM                  # one per six-term instantiation
    bad = {k: (ks[k].get('scratch_instructions'), ks[k].get('vgpr_spill_count'), ks[k].get('private_segment_fixed_size'))
           for k in two if ks[k].get('scratch_instructions', 0) or ks[k].get('vgpr_spill_count', 0)
           or ks[k].get('private_segment_fixed_size', 0)}
    assert not bad, f'two-term kernels with scratch / spilled registers: {bad}'
    # and the refactoring into shared bodies left the six-term ones without scratch as well
    bad = [k for k in six if ks[k].get('scratch_instructions', 0) or ks[k].get('vgpr_spill_count', 0)]
    assert not bad, bad


@pytest.mark.parametrize('K', [64, 256, 1024])
@pytest.mark.parametrize('scale', [1.0, 1e30, 1e-30])
def test_split_bound(K, scale):
    """|a.b - (a0.b0 + a0.b1 + a1.b0)| <= 3 * 2^-16 * sum|a||b| elementwise, and the six-term form below 2^-22 of the same sum
    (measured on this data: 5.4e-6 and 9.7e-9 of it).  Passes without the feature: it pins the derivation, not the code."""
    g = torch.Generator().manual_seed(K)
    a = (torch.randn(96, K, generator=g) * scale).float()
    b = (torch.randn(K, 80, generator=g) / scale).float()
    at, bt = split_terms(a), split_terms(b)
    if scale == 1.0:         # (at 1e-30 the third term of the smallest elements is subnormal: the bounds hold all the same)
        assert torch.equal(at[0] + at[1] + at[2], a.double()) and torch.equal(bt[0] + bt[1] + bt[2], b.double()), 'exact split'
    exact = a.double() @ b.double()
    mag = a.double().abs() @ b.double().abs()
    for products, bound in ((3, HIGH_BOUND), (6, 2.0 ** -22)):
        got = sum(at[i] @ bt[j] for i, j in PAIRS[products])
        worst = ((got - exact).abs() / mag).max().item()
        print(f'K={K} scale={scale:g} products={products}: max |err| / sum|a||b| = {worst:.3e}')
        assert worst <= bound, (products, worst)
