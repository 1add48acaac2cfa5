"""CPU: the host side of feature / score-map extraction at test time (test_cfg['feat_ext'] / ['score_ext'] / ['pool_opt']):
what the recognizer accepts and still rejects, the pool_opt parser and the output shapes against the reference's
(tests/golden/featext.npz), the new entry point's declaration, binding, argument checks and code objects, the result
files.  No GPU."""
import json
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

import dsgcn_amd as D
import feat_ext_cases as F
from dsgcn_amd import kernels as K
from dsgcn_amd import native
from test_oracle_golden import GOLD, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = load('featext.npz')


def _cfg(name='model_reduced_stgcn', **test_cfg):
    with open(os.path.join(GOLD, name + '_cfg.json')) as f:
        cfg = json.load(f)
    if 'tcn_ms_cfg' in cfg['backbone']:
        cfg['backbone']['tcn_ms_cfg'] = [tuple(c) if isinstance(c, list) else c for c in cfg['backbone']['tcn_ms_cfg']]
    cfg['test_cfg'] = test_cfg
    return cfg


# ---- the recognizer's constructor ---------------------------------------------------------------------------------------
def test_recognizer_accepts_the_extraction_keys():
    m = D.build_model(_cfg(feat_ext=True, pool_opt='nm'))
    assert m.extraction() == ('feat', 3)
    m = D.build_model(_cfg(score_ext=True))
    assert m.extraction() == ('score', 15)                      # pool_opt defaults to 'all'
    m = D.build_model(_cfg(score_ext=True, feat_ext=True, pool_opt='none'))
    assert m.extraction() == ('score', 0)                       # score_ext wins
    assert D.build_model(_cfg()).extraction() is None
    assert D.build_model(_cfg(feat_ext=False, pool_opt='xq')).extraction() is None      # unread without the keys


def test_recognizer_without_head_extracts_features_only():
    cfg = _cfg(feat_ext=True, pool_opt='tv')
    cfg['cls_head'] = None
    m = D.build_model(cfg)
    assert m.cls_head is None and m.extraction() == ('feat', 12)
    cfg['test_cfg'] = dict(score_ext=True)
    with pytest.raises(ValueError):                             # nothing to project with
        D.build_model(cfg)


@pytest.mark.parametrize('key', ['feat_ext', 'score_ext'])
def test_bad_pool_opt_is_an_assertion_error(key):
    with pytest.raises(AssertionError):
        D.build_model(_cfg(**{key: True, 'pool_opt': 'xq'}))
    with pytest.raises(AssertionError):
        D.build_model(_cfg(**{key: True, 'pool_opt': 3}))


def test_max_testing_views_still_raises():
    with pytest.raises(NotImplementedError):
        D.build_model(_cfg(max_testing_views=4))
    with pytest.raises(NotImplementedError):
        D.build_model(_cfg(feat_ext=True, pool_opt='n', max_testing_views=4))


# ---- pool_opt and shapes ------------------------------------------------------------------------------------------------
def test_parse_pool_opt():
    for mask in range(16):
        name = F.pool_name(mask)
        assert K.parse_pool_opt(name) == mask, name
        if mask:
            assert K.parse_pool_opt(name[::-1]) == mask                       # a set: the order does not matter
            assert K.parse_pool_opt(name + name[0] + name) == mask            # nor does a repeated letter
    assert K.parse_pool_opt('all') == K.parse_pool_opt('nmtv') == 15
    assert K.parse_pool_opt('none') == 0
    for bad in ('xq', 'nmtvx', 'a', 'ALL', 'n m', ''):
        if bad == '':
            assert K.parse_pool_opt(bad) == 0                                 # the reference's loop body never runs
            continue
        with pytest.raises(AssertionError):
            K.parse_pool_opt(bad)
    with pytest.raises(AssertionError):
        K.parse_pool_opt(None)


def test_shapes_over_all_masks_against_the_reference():
    c = F.CASES['all']
    sizes = (c['videos'], c['clips'], c['M'], c['C'], c['T'], c['V'])
    for mask in range(16):
        name = F.pool_name(mask)
        for mode, classes in (('feat', None), ('score', c['K'])):
            want = Z[F.key('all', mode, name) + '_r16'].shape
            assert K.feat_ext_shape(*sizes, name, classes) == want, (name, mode)
            assert K.feat_ext_shape(*sizes, mask, classes) == want
            assert K.feat_ext_shape(*sizes, name + name if mask else name, classes) == want
    assert K.feat_ext_shape(*sizes, 'all') == K.feat_ext_shape(*sizes, 'nmtv') == (2, 1, 1, 8, 1, 1)
    with pytest.raises(ValueError):
        K.feat_ext_shape(*sizes, 16)


def test_fixture_holds_every_run_of_the_case_table():
    assert [str(c) for c in Z['cases']] == list(F.CASES) and [str(m) for m in Z['models']] == list(F.MODELS)
    for name, c in F.CASES.items():
        assert F.case_x(Z, name).shape == (c['videos'], c['clips'], c['M'], c['C'], c['T'], c['V'])
        for mode, pool in F.runs(name):
            k = F.key(name, mode, pool)
            r16, r32 = F.ref16(Z, k), Z[k + '_r32']
            assert r16.dtype == np.float16 and r32.dtype == np.float32 and r16.shape == r32.shape == F.ref64(Z, k).shape
            with np.errstate(over='ignore'):
                assert np.array_equal(r16.view(np.uint16), r32.astype(np.float16).view(np.uint16))
    # the exactness case: every mean exact for the reference too, a float16 subnormal and two round-to-even ties among them
    for pool in F.ALL_POOLS:
        assert not Z[F.key('exact', 'feat', pool) + '_d64'].any()
    pooled = Z[F.key('exact', 'feat', 'nmtv') + '_r32'].reshape(-1)
    assert pooled[0] == 3 * 2.0 ** -17 and pooled[1] == 1 + 2.0 ** -11 and pooled[2] == 1 + 3 * 2.0 ** -11
    for m in F.MODELS:
        for mode, pool in F.MODEL_RUNS:
            assert F.key(m, mode, pool) + '_r32' in Z
    assert os.path.getsize(os.path.join(GOLD, 'featext.npz')) < 1 << 20


def test_fixture_regenerates_byte_identically_live(tmp_path):
    sys.path.insert(0, GOLD)
    import ref_shim
    if not ref_shim.available():
        pytest.skip('the reference checkout is not on this machine')
    subprocess.run([sys.executable, os.path.join(GOLD, 'gen_golden_featext.py'), '--out', str(tmp_path)], check=True,
                   capture_output=True)
    with open(os.path.join(GOLD, 'featext.npz'), 'rb') as f, open(tmp_path / 'featext.npz', 'rb') as g:
        assert f.read() == g.read()


# ---- the entry point ----------------------------------------------------------------------------------------------------
def test_entry_point_declared_exported_and_bound():
    from test_native_abi import declared_symbols
    assert 'dsgcn_feat_ext_fwd' in declared_symbols() and 'dsgcn_feat_ext_fwd' in native.SIGNATURES
    path = native.build()
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
    assert 'dsgcn_feat_ext_fwd' in set(re.findall(r' T (dsgcn_\w+)', out))
    assert len(native.SIGNATURES['dsgcn_feat_ext_fwd']) == 14
    for name in ('feat_ext', 'feat_ext_shape', 'parse_pool_opt'):
        assert hasattr(K, name), name


def feat_ext_argument_checks():
    """Every DSGCN_EINVAL condition include/dsgcn.h lists, and its DSGCN_EUNSUPPORTED limit; all return before any launch
    (the pointers are never dereferenced).  Shared with tests/test_feat_ext_gpu.py."""
    f = native.lib().dsgcn_feat_ext_fwd
    p = 4096
    ok = dict(x=p, w=p, b=None, videos=2, clips=10, M=2, C=256, T=16, V=25, K=60, mask=3, out32=None, out16=p)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a['x'], a['w'], a['b'], a['videos'], a['clips'], a['M'], a['C'], a['T'], a['V'], a['K'], a['mask'],
                 a['out32'], a['out16'], None)

    assert call(x=None) == -1
    for size in ('videos', 'clips', 'M', 'C', 'T', 'V', 'K'):
        assert call(**{size: 0}) == -1 and call(**{size: -3}) == -1, size
    assert call(out32=None, out16=None) == -1
    assert call(mask=16) == -1 and call(mask=-1) == -1 and call(mask=1 << 8) == -1
    assert call(C=513) == -2 and call(C=4096) == -2             # score mode: the [C][32] tile above 64 KB of LDS
    assert call(w=None, mask=16) == -1 and call(w=None, x=None) == -1
    assert call(clips=1 << 16, M=1 << 16, T=1, V=1, mask=0) == -2              # 2^32 positions per video


def test_argument_checks_without_gpu():
    feat_ext_argument_checks()


def test_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import codeobj_report
    native.build()
    ks = {k: v for k, v in codeobj_report.kernels(native.LIB_PATH).items() if k.startswith('k_feat_ext')}
    assert sorted(ks) == ['k_feat_ext<false>', 'k_feat_ext<true>']
    for name, k in ks.items():
        assert k.get('scratch_instructions', 0) == 0 and k.get('vgpr_spill_count', 0) == 0, (name, k)
        assert k.get('sgpr_spill_count', 0) == 0 and k.get('private_segment_fixed_size', 0) == 0, (name, k)


# ---- result files -------------------------------------------------------------------------------------------------------
def _maps(n=5, shape=(1, 3, 2, 7, 4, 5)):
    rng = np.random.default_rng(3)
    return [rng.standard_normal(shape).astype(np.float16) for _ in range(n)]


def test_pkl_keeps_float16(tmp_path):
    maps = _maps()
    path = D.dump_results(maps, str(tmp_path / 'sub' / 'maps.pkl'))
    with open(path, 'rb') as f:
        raw = pickle.load(f)
    back = D.load_results(path)
    for a, b, c in zip(maps, raw, back):
        assert b.dtype == c.dtype == np.float16 and b.shape == c.shape == a.shape
        assert np.array_equal(a.view(np.uint16), b.view(np.uint16)) and np.array_equal(a.view(np.uint16), c.view(np.uint16))
    # class scores are written as before
    scores = [np.random.default_rng(s).standard_normal(7) for s in range(3)]
    back = D.load_results(D.dump_results(scores, str(tmp_path / 'scores.pkl')))
    assert all(b.dtype == np.float32 and np.array_equal(b, a.astype(np.float32)) for a, b in zip(scores, back))
    back = D.load_results(D.dump_results(scores, str(tmp_path / 'scores.json')))
    assert all(b.dtype == np.float32 and np.array_equal(b, a.astype(np.float32)) for a, b in zip(scores, back))


def test_json_is_refused_for_extracted_arrays(tmp_path):
    with pytest.raises(ValueError, match='pkl'):
        D.dump_results(_maps(), str(tmp_path / 'maps.json'))
    assert not (tmp_path / 'maps.json').exists()
    # test_model refuses before it touches the dataset, the checkpoint or the device
    m = D.build_model(_cfg(score_ext=True, pool_opt='nm'))
    with pytest.raises(ValueError, match='pkl'):
        D.test_model(m, [dict(keypoint=None, label=0)] * 2, D.Config(dict()), out=str(tmp_path / 'maps.json'),
                     device='no such device')
