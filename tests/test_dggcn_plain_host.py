"""CPU: ``dggcn`` at numbers of subsets other than three — constructor parity with the reference (tests/golden/
unit_dggcn_k.npz, model_reduced_dggcn_k8.npz), the fp64 restatement (tests/dggcn_plain_fp64.py) that the full-size GPU
tests take as truth pinned to the reference's fp64 outputs, the supported range, the ``dsgcn_dynplain_*`` entry points
without a GPU, the code objects of the new kernels, and the unit's host wiring on the CPU seam."""
import copy
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import dsgcn_amd as D
import dggcn_plain_fp64 as F
from bench import other_cfg
from oracle import dsgcn_oracle as O
from test_oracle_golden import GOLD, load

Z = load('unit_dggcn_k.npz')
CASES = [str(c) for c in Z['cases']]
ZERO_GRAD_BIASES = ('pre.0.bias', 'post.bias', 'down.0.bias')     # under a train-mode BatchNorm: exactly zero


def graph_A(layout, K):
    np.random.seed(21)          # the fixture's graphs (mode='random' draws its off-diagonal weights)
    g = D.Graph(layout=layout, mode='random', num_filter=K, init_off=.04, init_std=.02)
    return torch.tensor(np.asarray(g.A), dtype=torch.float32)


def case_cfg(tag, z=Z):
    ci, co, K, V, sw, seed = [int(v) for v in z[tag + '_cfg']]
    ratio = float(z[tag + '_ratio'])
    return dict(ci=ci, co=co, K=K, V=V, subset_wise=bool(sw), seed=seed, ratio=None if np.isnan(ratio) else ratio,
                layout=str(z[tag + '_layout']))


def make_unit(tag, z=Z, live=True):
    """The unit of fixture case `tag`, built under the fixture's seed (live: with the fixture's alpha / beta)."""
    c = case_cfg(tag, z)
    A = graph_A(c['layout'], c['K'])
    torch.manual_seed(c['seed'])
    m = D.dggcn(c['ci'], c['co'], A, ratio=c['ratio'], subset_wise=c['subset_wise'])
    if live:
        with torch.no_grad():
            m.alpha.copy_(torch.from_numpy(z[tag + '_alpha']))
            m.beta.copy_(torch.from_numpy(z[tag + '_beta']))
    return m, c


def unit_inputs(tag, z=Z):
    """x, R of fixture case `tag`, regenerated from their seed and checked against the fixture's digest."""
    c = case_cfg(tag, z)
    x, r = F.unit_inputs(c['ci'], c['co'], c['V'], int(z[tag + '_input_seed']))
    assert hashlib.sha256(x.numpy().tobytes() + r.numpy().tobytes()).hexdigest() == str(z[tag + '_input_digest'])
    return x, r


def sd_digest(module):
    h = hashlib.sha256()
    for k, v in module.state_dict().items():
        h.update(k.encode())
        h.update(v.detach().cpu().numpy().tobytes())
    return h.hexdigest()


def k8_cfg(**bk):
    """The K = 8 DG-STGCN: bench.other_cfg('dggcn') with num_filter = 8 (gcn_ratio 0.125: K * mid == out_channels)."""
    cfg = other_cfg('dggcn', **bk)
    cfg['backbone']['graph_cfg'] = dict(cfg['backbone']['graph_cfg'], num_filter=8)
    return cfg


def reduced_k8():
    z = load('model_reduced_dggcn_k8.npz')
    with open(os.path.join(GOLD, 'model_reduced_dggcn_k8_cfg.json')) as f:
        cfg = json.load(f)
    cfg['backbone']['tcn_ms_cfg'] = [tuple(c) if isinstance(c, list) else c for c in cfg['backbone']['tcn_ms_cfg']]
    return z, cfg


# ---- 1. construction --------------------------------------------------------------------------------------------------

def test_k8_unit_constructs():
    m = D.dggcn(64, 64, graph_A('nturgb+d', 8), ratio=0.125)
    assert m.num_subsets == 8 and m.mid_channels == 8 and tuple(m.A.shape) == (8, 25, 25)
    assert not any(k.startswith('_') for k in dict(m.named_buffers()))       # the K = 3 helper constants are not made


@pytest.mark.parametrize('tag', CASES)
def test_state_dict_matches_reference_constructor(tag):
    """Same keys, shapes and initial values (same RNG use: same creation order) as the reference's dggcn."""
    m, c = make_unit(tag, live=False)
    assert m.num_subsets == c['K'] and m.mid_channels == int((c['ratio'] or 1 / c['K']) * c['co'])
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == json.loads(str(Z[tag + '_sd_manifest']))
    assert sd_digest(m) == str(Z[tag + '_init_digest'])


def test_k8_model_matches_reference_constructor():
    """build_model of the reduced K = 8 config under the fixture's seeds: the reference's keys, shapes and initial values;
    the full-width K = 8 DG-STGCN builds with eight subsets in every block and loads its own state_dict strictly."""
    z, cfg = reduced_k8()
    np.random.seed(int(z['init_seed']))
    torch.manual_seed(int(z['init_seed']))
    m = D.build_model(copy.deepcopy(cfg))
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == json.loads(str(z['init_manifest']))
    assert sd_digest(m) == str(z['init_digest'])
    m.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith('sd_')}, strict=True)
    full = D.build_model(k8_cfg())
    assert all(type(b.gcn).__name__ == 'dggcn' and b.gcn.num_subsets == 8 for b in full.backbone.gcn)
    assert [b.gcn.mid_channels for b in full.backbone.gcn] == [8, 8, 8, 8, 16, 16, 16, 32, 32, 32]
    D.build_model(k8_cfg()).load_state_dict(full.state_dict(), strict=True)


# ---- 2. the fp64 restatement against the reference ---------------------------------------------------------------------

@pytest.mark.parametrize('tag', CASES)
def test_fp64_restatement_matches_reference(tag):
    """tests/dggcn_plain_fp64.py against the reference's fp64 output, input gradient and every parameter gradient; the
    oracle's dggcn_forward agrees with it."""
    m, c = make_unit(tag)
    m = m.double()
    with torch.no_grad():                                       # (the fixture's values are fp32-exact; copy them in fp64)
        m.alpha.copy_(torch.from_numpy(Z[tag + '_alpha']))
        m.beta.copy_(torch.from_numpy(Z[tag + '_beta']))
    p = {k: v.detach().clone().requires_grad_() for k, v in m.named_parameters()}
    x, r = unit_inputs(tag)
    x = x.double().requires_grad_()
    y = F.unit_forward(p, x, c['subset_wise'])
    (y * r.double()).sum().backward()
    assert F.fixture_rel(Z, tag + '_y', y.detach().numpy()) < 1e-12
    assert F.fixture_rel(Z, tag + '_dx', x.grad.numpy()) < 1e-12
    for k, t in p.items():
        key = tag + '_grad_' + k
        got = t.grad if t.grad is not None else torch.zeros_like(t)
        if F.fixture_is_zero(Z, key):
            assert not torch.any(got), k                         # alpha[1:], beta[1:] without subset_wise
        elif k in ZERO_GRAD_BIASES:
            assert float(got.abs().max()) < 1e-10 and np.abs(Z[key]).max() < 1e-10, k
        else:
            assert F.fixture_rel(Z, key, got.numpy()) < 1e-12, (k, F.fixture_rel(Z, key, got.numpy()))
    with torch.no_grad():
        sd = {k: v.detach() for k, v in m.state_dict().items()}
        yo = O.dggcn_forward(x.detach(), sd, training=True, subset_wise=c['subset_wise'])
    assert float((yo - y.detach()).norm() / y.detach().norm()) < 1e-12


# ---- 3. the supported range ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('A,co,ratio,what', [(torch.rand(17, 25, 25), 64, None, '= 17'),
                                             (torch.rand(8, 25, 25), 520, 0.125, '= 65'),
                                             (torch.rand(8, 40, 40), 64, 0.125, '40 joints')])
def test_out_of_range_raises_naming_the_value(A, co, ratio, what):
    with pytest.raises(NotImplementedError, match=what):
        D.dggcn(64, co, A, ratio=ratio)


def test_typed_units_keep_three_subsets():
    g = D.Graph(layout='nturgb+d', mode='spatial')
    A = torch.rand(4, 25, 25)
    et, nt = torch.tensor(g.edge_type), torch.tensor(g.node_type)
    with pytest.raises(NotImplementedError):
        D.dghgcn(64, 64, A, et, nt)
    with pytest.raises(NotImplementedError):
        D.dgphgcn1(64, 64, A, et, nt)


# ---- 4. the C entry points without a GPU ---------------------------------------------------------------------------------

def test_dynplain_argument_rejection_without_gpu():
    """NULL pointers and out-of-range sizes are DSGCN_EINVAL (-1) before any launch; the pointers below are never read."""
    from dsgcn_amd import native
    lib = native.lib()
    p = 0x1000                                                   # non-null
    assert lib.dsgcn_dynplain_partial_stride(8, 25) == 8 * 625 + 16
    assert lib.dsgcn_dynplain_fwd(None, None, None, None, None, 1, 8, 8, 25, 32, None) == -1
    assert lib.dsgcn_dynplain_bwd(None, None, None, None, None, None, 5016, 1, 8, 8, 25, 32, None) == -1
    for i in range(5):
        ptrs = [p] * 5
        ptrs[i] = None
        assert lib.dsgcn_dynplain_fwd(*ptrs, 1, 8, 8, 25, 32, None) == -1
    for i in range(6):
        ptrs = [p] * 6
        ptrs[i] = None
        assert lib.dsgcn_dynplain_bwd(*ptrs, 5016, 1, 8, 8, 25, 32, None) == -1
    for n, K, mid, V, ld in ((0, 8, 8, 25, 32), (1, 0, 8, 25, 32), (1, 17, 8, 25, 32), (1, 8, 0, 25, 32),
                             (1, 8, 65, 25, 32), (1, 8, 8, 0, 32), (1, 8, 8, 33, 40), (1, 8, 8, 25, 24)):
        assert lib.dsgcn_dynplain_fwd(p, p, p, p, p, n, K, mid, V, ld, None) == -1, (n, K, mid, V, ld)
        assert lib.dsgcn_dynplain_bwd(p, p, p, p, p, p, 1 << 20, n, K, mid, V, ld, None) == -1, (n, K, mid, V, ld)
    assert lib.dsgcn_dynplain_bwd(p, p, p, p, p, p, 5015, 1, 8, 8, 25, 32, None) == -1          # partial rows too short


# ---- 5. the code objects ---------------------------------------------------------------------------------------------------

def test_plain_kb_kernels_have_no_scratch():
    """The new kernels (csrc/dynadj_plain.hip) in the built library: 0 scratch instructions, 0 spilled registers."""
    import sys
    from dsgcn_amd import native
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import codeobj_report
    native.build()
    ks = {k: v for k, v in codeobj_report.kernels(native.LIB_PATH).items() if k.startswith('k_dynplain')}
    assert {'k_dynplain_fwd<25>', 'k_dynplain_bwd<25>', 'k_dynplain_fwd<17>', 'k_dynplain_bwd<17>', 'k_dynplain_fwd<0>',
            'k_dynplain_bwd<0>'} == set(ks), sorted(ks)
    for name, k in ks.items():
        assert k.get('scratch_instructions', 0) == 0 and k.get('vgpr_spill_count', 0) == 0, (name, k)
        assert k.get('private_segment_fixed_size', 0) == 0, (name, k)


# ---- 6. host wiring on the CPU seam ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('tag', ['k8', 'k8_sw', 'k5'])
def test_unit_wiring_on_the_cpu_seam(tag):
    """The unit over the plain-torch op namespace (fp64): output, input gradient and parameter gradients equal the fp64
    restatement; the adjacency is one dynadj_plain call."""
    m, c = make_unit(tag)
    m = m.double().train()
    p = {k: v.detach().clone().requires_grad_() for k, v in m.named_parameters()}
    x32, r32 = unit_inputs(tag)
    calls = []
    x = x32.double().requires_grad_()
    with D.kernels.use_ops(F.cpu_ops(calls)):
        y = m(x)
    (y * r32.double()).sum().backward()
    assert calls == ['dynadj_plain']
    x64 = x32.double().requires_grad_()
    y64 = F.unit_forward(p, x64, c['subset_wise'])
    (y64 * r32.double()).sum().backward()
    assert float((y - y64).detach().norm() / y64.detach().norm()) < 1e-12
    assert float((x.grad - x64.grad).norm() / x64.grad.norm()) < 1e-12
    for k, t in m.named_parameters():
        if k in ZERO_GRAD_BIASES:
            continue
        want = p[k].grad
        if want is None or not torch.any(want):
            assert t.grad is None or not torch.any(t.grad), k
        else:
            assert float((t.grad - want).norm() / want.norm()) < 1e-10, (k, float((t.grad - want).norm() / want.norm()))


def test_three_subsets_keep_their_op_sequence():
    """K = 3: two dynadj calls and no dynadj_plain, as before; the choice follows A.size(0)."""
    torch.manual_seed(0)
    m = D.dggcn(64, 64, graph_A('nturgb+d', 3), ratio=0.25).train()
    assert {'_nt0', '_et0', '_we_eye'} <= set(dict(m.named_buffers()))
    calls = []
    with D.kernels.use_ops(F.cpu_ops(calls)):
        m(torch.randn(2, 64, 8, 25))
    assert calls == ['dynadj', 'dynadj']
