"""CPU: the ``dghgcn`` unit (DGSTGCN's default gcn_type) — constructor parity with the reference (tests/golden/
unit_dghgcn.npz), the flags without a HIP path, the default DGSTGCN, and the fp64 restatement (tests/dghgcn_fp64.py)
that the full-size GPU tests take as truth, pinned to the reference's fp64 outputs."""
import json

import numpy as np
import pytest
import torch

import dsgcn_amd as D
import dghgcn_fp64 as F
from test_oracle_golden import load

Z = load('unit_dghgcn.npz')
CASES = [str(c) for c in Z['cases']]


def make_unit(tag, z=Z):
    """The unit of fixture case `tag`, built under the fixture's seed, with the fixture's live alpha / beta."""
    ci, co, na, ea, at, sw, seed = [int(v) for v in z[tag + '_cfg']]
    V = z[tag + '_node_type'].shape[0]
    torch.manual_seed(seed)
    m = D.dghgcn(ci, co, graph_A(V), torch.from_numpy(z[tag + '_edge_type']), torch.from_numpy(z[tag + '_node_type']),
                 ratio=float(z[tag + '_ratio']), node_attention=bool(na), edge_attention=bool(ea), add_type=bool(at),
                 subset_wise=bool(sw))
    return m, dict(P=m.num_types if na else 1, add_type=bool(at), subset_wise=bool(sw))


def unit_inputs(tag, z=Z):
    """x, R of fixture case `tag`, regenerated from their seed and checked against the fixture's digest."""
    import hashlib
    ci, co = [int(v) for v in z[tag + '_cfg'][:2]]
    x, r = F.unit_inputs(ci, co, z[tag + '_node_type'].shape[0], int(z[tag + '_input_seed']))
    assert hashlib.sha256(x.numpy().tobytes() + r.numpy().tobytes()).hexdigest() == str(z[tag + '_input_digest'])
    return x, r


def graph_A(V):
    np.random.seed(21)          # the fixture's graphs (mode='random' draws its off-diagonal weights)
    g = D.Graph(layout='coco' if V == 17 else 'nturgb+d', mode='random', num_filter=3, init_off=.04, init_std=.02)
    return torch.tensor(np.asarray(g.A), dtype=torch.float32)


def sd_digest(module):
    import hashlib
    h = hashlib.sha256()
    for k, v in module.state_dict().items():
        h.update(k.encode())
        h.update(v.detach().cpu().numpy().tobytes())
    return h.hexdigest()


@pytest.mark.parametrize('tag', CASES)
def test_state_dict_matches_reference_constructor(tag):
    """Same keys, shapes and initial values (same RNG use: same creation order) as the reference's dghgcn."""
    m, _ = make_unit(tag)
    manifest = json.loads(str(Z[tag + '_sd_manifest']))
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == manifest
    assert sd_digest(m) == str(Z[tag + '_init_digest'])


@pytest.mark.parametrize('kw,flag', [(dict(ada_attention=True), 'ada_attention'),
                                     (dict(target_specific=True), 'target_specific'),
                                     (dict(ctr='NA'), 'ctr'), (dict(ada=None), 'ada'),
                                     (dict(ctr_act='sigmoid'), 'ctr_act'), (dict(ada_act='tanh'), 'ada_act'),
                                     (dict(act='GELU'), 'GELU'), (dict(ratio=0.5), 'ratio')])
def test_unsupported_flags_raise_naming_the_flag(kw, flag):
    A = graph_A(25)
    g = D.Graph(layout='nturgb+d', mode='spatial')
    with pytest.raises(NotImplementedError, match=flag):
        D.dghgcn(64, 256 if flag == 'ratio' else 64, A, torch.tensor(g.edge_type), torch.tensor(g.node_type), **kw)


def test_more_than_three_subsets_raise():
    g = D.Graph(layout='nturgb+d', mode='spatial')
    A = torch.rand(4, 25, 25)
    with pytest.raises(NotImplementedError, match='num_subsets'):
        D.dghgcn(64, 64, A, torch.tensor(g.edge_type), torch.tensor(g.node_type))


def test_default_dgstgcn_builds():
    """DGSTGCN at its own defaults: dghgcn + unit_tcn blocks (dgstgcn.py:29,40); with a 60-class GCNHead the reference
    model has 3 177 500 parameters (3 162 080 in the backbone); mid = 64 on the 256-channel stage."""
    model = D.build_model(dict(
        type='RecognizerGCN', cls_head=dict(type='GCNHead', num_classes=60, in_channels=256),
        backbone=dict(type='DGSTGCN', graph_cfg=dict(layout='nturgb+d', mode='random', num_filter=3, init_off=.04,
                                                     init_std=.02))))
    bb = model.backbone
    gcns = [b.gcn for b in bb.gcn]
    assert all(type(g).__name__ == 'dghgcn' for g in gcns)
    assert all(type(b.tcn).__name__ == 'unit_tcn' for b in bb.gcn)
    assert sum(p.numel() for p in model.parameters()) == 3177500
    assert sum(p.numel() for p in bb.parameters()) == 3162080
    assert gcns[-1].mid_channels == 64


@pytest.mark.parametrize('tag', CASES)
def test_fp64_restatement_matches_reference(tag):
    """tests/dghgcn_fp64.py against the reference's fp64 output, input gradient and every parameter gradient."""
    m, kw = make_unit(tag)
    m = m.double()
    with torch.no_grad():
        m.alpha.copy_(torch.from_numpy(Z[tag + '_alpha']))
        m.beta.copy_(torch.from_numpy(Z[tag + '_beta']))
    p = {k: v.detach().clone().requires_grad_() for k, v in m.named_parameters()}
    x, r = unit_inputs(tag)
    x = x.double().requires_grad_()
    y = F.unit_forward(p, x, Z[tag + '_node_type'], Z[tag + '_edge_type'], **kw)
    (y * r.double()).sum().backward()
    assert F.fixture_rel(Z, tag + '_y', y.detach().numpy()) < 1e-12
    assert F.fixture_rel(Z, tag + '_dx', x.grad.numpy()) < 1e-12
    for k, t in p.items():
        key = tag + '_grad_' + k
        got = t.grad if t.grad is not None else torch.zeros_like(t)
        if F.fixture_is_zero(Z, key):
            assert not torch.any(got), k                         # alpha[1:], beta[1:] without subset_wise
        elif k in ('pre.0.bias', 'post.bias', 'down.0.bias'):
            # a bias under a train-mode BatchNorm: the gradient is exactly zero, both sides hold rounding noise
            assert float(got.abs().max()) < 1e-10 and np.abs(Z[key]).max() < 1e-10, k
        else:
            assert F.fixture_rel(Z, key, got.numpy()) < 1e-12, (k, F.fixture_rel(Z, key, got.numpy()))


def test_probe_detects_a_single_wrong_element():
    """The compact fixture form: one element off by 1e-3 of the array's norm shows in the probes at that order."""
    a = np.random.default_rng(0).standard_normal(50000)
    z = {'k_probe': F.probe(a, 'k')}
    b = a.copy()
    b[12345] += 1e-3 * np.linalg.norm(a)
    assert F.fixture_rel(z, 'k', a) < 1e-14
    assert 3e-4 < F.fixture_rel(z, 'k', b) < 3e-3


def test_typed_kb_kernels_have_no_scratch():
    """The new kernels (csrc/dynadj_typed.hip) in the built library: 0 scratch instructions, 0 spilled registers."""
    import os
    import sys
    from dsgcn_amd import native
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import codeobj_report
    native.build()
    ks = {k: v for k, v in codeobj_report.kernels(native.LIB_PATH).items() if k.startswith('k_dyntyped')}
    assert {'k_dyntyped_select_fwd', 'k_dyntyped_select_bwd', 'k_dyntyped_fwd<25>', 'k_dyntyped_bwd<25>',
            'k_dyntyped_fwd<17>', 'k_dyntyped_bwd<17>', 'k_dyntyped_fwd<0>', 'k_dyntyped_bwd<0>'} <= set(ks), sorted(ks)
    for name, k in ks.items():
        assert k.get('scratch_instructions', 0) == 0 and k.get('vgpr_spill_count', 0) == 0, (name, k)
