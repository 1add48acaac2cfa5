"""CPU: ``dgmsmlp`` and ``tcn_type='mstcn'`` / ``'dgmsmlp'`` in DGSTGCN — constructor parity with the reference
(tests/golden/unit_dgmsmlp.npz), the fp64 restatement (tests/dgmsmlp_fp64.py) that the GPU tests take as truth pinned to the
reference's fp64 outputs, the module's wiring run through plain torch ops, checkpoint loading, the shipped config with each
``tcn_type``, what raises, and the argument checks of the new entry points."""
import copy
import hashlib
import json
import os
import types

import numpy as np
import pytest
import torch

import dsgcn_amd as D
import dgmsmlp_fp64 as F
import torch_ops
from dsgcn_amd import kernels, native
from test_oracle_golden import GOLD, load

Z = load('unit_dgmsmlp.npz')
CASES = [str(c) for c in Z['cases']]
assert CASES == [c[0] for c in F.CASES]

# torch_ops + the one call the unit adds: the namespace for ``kernels.use_ops``
OPS = types.SimpleNamespace(**{k: v for k, v in vars(torch_ops).items() if not k.startswith('__')})
OPS.NAME = 'torch_ops + temporal_dgmlp (test reference)'
OPS.temporal_dgmlp = F.temporal_dgmlp


def sd_digest(module):
    h = hashlib.sha256()
    for k, v in module.state_dict().items():
        h.update(k.encode())
        h.update(v.detach().cpu().numpy().tobytes())
    return h.hexdigest()


def make_unit(tag, live=True):
    """The unit of fixture case `tag`, built under the fixture's seed; live: add_coeff / alpha / BatchNorm weights drawn as
    the fixture's were (checked against its digest)."""
    c = F.case(tag)
    torch.manual_seed(int(Z[tag + '_seed']))
    m = D.dgmsmlp(c['C'], c['C'], **F.unit_kwargs(c))
    if live:
        F.liven_unit(m, int(Z[tag + '_live_seed']))
        assert sd_digest(m) == str(Z[tag + '_live_digest'])
    return m, c


def unit_inputs(tag):
    c = F.case(tag)
    x, r = F.unit_inputs(c, int(Z[tag + '_input_seed']))
    assert hashlib.sha256(x.numpy().tobytes() + r.numpy().tobytes()).hexdigest() == str(Z[tag + '_input_digest'])
    return x, r


def restatement_kw(c):
    return dict(ms_cfg=c['kw'].get('ms_cfg'), stride=c['stride'], merge_after=c['kw'].get('merge_after', False))


def state_of(m, dtype=None, device=None):
    """parameters (as fresh leaves) and buffers by state_dict key, for F.unit_forward"""
    p = {k: v.detach().to(dtype=dtype, device=device).clone().requires_grad_() for k, v in m.named_parameters()}
    for k, v in m.named_buffers():
        if k.endswith('alpha'):
            p[k] = v.detach().to(dtype=dtype, device=device)
    return p


def check_against_fixture(tag, y, dx, grads, bar, bar_dx, bar_p):
    """y, dx, grads by parameter name against the fixture's fp64 values -> the errors"""
    errs = {'y': F.fixture_rel(Z, tag + '_y', y), 'dx': F.fixture_rel(Z, tag + '_dx', dx)}
    assert errs['y'] < bar and errs['dx'] < bar_dx, errs
    for k, g in grads.items():
        key = tag + '_grad_' + k
        if bias_under_bn(k):
            continue
        assert not F.fixture_is_zero(Z, key), k
        assert g is not None, k
        errs[k] = F.fixture_rel(Z, key, np.asarray(g))
        assert errs[k] < bar_p, (k, errs[k])
    return errs


def bias_under_bn(k):
    """a conv bias whose output goes straight into a train-mode BatchNorm: its gradient is zero up to rounding"""
    return k == 'transform.2.bias' or (k.startswith('branches.') and k.endswith('.0.bias'))


@pytest.mark.parametrize('tag', CASES)
def test_state_dict_matches_reference_constructor(tag):
    """Same keys in the same order, shapes and initial values (same RNG use: same creation order) as the reference's."""
    m, _ = make_unit(tag, live=False)
    manifest = json.loads(str(Z[tag + '_sd_manifest']))
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == manifest
    assert sd_digest(m) == str(Z[tag + '_init_digest'])


def test_add_tcn_and_adaptive_decide_the_keys():
    keys = {tag: [k for k, _ in json.loads(str(Z[tag + '_sd_manifest']))] for tag in CASES}
    assert not any('conv2' in k or 'alpha' in k for k in keys['d64'])              # the class default: no dilated conv
    assert sum(k.endswith('3.alpha') for k in keys['tcn_after']) == 4
    m, _ = make_unit('tcn_after', live=False)
    assert sum(k.endswith('alpha') for k, _ in m.named_parameters()) == 4
    m, _ = make_unit('tcn_before_s2', live=False)                                  # adaptive=False: alpha is a buffer of ones
    assert not any(k.endswith('alpha') for k, _ in m.named_parameters())
    assert [float(v) for k, v in m.named_buffers() if k.endswith('alpha')] == [1.0] * 4
    assert dict(json.loads(str(Z['k5_sd_manifest'])))['branches.0.3.conv.weight'] == [16, 1, 3]


@pytest.mark.parametrize('tag', CASES)
def test_reference_checkpoint_loads_strict(tag):
    m, _ = make_unit(tag, live=False)
    g = torch.Generator().manual_seed(1)
    sd = {k: (torch.randn(shape, generator=g) if shape else torch.zeros((), dtype=torch.long))
          for k, shape in json.loads(str(Z[tag + '_sd_manifest']))}
    assert m.load_state_dict(sd, strict=True).missing_keys == []
    assert torch.equal(m.state_dict()['branches.0.3.conv1.weight'], sd['branches.0.3.conv1.weight'])


@pytest.mark.parametrize('tag', CASES)
def test_fp64_restatement_matches_reference(tag):
    """tests/dgmsmlp_fp64.py against the reference's fp64 output, input gradient and every parameter gradient."""
    m, c = make_unit(tag)
    p = state_of(m, torch.float64)
    x, r = unit_inputs(tag)
    x = x.double().requires_grad_()
    y = F.unit_forward(p, x, **restatement_kw(c))
    (y * r.double()).sum().backward()
    check_against_fixture(tag, y.detach().numpy(), x.grad.numpy(),
                          {k: (None if t.grad is None else t.grad.numpy()) for k, t in p.items() if t.requires_grad},
                          1e-12, 1e-12, 1e-11)


@pytest.mark.parametrize('tag', CASES)
def test_module_wiring_in_torch_ops_matches_reference(tag):
    """The module itself (stacked branch conv with the global joint, alpha-scaled convs, taps by channel, deferred
    BatchNorms) with every op in plain torch, in fp64."""
    m, _ = make_unit(tag)
    m = m.double().train()
    x, r = unit_inputs(tag)
    x = x.double().requires_grad_()
    with kernels.use_ops(OPS):
        y = m(x)
    (y * r.double()).sum().backward()
    check_against_fixture(tag, y.detach().numpy(), x.grad.numpy(),
                          {k: (None if p.grad is None else p.grad.numpy()) for k, p in m.named_parameters()},
                          1e-10, 1e-9, 1e-8)
    assert int(m.transform[0].num_batches_tracked) == 1 and int(m.branches[0][1].num_batches_tracked) == 1


@pytest.mark.parametrize('shape', [(3, 96, 7, 25, 2, dict(add_tcn=True)), (2, 60, 4, 17, 1, dict()),
                                   (2, 64, 6, 25, 1, dict(add_tcn=True, merge_after=True, ms_cfg=[(9, 1), ('max', 3), '1x1']))],
                         ids=repr)
def test_restatement_vs_reference_live(shape):
    """Beyond the fixtures: the restatement against the imported class, where the reference is present."""
    import ref_shim
    if not ref_shim.available():
        pytest.skip('the reference checkout is not on this machine')
    R = ref_shim.load()
    n, C, T, V, stride, kw = shape
    torch.manual_seed(3)
    ref = R.gutils.dgmsmlp(C, C, num_joints=V, stride=stride, **kw)
    F.liven_unit(ref, 4)
    ref = ref.double().train()
    p = state_of(ref, torch.float64)
    c = dict(C=C, T=T, V=V, stride=stride)
    x32, r32 = F.unit_inputs(c, 5, n=n)
    res = []
    for fn in (ref, lambda t: F.unit_forward(p, t, ms_cfg=kw.get('ms_cfg'), stride=stride,
                                             merge_after=kw.get('merge_after', False))):
        x = x32.double().requires_grad_()
        y = fn(x)
        (y * r32.double()).sum().backward()
        res.append((y.detach(), x.grad))
    for a, b in zip(*res):
        assert float((a - b).norm() / b.norm()) < 1e-12
    for k, t in ref.named_parameters():
        if not bias_under_bn(k):
            assert float((p[k].grad - t.grad).norm() / t.grad.norm()) < 1e-11, k


@pytest.mark.parametrize('kw,word', [
    (dict(channel_annention=True), 'channel_annention'),
    (dict(ms_cfg=[(3, 1), '1x1', ('max', 3)]), "'1x1'"),
    (dict(ms_cfg=[(3, 1), (5, 2), ('max', 3), '1x1']), 'kernel size'),
    (dict(ms_cfg=[(3, 1), ('max', 5), '1x1']), 'max-pool kernel 5'),
    (dict(ms_cfg=[(7, 1), ('max', 3), '1x1']), 'kernel size 7'),
])
def test_unsupported_options_raise_naming_the_option(kw, word):
    with pytest.raises(NotImplementedError, match=word):
        D.dgmsmlp(64, 64, **kw)


def ds_cfg(**bk):
    """configs/dsstgcn/DSSTGCN_model.py"""
    backbone = dict(
        type='DGSTGCN', gcn_type='dgphgcn1', gcn_ratio=0.125, gcn_node_attention=True, gcn_edge_attention=True,
        gcn_decompose=True, gcn_subset_wise=True, gcn_ctr='T', gcn_ada='T', tcn_type='dgmstcn',
        graph_cfg=dict(layout='nturgb+d', mode='random', num_filter=3, init_off=.04, init_std=.02),
        tcn_ms_cfg=[(3, 1), (3, 2), (3, 3), (3, 4), ('max', 3), '1x1'])
    backbone.update(bk)
    return dict(type='RecognizerGCN', backbone=backbone, cls_head=dict(type='GCNHead', num_classes=60, in_channels=256))


@pytest.mark.parametrize('bk,cls', [(dict(tcn_type='mstcn'), 'mstcn'), (dict(tcn_type='dgmsmlp'), 'dgmsmlp'),
                                    (dict(tcn_type='dgmsmlp', tcn_add_tcn=True, tcn_merge_after=True), 'dgmsmlp'),
                                    (dict(tcn_type='dgmsmlp', tcn_add_tcn=True, tcn_adaptive=False), 'dgmsmlp')],
                         ids=repr)
def test_shipped_model_file_with_each_tcn_type(bk, cls):
    """The `tcn_type` line of the shipped model file flipped to the two values that used to raise."""
    m = D.build_model(ds_cfg(**bk))
    assert [type(b.tcn).__name__ for b in m.backbone.gcn] == [cls] * 10
    assert [b.tcn.stride for b in m.backbone.gcn] == [1, 1, 1, 1, 2, 1, 1, 2, 1, 1]
    if cls == 'dgmsmlp':
        assert all(b.tcn.add_tcn == bk.get('tcn_add_tcn', False) for b in m.backbone.gcn)
        assert all(b.tcn.num_joints == 25 for b in m.backbone.gcn)


@pytest.mark.parametrize('tcn_type', ['mstcn', 'dgmsmlp'])
def test_tcn_dropout_reaches_the_unit(tcn_type):
    m = D.build_model(ds_cfg(tcn_type=tcn_type, tcn_dropout=0.25))
    # what _FusedBlock.forward_fused hands to fuse_out (the first block takes no dropout: dgstgcn.py:112)
    assert [b.tcn.drop.p for b in m.backbone.gcn] == [0.0] + [0.25] * 9


def test_unit_tcn_and_dgmstcn_are_built_as_before():
    assert type(D.build_model(ds_cfg()).backbone.gcn[0].tcn) is D.dgmstcn
    cfg = ds_cfg(tcn_type='unit_tcn')
    del cfg['backbone']['tcn_ms_cfg']
    assert type(D.build_model(cfg).backbone.gcn[0].tcn) is D.unit_tcn


@pytest.mark.parametrize('name', ['model_reduced_dg_mstcn', 'model_reduced_dg_msmlp'])
def test_reduced_model_fixture_loads_strict(name):
    z = load(name + '.npz')
    with open(os.path.join(GOLD, name + '_cfg.json')) as f:
        cfg = json.load(f)
    m = D.build_model(copy.deepcopy(cfg))
    m.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith('sd_')}, strict=True)
    assert len(m.backbone.gcn) == 4 and m.backbone.gcn[2].tcn.stride == 2


def test_flat_groups_and_fusable_pairs():
    m, _ = make_unit('tcn_after', live=False)
    groups = m.flat_groups()
    assert [len(g) for g in groups] == [6, 6, 5, 5]
    assert m.fusable_pairs() == [(m.transform[2], m.bn)]
    m.init_weights()


def test_window_tables():
    t = kernels._mlpwin_tables(F.DEFAULT_CFG, [14, 10, 10, 10, 10, 10], True, True)
    assert t == ([0, 0, 0, 0, 1, 1], [0, 14, 24, 34, 44, 54], [14, 10, 10, 10, 10, 10], [1, 2, 3, 4, 1, 1], [2, 2, 2, 2, 0, 0])
    assert kernels._mlpwin_tables(F.DEFAULT_CFG, [14, 10, 10, 10, 10, 10], True, False)[4] == [1, 1, 1, 1, 0, 0]
    assert kernels._mlpwin_tables(F.DEFAULT_CFG, [14, 10, 10, 10, 10, 10], False, True)[4] == [0] * 6


def _tabs(widths, cfg=F.DEFAULT_CFG, add_tcn=True, merge_after=True):
    return kernels._mlpwin_tables(cfg, widths, add_tcn, merge_after)


def test_range_query_without_gpu():
    """dsgcn_mlpwin_supported: width <= 64, KM in {2, 3, 5}, V1 <= 33, stride 1 or 2, any T >= 1, any n."""
    ok = kernels.mlpwin_supported
    w64, w256 = [14, 10, 10, 10, 10, 10], [46, 42, 42, 42, 42, 42]
    assert ok(128, 64, 64, 26, 1, 2, _tabs(w64)) and ok(1, 256, 1, 18, 2, 2, _tabs(w256)) and ok(2, 64, 9, 33, 1, 5, _tabs(w64))
    assert ok(2, 64, 9, 26, 1, 3, _tabs(w64)) and ok(2, 128, 9, 26, 1, 2, _tabs([64, 64], [(3, 1), '1x1']))
    assert not ok(2, 130, 9, 26, 1, 2, _tabs([65, 65], [(3, 1), '1x1']))          # window width 65
    assert not ok(2, 64, 9, 34, 1, 2, _tabs(w64))                                 # V1 = 34
    assert not ok(2, 64, 9, 26, 3, 2, _tabs(w64))                                 # stride 3
    assert not ok(2, 64, 9, 26, 1, 4, _tabs(w64))                                 # KM = 4
    assert not ok(2, 64, 9, 26, 1, 2, _tabs([32, 32], [('max', 3), '1x1']))       # no mlp window
    assert not ok(2, 65, 9, 26, 1, 2, _tabs(w64))                                 # the windows do not tile the channels


def test_argument_rejection_without_gpu():
    """NULL pointers / non-positive sizes: DSGCN_EINVAL (-1) before any launch; a shape out of range: DSGCN_EUNSUPPORTED."""
    lib = native.lib()
    ia, pa = kernels._int_array, kernels._ptr_array
    tabs = [ia(t) for t in _tabs([14, 10, 10, 10, 10, 10])]
    nul = pa([None] * 6)
    assert lib.dsgcn_mlpwin_fwd(None, None, None, None, None, 2, 64, 9, 26, 1, 2, 6, *tabs, nul, nul, None) == -1
    assert lib.dsgcn_mlpwin_bwd(None, None, None, None, None, None, None, None, None, 2, 64, 9, 26, 1, 2, 6, *tabs, nul, 0,
                                None) == -1
    one = 16       # (a non-NULL address that is never dereferenced: the sizes are rejected first)
    assert lib.dsgcn_mlpwin_fwd(one, one, one, one, one, 0, 64, 9, 26, 1, 2, 6, *tabs, nul, nul, None) == -1
    assert lib.dsgcn_mlpwin_fwd(one, one, one, one, one, 2, 64, 0, 26, 1, 2, 6, *tabs, nul, nul, None) == -1
    assert lib.dsgcn_mlpwin_bwd(one, one, one, one, one, one, one, one, one, 2, 64, 9, 26, 1, 2, 0, *tabs, nul, 0, None) == -1
    assert lib.dsgcn_mlpwin_fwd(one, one, one, one, one, 2, 64, 9, 34, 1, 2, 6, *tabs, nul, nul, None) == -2
    assert lib.dsgcn_mlpwin_fwd(one, one, one, one, one, 2, 64, 9, 26, 1, 2, 6, *tabs, nul, nul, None) == -1   # NULL W1
    assert lib.dsgcn_mlpwin_supported(2, 64, 9, 26, 1, 2, 6, None, None, None, None, None) == 0
    assert lib.dsgcn_mlpwin_partial_stride(64, 2, 6, tabs[0], tabs[2]) == 64 * 3 + 14 * 15 + 3 * 10 * 11
    assert lib.dsgcn_mlpwin_partial_stride(0, 2, 6, tabs[0], tabs[2]) == -1
