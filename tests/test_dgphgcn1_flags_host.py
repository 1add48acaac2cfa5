"""CPU: the ``dgphgcn1`` switches (the DS-GCN ablation arms) and ``DGSTGCN(gcn_stage=[...])`` — constructor parity with the
reference for every fixture unit (tests/golden/unit_dgphgcn1_flags.npz), the flags still without a HIP path, the staged
backbone, the fp64 restatement (tests/dgphgcn1_flags_fp64.py) pinned to the reference, the fixtures' regeneration, and
the new kernels' code objects."""
import copy
import hashlib
import json
import os
import re

import numpy as np
import pytest
import torch

import dsgcn_amd as D
import dgphgcn1_flags_fp64 as F
from test_dghgcn_host import graph_A, sd_digest
from test_oracle_golden import GOLD, load

Z = load('unit_dgphgcn1_flags.npz')
CASES = [str(c) for c in Z['cases']]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ['stage_odd', 'stage_head', 'node_off', 'edge_off', 'ada']
ZERO_GRAD_BIASES = ('pre.0.bias', 'post.bias', 'down.0.bias')     # under a train-mode BatchNorm: exactly zero


def _ref():
    """The imported reference (tests/golden/ref_shim.py), or a skip where its checkout is absent."""
    import ref_shim
    if not ref_shim.available():
        pytest.skip('the reference checkout is not on this machine')
    return ref_shim.load()


def case_cfg(tag, z=Z):
    return json.loads(str(z[tag + '_cfg']))


def make_unit(tag, z=Z, cls=None):
    """The unit of fixture case `tag`, built under the fixture's seed -> (unit, effective flags of the restatement)"""
    c = case_cfg(tag, z)
    V = z[tag + '_node_type'].shape[0]
    torch.manual_seed(c['seed'])
    m = (cls or D.dgphgcn1)(c['ci'], c['co'], graph_A(V), torch.from_numpy(z[tag + '_edge_type']),
                            torch.from_numpy(z[tag + '_node_type']), ratio=c['ratio'], **c['flags'])
    return m, F.effective_flags(**c['flags'])


def unit_inputs(tag, z=Z):
    c = case_cfg(tag, z)
    x, r = F.unit_inputs(c['ci'], c['co'], z[tag + '_node_type'].shape[0], int(z[tag + '_input_seed']))
    assert hashlib.sha256(x.numpy().tobytes() + r.numpy().tobytes()).hexdigest() == str(z[tag + '_input_digest'])
    return x, r


def test_fixture_holds_the_cases_the_arms_need():
    flags = {t: case_cfg(t)['flags'] for t in CASES}
    combos = {(f['decompose'], f['node_attention'], f['edge_attention']) for t, f in flags.items() if re.match(r'd\dn\de\d', t)}
    assert len(combos) == 8
    assert flags['subset_off']['subset_wise'] is False and flags['sub_att_off']['sub_att'] is False
    assert flags['stage_off']['stage'] is False and flags['add_type']['add_type'] is True
    assert flags['ada']['ada_attention'] and flags['ada']['decompose']
    assert flags['ada_plain']['ada_attention'] and not flags['ada_plain']['decompose']
    assert case_cfg('down')['co'] == 128 and case_cfg('coco')['layout'] == 'coco'
    assert (case_cfg('wide')['ci'], case_cfg('wide')['co']) == (128, 256)


@pytest.mark.parametrize('tag', CASES)
def test_state_dict_matches_reference_constructor(tag):
    """Same keys, shapes and initial values (same RNG use: same creation order) as the reference's dgphgcn1."""
    m, _ = make_unit(tag)
    manifest = json.loads(str(Z[tag + '_sd_manifest']))
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == manifest
    assert sd_digest(m) == str(Z[tag + '_init_digest'])


def test_quirks_of_the_reference_constructor():
    keys = {t: [k for k, _ in json.loads(str(Z[t + '_sd_manifest']))] for t in CASES}
    shapes = {t: dict(json.loads(str(Z[t + '_sd_manifest']))) for t in CASES}
    for t in ('d0n0e0', 'd0n1e1', 'stage_off', 'ada_plain'):        # decompose off: no semantic rows, edge flag ignored
        assert not any(k.startswith(('conv1_se', 'conv2_se', 'edge_linears')) for k in keys[t]), t
        assert shapes[t]['conv1.weight'][0] == 3 * 8
    assert shapes['d1n0e1']['conv1_se.weight'][0] == 8 and shapes['d1n1e1']['conv1_se.weight'][0] == 8 * 5
    assert 'conv2_se.weight' in keys['d1n0e0'] and 'edge_linears.weight' not in keys['d1n1e0']
    assert shapes['ada']['ada_linears.weight'] == [45, 3, 1, 1] and shapes['sub_att_off']['alpha'] == [3]
    m, _ = make_unit('stage_off')
    assert not (m.decompose or m.node_attention or m.edge_attention or m.subset_wise)


@pytest.mark.parametrize('tag', CASES)
def test_reference_state_dict_loads_strict_live(tag):
    """strict=True load of the imported reference unit's state_dict (reference checkout present), values included."""
    R = _ref()
    m, _ = make_unit(tag)
    ref, _ = make_unit(tag, cls=R.gutils.dgphgcn1)
    with torch.no_grad():
        for p in ref.parameters():
            p.add_(0.25)
    m.load_state_dict(ref.state_dict(), strict=True)
    for (k, a), (k2, b) in zip(m.state_dict().items(), ref.state_dict().items()):
        assert k == k2 and torch.equal(a, b), k


def test_manifest_loads_strict():
    """strict=True load of a state_dict with the reference's keys and shapes (from the fixture: no checkout needed)."""
    for tag in CASES:
        m, _ = make_unit(tag)
        sd = {k: torch.zeros(s, dtype=torch.int64 if k.endswith('num_batches_tracked') else torch.float32)
              for k, s in json.loads(str(Z[tag + '_sd_manifest']))}
        m.load_state_dict(sd, strict=True)


@pytest.mark.parametrize('kw,flag', [(dict(target_specific=True, decompose=True), 'target_specific'),
                                     (dict(ctr='NA'), 'ctr'), (dict(ctr=None), 'ctr'), (dict(ada=None), 'ada'),
                                     (dict(ada='NA'), 'ada'),
                                     (dict(ctr_act='sigmoid'), 'ctr_act'), (dict(ada_act='tanh'), 'ada_act'),
                                     (dict(act='GELU'), 'GELU'), (dict(ratio=0.5), 'mid'),
                                     (dict(ada_attention=True, edge_num=20), 'edge_num'),
                                     (dict(decompose=True, node_attention=True, num_types=20), 'num_types')])
def test_unsupported_flags_raise_naming_the_flag(kw, flag):
    g = D.Graph(layout='nturgb+d', mode='spatial')
    with pytest.raises(NotImplementedError, match=flag):
        D.dgphgcn1(64, 256 if flag == 'mid' else 64, graph_A(25), torch.tensor(g.edge_type), torch.tensor(g.node_type), **kw)


def test_more_than_three_subsets_and_wide_graphs_raise():
    g = D.Graph(layout='nturgb+d', mode='spatial')
    with pytest.raises(NotImplementedError, match='num_subsets'):
        D.dgphgcn1(64, 64, torch.rand(4, 25, 25), torch.tensor(g.edge_type), torch.tensor(g.node_type))
    with pytest.raises(NotImplementedError, match='joints'):
        D.dgphgcn1(64, 64, torch.rand(3, 40, 40), torch.zeros(40, 40), torch.zeros(40))


def ds_cfg(**bk):
    backbone = dict(
        type='DGSTGCN', gcn_type='dgphgcn1', gcn_ratio=0.125, gcn_node_attention=True, gcn_edge_attention=True,
        gcn_decompose=True, gcn_subset_wise=True, gcn_ctr='T', gcn_ada='T', tcn_type='dgmstcn',
        graph_cfg=dict(layout='nturgb+d', mode='random', num_filter=3, init_off=.04, init_std=.02),
        tcn_ms_cfg=[(3, 1), (3, 2), (3, 3), (3, 4), ('max', 3), '1x1'])
    backbone.update(bk)
    return dict(type='RecognizerGCN', backbone=backbone, cls_head=dict(type='GCNHead', num_classes=60, in_channels=256))


def test_gcn_stage_builds_and_marks_the_listed_blocks():
    stages = [1, 3, 5, 7, 9]
    m = D.build_model(ds_cfg(gcn_stage=stages))
    assert len(m.backbone.gcn) == 10
    for i, b in enumerate(m.backbone.gcn):
        assert hasattr(b.gcn, 'edge_linears') == (i in stages), i
        assert hasattr(b.gcn, 'conv1_se') == (i in stages), i
        assert b.gcn._shipped == (i in stages)


@pytest.mark.parametrize('stages', [[1, 3, 5, 7, 9], [0, 1, 2, 3], [4, 5, 6], [7, 8, 9], [0, 2, 4, 6, 8]])
def test_shipped_model_file_with_each_gcn_stage_line(stages):
    """configs/dsstgcn/DSSTGCN_model.py with its commented gcn_stage line enabled, for each list beside it."""
    m = D.build_model(ds_cfg(gcn_stage=stages))
    assert [i for i, b in enumerate(m.backbone.gcn) if b.gcn.decompose] == stages


@pytest.mark.parametrize('bk', [dict(gcn_add_type=False), dict(gcn_target_specific=False), dict(gcn_ada_attention=False),
                                dict(gcn_ada_attention=True), dict(gcn_sub_att=False), dict(gcn_num_types=5),
                                dict(gcn_edge_num=15), dict(gcn_node_attention=False), dict(gcn_edge_attention=False),
                                dict(gcn_decompose=False), dict(gcn_subset_wise=False)])
def test_shipped_model_file_with_each_switch(bk):
    D.build_model(ds_cfg(**bk))


def test_gcn_stage_reaches_only_units_that_take_it():
    """The reference hands gcn_stage to every gcn_type; only dgphgcn1 has the argument."""
    cfg = ds_cfg(gcn_stage=[1, 3])
    cfg['backbone']['gcn_type'] = 'dghgcn'
    del cfg['backbone']['gcn_decompose']
    with pytest.raises(TypeError, match='stage'):
        D.build_model(cfg)


@pytest.mark.parametrize('arm', MODELS)
def test_reduced_model_fixture_loads_strict(arm):
    z = load(f'model_reduced_ds_{arm}.npz')
    with open(os.path.join(GOLD, f'model_reduced_ds_{arm}_cfg.json')) as f:
        cfg = json.load(f)
    cfg['backbone']['tcn_ms_cfg'] = [tuple(c) if isinstance(c, list) else c for c in cfg['backbone']['tcn_ms_cfg']]
    m = D.build_model(copy.deepcopy(cfg))
    m.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith('sd_')}, strict=True)
    assert any(not b.gcn._shipped for b in m.backbone.gcn)


def _restatement(tag, z=Z):
    m, fl = make_unit(tag, z)
    m = m.double()
    with torch.no_grad():
        m.alpha.copy_(torch.from_numpy(z[tag + '_alpha']))
        m.beta.copy_(torch.from_numpy(z[tag + '_beta']))
    p = {k: v.detach().clone().requires_grad_() for k, v in m.named_parameters()}
    x, r = unit_inputs(tag, z)
    x = x.double().requires_grad_()
    y = F.unit_forward(p, x, z[tag + '_node_type'], z[tag + '_edge_type'], fl)
    (y * r.double()).sum().backward()
    return p, x, y


@pytest.mark.parametrize('tag', CASES)
def test_fp64_restatement_matches_reference_fixture(tag):
    """tests/dgphgcn1_flags_fp64.py against the reference's fp64 output, input gradient and every parameter gradient."""
    p, x, y = _restatement(tag)
    assert F.fixture_rel(Z, tag + '_y', y.detach().numpy()) < 1e-12
    assert F.fixture_rel(Z, tag + '_dx', x.grad.numpy()) < 1e-12
    for k, t in p.items():
        key = tag + '_grad_' + k
        got = t.grad if t.grad is not None else torch.zeros_like(t)
        if F.fixture_is_zero(Z, key):
            assert not torch.any(got), k                         # conv2_se; alpha[1:], beta[1:] without subset_wise
        elif k in ZERO_GRAD_BIASES:
            assert float(got.abs().max()) < 1e-10, k
        else:
            assert F.fixture_rel(Z, key, got.numpy()) < 1e-12, (k, F.fixture_rel(Z, key, got.numpy()))


@pytest.mark.parametrize('tag', CASES)
def test_fp64_restatement_matches_reference_live(tag):
    """Element by element against the imported reference class in fp64 (reference checkout present)."""
    R = _ref()
    p, x, y = _restatement(tag)
    ref, _ = make_unit(tag, cls=R.gutils.dgphgcn1)
    ref = ref.double()
    with torch.no_grad():
        ref.alpha.copy_(torch.from_numpy(Z[tag + '_alpha']))
        ref.beta.copy_(torch.from_numpy(Z[tag + '_beta']))
    x32, r = unit_inputs(tag)
    xr = x32.double().requires_grad_()
    yr = ref(xr)
    (yr * r.double()).sum().backward()

    def rel(a, b):
        return float((a - b).norm() / (b.norm() + 1e-300))
    assert rel(y.detach(), yr.detach()) < 1e-12 and rel(x.grad, xr.grad) < 1e-12
    for k, t in ref.named_parameters():
        if t.grad is None or k in ZERO_GRAD_BIASES or not torch.any(t.grad):
            assert p[k].grad is None or float(p[k].grad.abs().max()) < 1e-10, k
        else:
            assert rel(p[k].grad, t.grad) < 1e-12, (k, rel(p[k].grad, t.grad))


def test_fixtures_regenerate_byte_identically_live(tmp_path):
    """A fresh run of the generator (its own process: single-threaded, default state) rewrites every fixture byte for byte."""
    _ref()
    import subprocess
    import sys
    subprocess.run([sys.executable, os.path.join(GOLD, 'gen_golden_ablation.py'), '--out', str(tmp_path)], check=True,
                   capture_output=True)
    names = ['unit_dgphgcn1_flags.npz'] + [f'model_reduced_ds_{a}{s}' for a in MODELS for s in ('.npz', '_cfg.json')]
    for name in names:
        with open(os.path.join(GOLD, name), 'rb') as f, open(tmp_path / name, 'rb') as g:
            assert f.read() == g.read(), name
        assert os.path.getsize(os.path.join(GOLD, name)) < 500_000, name


def test_flag_kb_kernels_have_no_scratch():
    """The new kernels (csrc/dynadj_flags.hip) in the built library: 0 scratch instructions, 0 spilled registers."""
    import sys
    from dsgcn_amd import native
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import codeobj_report
    native.build()
    ks = {k: v for k, v in codeobj_report.kernels(native.LIB_PATH).items() if k.startswith('k_dynflag')}
    words = [0, 1, 2, 5, 6, 8, 9, 10, 13, 14]
    words += [w | 16 for w in words]
    want = {f'k_dynflag_fwd<{w}, {v}>' for w in words for v in (25, 0)}
    want |= {f'k_dynflag_bwd<{w}, 0>' for w in words} | {f'k_dynflag_bwd<{w}, 25>' for w in words if not w & 8}
    assert want <= set(ks), sorted(want - set(ks))
    for name, k in ks.items():
        assert k.get('scratch_instructions', 0) == 0 and k.get('vgpr_spill_count', 0) == 0, (name, k)
        assert k.get('group_segment_fixed_size', 0) <= 65536, (name, k)


def test_header_symbols_exported_and_bound():
    import subprocess
    from dsgcn_amd import native
    from test_native_abi import declared_symbols
    names = declared_symbols()
    new = {'dsgcn_dynflag_partial_stride', 'dsgcn_dynflag_fwd', 'dsgcn_dynflag_bwd'}
    assert new <= set(names) and new <= set(native.SIGNATURES)
    out = subprocess.run(['nm', '-D', '--defined-only', native.build()], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r' T (dsgcn_\w+)', out))) == names


def test_flag_kb_rejects_bad_arguments_without_gpu():
    lib = D.native.lib()
    assert lib.dsgcn_dynflag_partial_stride(8, 25, 15, 0) == 3 * 625 + 6
    assert lib.dsgcn_dynflag_partial_stride(8, 25, 15, 2 | 4 | 8 | 16) == 3 * 625 + 6 + 15 * 8 + 12 * 15
    assert lib.dsgcn_dynflag_fwd(*[None] * 11, 1, 8, 25, 32, 1, 15, 0, None) == -1           # NULL pointers
    one = 1                                                                                   # any non-NULL address
    assert lib.dsgcn_dynflag_fwd(one, None, None, None, None, one, one, one, None, None, one, 1, 8, 25, 32, 1, 15, 4,
                                 None) == -2                                                  # edge linear without decompose
    assert lib.dsgcn_dynflag_fwd(one, None, None, None, None, one, one, one, None, None, one, 1, 65, 25, 32, 1, 15, 0,
                                 None) == -2                                                  # mid beyond the kernel's limit
    assert lib.dsgcn_dynflag_fwd(one, None, None, None, None, one, one, one, None, None, one, 1, 8, 33, 40, 1, 15, 0,
                                 None) == -2
