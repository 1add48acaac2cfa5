"""-m gpu: ``dghgcn`` (DGSTGCN's default gcn_type) on the HIP path — the typed K-B (csrc/dynadj_typed.hip) with the K-C
projections and edge linear — against the reference's fixtures (tests/golden/unit_dghgcn.npz, model_reduced_dghgcn*),
against the fp64 restatement (tests/dghgcn_fp64.py) at full batch, and through a captured TrainEngine step."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import dsgcn_amd as D
import dghgcn_fp64 as F
from test_dghgcn_host import CASES, Z, make_unit, unit_inputs
from test_oracle_golden import GOLD, load, rel, sd_of
import test_kernels_gpu as KG

pytestmark = pytest.mark.gpu

ZERO_GRAD_BIASES = ('pre.0.bias', 'post.bias', 'down.0.bias')     # under a train-mode BatchNorm: exactly zero


@pytest.mark.parametrize('tag', CASES)
def test_dghgcn_unit_vs_reference_fixture(tag):
    """The unit on the HIP path against the reference's fp64 output, input gradient and every parameter gradient
    (tests/golden/unit_dghgcn.npz: whole arrays or their probes), and element by element against the fp64 restatement
    of the same weights (pinned to the reference by tests/test_dghgcn_host.py)."""
    m, kw = make_unit(tag)
    with torch.no_grad():
        m.alpha.copy_(torch.from_numpy(Z[tag + '_alpha']))
        m.beta.copy_(torch.from_numpy(Z[tag + '_beta']))
    p64 = {k: v.detach().double().cuda().requires_grad_() for k, v in m.named_parameters()}
    m = m.cuda().train()
    x32, r32 = unit_inputs(tag)
    x = x32.cuda().requires_grad_()
    y = m(x)
    (y * r32.cuda()).sum().backward()
    x64 = x32.double().cuda().requires_grad_()
    y64 = F.unit_forward(p64, x64, Z[tag + '_node_type'], Z[tag + '_edge_type'], **kw)
    (y64 * r32.double().cuda()).sum().backward()
    for got, want, key, bar in ((y, y64, '_y', 1e-5), (x.grad, x64.grad, '_dx', 5e-5)):
        e_fix = F.fixture_rel(Z, tag + key, got.detach().cpu().numpy())
        e_ful = rel(got.detach().cpu(), want.detach().cpu())
        assert e_fix < bar and e_ful < bar, (key, e_fix, e_ful)
    for k, p in m.named_parameters():
        key = tag + '_grad_' + k
        if k in ZERO_GRAD_BIASES:
            continue
        if F.fixture_is_zero(Z, key):              # alpha[1:], beta[1:] are unused without subset_wise
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
        else:
            e_fix = F.fixture_rel(Z, key, p.grad.cpu().numpy())
            e_ful = rel(p.grad.cpu(), p64[k].grad.cpu())
            assert e_fix < 1e-4 and e_ful < 1e-4, (k, e_fix, e_ful)


def _reduced(name):
    z = load(name + '.npz')
    with open(os.path.join(GOLD, name + '_cfg.json')) as f:
        cfg = json.load(f)
    if 'tcn_ms_cfg' in cfg['backbone']:
        cfg['backbone']['tcn_ms_cfg'] = [tuple(c) if isinstance(c, list) else c for c in cfg['backbone']['tcn_ms_cfg']]
    m = D.build_model(copy.deepcopy(cfg))
    m.load_state_dict(sd_of(z, 'sd_', torch.float32))
    return z, cfg, m


@pytest.mark.parametrize('name', ['model_reduced_dghgcn', 'model_reduced_dghgcn_default'])
def test_dghgcn_reduced_model_vs_golden(name):
    z, _, m = _reduced(name)
    assert all(type(b.gcn).__name__ == 'dghgcn' for b in m.backbone.gcn)
    m = m.cuda().train()
    x, y = torch.from_numpy(z['x']).cuda(), torch.from_numpy(z['label']).cuda()
    logits = m.cls_head(m.extract_feat(x[:, 0]))
    loss = m.cls_head.loss(logits, y.squeeze(-1))['loss_cls']
    loss.backward()
    assert rel(logits.detach().cpu(), z['logits_f64']) < 1e-4
    assert abs(loss.item() - float(z['loss_f64'])) / abs(float(z['loss_f64'])) < 1e-4
    num = den = num32 = 0.0
    for k, p in m.named_parameters():
        if 'g64_' + k in z:
            g64 = z['g64_' + k].astype(np.float64)
            num += float(((p.grad.double().cpu().numpy() - g64) ** 2).sum())
            num32 += float(((z['g32_' + k].astype(np.float64) - g64) ** 2).sum())
            den += float((g64 ** 2).sum())
    err, ref_err = (num / den) ** .5, (num32 / den) ** .5
    assert err < 2e-4, err                                    # whole-gradient relative L2 vs fp64 truth
    assert err <= 2 * ref_err, (err, ref_err)                 # ... and within 2x the reference's own fp32 error


@pytest.mark.parametrize('name', ['model_reduced_dghgcn', 'model_reduced_dghgcn_default'])
def test_dghgcn_eval_logits_and_fuse_conv_bn(name):
    z, _, m = _reduced(name)
    m = m.cuda().eval()
    x = torch.from_numpy(z['x']).cuda()
    with torch.no_grad():
        logits = m.cls_head(m.extract_feat(x[:, 0]))
        assert rel(logits.cpu(), z['logits_eval_f64']) < 1e-4, rel(logits.cpu(), z['logits_eval_f64'])
        D.fuse_conv_bn(m)
        fused = m.cls_head(m.extract_feat(x[:, 0]))
    assert rel(fused.cpu(), logits.cpu()) <= 1e-5, rel(fused.cpu(), logits.cpu())


# every (Ci, Co) of the 10-stage DS-STGCN at ratio 0.125 (the adjacency sees only xbar: T does not enter), and the
# 256-channel layer at 0.25 (mid = 64)
FULL = [(3, 64, 0.125), (64, 64, 0.125), (64, 128, 0.125), (128, 128, 0.125), (128, 256, 0.125), (256, 256, 0.125),
        (256, 256, 0.25)]


FULL_CASES = ([(c, 'node_edge') for c in FULL] + [(c, f) for c in ((64, 64, 0.125), (256, 256, 0.25))
                                                    for f in ('plain', 'node', 'edge', 'add_type')])


@pytest.mark.parametrize('case,flags', FULL_CASES)
def test_typed_kb_full_size_vs_fp64(case, flags):
    """n = 128, V = 25: Ahat, the input gradient (of the time mean) and every parameter gradient of the adjacency path
    (K-C projections + typed select + K-C edge linear + typed K-B) against the fp64 restatement."""
    KG.check_typed_kb(case, flags)


def _small_graph(V, P, E, seed):
    """A (3, V, V), node_type (V), edge_type (V*V) of a graph that is not NTU's."""
    gen = torch.Generator().manual_seed(seed)
    A = torch.randn(3, V, V, generator=gen) * 0.1
    return A, (torch.arange(V) % P).to(torch.int32), torch.randint(E, (V * V,), generator=gen).to(torch.int32)


# (n, Ci, mid, V, P, E): V = 17 is the second V-specialised instantiation; V = 32 fills the 1024-thread pair grid and the
# LDS maxima; V = 7 with mid = 11 is the generic one with a partial last round of the class bins (mid % 8 != 0)
SMALL = [(2, 8, 5, 17, 3, 4), (3, 16, 1, 32, 1, 16), (2, 8, 11, 7, 2, 3)]


@pytest.mark.parametrize('add_type', [False, True], ids=['node_edge', 'add_type'])
@pytest.mark.parametrize('shape', SMALL)
def test_typed_kb_small_shapes_vs_fp64(shape, add_type):
    """``kernels.dynadj_typed`` with hand-made weights at joint counts other than 25: Ahat (1e-5), the input gradient
    and every parameter gradient (1e-4) against the fp64 restatement, the bounds of the full-size test."""
    n, ci, mid, V, P, E = shape
    A, nt, et = _small_graph(V, P, E, 5)
    gen = torch.Generator().manual_seed(11)
    r = lambda *sh, scale=1.0: (torch.randn(*sh, generator=gen) * scale).cuda().requires_grad_()
    KM = 3 * mid
    p = dict(A=A.cuda().requires_grad_(), alpha=r(3, scale=.5), beta=r(3, scale=.5), w1=r(KM * P, ci, scale=ci ** -.5),
             b1=r(KM * P, scale=.1), w2=r(KM * P, ci, scale=ci ** -.5), b2=r(KM * P, scale=.1),
             we=r(E * KM, KM, scale=KM ** -.5), be=r(E * KM, scale=.1))
    xbar = r(n, ci, V)
    dah = torch.randn(n, KM, V, V, generator=gen).cuda()
    ahat = D.kernels.dynadj_typed(xbar, p['A'], p['alpha'], p['beta'], p['w1'], p['b1'], p['w2'], p['b2'], p['we'],
                                  p['be'], nt.cuda(), et.cuda(), P, add_type)
    (ahat * dah).sum().backward()
    p64 = {k: v.detach().double().requires_grad_() for k, v in p.items()}
    x64 = xbar.detach().double().requires_grad_()
    want = F.adjacency(x64, p64['A'], p64['alpha'], p64['beta'], p64['w1'], p64['b1'], p64['w2'], p64['b2'], p64['we'],
                       p64['be'], nt, et, P, add_type, True)
    (want * dah.double()).sum().backward()
    errs = dict(ahat=rel(ahat.detach().cpu(), want.detach().cpu()), xbar=rel(xbar.grad.cpu(), x64.grad.cpu()),
                **{k: rel(p[k].grad.cpu(), p64[k].grad.cpu()) for k in p})
    assert errs['ahat'] < 1e-5, errs['ahat']
    del errs['ahat']
    assert all(e < 1e-4 for e in errs.values()), errs


DGH_CFG = dict(
    type='RecognizerGCN',
    backbone=dict(
        type='DGSTGCN', gcn_type='dghgcn', gcn_ratio=0.125, gcn_node_attention=True, gcn_edge_attention=True,
        gcn_subset_wise=True, gcn_ctr='T', gcn_ada='T', tcn_type='dgmstcn',
        graph_cfg=dict(layout='nturgb+d', mode='random', num_filter=3, init_off=.04, init_std=.02),
        tcn_ms_cfg=[(3, 1), (3, 2), (3, 3), (3, 4), ('max', 3), '1x1']),
    cls_head=dict(type='GCNHead', num_classes=60, in_channels=256))


def test_dghgcn_train_engine_step_graphed_bit_identical():
    """A 64-clip TrainEngine step of the dghgcn DS-STGCN config, captured as a hipGraph: finite, and the gradients of two
    runs from the same weights are bit-identical (no float atomics on the new path)."""
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(64, 1, 2, 64, 25, 3, generator=gen).cuda()
    y = torch.randint(0, 60, (64, 1), generator=gen).cuda()
    torch.manual_seed(0)
    np.random.seed(0)
    sd = D.build_model(copy.deepcopy(DGH_CFG)).state_dict()
    runs = []
    for _ in range(2):
        m = D.build_model(copy.deepcopy(DGH_CFG))
        m.load_state_dict(sd)
        m = m.cuda().train()
        eng = D.TrainEngine(m, lr=0.05, use_graph=True, warmup_eager=2)
        for _ in range(3):
            logs = eng.step(x, y)
        torch.cuda.synchronize()
        assert eng.graphed(x, y), eng.capture_error
        assert torch.isfinite(logs['loss']).item()
        runs.append((eng.flat.flat_g.detach().clone(), eng.flat.flat_p.detach().clone()))
    assert torch.isfinite(runs[0][0]).all()
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])
