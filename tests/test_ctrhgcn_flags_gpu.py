"""-m gpu: the position-typed 1x1 conv (csrc/typedconv.hip) and ``unit_ctrhgcn``'s ``target_specific`` / ``full_channels``
/ ``add_type`` switches on it — the kernel against fp64 at the smallest shapes that can go wrong, the unit against the
reference's fixtures (tests/golden/unit_ctrhgcn_flags.npz) and the fp64 restatement (tests/ctrhgcn_flags_fp64.py), the
reduced shipped model with the switches on (model_reduced_ctrgcn_flags), the engines, and the switches off.

Bars: the ones tests/test_dghgcn_gpu.py applies to a unit on the fp32 MFMA path — relative L2 against fp64 of 1e-5
(output), 5e-5 (input gradient), 1e-4 (parameter gradients)."""
import copy
import functools
import json
import os
import types

import numpy as np
import pytest
import torch

import dsgcn_amd as D
import ctrhgcn_flags_fp64 as F
import torch_ops
from dsgcn_amd import kernels as K
from layout_cases import shifted_operands, with_pad
from test_ctrhgcn_flags_host import CASES, Z, make_unit, restatement_kw, shipped_cfg, unit_inputs
from test_oracle_golden import GOLD, load, rel, sd_of

pytestmark = pytest.mark.gpu

BAR_Y, BAR_DX, BAR_P = 1e-5, 5e-5, 1e-4


# ---- 1. the kernel against fp64 --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _graph(layout):
    return D.Graph(layout=layout, mode='spatial')


def _table(kind, V, P):
    """node: the layout's joint types (V entries); edge: its joint-pair classes (V*V); 'sparse': P = 16 with types 2, 7 and
    11 absent and the others in no order."""
    if kind == 'sparse':
        live = [t for t in range(P) if t not in (2, 7, 11)]
        return torch.tensor([live[(5 * v + 3) % len(live)] for v in range(V)], dtype=torch.int32)
    g = _graph('coco' if V == 17 else 'nturgb+d')
    t = np.asarray(g.node_type) if kind == 'node' else np.asarray(g.edge_type).reshape(-1)
    return torch.as_tensor(t.astype(np.int32))


# (kind, n, Ci, Co, T, V, P)
KERNEL_CASES = [
    ('node', 2, 3, 192, 5, 25, 5),         # 125 positions: ragged tile, K depth 3
    ('node', 3, 64, 192, 7, 17, 5),        # coco
    ('node', 2, 256, 768, 4, 25, 5),       # full width
    ('sparse', 2, 20, 72, 3, 25, 16),      # ragged channels, empty types give exact zeros
    ('edge', 2, 8, 64, 25, 25, 15),
    ('edge', 3, 32, 256, 17, 17, 15),
]


def run_typed(kind, n, Ci, Co, T, V, P):
    """-> (y, dx, dW, db) of kernels.typed_conv and of the fp64 restatement on the same operands, and the table"""
    g = torch.Generator().manual_seed(Ci * 7 + Co + T)
    table = _table(kind, V, P)
    x = torch.randn(n, Ci, T, V, generator=g)
    W = torch.randn(P, Co, Ci, generator=g) * Ci ** -.5
    b = torch.randn(P, Co, generator=g) * .1
    dy = torch.randn(n, Co, T, V, generator=g)
    out = []
    for dt in (torch.float32, torch.float64):
        xs, Ws, bs = [t.to(dt).cuda().requires_grad_() for t in (x, W, b)]
        if dt == torch.float32:
            y = K.typed_conv(xs, Ws, bs, table.cuda(), P)
        else:
            y = F.typed_conv(xs, Ws, bs, table, P)
        y.backward(dy.to(dt).cuda())
        assert Ws.grad is not None and bs.grad is not None and tuple(Ws.grad.shape) == (P, Co, Ci)
        out.append((y.detach(), xs.grad, Ws.grad, bs.grad))
    return out[0], out[1], table


def check_typed(kind, n, Ci, Co, T, V, P):
    got, want, table = run_typed(kind, n, Ci, Co, T, V, P)
    errs = [rel(a.cpu(), w.cpu()) for a, w in zip(got, want)]
    print(f'typed_conv {kind} n={n} {Ci}->{Co} T={T} V={V} P={P}: y {errs[0]:.2e} dx {errs[1]:.2e} dW {errs[2]:.2e} db {errs[3]:.2e}')
    assert errs[0] < BAR_Y and errs[1] < BAR_DX and errs[2] < BAR_P and errs[3] < BAR_P, errs
    absent = sorted(set(range(P)) - set(table.tolist()))
    for p in absent:                               # a type no position carries: exact zeros, as tensors
        assert not got[2][p].any() and not got[3][p].any(), p
    return got, absent


@pytest.mark.parametrize('case', KERNEL_CASES, ids=repr)
def test_typed_conv_vs_fp64(case):
    _, absent = check_typed(*case)
    assert (len(absent) >= 2) == (case[0] == 'sparse')


@pytest.mark.parametrize('case', [KERNEL_CASES[0], KERNEL_CASES[3], KERNEL_CASES[4]], ids=repr)
def test_typed_conv_two_runs_are_bit_identical(case):
    a, _, _ = run_typed(*case)
    b, _, _ = run_typed(*case)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize('k', [1, 2, 3])
@pytest.mark.parametrize('case', [KERNEL_CASES[0], KERNEL_CASES[3], KERNEL_CASES[4]], ids=repr)
def test_typed_conv_operands_at_4_8_12_mod_16(case, k, monkeypatch):
    """x, W, b and the incoming gradient handed to the kernels as copies at address 4k mod 16 (the pattern of
    tests/test_alignment_gpu.py): the same bars."""
    moved = shifted_operands(monkeypatch, k)
    check_typed(*case)
    assert moved.count >= 4, 'vacuous: no operand went through _f32c'


@pytest.mark.parametrize('shape', [(2, 3, 192, 5, 25), (2, 64, 96, 8, 17)], ids=repr)
def test_one_type_is_the_plain_conv(shape):
    """P = 1 against ops.pwconv on the same operands.  Two fp32-accumulating kernels with different summation orders: each
    lies within its bar of fp64, so they agree within the sum of the bars (no bit equality)."""
    n, Ci, Co, T, V = shape
    g = torch.Generator().manual_seed(3)
    x, W, b, dy = (torch.randn(n, Ci, T, V, generator=g), torch.randn(1, Co, Ci, generator=g) * Ci ** -.5,
                   torch.randn(1, Co, generator=g) * .1, torch.randn(n, Co, T, V, generator=g))
    res = []
    for typed in (True, False):
        xs, Ws, bs = [t.clone().cuda().requires_grad_() for t in (x, W, b)]
        if typed:
            y = K.typed_conv(xs, Ws, bs, torch.zeros(V, dtype=torch.int32).cuda(), 1)
        else:
            y = K.pwconv(xs, None, None, None, False, Ws[0], bs[0], 1, False)[0]
        y.backward(dy.cuda())
        res.append((y.detach(), xs.grad, Ws.grad, bs.grad))
    errs = [rel(a.cpu(), w.cpu()) for a, w in zip(*res)]
    assert errs[0] < 2 * BAR_Y and errs[1] < 2 * BAR_DX and errs[2] < 2 * BAR_P and errs[3] < 2 * BAR_P, errs


# ---- 2. the unit against the reference's fixtures and the restatement -----------------------------------------------------
@pytest.mark.parametrize('tag', CASES)
def test_unit_vs_reference_fixture_and_restatement(tag):
    m, _ = make_unit(tag)
    p64 = {k: v.detach().double().cuda().requires_grad_() for k, v in m.named_parameters()}
    m = m.cuda().train()
    x32, r32 = unit_inputs(tag)
    x = x32.cuda().requires_grad_()
    y = m(x)
    (y * r32.cuda()).sum().backward()
    x64 = x32.double().cuda().requires_grad_()
    y64 = F.unit_forward(p64, x64, Z[tag + '_node_type'], Z[tag + '_edge_type'], **restatement_kw(tag))
    (y64 * r32.double().cuda()).sum().backward()
    for got, want, key, bar in ((y, y64, '_y', BAR_Y), (x.grad, x64.grad, '_dx', BAR_DX)):
        e_fix = F.fixture_rel(Z, tag + key, got.detach().cpu().numpy())
        e_ful = rel(got.detach().cpu(), want.detach().cpu())
        print(f'{tag}{key}: fixture {e_fix:.2e} restatement {e_ful:.2e}')
        assert e_fix < bar and e_ful < bar, (key, e_fix, e_ful)
    for k, p in m.named_parameters():
        key = tag + '_grad_' + k
        if k == 'down.0.bias':                           # under a train-mode BatchNorm: exactly zero
            continue
        if F.fixture_is_zero(Z, key):                    # subset 0's conv4 under full_channels without add_type
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
        else:
            e_fix = F.fixture_rel(Z, key, p.grad.cpu().numpy())
            e_ful = rel(p.grad.cpu(), p64[k].grad.cpu())
            e_ref = F.fixture_rel(Z, key, Z[tag + '_g32_' + k]) if tag + '_g32_' + k in Z else float('nan')
            print(f'{tag} {k}: fixture {e_fix:.2e} restatement {e_ful:.2e} (reference fp32 {e_ref:.2e})')
            assert e_fix < BAR_P and e_ful < BAR_P, (k, e_fix, e_ful)


# ---- 3. the reduced shipped model with the three switches on ---------------------------------------------------------------
NAME = 'model_reduced_ctrgcn_flags'


def _reduced():
    z = load(NAME + '.npz')
    with open(os.path.join(GOLD, NAME + '_cfg.json')) as f:
        cfg = json.load(f)
    m = D.build_model(copy.deepcopy(cfg))
    m.load_state_dict(sd_of(z, 'sd_', torch.float32), strict=True)
    return z, cfg, m


def test_reduced_model_vs_golden():
    """The rule of test_dghgcn_reduced_model_vs_golden."""
    z, _, m = _reduced()
    units = [b.gcn1 for b in m.backbone.net]
    assert [u.target_specific for u in units] == [True, True, False, True]
    assert [hasattr(u, 'edge_plan') for u in units] == [True, True, False, True]
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
    print(f'{NAME}: whole-gradient error {err:.3e}, the reference in fp32 {ref_err:.3e}')
    assert err < 2e-4, err                                    # whole-gradient relative L2 vs fp64 truth
    assert err <= 2 * ref_err, (err, ref_err)                 # ... and within 2x the reference's own fp32 error


def test_eval_logits_and_fuse_conv_bn():
    z, _, m = _reduced()
    m = m.cuda().eval()
    x = torch.from_numpy(z['x']).cuda()
    with torch.no_grad():
        logits = m.cls_head(m.extract_feat(x[:, 0]))
        assert rel(logits.cpu(), z['logits_eval_f64']) < 1e-4, rel(logits.cpu(), z['logits_eval_f64'])
        D.fuse_conv_bn(m)
        fused = m.cls_head(m.extract_feat(x[:, 0]))
    assert rel(fused.cpu(), logits.cpu()) <= 1e-5, rel(fused.cpu(), logits.cpu())


# ---- 4. the engines ----------------------------------------------------------------------------------------------------
def _train_run(use_graph, k=0, lr=0.05, steps=4):
    z, _, m = _reduced()
    m = with_pad(m, k).cuda().train()
    eng = D.TrainEngine(m, lr=lr, use_graph=use_graph, warmup_eager=1)
    x, y = torch.from_numpy(z['x']).cuda(), torch.from_numpy(z['label']).cuda()
    for _ in range(steps):
        logs = eng.step(x, y)
    torch.cuda.synchronize()
    assert torch.isfinite(logs['loss']).item()
    assert bool(eng.graphed(x, y)) == bool(use_graph), eng.capture_error
    return eng.flat.flat_p.detach().clone()[k:], eng.flat.flat_g.detach().clone()[k:]


def test_train_engine_captured_equals_eager_bit_for_bit():
    p_eager, g_eager = _train_run(False)
    p_graph, g_graph = _train_run(True)
    assert torch.equal(p_eager, p_graph) and torch.equal(g_eager, g_graph)
    z, _, m = _reduced()
    p0 = torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    assert not torch.equal(p_eager.cpu(), p0)                 # the steps moved the parameters


@pytest.mark.parametrize('k', [1, 2, 3])
def test_parameters_shifted_through_flatparams_give_the_same_gradient_bits(k):
    """The pattern of tests/test_layout_gpu.py: the flat parameter buffer starts k floats late, rate 0."""
    _, g0 = _base_gradient()
    _, gk = _train_run(True, k=k, lr=0.0, steps=3)
    assert torch.equal(g0, gk.cpu())


@functools.lru_cache(maxsize=None)
def _base_gradient():
    p, g = _train_run(True, k=0, lr=0.0, steps=3)
    return p.cpu(), g.cpu()


def test_infer_engine_equals_forward_test():
    """The replayed InferEngine against forward_test on the same clips.  The engine's fused head sums the 32 channels in
    another order than the framework's Linear: a few fp32 ulps on probabilities of order 1/12 (1e-5 relative L2)."""
    z, _, m = _reduced()
    m = m.cuda().eval()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, 2, 2, 16, 25, 3, generator=g).cuda()
    want = torch.as_tensor(m.forward_test(x))
    eng = D.InferEngine(m)
    for _ in range(eng.warmup_eager + 2):
        got = eng(x)
    assert eng.capture_error is None and eng.graphed(x)
    assert tuple(got.shape) == tuple(want.shape) == (3, 12)
    assert rel(got.cpu(), want) < 1e-5, rel(got.cpu(), want)
    eager = D.InferEngine(m, use_graph=False)(x)
    assert torch.equal(got, eager)


# ---- 5. the switches off: the path of the shipped flags is the one it was ---------------------------------------------------
def test_shipped_flags_take_the_existing_path_and_give_the_same_bits():
    """A unit_ctrhgcn with the shipped flags: ``ctr_topology`` is called as before (no edge_mode), ``typed_conv`` never, the
    three switches given as False change no bit, and the output equals the plain-torch statement (tests/torch_ops.py, which
    knows nothing of the switches) the way the existing unit tests compare it."""
    g = D.Graph(layout='nturgb+d', mode='random', num_filter=3, init_off=.04, init_std=.02)
    A = torch.tensor(np.asarray(g.A), dtype=torch.float32)
    kw = dict(semantic_index=True, node_attention=True, edge_attention=True, ada=True)
    outs = []
    for extra in ({}, dict(target_specific=False, full_channels=False, add_type=False)):
        torch.manual_seed(5)
        m = D.unit_ctrhgcn(64, 128, A, torch.tensor(g.edge_type), torch.tensor(g.node_type), **kw, **extra)
        with torch.no_grad():
            m.alpha.copy_(torch.tensor([.3, -.2, .4]))
            for c in m.convs:
                c.beta.fill_(.25)
        assert not hasattr(m, 'node_plan') and not hasattr(m, 'edge_plan')
        m = m.cuda().train()
        calls = []
        spy = types.SimpleNamespace(**{k: v for k, v in vars(K).items() if not k.startswith('__')})

        def ctr_topology(*a, **k):
            calls.append(sorted(k))
            return K.ctr_topology(*a, **k)

        def typed_conv(*a, **k):
            raise AssertionError('typed_conv on the shipped flags')

        spy.ctr_topology, spy.typed_conv = ctr_topology, typed_conv
        x = torch.randn(2, 64, 8, 25, generator=torch.Generator().manual_seed(1)).cuda().requires_grad_()
        with K.use_ops(spy):
            y = m(x)
        y.square().sum().backward()
        assert calls == [[]]
        outs.append((y.detach(), x.grad, m.convs[0].edge_att_conv.weight.grad, m))
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert torch.equal(a, b)
    m = outs[0][3]
    x = torch.randn(2, 64, 8, 25, generator=torch.Generator().manual_seed(1)).cuda()
    with K.use_ops(torch_ops):
        want = m(x)
    assert rel(outs[0][0].cpu(), want.detach().cpu()) < BAR_Y


def test_shipped_config_with_add_type_flipped_runs():
    """The `gcn_add_type = False` line of the shipped model file flipped: one training forward / backward at full width."""
    torch.manual_seed(0)
    np.random.seed(0)
    m = D.build_model(shipped_cfg(gcn_add_type=True)).cuda().train()
    with torch.no_grad():
        for b in m.backbone.net:
            b.gcn1.alpha.fill_(0.3)                      # (the constructor's zero switches the refinement off)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 2, 16, 25, 3, generator=g).cuda()
    y = torch.randint(0, 60, (2,), generator=g).cuda()
    logits = m.cls_head(m.extract_feat(x))
    m.cls_head.loss(logits, y)['loss_cls'].backward()
    assert torch.isfinite(logits).all()
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
    assert m.backbone.net[3].gcn1.convs[0].conv4.weight.grad.abs().max() > 0
