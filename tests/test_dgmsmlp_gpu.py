"""-m gpu: the mlp-window kernel (csrc/mlpwin.hip) inside ``kernels.temporal_dgmlp`` and the units on it — the op against the
fp64 restatement (tests/dgmsmlp_fp64.py) at the smallest shapes that can go wrong, with the kernel and with the staged
launches (DSGCN_MLPWIN=0), ``dgmsmlp`` against the reference's fixtures (tests/golden/unit_dgmsmlp.npz), the two reduced
DGSTGCN models (tcn_type 'mstcn' and 'dgmsmlp'), and the engines.

Bars: the op — 2e-5 relative L2 against fp64 on every output and gradient, the bar of check_temporal_unitmlp_bn
(tests/test_kernels_gpu.py); units — 1e-5 (output), 5e-5 (input gradient), 1e-4 (parameter gradients); reduced models —
1e-4 (logits, loss), 2e-4 whole-gradient relative L2 and at most twice the reference's own fp32 error."""
import copy
import functools
import json
import os

import numpy as np
import pytest
import torch

import dsgcn_amd as D
import dgmsmlp_fp64 as F
from dsgcn_amd import kernels as K
from layout_cases import shifted_operands
from test_dgmsmlp_host import CASES, Z, bias_under_bn, make_unit, restatement_kw, state_of, unit_inputs
from test_oracle_golden import GOLD, load, rel, sd_of

pytestmark = pytest.mark.gpu

BAR_OP = 2e-5
BAR_Y, BAR_DX, BAR_P = 1e-5, 5e-5, 1e-4


@pytest.fixture(autouse=True)
def kernel_path(monkeypatch):
    """Every test here runs csrc/mlpwin.hip wherever its range allows (DSGCN_MLPWIN=1), unless it sets another mode: the
    default mode 'auto' keeps the kernel for calls without a backward."""
    monkeypatch.setattr(K, 'MLPWIN', True)


# ---- 1. the op against fp64 ------------------------------------------------------------------------------------------------
# the eight fixture shapes (n = 2) + one frame, three samples
STAGE_CASES = {c[0]: dict(n=2, C=c[1], stride=c[2], T=c[3], V=c[4], kw=dict(c[5])) for c in F.CASES}
STAGE_CASES['t1'] = dict(n=3, C=64, stride=1, T=1, V=25, kw={})
WIDE65 = dict(n=2, C=130, stride=2, T=7, V=25, kw=dict(ms_cfg=[(3, 2), '1x1'], add_tcn=True))       # window width 65
FULL = dict(n=128, C=64, stride=1, T=64, V=25, kw=dict(add_tcn=True, merge_after=True))             # the bench batch


def _widths(C, cfg):
    mid = C // len(cfg)
    return [C - mid * (len(cfg) - 1)] + [mid] * (len(cfg) - 1)


def stage_operands(c):
    """Every operand of temporal_dgmlp for case c (fp32, on the host), the gradients fed back, and the static arguments."""
    cfg = [tuple(b) if isinstance(b, (list, tuple)) else b for b in c['kw'].get('ms_cfg', F.DEFAULT_CFG)]
    n, C, T, V, stride = c['n'], c['C'], c['T'], c['V'], c['stride']
    g = torch.Generator().manual_seed(C * 5 + T * 3 + V + stride)
    rnd = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale        # noqa: E731
    widths = _widths(C, cfg)
    n_act = sum(w for w, b in zip(widths, cfg) if b != '1x1')
    mlp = [b != '1x1' and b[0] != 'max' for b in cfg]
    KM = ({(b[0] + 1) // 2 for b, m in zip(cfg, mlp) if m} or {2}).pop()
    t = dict(z=rnd(n, C, T, V), zaug=rnd(n, C, T), scale=torch.cat([torch.rand(n_act, generator=g) + 0.5, torch.ones(C - n_act)]),
             shift=torch.cat([rnd(n_act, scale=0.3), torch.zeros(C - n_act)]), add_coeff=rnd(V, scale=0.5),
             gamma=torch.rand(C, generator=g) + 0.5, beta=rnd(C, scale=0.2))
    rows_w, rows_b, dil = [], [], []
    for i, (w, b, m) in enumerate(zip(widths, cfg, mlp)):
        rows_w.append(rnd(w, KM, scale=0.5) if m else torch.zeros(w, KM))
        rows_b.append(rnd(w, scale=0.1) if m else torch.zeros(w))
        dil += [int(b[1]) if m else 0] * w
        if m:
            t[f'w1_{i}'], t[f'b1_{i}'] = rnd(w, w, scale=w ** -0.5), rnd(w, scale=0.1)
            if c['kw'].get('add_tcn'):
                t[f'cw_{i}'], t[f'cb_{i}'] = rnd(w, w, b[0], 1, scale=(b[0] * w) ** -0.5), rnd(w, scale=0.1)
    t['dw_w'], t['dw_b'] = torch.cat(rows_w), torch.cat(rows_b)
    Tout = (T + stride - 1) // stride
    fed = dict(f=rnd(n, C, Tout, V), sc=rnd(C), sh=rnd(C))
    static = dict(cfg=cfg, widths=widths, n_act=n_act, mlp=mlp, dil=torch.tensor(dil, dtype=torch.int32), KM=KM,
                  merge_after=bool(c['kw'].get('merge_after')), stride=stride)
    return t, fed, static


def run_stage(mod, c, dt, dev):
    """-> outputs and every gradient of mod.temporal_dgmlp on case c, by name"""
    t, fed, s = stage_operands(c)
    p = {k: v.to(dev, dt).requires_grad_() for k, v in t.items()}
    idx = [i for i, m in enumerate(s['mlp']) if m]
    pick = lambda name: [p[f'{name}_{i}'] for i in idx] if f'{name}_{idx[0]}' in p else None        # noqa: E731
    f, sc, sh, mean, var = mod.temporal_dgmlp(p['z'], p['zaug'], p['scale'], p['shift'], s['n_act'], s['cfg'], s['widths'],
                                              pick('cw'), pick('cb'), p['dw_w'], p['dw_b'], s['dil'].to(dev), pick('w1'),
                                              pick('b1'), p['add_coeff'], s['merge_after'], s['stride'], p['gamma'],
                                              p['beta'], 1e-5, True)
    ((f * fed['f'].to(dev, dt)).sum() + (sc * fed['sc'].to(dev, dt)).sum() + (sh * fed['sh'].to(dev, dt)).sum()).backward()
    res = dict(f=f, sc=sc, sh=sh, mean=mean, var=var)
    for k, v in p.items():
        assert v.grad is not None, k
        res['d_' + k] = v.grad
    return {k: v.detach() for k, v in res.items()}


_truth = {}


def truth(name, c):
    """the fp64 restatement of case c: once, shared by the tests that need it (on the GPU for the full-size case)"""
    if name not in _truth:
        _truth[name] = run_stage(F, c, torch.float64, 'cuda' if c['n'] >= 64 else 'cpu')
    return _truth[name]


def supported(c):
    _, _, s = stage_operands(c)
    tabs = K._mlpwin_tables(s['cfg'], s['widths'], bool(c['kw'].get('add_tcn')), s['merge_after'])
    return K.mlpwin_supported(c['n'], c['C'], c['T'], c['V'] + 1, c['stride'], s['KM'], tabs)


def check_stage(name, c, kernel, monkeypatch):
    """kernel: csrc/mlpwin.hip must take the case (asserted through dsgcn_mlpwin_supported and a count of its launches);
    otherwise the staged launches."""
    monkeypatch.setattr(K, 'MLPWIN', bool(kernel))
    launches = []
    apply = K._MlpWin.apply
    monkeypatch.setattr(K._MlpWin, 'apply', lambda *a: launches.append(1) or apply(*a))
    if kernel:
        assert supported(c), 'the case is outside dsgcn_mlpwin_supported'
    got = run_stage(K, c, torch.float32, 'cuda')
    assert len(launches) == (1 if kernel else 0)
    want = truth(name, c)
    errs = {k: rel(got[k].cpu(), v.cpu()) for k, v in want.items()}
    print(f"temporal_dgmlp {name} {'kernel' if kernel else 'staged'}: " + ' '.join(f'{k} {e:.1e}' for k, e in errs.items()))
    bad = {k: e for k, e in errs.items() if not e < BAR_OP}
    assert not bad, bad
    _, _, s = stage_operands(c)
    off = (s['dil'] == 0).nonzero().view(-1)                       # taps outside the mlp windows: exact zeros
    assert not got['d_dw_w'][off.cuda()].any() and not got['d_dw_b'][off.cuda()].any()
    return got


@pytest.mark.parametrize('kernel', [True, False], ids=['kernel', 'staged'])
@pytest.mark.parametrize('name', list(STAGE_CASES))
def test_temporal_dgmlp_vs_fp64(name, kernel, monkeypatch):
    check_stage(name, STAGE_CASES[name], kernel, monkeypatch)


@pytest.mark.parametrize('name', ['d128s2', 'tcn_before_s2', 'coco'])
def test_two_runs_are_bit_identical(name, monkeypatch):
    a = check_stage(name, STAGE_CASES[name], True, monkeypatch)
    b = run_stage(K, STAGE_CASES[name], torch.float32, 'cuda')
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('k', [1, 2, 3])
@pytest.mark.parametrize('name', ['d64', 'tcn_before_s2', 'coco'])
def test_operands_at_4_8_12_mod_16(name, k, monkeypatch):
    """Every operand handed to the kernels as a copy at address 4k mod 16 (the pattern of tests/test_alignment_gpu.py)."""
    moved = shifted_operands(monkeypatch, k)
    check_stage(name, STAGE_CASES[name], True, monkeypatch)
    assert moved.count >= 8, 'vacuous: no operand went through _f32c'


def test_window_of_65_channels_takes_the_staged_form(monkeypatch):
    assert not supported(WIDE65)
    launches = []
    apply = K._MlpWin.apply
    monkeypatch.setattr(K._MlpWin, 'apply', lambda *a: launches.append(1) or apply(*a))
    got = run_stage(K, WIDE65, torch.float32, 'cuda')
    assert not launches
    want = truth('wide65', WIDE65)
    bad = {k: rel(got[k].cpu(), v) for k, v in want.items() if not rel(got[k].cpu(), v) < BAR_OP}
    assert not bad, bad


def test_full_width_at_the_bench_batch(monkeypatch):
    """n = 128 person-samples, C = 64, T = 64, V = 25: the grid and the indexing at real size (fp64 truth on the GPU)."""
    check_stage('full', FULL, True, monkeypatch)


def test_default_mode_takes_the_kernel_only_without_a_backward(monkeypatch):
    """DSGCN_MLPWIN unset ('auto'): a call that records a backward takes the staged launches, a call under no_grad the
    kernel; the two agree within the sum of their bars."""
    monkeypatch.setattr(K, 'MLPWIN', 'auto')
    launches = []
    apply = K._MlpWin.apply
    monkeypatch.setattr(K._MlpWin, 'apply', lambda *a: launches.append(1) or apply(*a))
    m, _ = make_unit('tcn_after')
    m = m.cuda().train()
    x = unit_inputs('tcn_after')[0].cuda()
    y = m(x.clone().requires_grad_())
    assert not launches
    with torch.no_grad():
        y0 = m(x)
    assert len(launches) == 1
    assert rel(y0.cpu(), y.detach().cpu()) < 2 * BAR_Y


# ---- 2. the unit against the reference's fixtures and the restatement -----------------------------------------------------
@pytest.mark.parametrize('tag', CASES)
def test_unit_vs_reference_fixture_and_restatement(tag, monkeypatch):
    launches = []
    apply = K._MlpWin.apply
    monkeypatch.setattr(K._MlpWin, 'apply', lambda *a: launches.append(1) or apply(*a))
    m, c = make_unit(tag)
    p64 = state_of(m, torch.float64, 'cuda')
    m = m.cuda().train()
    x32, r32 = unit_inputs(tag)
    x = x32.cuda().requires_grad_()
    y = m(x)
    (y * r32.cuda()).sum().backward()
    assert len(launches) == 1                                  # the kernel path
    x64 = x32.double().cuda().requires_grad_()
    y64 = F.unit_forward(p64, x64, **restatement_kw(c))
    (y64 * r32.double().cuda()).sum().backward()
    for got, want, key, bar in ((y, y64, '_y', BAR_Y), (x.grad, x64.grad, '_dx', BAR_DX)):
        e_fix = F.fixture_rel(Z, tag + key, got.detach().cpu().numpy())
        e_ful = rel(got.detach().cpu(), want.detach().cpu())
        print(f'{tag}{key}: fixture {e_fix:.2e} restatement {e_ful:.2e}')
        assert e_fix < bar and e_ful < bar, (key, e_fix, e_ful)
    for k, p in m.named_parameters():
        if bias_under_bn(k):                                   # under a train-mode BatchNorm: zero up to rounding
            continue
        key = tag + '_grad_' + k
        e_fix = F.fixture_rel(Z, key, p.grad.cpu().numpy())
        e_ful = rel(p.grad.cpu(), p64[k].grad.cpu())
        e_ref = F.fixture_rel(Z, key, Z[tag + '_g32_' + k]) if tag + '_g32_' + k in Z else float('nan')
        print(f'{tag} {k}: fixture {e_fix:.2e} restatement {e_ful:.2e} (reference fp32 {e_ref:.2e})')
        assert e_fix < BAR_P and e_ful < BAR_P, (k, e_fix, e_ful)


# ---- 3. the reduced DGSTGCN models -----------------------------------------------------------------------------------------
MODELS = ['model_reduced_dg_mstcn', 'model_reduced_dg_msmlp']


def _reduced(name):
    z = load(name + '.npz')
    with open(os.path.join(GOLD, name + '_cfg.json')) as f:
        cfg = json.load(f)
    m = D.build_model(copy.deepcopy(cfg))
    m.load_state_dict(sd_of(z, 'sd_', torch.float32), strict=True)
    return z, cfg, m


@pytest.mark.parametrize('mode', [True, 'auto'], ids=['kernel', 'auto'])
@pytest.mark.parametrize('name', MODELS)
def test_reduced_model_vs_golden(name, mode, monkeypatch):
    """The rule of test_dghgcn_reduced_model_vs_golden; with the kernel in both directions, and in the default mode (the
    staged launches where a backward is recorded)."""
    monkeypatch.setattr(K, 'MLPWIN', mode)
    z, _, m = _reduced(name)
    assert {type(b.tcn).__name__ for b in m.backbone.gcn} == {'mstcn' if name.endswith('mstcn') else 'dgmsmlp'}
    m = m.cuda().train()
    x, y = torch.from_numpy(z['x']).cuda(), torch.from_numpy(z['label']).cuda()
    logits = m.cls_head(m.extract_feat(x[:, 0]))
    loss = m.cls_head.loss(logits, y.squeeze(-1))['loss_cls']
    loss.backward()
    e_logits = rel(logits.detach().cpu(), z['logits_f64'])
    e_loss = abs(loss.item() - float(z['loss_f64'])) / abs(float(z['loss_f64']))
    num = den = num32 = 0.0
    for k, p in m.named_parameters():
        if 'g64_' + k in z:
            g64 = z['g64_' + k].astype(np.float64)
            num += float(((p.grad.double().cpu().numpy() - g64) ** 2).sum())
            num32 += float(((z['g32_' + k].astype(np.float64) - g64) ** 2).sum())
            den += float((g64 ** 2).sum())
    err, ref_err = (num / den) ** .5, (num32 / den) ** .5
    print(f'{name}: logits {e_logits:.2e} loss {e_loss:.2e} whole-gradient error {err:.3e}, the reference in fp32 {ref_err:.3e}')
    assert e_logits < 1e-4 and e_loss < 1e-4, (e_logits, e_loss)
    assert err < 2e-4, err                                    # whole-gradient relative L2 vs fp64 truth
    assert err <= 2 * ref_err, (err, ref_err)                 # ... and within 2x the reference's own fp32 error


@pytest.mark.parametrize('name', MODELS)
def test_eval_logits_and_fuse_conv_bn(name):
    z, _, m = _reduced(name)
    m = m.cuda().eval()
    x = torch.from_numpy(z['x']).cuda()
    with torch.no_grad():
        logits = m.cls_head(m.extract_feat(x[:, 0]))
        assert rel(logits.cpu(), z['logits_eval_f64']) < 1e-4, rel(logits.cpu(), z['logits_eval_f64'])
        D.fuse_conv_bn(m)
        fused = m.cls_head(m.extract_feat(x[:, 0]))
    assert rel(fused.cpu(), logits.cpu()) <= 1e-5, rel(fused.cpu(), logits.cpu())


# ---- 4. the engines ----------------------------------------------------------------------------------------------------
def _train_run(name, use_graph, lr=0.05, steps=4):
    z, _, m = _reduced(name)
    m = m.cuda().train()
    eng = D.TrainEngine(m, lr=lr, use_graph=use_graph, warmup_eager=1)
    x, y = torch.from_numpy(z['x']).cuda(), torch.from_numpy(z['label']).cuda()
    for _ in range(steps):
        logs = eng.step(x, y)
    torch.cuda.synchronize()
    assert torch.isfinite(logs['loss']).item()
    assert bool(eng.graphed(x, y)) == bool(use_graph), eng.capture_error
    return eng.flat.flat_p.detach().clone(), eng.flat.flat_g.detach().clone()


@pytest.mark.parametrize('name', MODELS)
def test_train_engine_captured_equals_eager_bit_for_bit(name):
    p_eager, g_eager = _train_run(name, False)
    p_graph, g_graph = _train_run(name, True)
    assert torch.equal(p_eager, p_graph) and torch.equal(g_eager, g_graph)
    z, _, m = _reduced(name)
    p0 = torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    assert not torch.equal(p_eager.cpu(), p0)                 # the steps moved the parameters


@pytest.mark.parametrize('name', MODELS)
def test_infer_engine_equals_forward_test(name):
    """The replayed InferEngine against forward_test on the same clips (the bar of tests/test_ctrhgcn_flags_gpu.py: the
    engine's fused head sums the 32 channels in another order than the framework's Linear)."""
    z, _, m = _reduced(name)
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


def test_tcn_dropout_runs_through_fuse_out():
    """tcn_dropout with the new unit: the fused dropout of the block's fuse_out, as for dgmstcn."""
    z, cfg, _ = _reduced('model_reduced_dg_msmlp')
    cfg = copy.deepcopy(cfg)
    cfg['backbone']['tcn_dropout'] = 0.5
    m = D.build_model(cfg)
    m.load_state_dict(sd_of(z, 'sd_', torch.float32), strict=True)
    m = m.cuda().train()
    x = torch.from_numpy(z['x']).cuda()
    a = m.cls_head(m.extract_feat(x[:, 0]))
    m.eval()
    with torch.no_grad():
        b = m.cls_head(m.extract_feat(x[:, 0]))
    assert torch.isfinite(a).all() and not torch.allclose(a.detach(), b, atol=1e-3)
