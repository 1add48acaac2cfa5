"""-m gpu: gradient clipping on the device (csrc/clip.hip: dsgcn_grad_norm_partials + dsgcn_sgd_step_clip) against numpy
fp64 and torch's clip_grad_norm_ + SGD, its determinism, and TrainEngine with grad_clip eagerly and as replayed
hipGraphs."""
import functools

import numpy as np
import pytest
import torch

import dsgcn_amd as D
from dsgcn_amd import native

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SLICE = 8192                                  # elements per partial row (include/dsgcn.h)
SIZES = [1, 3, 255, 4101, 1376950]            # below one vector, ragged tail, below one workgroup, several slices with a
#                                               ragged last one, the DS-STGCN flat size
COMBOS = [(0.9, 5e-4, True), (0.9, 0.0, False), (0.0, 1e-3, False)]


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _case(n):
    """(g, p) fp32 on the host and the fp64 reference norms of g — computed once per size, never modified."""
    gen = torch.Generator().manual_seed(1000 + n)
    g = torch.randn(n, generator=gen)
    p = torch.randn(n, generator=gen)
    g64 = g.numpy().astype(np.float64)
    rows = (n + SLICE - 1) // SLICE
    sq = np.array([np.sum(g64[r * SLICE:(r + 1) * SLICE] ** 2) for r in range(rows)])
    mx = np.array([np.max(np.abs(g64[r * SLICE:(r + 1) * SLICE])) for r in range(rows)])
    return g, p, {2: (sq, float(np.sqrt(np.sum(g64 ** 2)))), 0: (mx, float(np.max(np.abs(g64))))}


def _partials(g, norm_type):
    lib = native.lib()
    rows = lib.dsgcn_grad_norm_rows(g.numel())
    partial = torch.full((rows,), -1.0, dtype=torch.float64, device=DEV)
    assert lib.dsgcn_grad_norm_partials(g.data_ptr(), g.numel(), norm_type, partial.data_ptr(), _stream()) == 0
    return partial


def _step_clip(p, g, buf, lr_t, norm_type, max_norm, mom, wd, nesterov):
    """One clipped step in place; -> (partial, grad_norm)."""
    partial = _partials(g, norm_type)
    out = torch.full((1,), -1.0, device=DEV)
    rc = native.lib().dsgcn_sgd_step_clip(p.data_ptr(), g.data_ptr(), None if buf is None else buf.data_ptr(), lr_t.data_ptr(),
                                          partial.data_ptr(), partial.numel(), norm_type, max_norm, out.data_ptr(), mom, wd,
                                          int(nesterov), p.numel(), _stream())
    assert rc == 0
    return partial, out


def _step_plain(p, g, buf, lr_t, mom, wd, nesterov):
    rc = native.lib().dsgcn_sgd_step(p.data_ptr(), g.data_ptr(), None if buf is None else buf.data_ptr(), lr_t.data_ptr(), mom,
                                     wd, int(nesterov), p.numel(), _stream())
    assert rc == 0


@pytest.mark.parametrize('norm_type', [2, 0])
@pytest.mark.parametrize('n', SIZES)
def test_norm_and_clip_vs_fp64(n, norm_type):
    """partial rows, the stored total and the clipped gradient against numpy fp64.  L2: every square is exact in fp64 and a
    sum of <= 1.4 M such terms carries a relative error below 2e-10, so after the rounding of sqrt and of the conversion
    the stored fp32 norm lies within 2 ulp of the fp64 value; inf: exact."""
    g_h, p_h, ref = _case(n)
    rows_ref, total_ref = ref[norm_type]
    g, p = g_h.to(DEV), p_h.to(DEV)
    buf = torch.zeros_like(p)
    lr_t = torch.full((1,), 0.1, device=DEV)
    assert native.lib().dsgcn_grad_norm_rows(n) == len(rows_ref)
    max_norm = 0.5 * total_ref                                  # clipping is active
    partial, out = _step_clip(p, g, buf, lr_t, norm_type, max_norm, 0.9, 5e-4, True)
    partial, got = partial.cpu().numpy(), float(out)
    if norm_type == 0:
        assert np.array_equal(partial, rows_ref)
        assert got == float(np.float32(total_ref)) == total_ref
    else:
        print('partial rel err', np.max(np.abs(partial - rows_ref) / rows_ref))
        assert np.all(np.abs(partial - rows_ref) <= 2e-10 * rows_ref)
        ulp = float(np.spacing(np.float32(total_ref)))
        print('grad_norm', got, 'fp64', total_ref, 'ulps', abs(got - total_ref) / ulp)
        assert abs(got - total_ref) <= 2 * ulp
    coef = min(1.0, max_norm / (total_ref + 1e-6))
    want = g_h.numpy().astype(np.float64) * coef
    gerr = np.abs(g.cpu().numpy().astype(np.float64) - want)
    print('clipped g max rel err', float(np.max(gerr / np.maximum(np.abs(want), 1e-300))))
    assert np.all(gerr <= 1e-6 * np.abs(want))


@pytest.mark.parametrize('norm_type', [2, 0])
@pytest.mark.parametrize('mom,wd,nesterov', COMBOS)
def test_below_max_norm_is_the_plain_step_bit_for_bit(mom, wd, nesterov, norm_type):
    """total < max_norm: the coefficient is 1, the product g * 1 is exact — p, buf and g come out as dsgcn_sgd_step
    leaves them, over three steps with a changing rate (n = 4101: full vectors, a guarded block and a one-element tail)."""
    n = 4101
    g_h, p_h, ref = _case(n)
    max_norm = 2.0 * ref[norm_type][1]
    pa, pb = p_h.to(DEV), p_h.to(DEV)
    ba = torch.zeros_like(pa) if mom else None
    bb = torch.zeros_like(pb) if mom else None
    lr_t = torch.zeros(1, device=DEV)
    for it in range(3):
        lr_t.fill_(0.1 / (it + 1))
        ga = (g_h * (1.0 - 0.25 * it)).to(DEV)
        gb = ga.clone()
        _, out = _step_clip(pa, ga, ba, lr_t, norm_type, max_norm, mom, wd, nesterov)
        _step_plain(pb, gb, bb, lr_t, mom, wd, nesterov)
        assert float(out) < max_norm
        assert torch.equal(pa, pb) and torch.equal(ga, gb)
        if mom:
            assert torch.equal(ba, bb)


@pytest.mark.parametrize('norm_type', [2, 0])
@pytest.mark.parametrize('mom,wd,nesterov', COMBOS)
def test_above_max_norm_matches_torch_clip_and_sgd(mom, wd, nesterov, norm_type):
    """total > max_norm: torch.nn.utils.clip_grad_norm_ + torch.optim.SGD, three steps with a changing rate — the protocol
    and the 1e-6 absolute bound of test_sgd_step_matches_torch; the gradient written back within 1e-6 relative of g * coef."""
    n = 4101
    g_h, p_h, ref = _case(n)
    total = ref[norm_type][1]
    max_norm = 0.25 * total
    tnorm = 2.0 if norm_type == 2 else float('inf')
    refp = torch.nn.Parameter(p_h.clone().to(DEV))
    topt = torch.optim.SGD([refp], lr=0.1, momentum=mom, weight_decay=wd, nesterov=nesterov)
    p = p_h.clone().to(DEV)
    buf = torch.zeros_like(p) if mom else None
    lr_t = torch.zeros(1, device=DEV)
    for it in range(3):
        lr = 0.1 / (it + 1)
        scale = 1.0 - 0.25 * it
        topt.param_groups[0]['lr'] = lr
        refp.grad = (g_h * scale).to(DEV)
        tt = torch.nn.utils.clip_grad_norm_([refp], max_norm, norm_type=tnorm)
        topt.step()
        lr_t.fill_(lr)
        g = (g_h * scale).to(DEV)
        _, out = _step_clip(p, g, buf, lr_t, norm_type, max_norm, mom, wd, nesterov)
        assert float(out) > max_norm and abs(float(out) - float(tt)) <= 1e-6 * float(tt)
        coef = max_norm / (total * scale + 1e-6)
        want = (g_h * scale).double() * coef
        assert torch.all((g.cpu().double() - want).abs() <= 1e-6 * want.abs())
    err = (p - refp.detach()).abs().max().item()
    print('p max abs err vs torch', err)
    assert err < 1e-6
    if mom:
        assert (buf - topt.state[refp]['momentum_buffer']).abs().max().item() < 1e-6


@pytest.mark.parametrize('norm_type', [2, 0])
def test_zero_gradient_moves_by_weight_decay_and_momentum_only(norm_type):
    n = 4101
    _, p_h, _ = _case(n)
    lr, mom, wd = 0.1, 0.9, 5e-4
    pa, pb = p_h.to(DEV), p_h.to(DEV)
    ga, gb = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    ba, bb = torch.zeros_like(pa), torch.zeros_like(pb)
    lr_t = torch.full((1,), lr, device=DEV)
    _, out = _step_clip(pa, ga, ba, lr_t, norm_type, 1.0, mom, wd, True)
    _step_plain(pb, gb, bb, lr_t, mom, wd, True)
    assert float(out) == 0.0                                    # coef = min(1, 1 / 1e-6) = 1
    assert not ga.any()
    assert torch.equal(pa, pb) and torch.equal(ba, bb)
    p64 = p_h.double()
    want = p64 - lr * (wd * p64 + mom * (wd * p64))             # g' = wd p;  buf = g';  step = g' + mom buf
    assert (pa.cpu().double() - want).abs().max().item() < 1e-6
    assert (ba.cpu().double() - wd * p64).abs().max().item() < 1e-9


@pytest.mark.parametrize('norm_type', [2, 0])
@pytest.mark.parametrize('n', [4101, 1376950])
def test_two_runs_give_the_same_bits(n, norm_type):
    g_h, p_h, ref = _case(n)
    runs = []
    for _ in range(2):
        p, g = p_h.to(DEV), g_h.to(DEV)
        buf = torch.full_like(p, 0.01)
        lr_t = torch.full((1,), 0.05, device=DEV)
        partial, out = _step_clip(p, g, buf, lr_t, norm_type, 0.5 * ref[norm_type][1], 0.9, 5e-4, True)
        runs.append([t.cpu() for t in (partial, out, p, buf, g)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- through the engine -------------------------------------------------------------------------------------------------

CFG = dict(type='RecognizerGCN',
           backbone=dict(type='DGSTGCN', gcn_type='dgphgcn1', gcn_ratio=0.125, gcn_node_attention=True,
                         gcn_edge_attention=True, gcn_decompose=True, gcn_subset_wise=True, gcn_ctr='T', gcn_ada='T',
                         tcn_type='dgmstcn', base_channels=16, num_stages=4, inflate_stages=[3], down_stages=[3],
                         graph_cfg=dict(layout='nturgb+d', mode='random', num_filter=3, init_off=.04, init_std=.02),
                         tcn_ms_cfg=[(3, 1), (3, 2), (3, 3), (3, 4), ('max', 3), '1x1']),
           cls_head=dict(type='GCNHead', num_classes=12, in_channels=32))


def _engine_run(steps, **engine_kw):
    torch.manual_seed(5)
    np.random.seed(5)
    m = D.build_model(CFG).cuda().train()
    eng = D.TrainEngine(m, lr=0.05, momentum=0.9, weight_decay=5e-4, nesterov=True, warmup_eager=2, **engine_kw)
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(4, 1, 2, 16, 25, 3, generator=gen).cuda()
    y = torch.randint(0, 12, (4, 1), generator=gen).cuda()
    logs = [{k: v.clone() for k, v in eng.step(x, y, lr=0.05 / (i + 1)).items()} for i in range(steps)]
    torch.cuda.synchronize()
    return eng, x, y, logs


def test_engine_clips_eagerly_and_in_replayed_graphs_bit_identically():
    """The reduced DS-STGCN, 4 clips, T = 16: four steps with grad_clip eagerly and with steps 3-4 replayed from the two
    hipGraphs (the clip rides in graph B with the update).  max_norm = 1e-3 lies far below the gradient norm, so every step
    is clipped."""
    max_norm = 1e-3
    clip = dict(max_norm=max_norm)
    ea, x, y, la = _engine_run(4, use_graph=False, grad_clip=clip)
    eb, _, _, lb = _engine_run(4, use_graph=True, grad_clip=clip)
    assert eb.capture_error is None and eb.graphed(x, y) and not ea.graphed(x, y)
    norms = [float(l['grad_norm']) for l in la]
    print('grad_norm per step', norms)
    assert all(nrm > max_norm for nrm in norms)
    assert norms == [float(l['grad_norm']) for l in lb]
    assert [float(l['loss']) for l in la] == [float(l['loss']) for l in lb]
    assert torch.equal(ea.flat.flat_p, eb.flat.flat_p) and torch.equal(ea.opt.buf, eb.opt.buf)
    assert torch.equal(ea.flat.flat_g, eb.flat.flat_g)
    # the flat buffer holds the clipped gradient: its norm is max_norm * total / (total + 1e-6)
    assert float(eb.flat.flat_g.double().norm()) == pytest.approx(max_norm, rel=1e-3)
    # ... and the clipped run is not the unclipped one
    ec, _, _, lc = _engine_run(4, use_graph=True)
    assert 'grad_norm' not in lc[0] and not torch.equal(ec.flat.flat_p, eb.flat.flat_p)


def test_engine_grad_clip_none_is_the_engine_without_the_argument():
    ea, _, _, la = _engine_run(2, use_graph=False, grad_clip=None)
    eb, _, _, lb = _engine_run(2, use_graph=False)
    assert ea.opt.grad_norm is None and 'grad_norm' not in la[0]
    assert torch.equal(ea.flat.flat_p, eb.flat.flat_p) and torch.equal(ea.opt.buf, eb.opt.buf)
    assert [float(l['loss']) for l in la] == [float(l['loss']) for l in lb]
