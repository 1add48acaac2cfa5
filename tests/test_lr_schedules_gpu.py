"""-m gpu: the six update launches that read momentum / beta1 from device memory (csrc/head.hip k_sgd_hyper, csrc/clip.hip
k_sgd_clip_hyper, csrc/optim.hip k_optim<.., DEV>): bit for bit their by-value parents at a constant value, torch's
optimizers with the param group changed before every step when the value moves, a TrainEngine whose captured update
follows a momentum schedule, and ``train_model`` with the OneCycle pair through the graph path.

The error rule of the comparison with torch is tests/test_optim_gpu.py's: per quantity, with scale_i = max(|x64_i|, floor),
max_i |ours_i - x64_i| / scale_i <= 2 max_i |ref32_i - x64_i| / scale_i + K 2^-23, K the number of steps."""
import functools
import json
import math
import os
import types

import numpy as np
import pytest
import torch

import dsgcn_amd as D
from dsgcn_amd import native
from dsgcn_amd.apis import train_model
from dsgcn_amd.train import SKIP, GroupTable
from test_optim_host import rule_sides

pytestmark = pytest.mark.gpu

DEV = 'cuda'
N = 4096 * 2 + 5                                    # two full workgroup chunks, one float4 of a third and a 1-element tail
# the grouped forms: boundaries at 1, right behind the first chunk edge and inside a 16-byte vector; one skipped tensor
ENDS = [1, 4097, 6002, 7000, N]
GIDS = [0, 1, 2, SKIP, 0]
GROUPS = [(0.1, 5e-4), (0.05, 0.0), (0.2, 1e-3)]    # (lr, wd) of the three groups
LR, WD = 0.1, 5e-4                                  # the one-rate forms
SENTINEL = 0.25
FORMS = ['sgd', 'sgd_clip', 'sgd_group', 'sgd_group_clip', 'adam', 'adam_clip']
SCHEDULE = (0.95, 0.9, 0.5, 0.0, 0.85)


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _inputs():
    gen = torch.Generator().manual_seed(2000 + N)
    return torch.randn(N, generator=gen), torch.randn(N, generator=gen)          # g, p — never modified


def _grad(it):
    return _inputs()[0] * (1.0 - 0.15 * it)


def _rate(it):
    return 1.0 / (it + 1)


def _view(src):
    """``src`` on the device as a view that starts 16 bytes into its storage."""
    store = torch.empty(N + 4, device=DEV, dtype=src.dtype)
    v = store[4:]
    v.copy_(src)
    assert v.data_ptr() == store.data_ptr() + 16 and v.data_ptr() % 16 == 0
    return v


def _skip_mask():
    mask = torch.zeros(N, dtype=torch.bool)
    for s, e, g in zip([0] + ENDS[:-1], ENDS, GIDS):
        mask[s:e] = g == SKIP
    return mask


def _table(p):
    flat = types.SimpleNamespace(flat_p=p, slices=[(s, e - s) for s, e in zip([0] + ENDS[:-1], ENDS)])
    pairs = [GROUPS[g if g != SKIP else 0] for g in GIDS]
    t = GroupTable(flat, [a for a, _ in pairs], [b for _, b in pairs])
    assert t.base_lrs == [a for a, _ in GROUPS]
    t.fix_live([g != SKIP for g in GIDS])
    return t


def _run(form, dev_hyper, values, clip_scale=None, decoupled=False, nesterov=True):
    """One update per entry of ``values`` (the momentum / beta1 of that step) from _inputs(): the parent entry point with the
    value as an argument, or its *_hyper form with the value written to device memory first.  -> per step a dict of
    everything the launch writes."""
    lib = native.lib()
    grouped, adam, clip = form != 'sgd' and form != 'sgd_clip', form.startswith('adam'), form.endswith('clip')
    p = _view(_inputs()[1])
    skip = _skip_mask() if grouped else torch.zeros(N, dtype=torch.bool)
    state0 = torch.where(skip, torch.full((N,), SENTINEL), torch.zeros(N))
    s1, s2 = _view(state0), _view(state0)
    t = _table(p) if grouped else None
    lr_t = torch.zeros(1, device=DEV)
    hyper = torch.zeros(1, dtype=torch.float64, device=DEV)
    step = torch.zeros(lib.dsgcn_optim_chunks(N), dtype=torch.int32, device=DEV)
    rows = lib.dsgcn_grad_norm_rows(N)
    partial = torch.zeros(rows, dtype=torch.float64, device=DEV)
    out = torch.full((1,), -1.0, device=DEV)
    max_norm = clip_scale * float(_inputs()[0].double().norm()) if clip else 0.0
    steps = []
    for it, val in enumerate(values):
        g = _view(_grad(it))
        if grouped:
            t.set_lrs([b * _rate(it) for b in t.base_lrs])
        else:
            lr_t.fill_(LR * _rate(it))
        hyper.fill_(val)
        if clip:
            assert lib.dsgcn_grad_norm_partials(g.data_ptr(), N, 2, partial.data_ptr(), _stream()) == 0
        h = hyper.data_ptr() if dev_hyper else val
        pp, gp, ap, bp, st = p.data_ptr(), g.data_ptr(), s1.data_ptr(), s2.data_ptr(), _stream()
        if form == 'sgd':
            fn = lib.dsgcn_sgd_step_hyper if dev_hyper else lib.dsgcn_sgd_step
            rc = fn(pp, gp, ap, lr_t.data_ptr(), h, WD, int(nesterov), N, st)
        elif form == 'sgd_clip':
            fn = lib.dsgcn_sgd_step_clip_hyper if dev_hyper else lib.dsgcn_sgd_step_clip
            rc = fn(pp, gp, ap, lr_t.data_ptr(), partial.data_ptr(), rows, 2, max_norm, out.data_ptr(), h, WD, int(nesterov),
                    N, st)
        elif form == 'sgd_group':
            fn = lib.dsgcn_sgd_group_step_hyper if dev_hyper else lib.dsgcn_sgd_group_step
            rc = fn(pp, gp, ap, *t.pointers(), h, int(nesterov), N, st)
        elif form == 'sgd_group_clip':
            fn = lib.dsgcn_sgd_group_step_clip_hyper if dev_hyper else lib.dsgcn_sgd_group_step_clip
            rc = fn(pp, gp, ap, *t.pointers(), partial.data_ptr(), rows, 2, max_norm, out.data_ptr(), h, int(nesterov), N, st)
        elif form == 'adam':
            fn = lib.dsgcn_adam_step_hyper if dev_hyper else lib.dsgcn_adam_step
            rc = fn(pp, gp, ap, bp, step.data_ptr(), *t.pointers(), h, 0.999, 1e-8, int(decoupled), N, st)
        else:
            fn = lib.dsgcn_adam_step_clip_hyper if dev_hyper else lib.dsgcn_adam_step_clip
            rc = fn(pp, gp, ap, bp, step.data_ptr(), *t.pointers(), partial.data_ptr(), rows, 2, max_norm, out.data_ptr(), h,
                    0.999, 1e-8, int(decoupled), N, st)
        assert rc == 0, (form, dev_hyper, it, rc)
        steps.append(dict(p=p.cpu(), s1=s1.cpu(), s2=s2.cpu(), step=step.cpu(), g=g.cpu(), norm=out.cpu()))
    torch.cuda.synchronize()
    return steps


# ---- a constant value: the parent's bits --------------------------------------------------------------------------------

def _cases():
    for form in FORMS:
        for clip_scale in ((0.5, 2.0) if form.endswith('clip') else (None,)):      # coefficient < 1 / exactly 1
            yield form, clip_scale, 0.9
    yield 'sgd', None, 0.0                             # the parents drop the buffer at 0: so do these
    yield 'sgd_group_clip', 0.5, 0.0


@pytest.mark.parametrize('form,clip_scale,value', list(_cases()))
def test_constant_value_is_the_parent_bit_for_bit(form, clip_scale, value):
    want = _run(form, False, [value] * 3, clip_scale, decoupled=True)
    got = _run(form, True, [value] * 3, clip_scale, decoupled=True)
    for it, (a, b) in enumerate(zip(got, want)):
        for key in a:
            assert torch.equal(a[key], b[key]), (form, clip_scale, it, key)
    last, first = want[-1], want[0]
    assert not torch.equal(last['p'], first['p'])
    if form.startswith('adam'):
        assert torch.equal(last['step'], torch.full_like(last['step'], 3))
    if clip_scale is not None:                         # the clip was (in)active as the case says
        assert float(first['norm']) > 0 and torch.equal(first['g'], _grad(0)) == (clip_scale > 1)
    if value == 0.0:                                   # the buffer stayed what it was
        assert torch.equal(got[-1]['s1'], torch.where(_skip_mask() & (form != 'sgd'), torch.full((N,), SENTINEL),
                                                      torch.zeros(N)))
    elif form not in ('sgd', 'sgd_clip'):              # the skipped tensor: untouched
        skip = _skip_mask()
        assert torch.equal(got[-1]['p'][skip], _inputs()[1][skip])
        assert torch.equal(got[-1]['s1'][skip], torch.full((int(skip.sum()),), SENTINEL))


# ---- a value that moves: torch with the param group changed before every step --------------------------------------------

@functools.lru_cache(maxsize=None)
def _reference(form, kind, clip_scale):
    """len(SCHEDULE) steps of torch.optim.SGD / Adam / AdamW on the CPU in fp64 and fp32 (foreach=False), one tensor per
    table row (one in all for the one-rate forms), ``momentum`` / ``betas[0]`` of every group rewritten before each step."""
    g_h, p_h = _inputs()
    grouped = form not in ('sgd', 'sgd_clip')
    ends, gids = (ENDS, GIDS) if grouped else ([N], [0])
    pairs = GROUPS if grouped else [(LR, WD)]
    starts = [0] + ends[:-1]
    max_norm = None if clip_scale is None else clip_scale * float(g_h.double().norm())
    out = {}
    for dtype in (torch.float64, torch.float32):
        params = [torch.nn.Parameter(p_h[s:e].to(dtype).clone()) for s, e in zip(starts, ends)]
        groups = [dict(params=[q], lr=pairs[g][0], weight_decay=pairs[g][1]) for q, g in zip(params, gids) if g != SKIP]
        kw = {} if dtype == torch.float64 else dict(foreach=False)
        if kind == 'SGD':
            opt = torch.optim.SGD(groups, lr=0.1, momentum=SCHEDULE[0], nesterov=True, **kw)
        else:
            opt = getattr(torch.optim, kind)(groups, lr=0.1, betas=(SCHEDULE[0], 0.999), eps=1e-8, **kw)
        base = [grp['lr'] for grp in opt.param_groups]
        gmax = 0.0
        for it, val in enumerate(SCHEDULE):
            for grp, b in zip(opt.param_groups, base):
                grp['lr'] = b * _rate(it)
                if kind == 'SGD':
                    grp['momentum'] = val
                else:
                    grp['betas'] = (val, 0.999)
            gi = _grad(it).to(dtype)
            for q, s, e in zip(params, starts, ends):
                q.grad = gi[s:e].clone()
            if max_norm is not None:
                torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)
            gmax = max(gmax, max(float(q.grad.abs().max()) for q in params))
            opt.step()
        keys = ('momentum_buffer', None) if kind == 'SGD' else ('exp_avg', 'exp_avg_sq')
        held = lambda q, k: opt.state.get(q, {}).get(k) if k else None
        state = [[held(q, k) if held(q, k) is not None else torch.zeros_like(q) for q in params] for k in keys]
        out[dtype] = dict(p=torch.cat([q.detach() for q in params]), s1=torch.cat([s.detach() for s in state[0]]),
                          s2=torch.cat([s.detach() for s in state[1]]))
        if dtype == torch.float64:
            out['gmax'] = gmax
    return out


@pytest.mark.parametrize('form,kind', [(f, 'SGD') for f in FORMS[:4]] + [(f, k) for f in FORMS[4:] for k in ('Adam', 'AdamW')])
def test_a_moving_value_follows_torch(form, kind):
    clip_scale = 0.5 if form.endswith('clip') else None
    K = len(SCHEDULE)
    got = _run(form, True, SCHEDULE, clip_scale, decoupled=kind == 'AdamW')[-1]
    ref = _reference(form, kind, clip_scale)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    grouped = form not in ('sgd', 'sgd_clip')
    skip = _skip_mask() if grouped else torch.zeros(N, dtype=torch.bool)
    live = ~skip
    lr_floor = torch.full((N,), LR, dtype=torch.float64)
    if grouped:
        for s, e, g in zip([0] + ENDS[:-1], ENDS, GIDS):
            lr_floor[s:e] = GROUPS[g][0] if g != SKIP else 0.0
    sides = {}
    for key, floor in (('p', lr_floor[live]), ('s1', ref['gmax']), ('s2', ref['gmax'] ** 2)):
        if kind == 'SGD' and key == 's2':
            continue
        a, b = rule_sides(got[key][live], r32[key][live], r64[key][live], floor)
        bound = 2 * b + K * 2.0 ** -23
        print(f'error rule {form} {kind} {key}: ours {a:.3e}  ref32 {b:.3e}  bound {bound:.3e}')
        sides[key] = (a, b, bound)
    assert torch.equal(got['p'][skip], _inputs()[1][skip])
    assert torch.equal(got['s1'][skip], torch.full((int(skip.sum()),), SENTINEL))
    if kind != 'SGD':
        assert torch.equal(got['step'], torch.full_like(got['step'], K))
    for key, (a, b, bound) in sides.items():
        assert a <= bound, (form, kind, key, a, b, bound)
    # the schedule matters at this bar: the same steps at the first value throughout land far outside it
    const = _run(form, True, [SCHEDULE[0]] * K, clip_scale, decoupled=kind == 'AdamW')[-1]
    a, _ = rule_sides(const['p'][live], r32['p'][live], r64['p'][live], lr_floor[live])
    assert a > 100 * sides['p'][2], (a, sides['p'])


# ---- rejected arguments (no launch) -------------------------------------------------------------------------------------

def test_rejected_arguments():
    lib = native.lib()
    p, g, s1, s2 = (_view(torch.zeros(N)) for _ in range(4))
    t = _table(p)
    lr_t = torch.zeros(1, device=DEV)
    hyper = torch.zeros(2, dtype=torch.float64, device=DEV)
    step = torch.zeros(lib.dsgcn_optim_chunks(N), dtype=torch.int32, device=DEV)
    rows = lib.dsgcn_grad_norm_rows(N)
    partial = torch.zeros(rows, dtype=torch.float64, device=DEV)
    out = torch.zeros(1, device=DEV)
    pp, gp, ap, bp, st = p.data_ptr(), g.data_ptr(), s1.data_ptr(), s2.data_ptr(), _stream()
    clip = (partial.data_ptr(), rows, 2, 1.0, out.data_ptr())

    def call(form, h, buf=ap):
        if form == 'sgd':
            return lib.dsgcn_sgd_step_hyper(pp, gp, buf, lr_t.data_ptr(), h, WD, 1, N, st)
        if form == 'sgd_clip':
            return lib.dsgcn_sgd_step_clip_hyper(pp, gp, buf, lr_t.data_ptr(), *clip, h, WD, 1, N, st)
        if form == 'sgd_group':
            return lib.dsgcn_sgd_group_step_hyper(pp, gp, buf, *t.pointers(), h, 1, N, st)
        if form == 'sgd_group_clip':
            return lib.dsgcn_sgd_group_step_clip_hyper(pp, gp, buf, *t.pointers(), *clip, h, 1, N, st)
        if form == 'adam':
            return lib.dsgcn_adam_step_hyper(pp, gp, buf, bp, step.data_ptr(), *t.pointers(), h, 0.999, 1e-8, 0, N, st)
        return lib.dsgcn_adam_step_clip_hyper(pp, gp, buf, bp, step.data_ptr(), *t.pointers(), *clip, h, 0.999, 1e-8, 0, N, st)

    for form in FORMS:
        assert call(form, None) == -1, form                          # NULL
        assert call(form, hyper.data_ptr() + 4) == -1, form          # not 8-byte aligned
        assert call(form, hyper.data_ptr(), None) == -1, form        # buf (SGD) / m (Adam) NULL
        assert call(form, hyper.data_ptr() + 8) == 0, form           # (any 8-byte aligned address is taken)
    torch.cuda.synchronize()
    assert not bool(p.any())                                          # (g = 0, p = 0: the accepted calls moved nothing)


# ---- a captured step follows the schedule ---------------------------------------------------------------------------------

def _cfg():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'model_reduced_cfg.json')) as f:
        cfg = json.load(f)
    cfg['backbone']['tcn_ms_cfg'] = [tuple(c) if isinstance(c, list) else c for c in cfg['backbone']['tcn_ms_cfg']]
    return cfg


SGD = dict(type='SGD', lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True)
ADAMW = dict(type='AdamW', lr=1e-3, weight_decay=0.01)
MOMENTA = (0.95, 0.9, 0.5, 0.0, 0.85, 0.6)


def _engine_run(optimizer, accumulate, use_graph):
    """Six updates with a rate and a momentum of their own; -> (engine, batch, the flat parameters and the optimizer's first
    state buffer after every call).  Under accumulation the micro-iterations carry a decoy momentum: the update uses the
    value given at the stepping call."""
    torch.manual_seed(5)
    np.random.seed(5)
    m = D.build_model(_cfg()).cuda().train()
    eng = D.TrainEngine(m, optimizer=optimizer, use_graph=use_graph, warmup_eager=1, accumulate=accumulate,
                        scheduled_momentum=True)
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(2, 1, 2, 16, 25, 3, generator=gen).cuda()
    y = torch.randint(0, 12, (2, 1), generator=gen).cuda()
    base = eng.opt.base_lr
    state = (lambda: eng.opt.buf) if isinstance(eng.opt, D.FlatSGD) else (lambda: eng.opt.m)
    snaps = []
    for i, mom in enumerate(MOMENTA):
        for micro in range(accumulate):
            stepping = micro + 1 == accumulate
            eng.step(x, y, lr=base / (i + 1), momentum=mom if stepping else 0.123)
            snaps.append((eng.flat.flat_p.clone(), state().clone()))
    torch.cuda.synchronize()
    return eng, x, y, snaps


@pytest.mark.parametrize('optimizer,accumulate', [(SGD, 1), (SGD, 2), (ADAMW, 1)])
def test_captured_step_follows_the_momentum_schedule(optimizer, accumulate):
    ea, x, y, sa = _engine_run(optimizer, accumulate, use_graph=False)
    eb, _, _, sb = _engine_run(optimizer, accumulate, use_graph=True)
    assert eb.capture_error is None and eb.graphed(x, y) and not ea.graphed(x, y)
    assert eb.opt.scheduled_momentum and float(eb.opt.hyper_t) == MOMENTA[-1]
    assert len(sa) == len(sb) == len(MOMENTA) * accumulate
    for i, ((pa, ba), (pb, bb)) in enumerate(zip(sa, sb)):
        assert torch.equal(pa, pb) and torch.equal(ba, bb), i
    # the replayed update read the value of its own step: the state after the step at momentum 0 (SGD: the buffer is left
    # alone) resp. every step (Adam: exp_avg moves whatever beta1 is) shows it
    at_zero = (MOMENTA.index(0.0) + 1) * accumulate - 1
    if optimizer is SGD:
        assert torch.equal(sb[at_zero][1], sb[at_zero - 1][1]) and not torch.equal(sb[at_zero][0], sb[at_zero - 1][0])
        assert not torch.equal(sb[-1][1], sb[at_zero][1])
        group = eb.opt.state_dict()['param_groups'][0]
        assert group['momentum'] == MOMENTA[-1] and group['initial_momentum'] == 0.9
    else:
        assert eb.opt.steps == len(MOMENTA)
        group = eb.opt.state_dict()['param_groups'][0]
        assert group['betas'] == (MOMENTA[-1], 0.999) and group['initial_momentum'] == 0.9


# ---- train_model: the OneCycle pair through the graph path ------------------------------------------------------------------

def _cos(a, b, f):
    return b + 0.5 * 1 * (a - b) * (math.cos(math.pi * f) + 1)


def _onecycle(values, steps, pct):
    """mmcv's two-phase walk over ``values`` = (start, middle, end)."""
    rows, ends = [], (float(pct * steps) - 1, steps - 1)
    for it in range(steps):
        if it <= ends[0]:
            rows.append(_cos(values[0], values[1], (it - 0) / (ends[0] - 0)))
        else:
            rows.append(_cos(values[1], values[2], (it - ends[0]) / (ends[1] - ends[0])))
    return rows


def test_train_model_onecycle_pair_through_the_graph():
    torch.manual_seed(5)
    np.random.seed(5)
    m = D.build_model(_cfg())
    gen = torch.Generator().manual_seed(3)
    data = [dict(keypoint=torch.randn(1, 2, 16, 25, 3, generator=gen).numpy(), label=i % 12) for i in range(8)]
    cfg = dict(data=dict(videos_per_gpu=2), seed=0, total_epochs=1, optimizer=dict(SGD), optimizer_config=dict(grad_clip=None),
               lr_config=dict(policy='OneCycle', max_lr=[0.2], pct_start=0.4),
               momentum_config=dict(policy='OneCycle', pct_start=0.4), checkpoint_config=None, log_config=dict(interval=1))
    runner = train_model(m, data, cfg, device='cuda', use_graph=True)
    eng = runner.engine
    assert runner.iter == 4 and len(runner.log) == 4
    assert eng.capture_error is None and len(eng._graphs) == 1 and eng.opt.scheduled_momentum       # two eager steps, then replays
    base = 0.2 / 25
    rates = _onecycle((base * 1, base * 25, base * (1 / 1e4)), 4, 0.4)
    moms = _onecycle((0.95, 0.85, 0.95), 4, 0.4)
    assert [r['lr'] for r in runner.log] == rates
    assert [r['momentum'] for r in runner.log] == moms
    assert len(set(moms)) >= 3 and len(set(rates)) == 4
    assert float(eng.opt.hyper_t) == moms[-1] and float(eng.opt.lr_t) == np.float32(rates[-1])
    assert all(math.isfinite(r['loss']) for r in runner.log)
