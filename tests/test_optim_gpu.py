"""-m gpu: the grouped update kernels of csrc/optim.hip (dsgcn_sgd_group_step[_clip], dsgcn_adam_step[_clip]) against
torch.optim under the error rule of tests/test_optim_host.py, on tables whose tensor boundaries fall everywhere; their
bit-identity with the plain SGD kernel and between the clipped and the unclipped forms; determinism; FlatAdam.step() replayed
from a hipGraph; TrainEngine with paramwise AdamW and grad_clip eagerly and as replayed hipGraphs."""
import functools
import itertools
import json
import os
import types

import numpy as np
import pytest
import torch

import dsgcn_amd as D
from dsgcn_amd import native
from dsgcn_amd.train import SKIP, GroupTable
from test_optim_host import Hand, rule_sides

pytestmark = pytest.mark.gpu
DEV = 'cuda'
K = 3
CHUNK = 4096                                        # elements per workgroup (include/dsgcn.h)
COMBOS = [(0.9, 5e-4, True), (0.9, 0.0, False), (0.0, 1e-3, False)]       # tests/test_grad_clip_gpu.py::COMBOS
GROUPS = [(0.1, 5e-4), (0.0, 5e-4), (0.05, 0.0), (0.2, 1e-3)]              # (lr, wd): one without rate, one without decay
SENTINEL = 0.25                                     # state of the skipped elements before the first step


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _layout(n):
    """-> (ends, group id per tensor) for a flat buffer of n elements.  n >= 255: 64 one-element tensors alternating between
    groups 0 and 1; then lengths 1, 1, 2, 3, 1, 5, 16, 1, ... (boundaries at every offset modulo 4); a tensor that ends on the
    first workgroup's chunk edge (4096) and a one-element tensor right behind it; large tensors; a one-element last tensor.
    Group ids cycle over the four groups and SKIP."""
    if n < 255:
        ends = [1, n] if n > 1 else [1]
        return ends, [0, 2][:len(ends)]
    ends = list(range(1, 65))
    pos = 64
    for length in itertools.cycle([1, 1, 2, 3, 1, 5, 16, 1, 7, 4, 2, 9]):
        if pos + length > min(n - 1, 600):
            break
        pos += length
        ends.append(pos)
    if n - 1 > CHUNK + 1:
        ends += [CHUNK, CHUNK + 1]
        pos = CHUNK + 1
        for length in itertools.cycle([1500, 4096, 8191, 30001, 7, 2 * CHUNK - 7]):
            if pos + length > n - 1:
                break
            pos += length
            ends.append(pos)
    if ends[-1] < n - 1:
        ends.append(n - 1)
    ends.append(n)
    cyc = [0, 1, 2, 3, SKIP]
    gids = [0, 1] * 32 + [cyc[(t + 2) % 5] for t in range(len(ends) - 64)]
    gids[-1] = 3                                                 # the one-element last tensor is updated
    assert sorted(set(ends)) == ends and {0, 1, 2, 3, SKIP} <= set(gids)
    assert {e % 4 for e in ends} == {0, 1, 2, 3}
    return ends, gids


@functools.lru_cache(maxsize=None)
def _inputs(n):
    gen = torch.Generator().manual_seed(2000 + n)
    return torch.randn(n, generator=gen), torch.randn(n, generator=gen)          # g, p — never modified


def _table(n, p_dev, single=False):
    ends, gids = _layout(n)
    starts = [0] + ends[:-1]
    flat = types.SimpleNamespace(flat_p=p_dev, slices=[(s, e - s) for s, e in zip(starts, ends)])
    if single:
        return GroupTable(flat, [GROUPS[0][0]] * len(ends), [GROUPS[0][1]] * len(ends))
    live = [g != SKIP for g in gids]
    pairs = [GROUPS[g if g != SKIP else 0] for g in gids]
    t = GroupTable(flat, [a for a, _ in pairs], [b for _, b in pairs])
    if n >= 255:
        assert t.base_lrs == [a for a, _ in GROUPS] and t.wds == [b for _, b in GROUPS]
    t.fix_live(live)
    return t


def _skip_mask(n):
    ends, gids = _layout(n)
    mask = torch.zeros(n, dtype=torch.bool)
    for s, e, g in zip([0] + ends[:-1], ends, gids):
        mask[s:e] = g == SKIP
    return mask


def _rate(it):
    return 1.0 / (it + 1)                                        # the schedule: every group's rate times this


def _grad(n, it):
    return _inputs(n)[0] * (1.0 - 0.25 * it)


@functools.lru_cache(maxsize=None)
def _reference(n, kind, combo, clip_scale):
    """K steps of torch.optim over one tensor per table row, in fp64 and in fp32 (foreach=False) on the CPU: -> dict of flat
    p / s1 (momentum buffer or exp_avg) / s2 (exp_avg_sq) per precision, the fp64 norms, max |g| fed to the optimizer."""
    g_h, p_h = _inputs(n)
    ends, gids = _layout(n)
    starts = [0] + ends[:-1]
    norm0 = float(g_h.double().norm())
    max_norm = None if clip_scale is None else clip_scale * norm0
    out = dict(max_norm=max_norm, norms=[float(_grad(n, it).double().norm()) for it in range(K)])
    for dtype in (torch.float64, torch.float32):
        params = [torch.nn.Parameter(p_h[s:e].to(dtype).clone()) for s, e in zip(starts, ends)]
        groups = [dict(params=[q], lr=GROUPS[g][0], weight_decay=GROUPS[g][1]) for q, g in zip(params, gids) if g != SKIP]
        kw = {} if dtype == torch.float64 else dict(foreach=False)
        if kind == 'SGD':
            mom, wd, nesterov = combo
            for grp in groups:
                grp['weight_decay'] = grp['weight_decay'] and wd         # the combo's decay where the group has one
            opt = torch.optim.SGD(groups, lr=0.1, momentum=mom, nesterov=nesterov, **kw)
        else:
            opt = getattr(torch.optim, kind)(groups, lr=0.1, betas=(0.9, 0.999), eps=1e-8, **kw)
        base = [grp['lr'] for grp in opt.param_groups]
        gmax = 0.0
        for it in range(K):
            for grp, b in zip(opt.param_groups, base):
                grp['lr'] = b * _rate(it)
            gi = _grad(n, it).to(dtype)
            for q, s, e in zip(params, starts, ends):
                q.grad = gi[s:e].clone()
            if max_norm is not None:
                torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)       # global: the skipped tensors count
            gmax = max(gmax, max(float(q.grad.abs().max()) for q in params))
            opt.step()
        zeros = lambda q: torch.zeros_like(q)
        keys = ('momentum_buffer', None) if kind == 'SGD' else ('exp_avg', 'exp_avg_sq')
        held = lambda q, k: opt.state.get(q, {}).get(k) if k else None
        state = [[held(q, k) if held(q, k) is not None else zeros(q) for q in params] for k in keys]
        out[dtype] = dict(p=torch.cat([q.detach() for q in params]), s1=torch.cat([s.detach() for s in state[0]]),
                          s2=torch.cat([s.detach() for s in state[1]]), g=torch.cat([q.grad for q in params]))
        out['gmax'] = gmax if dtype == torch.float64 else out['gmax']
    return out


def _device_table(n, p, kind, combo):
    """The table of _layout(n); under SGD the groups that have a weight decay carry the combo's value, as in _reference."""
    t = _table(n, p)
    if kind == 'SGD':
        t.wds = [wd and combo[1] for wd in t.wds]
        t.wd_t.copy_(torch.tensor(t.wds, dtype=torch.float64))
        t.fix_live(t.live)                                       # (re-checks the table with the new decays)
    return t


def _run(n, kind, combo, clip_scale, table=None, max_norm=None):
    """K steps on the device from _inputs(n): -> dict(p, s1, s2, g (of the last step), norms, step)."""
    lib = native.lib()
    g_h, p_h = _inputs(n)
    p = p_h.to(DEV)
    t = table(p) if table is not None else _device_table(n, p, kind, combo)
    skip = _skip_mask(n).to(DEV) if table is None else torch.zeros(n, dtype=torch.bool, device=DEV)
    s1 = torch.where(skip, torch.full_like(p, SENTINEL), torch.zeros_like(p))
    s2 = s1.clone()
    step = torch.zeros(t.chunks, dtype=torch.int32, device=DEV)
    rows = lib.dsgcn_grad_norm_rows(n)
    partial = torch.zeros(rows, dtype=torch.float64, device=DEV)
    out = torch.full((1,), -1.0, device=DEV)
    if max_norm is None and clip_scale is not None:
        max_norm = clip_scale * float(g_h.double().norm())
    norms, base = [], list(t.base_lrs)
    for it in range(K):
        t.set_lrs([b * _rate(it) for b in base])
        g = _grad(n, it).to(DEV)
        if max_norm is not None:
            assert lib.dsgcn_grad_norm_partials(g.data_ptr(), n, 2, partial.data_ptr(), _stream()) == 0
        clip = (partial.data_ptr(), rows, 2, max_norm, out.data_ptr())
        if kind == 'SGD':
            mom, _, nesterov = combo
            head = (p.data_ptr(), g.data_ptr(), s1.data_ptr() if mom else None) + t.pointers()
            if max_norm is not None:
                rc = lib.dsgcn_sgd_group_step_clip(*head, *clip, mom, int(nesterov), n, _stream())
            else:
                rc = lib.dsgcn_sgd_group_step(*head, mom, int(nesterov), n, _stream())
        else:
            head = (p.data_ptr(), g.data_ptr(), s1.data_ptr(), s2.data_ptr(), step.data_ptr()) + t.pointers()
            tail = (0.9, 0.999, 1e-8, int(kind == 'AdamW'), n, _stream())
            rc = lib.dsgcn_adam_step_clip(*head, *clip, *tail) if max_norm is not None else lib.dsgcn_adam_step(*head, *tail)
        assert rc == 0
        norms.append(float(out))
    torch.cuda.synchronize()
    return dict(p=p.cpu(), s1=s1.cpu(), s2=s2.cpu(), g=g.cpu(), norms=norms, step=step.cpu())


def _check_against_torch(n, kind, combo, clip_scale):
    ref = _reference(n, kind, combo, clip_scale)
    got = _run(n, kind, combo, clip_scale)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    ends, gids = _layout(n)
    skip = _skip_mask(n)
    live = ~skip
    lr_floor = torch.zeros(n, dtype=torch.float64)
    for s, e, g in zip([0] + ends[:-1], ends, gids):
        lr_floor[s:e] = GROUPS[g][0] if g != SKIP else 0.0
    tag = f'{kind} n={n} combo={combo} clip={clip_scale}'
    sides = {}
    for key, floor in (('p', lr_floor[live]), ('s1', ref['gmax']), ('s2', ref['gmax'] ** 2)):
        if (kind == 'SGD' and (key == 's2' or (key == 's1' and not combo[0]))):
            continue
        a, b = rule_sides(got[key][live], r32[key][live], r64[key][live], floor)
        bound = 2 * b + K * 2.0 ** -23
        print(f'error rule {tag} {key}: ours {a:.3e}  ref32 {b:.3e}  bound {bound:.3e}')
        sides[key] = (a, b, bound)
    # the skipped elements: bit for bit what went in
    assert torch.equal(got['p'][skip], _inputs(n)[1][skip])
    assert torch.equal(got['s1'][skip], torch.full((int(skip.sum()),), SENTINEL))
    assert torch.equal(got['s2'][skip], torch.full((int(skip.sum()),), SENTINEL))
    if kind != 'SGD':
        assert torch.equal(got['step'], torch.full_like(got['step'], K))
    if clip_scale is not None:
        for it, (a, want) in enumerate(zip(got['norms'], ref['norms'])):
            ulp = float(np.spacing(np.float32(want)))
            print(f'grad_norm step {it}: {a} fp64 {want} ulps {abs(a - want) / ulp:.2f}')
            assert abs(a - want) <= 2 * ulp
        want_g = r64['g']                                         # g * coef of the last step, every element (skipped too)
        gerr = (got['g'].double() - want_g).abs()
        print('clipped g max rel err', float((gerr / want_g.abs().clamp_min(1e-300)).max()))
        assert torch.all(gerr <= 1e-6 * want_g.abs())
        assert (ref['norms'][0] > ref['max_norm']) == (clip_scale < 1)
    for key, (a, b, bound) in sides.items():
        assert a <= bound, (tag, key, a, b, bound)


SMALL = [1, 3, 255, 4101]


@pytest.mark.parametrize('clip_scale', [None, 0.5, 2.0])
@pytest.mark.parametrize('combo', COMBOS)
@pytest.mark.parametrize('n', SMALL)
def test_grouped_sgd_vs_torch(n, combo, clip_scale):
    _check_against_torch(n, 'SGD', combo, clip_scale)


@pytest.mark.parametrize('clip_scale', [None, 0.5, 2.0])
@pytest.mark.parametrize('kind', ['Adam', 'AdamW'])
@pytest.mark.parametrize('n', SMALL)
def test_adam_vs_torch(n, kind, clip_scale):
    _check_against_torch(n, kind, None, clip_scale)


@pytest.mark.parametrize('kind,combo', [('SGD', COMBOS[0]), ('AdamW', None)])
def test_flat_size_of_dsstgcn_vs_torch(kind, combo):
    _check_against_torch(1376950, kind, combo, 0.5)


# ---- bit-identity with the plain kernel and between the clipped and unclipped forms -------------------------------------

@pytest.mark.parametrize('n', [255, 4101])
@pytest.mark.parametrize('mom,wd,nesterov', COMBOS)
def test_one_group_is_the_plain_sgd_kernel_bit_for_bit(mom, wd, nesterov, n):
    g_h, p_h = _inputs(n)

    def single(p):
        t = _table(n, p, single=True)
        t.base_lrs, t.wds = [0.1], [wd]
        t.wd_t.fill_(wd)
        return t
    got = _run(n, 'SGD', (mom, wd, nesterov), None, table=single)
    p = p_h.to(DEV)
    buf = torch.zeros_like(p) if mom else None
    lr_t = torch.zeros(1, device=DEV)
    for it in range(K):
        lr_t.fill_(0.1 * _rate(it))
        g = _grad(n, it).to(DEV)
        rc = native.lib().dsgcn_sgd_step(p.data_ptr(), g.data_ptr(), buf.data_ptr() if mom else None, lr_t.data_ptr(), mom, wd,
                                         int(nesterov), n, _stream())
        assert rc == 0
    assert torch.equal(got['p'], p.cpu())
    if mom:
        assert torch.equal(got['s1'], buf.cpu())


@pytest.mark.parametrize('kind,combo', [('SGD', c) for c in COMBOS] + [('Adam', None), ('AdamW', None)])
def test_clip_coefficient_one_is_the_unclipped_update_bit_for_bit(kind, combo):
    n = 4101
    a = _run(n, kind, combo, None)
    b = _run(n, kind, combo, 2.0)
    assert all(nrm < 2.0 * float(_inputs(n)[0].double().norm()) for nrm in b['norms'])
    for key in ('p', 's1', 's2', 'g', 'step'):
        assert torch.equal(a[key], b[key]), key


@pytest.mark.parametrize('n', [4101, 1376950])
@pytest.mark.parametrize('kind,combo', [('SGD', COMBOS[0]), ('AdamW', None)])
def test_two_runs_give_the_same_bits(kind, combo, n):
    a, b = _run(n, kind, combo, 0.5), _run(n, kind, combo, 0.5)
    assert a['norms'] == b['norms']
    for key in ('p', 's1', 's2', 'g', 'step'):
        assert torch.equal(a[key], b[key]), key


# ---- FlatAdam.step() replayed from a hipGraph -------------------------------------------------------------------------

PW = dict(norm_decay_mult=0., bias_lr_mult=2., custom_keys={'alpha': dict(lr_mult=0.1, decay_mult=0.)})


def _hand_adam(clip):
    torch.manual_seed(0)
    net = Hand().to(DEV)
    opt = D.build_optimizer(D.FlatParams(net), dict(type='AdamW', lr=1e-2, weight_decay=0.01, paramwise_cfg=PW), grad_clip=clip)
    gen = torch.Generator().manual_seed(9)
    opt.flat.flat_g.copy_(torch.randn(opt.flat.flat_g.numel(), generator=gen))
    return net, opt


@pytest.mark.parametrize('clip', [None, dict(max_norm=0.5)])
def test_flat_adam_step_replayed_from_a_graph(clip):
    _, warm = _hand_adam(clip)
    warm.step()                                                  # (the code object is loaded before any capture)
    _, eager = _hand_adam(clip)
    _, graphed = _hand_adam(clip)
    g0 = eager.flat.flat_g.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.step()
    assert graphed.steps == 0                                    # captured, not run
    bases = eager.group_base_lrs
    assert len(set(bases)) == 3
    for it in range(3):
        rates = [b / (it + 1) for b in bases]
        for opt in (eager, graphed):
            opt.set_lr(rates)
            opt.flat.flat_g.copy_(g0)                            # (the clipped step writes g * coef back)
        eager.step()
        graph.replay()
    torch.cuda.synchronize()
    assert eager.steps == graphed.steps == 3
    assert torch.equal(graphed.step_t, torch.full_like(graphed.step_t, 3))
    for a, b in ((eager.flat.flat_p, graphed.flat.flat_p), (eager.m, graphed.m), (eager.v, graphed.v)):
        assert torch.equal(a, b)
    if clip:
        assert torch.equal(eager.grad_norm, graphed.grad_norm) and float(eager.grad_norm) > 0.5
    assert torch.equal(next(p for k, p in graphed.flat.module.named_parameters() if k == 'frozen'), torch.ones(2, device=DEV))


# ---- through the engine -------------------------------------------------------------------------------------------------

def _cfg():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'model_reduced_cfg.json')) as f:
        cfg = json.load(f)
    cfg['backbone']['tcn_ms_cfg'] = [tuple(c) if isinstance(c, list) else c for c in cfg['backbone']['tcn_ms_cfg']]
    return cfg


OPT = dict(type='AdamW', lr=1e-3, weight_decay=0.01, paramwise_cfg=PW)


def _engine_run(steps, flush=False, **engine_kw):
    torch.manual_seed(5)
    np.random.seed(5)
    m = D.build_model(_cfg()).cuda().train()
    p0 = {k: p.detach().clone() for k, p in m.named_parameters()}
    eng = D.TrainEngine(m, optimizer=OPT, grad_clip=dict(max_norm=1e-3), warmup_eager=2, **engine_kw)
    bases = eng.opt.group_base_lrs
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(4, 1, 2, 16, 25, 3, generator=gen).cuda()
    y = torch.randint(0, 12, (4, 1), generator=gen).cuda()
    logs = [{k: v.clone() for k, v in eng.step(x, y, lr=[b / (i + 1) for b in bases]).items()} for i in range(steps)]
    if flush:
        logs.append({k: v.clone() for k, v in eng.flush().items()})
    torch.cuda.synchronize()
    return eng, x, y, logs, p0


@pytest.mark.parametrize('accumulate,steps,flush', [(1, 4, False), (2, 9, True)])
def test_engine_paramwise_adamw_eager_and_graphed_bit_identically(accumulate, steps, flush):
    ea, x, y, la, p0 = _engine_run(steps, flush, use_graph=False, accumulate=accumulate)
    eb, _, _, lb, _ = _engine_run(steps, flush, use_graph=True, accumulate=accumulate)
    assert eb.capture_error is None and eb.graphed(x, y) and not ea.graphed(x, y)
    assert len(set(ea.opt.group_base_lrs)) == 3
    updates = steps // accumulate + int(flush)
    assert ea.opt.steps == eb.opt.steps == updates
    norms = [float(l['grad_norm']) for l in la if 'grad_norm' in l]
    assert norms == [float(l['grad_norm']) for l in lb if 'grad_norm' in l]
    # (a micro-iteration reports the norm of the last update: none yet on the first accumulate - 1 calls)
    assert not any(norms[:accumulate - 1]) and all(nrm > 1e-3 for nrm in norms[accumulate - 1:])
    assert [float(l['loss']) for l in la if 'loss' in l] == [float(l['loss']) for l in lb if 'loss' in l]
    for a, b in ((ea.flat.flat_p, eb.flat.flat_p), (ea.opt.m, eb.opt.m), (ea.opt.v, eb.opt.v), (ea.flat.flat_g, eb.flat.flat_g)):
        assert torch.equal(a, b)
    live = eb.opt.table.live
    dead = [k for (k, _), alive in zip(((k, p) for k, p in eb.model.named_parameters() if p.requires_grad), live) if not alive]
    assert len(dead) >= 2 and any('conv2_se' in k for k in dead)
    P = dict(eb.model.named_parameters())
    for k in dead:
        assert torch.equal(P[k], p0[k]), k
    assert sum(not torch.equal(P[k], p0[k]) for k in P) > len(P) // 2
    state = eb.opt.state_dict()['state']
    names = list(P)
    assert all(names.index(k) not in state for k in dead) and len(state) == len(P) - len(dead)


def test_engine_needs_an_eager_first_step():
    m = D.build_model(_cfg()).cuda().train()
    with pytest.raises(ValueError, match='warmup_eager'):
        D.TrainEngine(m, optimizer=OPT, warmup_eager=0)
    with pytest.raises(ValueError, match='warmup_eager'):
        D.TrainEngine(m, optimizer=dict(type='SGD', lr=0.1, weight_decay=5e-4, paramwise_cfg=PW), warmup_eager=0)
    assert D.TrainEngine(m, optimizer=dict(type='SGD', lr=0.1, weight_decay=5e-4), warmup_eager=0).opt.table is None
