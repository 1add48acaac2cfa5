"""CPU: mmcv's rate policies (Exp, Poly, Inv, CosineRestart, Cyclic, OneCycle; CosineAnnealing by epoch / with a ratio;
step by iteration) and its two momentum policies (cyclic, OneCycle) in ``apis.EpochRunner``, and the optimizers'
``scheduled_momentum`` on their torch-op path.

References: torch's own schedulers where they define the same curve (both sides fp64 closed forms a few dozen roundings
long: 1e-12 relative), tables written out from mmcv's formulas (the same Python-float expressions: exact), and for whole
runs real torch optimizers driven by ``OneCycleLR(cycle_momentum=True)`` under the error rule of tests/test_optim_host.py."""
import copy
import math
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.optim import lr_scheduler as S

import dsgcn_amd as D
import torch_ops
from dsgcn_amd.apis import EpochRunner, epoch_indices, train_model
from dsgcn_amd.train import build_optimizer
from test_optim_host import rule_sides
from test_train_loop import _setup

ITERS = 37
BASE = 0.1


def _runner(lr_config, momentum_config=None, samples=ITERS, batch=1, epochs=1, opt=None):
    """An EpochRunner over a stand-in engine: the schedules read ``opt.base_lr`` and, with a momentum_config, the
    optimizer's ``scheduled_momentum`` / ``initial_momentum`` (and ``betas`` to tell Adam from SGD)."""
    if opt is None:
        opt = types.SimpleNamespace(base_lr=BASE, scheduled_momentum=True, initial_momentum=0.9)
    cfg = dict(data=dict(videos_per_gpu=batch), total_epochs=epochs, lr_config=lr_config)
    if momentum_config is not None:
        cfg['momentum_config'] = momentum_config
    return EpochRunner(None, types.SimpleNamespace(opt=opt), list(range(samples)), cfg)


def _walk(runner):
    """(rate, momentum) of every iteration of the run."""
    rates, moms = [], []
    for it in range(runner.max_iters):
        runner.iter, runner.epoch = it, it // runner.iters_per_epoch
        rates.append(runner.current_lr())
        moms.append(runner.current_momentum())
    return rates, moms


def _torch_walk(make_opt, make_sched, iters=ITERS):
    """The param group's lr and momentum (betas[0]) before every optimizer step of a torch loop."""
    opt = make_opt([nn.Parameter(torch.zeros(1))])
    sched = make_sched(opt)
    rates, moms = [], []
    for it in range(iters):
        g = opt.param_groups[0]
        rates.append(g['lr'])
        moms.append(g['betas'][0] if 'betas' in g else g['momentum'])
        opt.step()
        if it + 1 < iters:
            sched.step()
    return rates, moms


def _close(got, want):
    assert len(got) == len(want)
    for it, (a, b) in enumerate(zip(got, want)):
        assert abs(a - b) <= 1e-12 * abs(b), (it, a, b)


# ---- against torch's schedulers ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('pct_start', [0.3, 0.1])          # 0.1 * 37 - 1 = 2.7: a fractional phase end
@pytest.mark.parametrize('strategy', ['cos', 'linear'])
@pytest.mark.parametrize('three_phase', [False, True])
@pytest.mark.parametrize('kind', ['SGD', 'Adam'])
def test_onecycle_pair_is_torchs_onecyclelr(kind, three_phase, strategy, pct_start):
    if kind == 'SGD':
        stand_in = types.SimpleNamespace(base_lr=BASE, scheduled_momentum=True, initial_momentum=0.9)
        make_opt = lambda ps: torch.optim.SGD(ps, lr=BASE, momentum=0.9)
    else:
        stand_in = types.SimpleNamespace(base_lr=BASE, scheduled_momentum=True, initial_momentum=0.9, betas=(0.9, 0.999))
        make_opt = lambda ps: torch.optim.Adam(ps, lr=BASE, betas=(0.9, 0.999))
    runner = _runner(dict(policy='OneCycle', max_lr=[0.5], pct_start=pct_start, anneal_strategy=strategy,
                          three_phase=three_phase),
                     dict(policy='OneCycle', pct_start=pct_start, anneal_strategy=strategy, three_phase=three_phase),
                     opt=stand_in)
    assert runner.max_iters == ITERS
    rates, moms = _walk(runner)
    want_r, want_m = _torch_walk(make_opt, lambda o: S.OneCycleLR(
        o, max_lr=0.5, total_steps=ITERS, pct_start=pct_start, anneal_strategy=strategy, three_phase=three_phase,
        div_factor=25, final_div_factor=1e4, base_momentum=0.85, max_momentum=0.95))
    _close(rates, want_r)
    _close(moms, want_m)
    assert rates[0] == pytest.approx(0.5 / 25, rel=1e-12) and moms[0] == pytest.approx(0.95, rel=1e-12)
    assert max(rates) <= 0.5 * (1 + 1e-12) and min(moms) >= 0.85 * (1 - 1e-12)


def test_cosine_restart_equal_periods_is_torchs_warm_restarts():
    runner = _runner(dict(policy='CosineRestart', periods=[10] * 4, restart_weights=[1] * 4, min_lr=1e-3, by_epoch=False))
    want, _ = _torch_walk(lambda ps: torch.optim.SGD(ps, lr=BASE, momentum=0.9),
                          lambda o: S.CosineAnnealingWarmRestarts(o, T_0=10, T_mult=1, eta_min=1e-3))
    _close(_walk(runner)[0], want)


def test_exp_is_torchs_exponential_lr():
    runner = _runner(dict(policy='Exp', gamma=0.93, by_epoch=False))
    want, _ = _torch_walk(lambda ps: torch.optim.SGD(ps, lr=BASE, momentum=0.9), lambda o: S.ExponentialLR(o, gamma=0.93))
    _close(_walk(runner)[0], want)


@pytest.mark.parametrize('step', [5, [4, 11, 30]])
def test_step_by_iteration_is_torchs_step_lr(step):
    runner = _runner(dict(policy='step', step=step, gamma=0.5, by_epoch=False))
    make = (lambda o: S.StepLR(o, step_size=step, gamma=0.5)) if isinstance(step, int) else \
        (lambda o: S.MultiStepLR(o, milestones=step, gamma=0.5))
    want, _ = _torch_walk(lambda ps: torch.optim.SGD(ps, lr=BASE, momentum=0.9), make)
    got = _walk(runner)[0]
    _close(got, want)
    assert len(set(got)) == (8 if isinstance(step, int) else 4)


# ---- tables written out from mmcv's formulas: exact ----------------------------------------------------------------------

def _cos(a, b, f, w=1):
    return b + 0.5 * w * (a - b) * (math.cos(math.pi * f) + 1)


def _lin(a, b, f):
    return (b - a) * f + a


def _cyclic_table(base, max_iters, ratio, times, up_ratio, anneal):
    rows = []
    L = max_iters // times
    up = int(up_ratio * L)
    for it in range(max_iters):
        c = it % L
        if c < up:
            rows.append(anneal(base, base * ratio[0], c / up))
        else:
            rows.append(anneal(base * ratio[0], base * ratio[1], (c - up) / (L - up)))
    return rows


@pytest.mark.parametrize('times,up_ratio,strategy', [(1, 0.4, 'cos'), (2, 0.4, 'linear'), (3, 0.05, 'cos')])
def test_cyclic_rate_and_momentum_tables(times, up_ratio, strategy):
    """37 iterations: cyclic_times 2 and 3 do not divide them (the last iteration starts a new cycle), and with
    step_ratio_up 0.05 a cycle of 12 has no rising part (up == 0)."""
    runner = _runner(dict(policy='cyclic', target_ratio=(8, 1e-3), cyclic_times=times, step_ratio_up=up_ratio,
                          anneal_strategy=strategy),
                     dict(policy='cyclic', cyclic_times=times, step_ratio_up=up_ratio))
    rates, moms = _walk(runner)
    assert rates == _cyclic_table(BASE, ITERS, (8, 1e-3), times, up_ratio, _cos if strategy == 'cos' else _lin)
    assert moms == _cyclic_table(0.9, ITERS, (0.85 / 0.95, 1), times, up_ratio, _cos)      # the momentum: always cosine
    L = ITERS // times
    assert ITERS % L != 0 or times == 1
    if up_ratio == 0.05:
        assert int(up_ratio * L) == 0 and rates[0] == pytest.approx(BASE * 8, rel=1e-12)
    else:
        assert rates[0] == pytest.approx(BASE, rel=1e-12) and rates[int(up_ratio * L)] == pytest.approx(BASE * 8, rel=1e-12)
    if times > 1:
        assert rates[L] == rates[0] and rates[ITERS - 1] == rates[ITERS - 1 - L]
    # the defaults: target_ratio (10, 1e-4), one cycle, 40 % rising, cosine
    assert _walk(_runner(dict(policy='Cyclic')))[0] == _cyclic_table(BASE, ITERS, (10, 1e-4), 1, 0.4, _cos)


def test_poly_and_inv_tables():
    rates = _walk(_runner(dict(policy='Poly', power=0.9, min_lr=1e-4, by_epoch=False)))[0]
    assert rates == [(BASE - 1e-4) * (1 - it / ITERS) ** 0.9 + 1e-4 for it in range(ITERS)]
    assert _walk(_runner(dict(policy='Poly', by_epoch=False)))[0] == [(BASE - 0.) * (1 - it / ITERS) ** 1. + 0.
                                                                       for it in range(ITERS)]
    rates = _walk(_runner(dict(policy='Inv', gamma=0.01, power=0.75, by_epoch=False)))[0]
    assert rates == [BASE * (1 + 0.01 * it) ** (-0.75) for it in range(ITERS)]
    assert _walk(_runner(dict(policy='Inv', gamma=0.01, by_epoch=False)))[0] == [BASE * (1 + 0.01 * it) ** (-1.)
                                                                                 for it in range(ITERS)]
    # by epoch (mmcv's default): 12 samples, batches of 4, 5 epochs — the rate moves once per epoch
    by_epoch = _walk(_runner(dict(policy='Poly', power=2.), samples=12, batch=4, epochs=5))[0]
    assert by_epoch == [(BASE - 0.) * (1 - (it // 3) / 5) ** 2. + 0. for it in range(15)]
    by_epoch = _walk(_runner(dict(policy='Exp', gamma=0.5), samples=12, batch=4, epochs=5))[0]
    assert by_epoch == [BASE * 0.5 ** (it // 3) for it in range(15)]


def test_cosine_annealing_by_epoch_and_with_a_ratio():
    by_epoch = _walk(_runner(dict(policy='CosineAnnealing', min_lr=1e-3), samples=12, batch=4, epochs=5))[0]
    assert by_epoch == [1e-3 + 0.5 * (BASE - 1e-3) * (1 + math.cos(math.pi * (it // 3) / 5)) for it in range(15)]
    ratio = _walk(_runner(dict(policy='CosineAnnealing', min_lr_ratio=0.05, by_epoch=False)))[0]
    t = BASE * 0.05
    assert ratio == [t + 0.5 * (BASE - t) * (1 + math.cos(math.pi * it / ITERS)) for it in range(ITERS)]
    both = _walk(_runner(dict(policy='CosineAnnealing', min_lr_ratio=0.05), samples=12, batch=4, epochs=5))[0]
    assert both == [t + 0.5 * (BASE - t) * (1 + math.cos(math.pi * (it // 3) / 5)) for it in range(15)]


def test_cosine_restart_unequal_periods_and_weights():
    periods, weights = [5, 12, 20], [1, 0.5, 0.25]
    rates = _walk(_runner(dict(policy='CosineRestart', periods=periods, restart_weights=weights, min_lr_ratio=0.01,
                               by_epoch=False)))[0]
    want, target = [], BASE * 0.01
    for it in range(ITERS):
        i = 0 if it < 5 else (1 if it < 17 else 2)
        start = (0, 5, 17)[i]
        alpha = min((it - start) / periods[i], 1)
        want.append(target + 0.5 * weights[i] * (BASE - target) * (math.cos(math.pi * alpha) + 1))
    assert rates == want
    assert rates[5] == target + 0.5 * (BASE - target) and rates[17] == target + 0.25 * (BASE - target)
    from dsgcn_amd.train import cosine_restart_lr
    with pytest.raises(ValueError, match='exceeds'):
        cosine_restart_lr(BASE, 37, periods, weights, min_lr=0.)


def _onecycle_table(base, S_, pct, anneal, three, div=25, final=1e4):
    phases = [(float(pct * S_) - 1, 1, div)]
    if three:
        phases += [(float(2 * pct * S_) - 2, div, 1), (S_ - 1, 1, 1 / final)]
    else:
        phases += [(S_ - 1, div, 1 / final)]
    rows = []
    for it in range(S_):
        start = 0
        for end, r0, r1 in phases:
            if it <= end:
                rows.append(anneal(base * r0, base * r1, (it - start) / (end - start)))
                break
            start = end
    return rows


def test_warmup_on_top_of_onecycle():
    cfg = dict(policy='OneCycle', max_lr=0.5, warmup='linear', warmup_iters=6, warmup_ratio=0.2)
    rates = _walk(_runner(cfg))[0]
    regular = _onecycle_table(0.5 / 25, ITERS, 0.3, _cos, False)
    assert rates == [r * (1 - (1 - it / 6) * (1 - 0.2)) if it < 6 else r for it, r in enumerate(regular)]
    assert _walk(_runner(dict(policy='OneCycle', max_lr=0.5)))[0] == regular
    # total_steps beyond the run: the cycle is cut short, not rescaled
    longer = _walk(_runner(dict(policy='OneCycle', max_lr=0.5, total_steps=50, three_phase=True)))[0]
    assert longer == _onecycle_table(0.5 / 25, 50, 0.3, _cos, True)[:ITERS]


class Hand(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 4, 1)
        self.bn = nn.BatchNorm2d(4)
        self.alpha = nn.Parameter(torch.zeros(1))

    def forward(self, x):
        return (self.bn(self.conv(x)) * (1 + self.alpha)).square().mean()


def test_onecycle_gives_every_paramwise_group_one_rate():
    """mmcv's OneCycle overwrites every group's initial rate with max_lr / div_factor: lr_mult is discarded."""
    pw = dict(bias_lr_mult=2., custom_keys={'alpha': dict(lr_mult=0.1)})
    opt = build_optimizer(D.FlatParams(Hand()), dict(type='SGD', lr=BASE, momentum=0.9, paramwise_cfg=pw))
    assert len(set(opt.group_base_lrs)) == 3
    runner = _runner(dict(policy='OneCycle', max_lr=[0.5]), opt=opt)
    table = _onecycle_table(0.5 / 25, ITERS, 0.3, _cos, False)
    for it in (0, 7, 36):
        runner.iter = it
        assert runner.current_lrs() == [table[it]] * len(opt.group_base_lrs)
    cosine = _runner(dict(policy='CosineAnnealing', min_lr=1e-3, by_epoch=False), opt=opt)
    cosine.iter = 7
    assert len(set(cosine.current_lrs())) == 3                 # (every other policy keeps the groups apart)


# ---- whole runs ---------------------------------------------------------------------------------------------------------

ONECYCLE = dict(pct_start=0.4, anneal_strategy='cos', three_phase=False)


def _reference(model, data, cfg, make_opt, max_lr, dtype, dense_grads):
    """The loop train_model runs, driven by a real torch optimizer and torch's OneCycleLR with cycle_momentum over ``model``;
    -> the parameters after every iteration.  dense_grads: every parameter carries a gradient tensor (zeros where the
    backward pass delivers none) — the plain FlatSGD updates ALL elements of the flat buffer, so the conv2_se tensors that
    never receive a gradient still decay (train.py, quirk Q10); FlatAdam skips them as torch skips a ``.grad`` of None."""
    model = model.to(dtype).train()
    opt = make_opt(model)
    if dense_grads:
        for p in model.parameters():
            p.grad = torch.zeros_like(p)
    bs, n = cfg['data']['videos_per_gpu'], len(data)
    ipe = int(math.ceil(n / bs))
    total = cfg['total_epochs'] * ipe
    sched = S.OneCycleLR(opt, max_lr=max_lr, total_steps=total, cycle_momentum=True, base_momentum=0.85, max_momentum=0.95,
                         div_factor=25, final_div_factor=1e4, **ONECYCLE)
    snaps, it = [], 0
    with D.kernels.use_ops(torch_ops):
        for ep in range(cfg['total_epochs']):
            order = epoch_indices(n, ep, cfg['seed'], 0, 1, True)
            for b in range(ipe):
                idx = order[b * bs:(b + 1) * bs]
                kp = torch.stack([torch.as_tensor(np.asarray(data[i]['keypoint']), dtype=dtype) for i in idx])
                lb = torch.as_tensor([data[i]['label'] for i in idx], dtype=torch.int64).view(-1, 1)
                opt.zero_grad(set_to_none=not dense_grads)
                if dtype == torch.float32:
                    model.train_step(dict(keypoint=kp, label=lb), None, sync_log_vars=False)['loss'].backward()
                else:
                    feat = model.extract_feat(kp[:, 0])
                    model.cls_head.loss(model.cls_head(feat), lb.squeeze(-1))['loss_cls'].backward()
                opt.step()
                it += 1
                if it < total:
                    sched.step()
                snaps.append({k: p.detach().clone() for k, p in model.named_parameters()})
    return snaps


def _schedule_cfg(cfg, kind, max_lr):
    if kind == 'SGD':
        cfg['optimizer'] = dict(type='SGD', lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True)
    else:
        cfg['optimizer'] = dict(type='AdamW', lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01)
    cfg['lr_config'] = dict(policy='OneCycle', max_lr=[max_lr], **ONECYCLE)
    cfg['momentum_config'] = dict(policy='OneCycle', **ONECYCLE)
    return cfg


@pytest.mark.parametrize('kind', ['SGD', 'AdamW'])
def test_train_model_onecycle_pair_matches_torch(tmp_path, kind, monkeypatch):
    z, tr, m, data, cfg = _setup(tmp_path)
    max_lr = 0.2 if kind == 'SGD' else 5e-3
    _schedule_cfg(cfg, kind, max_lr)
    cfg['checkpoint_config'] = None
    if kind == 'SGD':
        mk = lambda **kw: (lambda mod: torch.optim.SGD(mod.parameters(), lr=0.1, momentum=0.9, weight_decay=5e-4,
                                                       nesterov=True, **kw))
    else:
        mk = lambda **kw: (lambda mod: torch.optim.AdamW(mod.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01,
                                                         **kw))
    s64 = _reference(copy.deepcopy(m), data, cfg, mk(), max_lr, torch.float64, kind == 'SGD')
    s32 = _reference(copy.deepcopy(m), data, cfg, mk(foreach=False), max_lr, torch.float32, kind == 'SGD')
    ours, step = [], D.TrainEngine.step

    def recording_step(self, *args, **kwargs):
        out = step(self, *args, **kwargs)
        ours.append(self.flat.flat_p.detach().clone())
        return out
    monkeypatch.setattr(D.TrainEngine, 'step', recording_step)
    with D.kernels.use_ops(torch_ops):
        runner = train_model(m, data, cfg, device='cpu', use_graph=False)
    opt = runner.engine.opt
    assert opt.scheduled_momentum and runner.iter == 6 and len(ours) == 6
    # the log carries the host schedule's numbers, which are torch's
    table = _onecycle_table(max_lr / 25, 6, 0.4, _cos, False)
    assert [r['lr'] for r in runner.log] == table
    moms = [r['momentum'] for r in runner.log]
    want_r, want_m = _torch_walk((lambda ps: torch.optim.SGD(ps, lr=0.1, momentum=0.9)) if kind == 'SGD' else
                                 (lambda ps: torch.optim.AdamW(ps, lr=1e-3)),
                                 lambda o: S.OneCycleLR(o, max_lr=max_lr, total_steps=6, base_momentum=0.85,
                                                        max_momentum=0.95, **ONECYCLE), iters=6)
    _close(table, want_r)
    _close(moms, want_m)
    assert len(set(moms)) > 3
    names = {id(p): k for k, p in m.named_parameters()}
    floor = max_lr / 25                                         # the rate the run starts from
    worst, near = (0.0, 0.0), 0.0
    for it in range(6):
        for p, (off, n) in zip(opt.flat.params, opt.flat.slices):
            k = names[id(p)]
            a, b = rule_sides(ours[it][off:off + n], s32[it][k], s64[it][k], floor)
            assert a <= 2 * b + (it + 1) * 2.0 ** -23, (it, k, a, b)
            worst = max(worst, (a, b))
            # the fp32 reference runs the same torch ops with hyper-parameters that agree to 1e-12: a wrong momentum or
            # rate would show at 1e-2 of an update, rounding differences (the rate as a device float, one fused
            # multiply-add) stay some ulps of the parameter per step
            near = max(near, float((ours[it][off:off + n] - s32[it][k].reshape(-1)).abs().max()
                                   / s32[it][k].abs().max().clamp_min(floor)))
    print(f'largest distance from the fp32 torch run, relative to the tensor\'s largest element: {near:.3e}')
    assert near <= 6 * 16 * 2.0 ** -24, near
    print(f'error rule {kind} OneCycle + OneCycle momentum, worst parameter of any iteration: ours {worst[0]:.3e}  '
          f'ref32 {worst[1]:.3e}')
    sd = opt.state_dict()['param_groups'][0]
    assert (sd['momentum'] if kind == 'SGD' else sd['betas'][0]) == moms[-1] and sd['initial_momentum'] == 0.9


@pytest.mark.parametrize('kind', ['SGD', 'AdamW'])
def test_resumed_run_continues_both_schedules(tmp_path, kind):
    """Stop after epoch 1 of 3 and resume: the schedules are functions of the iteration alone."""
    max_lr = 0.2 if kind == 'SGD' else 5e-3
    z, tr, m, data, cfg = _setup(tmp_path, total_epochs=3)
    with D.kernels.use_ops(torch_ops):
        full = train_model(m, data, _schedule_cfg(cfg, kind, max_lr), device='cpu', use_graph=False)
    assert full.iter == 9 and all('momentum' in r for r in full.log)
    _, _, m2, data2, cfg2 = _setup(tmp_path / 'second', total_epochs=3, resume_from=str(tmp_path / 'epoch_1.pth'))
    with D.kernels.use_ops(torch_ops):
        part = train_model(m2, data2, _schedule_cfg(cfg2, kind, max_lr), device='cpu', use_graph=False)
    assert part.iter == 9 and len(part.log) == 6
    assert [r['lr'] for r in part.log] == [r['lr'] for r in full.log][3:]
    assert [r['momentum'] for r in part.log] == [r['momentum'] for r in full.log][3:]
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    assert part.engine.opt.initial_momentum == 0.9              # the schedule's base comes from the config


def test_checkpoint_restores_the_current_momentum():
    torch.manual_seed(0)
    net = Hand()
    x = torch.randn(5, 3, 4, 4)
    for cfg, read in ((dict(type='SGD', lr=0.1, momentum=0.9, nesterov=True), lambda g: g['momentum']),
                      (dict(type='AdamW', lr=1e-3, betas=(0.8, 0.99)), lambda g: g['betas'][0])):
        base = read(cfg)
        opt = build_optimizer(D.FlatParams(copy.deepcopy(net)), cfg, scheduled_momentum=True)
        assert opt.hyper_t.dtype == torch.float64 and opt.hyper_t.numel() == 1 and float(opt.hyper_t) == base
        opt.zero_grad()
        opt.flat.module(x).backward()
        opt.set_momentum(0.5)
        opt.step()
        sd = opt.state_dict()
        assert all(read(g) == 0.5 and g['initial_momentum'] == base for g in sd['param_groups'])
        other = build_optimizer(D.FlatParams(copy.deepcopy(net)), cfg, scheduled_momentum=True)
        other.load_state_dict(copy.deepcopy(sd))
        assert read(other.state_dict()['param_groups'][0]) == 0.5 and float(other.hyper_t) == 0.5
        assert other.initial_momentum == base
        for bad in (1.0, -0.1, float('nan')):
            with pytest.raises(ValueError, match=r'outside \[0, 1\)'):
                opt.set_momentum(bad)
        assert float(opt.hyper_t) == 0.5


@pytest.mark.parametrize('paramwise', [False, True])
def test_flat_sgd_follows_torch_through_a_momentum_of_zero(paramwise):
    """The eager torch-op paths honour the current value; at 0 the buffer is left alone, as torch leaves it."""
    torch.manual_seed(0)
    net = Hand()
    ref = copy.deepcopy(net)
    x = torch.randn(5, 3, 4, 4)
    cfg = dict(type='SGD', lr=0.05, momentum=0.9, weight_decay=1e-3, nesterov=False)
    if paramwise:
        cfg['paramwise_cfg'] = dict(bias_lr_mult=1.)
    opt = build_optimizer(D.FlatParams(net), cfg, scheduled_momentum=True)
    topt = torch.optim.SGD(ref.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-3, foreach=False)
    for mom in (0.95, 0.9, 0.5, 0.0, 0.85):
        opt.set_momentum(mom)
        topt.param_groups[0]['momentum'] = mom
        for mod, o in ((net, opt), (ref, topt)):
            o.zero_grad()
            mod(x).backward()
            o.step()
        for (k, a), (_, b) in zip(net.named_parameters(), ref.named_parameters()):
            assert torch.allclose(a, b, rtol=1e-6, atol=1e-8), (mom, k)


# ---- what raises ---------------------------------------------------------------------------------------------------------

def test_rejected_policies_and_options():
    for cfg, name in ((dict(policy='FlatCosineAnnealing', min_lr=0), 'FlatCosineAnnealing'),
                      (dict(policy='LinearAnnealing', min_lr=0), 'LinearAnnealing'),
                      (dict(policy='Cyclic', gamma=0.5), 'gamma'),
                      (dict(policy='OneCycle', max_lr=0.5, cycle_momentum=True), 'cycle_momentum'),
                      (dict(policy='Exp', gamma=0.9, min_lr=0), 'min_lr'),
                      (dict(policy='Poly', periods=[3]), 'periods'),
                      (dict(policy='fixed', gamma=0.9), 'gamma'),
                      (dict(policy='Cyclic', by_epoch=True), 'by_epoch'),
                      (dict(policy='OneCycle', max_lr=0.5, by_epoch=True), 'by_epoch'),
                      (dict(policy='OneCycle', max_lr=[0.5, 0.1]), 'max_lr')):
        with pytest.raises(NotImplementedError, match=name):
            _runner(cfg)
    for cfg, name in ((dict(policy='step', step=[3]), 'step'), (dict(policy='CosineAnnealing', min_lr=0), 'CosineAnnealing'),
                      (dict(policy='cyclic', gamma=0.5), 'gamma'), (dict(policy='cyclic', anneal_strategy='cos'), 'anneal'),
                      (dict(policy='OneCycle', total_steps=40), 'total_steps')):
        with pytest.raises(NotImplementedError, match=name):
            _runner(dict(policy='OneCycle', max_lr=0.5), cfg)
    with pytest.raises(NotImplementedError, match='warmup'):
        _runner(dict(policy='OneCycle', max_lr=0.5), dict(policy='cyclic', warmup='linear'))
    with pytest.raises(NotImplementedError, match='by_epoch'):
        _runner(dict(policy='OneCycle', max_lr=0.5), dict(policy='cyclic', by_epoch=True))


def test_rejected_values():
    with pytest.raises(ValueError, match='total steps'):
        _runner(dict(policy='OneCycle', max_lr=0.5, total_steps=ITERS - 1))
    _runner(dict(policy='OneCycle', max_lr=0.5, total_steps=ITERS))
    with pytest.raises(ValueError, match='anneal_strategy'):
        _runner(dict(policy='OneCycle', max_lr=0.5, anneal_strategy='exp'))
    with pytest.raises(ValueError, match='pct_start'):
        _runner(dict(policy='OneCycle', max_lr=0.5, pct_start=1.5))
    with pytest.raises(ValueError, match='max_lr'):
        _runner(dict(policy='OneCycle'))
    with pytest.raises(ValueError, match='exactly one'):
        _runner(dict(policy='CosineAnnealing', min_lr=0, min_lr_ratio=0.1, by_epoch=False))
    with pytest.raises(ValueError, match='exactly one'):
        _runner(dict(policy='CosineRestart', periods=[40], by_epoch=False))
    with pytest.raises(ValueError, match='same length'):
        _runner(dict(policy='CosineRestart', periods=[20, 20], min_lr=0, by_epoch=False))
    with pytest.raises(ValueError, match='periods cover'):
        _runner(dict(policy='CosineRestart', periods=[36], min_lr=0, by_epoch=False))
    with pytest.raises(ValueError, match='cyclic_times'):
        _runner(dict(policy='Cyclic', cyclic_times=ITERS + 1))
    with pytest.raises(ValueError, match='step_ratio_up'):
        _runner(dict(policy='Cyclic', step_ratio_up=1.0))
    with pytest.raises(ValueError, match='gamma'):
        _runner(dict(policy='Exp', by_epoch=False))
    lr = dict(policy='OneCycle', max_lr=0.5)
    # a scheduled momentum outside [0, 1): the schedule's extremes are evaluated at construction
    for mom in (dict(policy='OneCycle', max_momentum=1.0), dict(policy='OneCycle', base_momentum=-0.1),
                dict(policy='cyclic', target_ratio=(1.2, 1)), dict(policy='cyclic', target_ratio=(0.9, -1))):
        with pytest.raises(ValueError, match=r'outside \[0, 1\)'):
            _runner(lr, mom)
    _runner(lr, dict(policy='cyclic', target_ratio=(1.1, 1)))    # 0.99: inside
    with pytest.raises(ValueError, match='momentum=0'):
        _runner(lr, dict(policy='cyclic'), opt=types.SimpleNamespace(base_lr=BASE, scheduled_momentum=True,
                                                                     initial_momentum=0.0))
    # Adam's beta1 may start at 0 only if the schedule keeps it in range: OneCycle does not read the base at all
    _runner(lr, dict(policy='OneCycle'), opt=types.SimpleNamespace(base_lr=BASE, scheduled_momentum=True,
                                                                   initial_momentum=0.0, betas=(0.0, 0.999)))
    with pytest.raises(ValueError, match='scheduled_momentum'):
        _runner(lr, dict(policy='cyclic'), opt=types.SimpleNamespace(base_lr=BASE, scheduled_momentum=False))


def test_momentum_config_on_sgd_without_momentum_raises_in_train_model(tmp_path):
    z, tr, m, data, cfg = _setup(tmp_path)
    cfg['optimizer'] = dict(type='SGD', lr=0.1, momentum=0, weight_decay=5e-4)
    cfg['momentum_config'] = dict(policy='cyclic')
    with pytest.raises(ValueError, match='momentum=0'):
        train_model(m, data, cfg, device='cpu', use_graph=False)


# ---- without the flag nothing changes -----------------------------------------------------------------------------------

def test_optimizers_without_the_flag_are_what_they_were(tmp_path):
    for cfg in (dict(type='SGD', lr=0.1, momentum=0.9, nesterov=True), dict(type='AdamW', lr=1e-3),
                dict(type='SGD', lr=0.1, momentum=0.9, paramwise_cfg=dict(bias_lr_mult=2.))):
        opt = build_optimizer(D.FlatParams(Hand()), cfg)
        assert opt.scheduled_momentum is False and opt.hyper_t is None and opt.initial_momentum is None
        assert all('initial_momentum' not in g for g in opt.state_dict()['param_groups'])
        with pytest.raises(RuntimeError, match='scheduled_momentum=True'):
            opt.set_momentum(0.5)
    assert D.FlatSGD(D.FlatParams(Hand()), momentum=0.0, capturable=True).buf is None
    assert D.FlatSGD(D.FlatParams(Hand()), momentum=0.9, capturable=True, scheduled_momentum=True).buf is not None
    # a run without the new keys logs no momentum and builds the plain optimizer
    z, tr, m, data, cfg = _setup(tmp_path)
    cfg['checkpoint_config'] = None
    with D.kernels.use_ops(torch_ops):
        runner = train_model(m, data, cfg, device='cpu', use_graph=False)
    assert not runner.engine.opt.scheduled_momentum and runner.momentum_cfg is None
    assert all('momentum' not in r for r in runner.log)
    with pytest.raises(RuntimeError, match='scheduled_momentum=True'):
        runner.engine.step(torch.zeros(1), torch.zeros(1), momentum=0.5)
