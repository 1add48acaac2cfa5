"""CPU: Adam / AdamW and mmcv's paramwise_cfg on the flat buffers (train.FlatAdam, FlatSGD with a group table, paramwise.py)
on their torch-op path — through ``train_model`` against the real torch.optim classes, the parser rule by rule, the
torch-layout checkpoints both ways, resume, two gloo ranks, and the argument checks of the C entry points (no launch).

The error rule (shared with tests/test_optim_gpu.py): torch's own optimizer is the reference arithmetic.  From one start,
fp64 = torch.optim.X on float64 copies, ref32 = torch.optim.X(foreach=False) in fp32 on the CPU, ours.  Per quantity
(p, m, v) with scale_i = max(|x64_i|, floor):   max_i |ours_i - x64_i| / scale_i  <=  2 max_i |ref32_i - x64_i| / scale_i
+ K 2^-23, K the number of steps.  floor: the group's rate for p, the largest |g| seen for m, its square for v."""
import copy
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.nn as nn

import dsgcn_amd as D
import torch_ops
from dsgcn_amd import native
from dsgcn_amd.apis import EpochRunner, _BatchSource, epoch_indices, train_model
from dsgcn_amd.paramwise import param_rules
from dsgcn_amd.train import build_optimizer
from test_data_parallel import batch_for, make_model
from test_train_loop import _setup


def rule_sides(ours, ref32, x64, floor):
    """-> (ours' error, the reference's own fp32 error), both relative to max(|x64|, floor); floor a number or a tensor.
    Where the scale is 0 (an exact zero under a zero floor) only an exact zero has no error."""
    x64 = x64.detach().double().cpu().reshape(-1)
    scale = torch.maximum(x64.abs(), torch.as_tensor(floor, dtype=torch.float64).reshape(-1).expand_as(x64))

    def side(x):
        d = (x.detach().double().cpu().reshape(-1) - x64).abs()
        r = torch.where(scale > 0, d / scale.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, math.inf), d))
        return float(r.max()) if r.numel() else 0.0
    return side(ours), side(ref32)


def check_rule(what, ours, ref32, x64, floor, steps):
    a, b = rule_sides(ours, ref32, x64, floor)
    bound = 2 * b + steps * 2.0 ** -23
    print(f'error rule {what}: ours {a:.3e}  ref32 {b:.3e}  bound {bound:.3e}')
    assert a <= bound, (what, a, b, bound)
    return a, b


# ---- train_model with Adam / AdamW against torch.optim on the same model ---------------------------------------------

def _reference_run(model, data, cfg, make_opt, dtype, rates_of):
    """The loop train_model runs, driven by a real torch optimizer over ``model`` (a deepcopy): the same batches in the
    same sampler order, the same per-iteration rates written into the param groups."""
    model = model.to(dtype).train()
    opt = make_opt(model)
    for grp in opt.param_groups:
        grp['initial_lr'] = grp['lr']
    bs, n = cfg['data']['videos_per_gpu'], len(data)
    ipe = int(math.ceil(n / bs))
    total = cfg['total_epochs'] * ipe
    it = 0
    with D.kernels.use_ops(torch_ops):
        for ep in range(cfg['total_epochs']):
            order = epoch_indices(n, ep, cfg['seed'], 0, 1, True)
            for b in range(ipe):
                idx = order[b * bs:(b + 1) * bs]
                kp = torch.stack([torch.as_tensor(np.asarray(data[i]['keypoint']), dtype=dtype) for i in idx])
                lb = torch.as_tensor([data[i]['label'] for i in idx], dtype=torch.int64).view(-1, 1)
                for grp in opt.param_groups:
                    grp['lr'] = rates_of(grp['initial_lr'], it, total)
                opt.zero_grad(set_to_none=True)
                if dtype == torch.float32:                     # the step train_model takes
                    model.train_step(dict(keypoint=kp, label=lb), None, sync_log_vars=False)['loss'].backward()
                else:     # forward_train without its cast of the input to fp32: the float64 copy runs in float64
                    feat = model.extract_feat(kp[:, 0])
                    model.cls_head.loss(model.cls_head(feat), lb.squeeze(-1))['loss_cls'].backward()
                opt.step()
                it += 1
    return model, opt


def _cosine(base, it, total, min_lr=0.0):
    return min_lr + 0.5 * (base - min_lr) * (1 + math.cos(math.pi * it / total))


@pytest.mark.parametrize('kind', ['AdamW', 'Adam'])
def test_train_model_adam_matches_torch(tmp_path, kind):
    z, tr, m, data, cfg = _setup(tmp_path)
    cfg['optimizer'] = dict(type=kind, lr=1e-3, weight_decay=0.01)
    cls = getattr(torch.optim, kind)
    p0 = {k: p.detach().clone() for k, p in m.named_parameters()}
    m64, _ = _reference_run(copy.deepcopy(m), data, cfg, lambda mod: cls(mod.parameters(), lr=1e-3, weight_decay=0.01),
                            torch.float64, _cosine)
    m32, _ = _reference_run(copy.deepcopy(m), data, cfg,
                            lambda mod: cls(mod.parameters(), lr=1e-3, weight_decay=0.01, foreach=False), torch.float32,
                            _cosine)
    with D.kernels.use_ops(torch_ops):
        runner = train_model(m, data, cfg, device='cpu', use_graph=False)
    opt = runner.engine.opt
    assert isinstance(opt, D.FlatAdam) and opt.decoupled == (kind == 'AdamW') and opt.steps == 6 and runner.iter == 6
    assert [r['lr'] for r in runner.log] == [_cosine(1e-3, it, 6) for it in range(6)]
    P64, P32 = dict(m64.named_parameters()), dict(m32.named_parameters())
    worst = (0.0, 0.0)
    for k, p in m.named_parameters():
        a, b = rule_sides(p, P32[k], P64[k], 1e-3)
        assert a <= 2 * b + 6 * 2.0 ** -23, (k, a, b)
        worst = max(worst, (a, b))
    print(f'error rule {kind} train_model, worst parameter: ours {worst[0]:.3e}  ref32 {worst[1]:.3e}')
    # the parameters that never receive a gradient (quirk Q1: conv2_se) are where they started and have no state
    names = [k for k, _ in m.named_parameters()]
    dead = [k for k in names if 'conv2_se' in k]
    assert len(dead) >= 2
    state = opt.state_dict()['state']
    for k in dead:
        assert torch.equal(dict(m.named_parameters())[k], p0[k]), k
        assert names.index(k) not in state
    assert sum(1 for k in names if names.index(k) in state) == len(names) - len([i for i in range(len(names))
                                                                               if not opt._live(i)])
    moved = [k for k in names if k not in dead and not torch.equal(dict(m.named_parameters())[k], p0[k])]
    assert len(moved) > len(names) // 2


def test_train_model_adam_resume_continues_the_step_count(tmp_path):
    z, tr, m, data, cfg = _setup(tmp_path)
    cfg['optimizer'] = dict(type='AdamW', lr=1e-3, weight_decay=0.01)
    with D.kernels.use_ops(torch_ops):
        runner = train_model(m, data, cfg, device='cpu', use_graph=False)
    final = {k: v.clone() for k, v in m.state_dict().items()}
    ck = torch.load(tmp_path / 'epoch_1.pth', weights_only=False)['optimizer']
    assert {float(s['step']) for s in ck['state'].values()} == {3.0}
    assert len(ck['param_groups']) == 1 and ck['param_groups'][0]['initial_lr'] == 1e-3
    _, _, m2, data2, cfg2 = _setup(tmp_path / 'second', resume_from=str(tmp_path / 'epoch_1.pth'))
    cfg2['optimizer'] = dict(type='AdamW', lr=1e-3, weight_decay=0.01)
    with D.kernels.use_ops(torch_ops):
        r2 = train_model(m2, data2, cfg2, device='cpu', use_graph=False)
    assert r2.iter == 6 and r2.engine.opt.steps == 6 and len(r2.log) == 3
    for k, v in m2.state_dict().items():
        assert torch.equal(v, final[k]), k
    assert torch.equal(r2.engine.opt.m, runner.engine.opt.m) and torch.equal(r2.engine.opt.v, runner.engine.opt.v)


def test_train_model_rejects_what_is_not_implemented(tmp_path):
    z, tr, m, data, cfg = _setup(tmp_path)
    for opt, key in ((dict(type='Adam', amsgrad=True), 'amsgrad'), (dict(type='SGD', lr=0.1, dampening=0.5), 'dampening'),
                     (dict(type='AdamW', maximize=True), 'maximize'), (dict(type='SGD', lr=0.1, maximize=True), 'maximize'),
                     (dict(type='RMSprop', lr=0.1), 'RMSprop'),
                     (dict(type='SGD', lr=0.1, constructor='LayerDecayOptimizerConstructor'), 'constructor'),
                     (dict(type='SGD', lr=0.1, paramwise_cfg=dict(dcn_offset_lr_mult=0.1)), 'dcn_offset_lr_mult')):
        with pytest.raises(NotImplementedError, match=key):
            train_model(m, data, dict(cfg, optimizer=opt), device='cpu', use_graph=False)


# ---- the paramwise_cfg parser -----------------------------------------------------------------------------------------

class Hand(nn.Module):
    def __init__(self):
        super().__init__()
        self.alpha = nn.Parameter(torch.full((1,), 0.5))
        self.frozen = nn.Parameter(torch.ones(2), requires_grad=False)
        self.conv = nn.Conv2d(3, 4, 1, bias=True)
        self.dw = nn.Conv2d(4, 4, 3, padding=1, groups=4, bias=True)          # depthwise: groups == in_channels
        self.bn = nn.BatchNorm2d(4)
        self.gate_alpha = nn.Parameter(torch.zeros(3))

    def forward(self, x):
        return (self.bn(self.dw(self.conv(x))) * self.alpha).sum() + (self.gate_alpha * self.frozen.sum()).sum()


def _rules(mod, cfg, lr=0.1, wd=5e-4):
    return {r.name: (r.lr, r.weight_decay) for r in param_rules(mod, lr, wd, cfg)}


def test_paramwise_rules_on_a_hand_made_module():
    mod = Hand()
    names = [k for k, _ in mod.named_parameters()]
    assert [r.name for r in param_rules(mod, 0.1, 5e-4, {})] == names          # one rule per tensor, parameters() order
    assert [r.param is p for r, p in zip(param_rules(mod, 0.1, 5e-4, {}), mod.parameters())] == [True] * len(names)
    base = (0.1, 5e-4)
    assert set(_rules(mod, None).values()) == {base} and set(_rules(mod, {}).values()) == {base}
    got = _rules(mod, dict(bias_lr_mult=2., bias_decay_mult=0.5, norm_decay_mult=0., dwconv_decay_mult=0.25,
                           bypass_duplicate=True))
    assert got['conv.weight'] == base
    assert got['conv.bias'] == (0.1 * 2., 5e-4 * 0.5)
    assert got['dw.weight'] == (0.1, 5e-4 * 0.25)
    assert got['dw.bias'] == (0.1 * 2., 5e-4 * 0.25)            # the depthwise rule comes before the bias rule
    assert got['bn.weight'] == (0.1, 0.0)
    assert got['bn.bias'] == (0.1, 0.0)                         # a norm layer's bias: no bias_lr_mult, norm_decay_mult
    assert got['alpha'] == base and got['gate_alpha'] == base
    assert got['frozen'] == base                                # keeps its slot with the defaults
    # custom keys: the longest matching key wins, and a custom key overrides every other rule
    ck = {'alpha': dict(lr_mult=0.1, decay_mult=0.), 'gate_alpha': dict(lr_mult=3.), 'bn': dict(decay_mult=2.),
          'frozen': dict(lr_mult=7.)}
    got = _rules(mod, dict(custom_keys=ck, norm_decay_mult=0., bias_lr_mult=2.))
    assert got['alpha'] == (0.1 * 0.1, 0.0)
    assert got['gate_alpha'] == (0.1 * 3., 5e-4)                # 'gate_alpha' beats 'alpha'
    assert got['bn.weight'] == (0.1, 5e-4 * 2.) == got['bn.bias']        # not norm_decay_mult
    assert got['conv.bias'] == (0.1 * 2., 5e-4)
    assert got['frozen'] == base                                # requires_grad=False: no rule applies
    # same length: alphabetical order decides
    got = _rules(mod, dict(custom_keys={'bn.': dict(lr_mult=2.), 'bia': dict(lr_mult=5.)}))
    assert got['bn.bias'] == (0.1 * 5., 5e-4) and got['bn.weight'] == (0.1 * 2., 5e-4) and got['conv.bias'] == (0.1 * 5., 5e-4)
    # without weight_decay in the optimizer dict: rates still apply, decay multipliers raise
    got = {r.name: (r.lr, r.weight_decay) for r in param_rules(mod, 0.1, None, dict(bias_lr_mult=2.))}
    assert got['conv.bias'] == (0.2, None) and got['conv.weight'] == (0.1, None)


def test_paramwise_error_cases():
    mod = Hand()
    for bad in ('dcn_offset_lr_mult', 'layer_decay_rate', 'anything'):
        with pytest.raises(NotImplementedError, match=bad):
            param_rules(mod, 0.1, 5e-4, {bad: 0.1})
    with pytest.raises(TypeError, match='custom_keys'):
        param_rules(mod, 0.1, 5e-4, dict(custom_keys=['alpha']))
    with pytest.raises(TypeError):
        param_rules(mod, 0.1, 5e-4, ['norm_decay_mult'])
    for cfg in (dict(norm_decay_mult=0.), dict(bias_decay_mult=0.), dict(dwconv_decay_mult=0.),
                dict(custom_keys={'alpha': dict(decay_mult=0.)})):
        with pytest.raises(ValueError, match='base_wd should not be None'):
            param_rules(mod, 0.1, None, cfg)
    flat = D.FlatParams(mod)
    with pytest.raises(ValueError, match='base_wd should not be None'):
        build_optimizer(flat, dict(type='SGD', lr=0.1, paramwise_cfg=dict(norm_decay_mult=0.)))
    with pytest.raises(NotImplementedError, match='constructor'):
        build_optimizer(flat, dict(type='SGD', lr=0.1, constructor='Other'))


def test_paramwise_rules_on_the_reduced_model(tmp_path):
    z, tr, m, data, cfg = _setup(tmp_path)
    pw = dict(norm_decay_mult=0., custom_keys={'alpha': dict(decay_mult=0.)})             # the way out of quirk Q10
    rules = param_rules(m, 0.1, 5e-4, pw)
    mods = dict(m.named_modules())
    assert [r.name for r in rules] == [k for k, _ in m.named_parameters()]
    n_norm = n_alpha = 0
    for r in rules:
        owner = mods[r.name.rsplit('.', 1)[0]]
        if 'alpha' in r.name:
            n_alpha += 1
            assert (r.lr, r.weight_decay) == (0.1, 0.0), r.name
        elif isinstance(owner, nn.modules.batchnorm._BatchNorm):
            n_norm += 1
            assert (r.lr, r.weight_decay) == (0.1, 0.0), r.name
        else:
            assert (r.lr, r.weight_decay) == (0.1, 5e-4), r.name
    assert n_norm > 10 and n_alpha > 0
    opt = build_optimizer(D.FlatParams(m, gather=True), dict(type='SGD', lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True,
                                                            paramwise_cfg=pw))
    assert opt.table.base_lrs == [0.1, 0.1] and sorted(opt.table.wds) == [0.0, 5e-4]       # two device groups
    sd = opt.state_dict()
    assert len(sd['param_groups']) == len(rules) and all(g['initial_lr'] == 0.1 for g in sd['param_groups'])
    assert [g['params'] for g in sd['param_groups']] == [[i] for i in range(len(rules))]


# ---- SGD with paramwise_cfg against torch.optim.SGD over hand-built param groups ---------------------------------------

PW = dict(norm_decay_mult=0., bias_lr_mult=2., custom_keys={'alpha': dict(lr_mult=0.1, decay_mult=0.)})
LR_CFG = dict(policy='CosineAnnealing', min_lr=1e-3, by_epoch=False, warmup='linear', warmup_iters=4, warmup_ratio=0.1)


def _hand_groups(model, lr, wd):
    """The param groups mmcv builds for PW, written out by hand from the module tree."""
    mods = dict(model.named_modules())
    groups = []
    for k, p in model.named_parameters():
        owner, leaf = mods[k.rsplit('.', 1)[0]], k.rsplit('.', 1)[1]
        norm = isinstance(owner, nn.modules.batchnorm._BatchNorm)
        if 'alpha' in k:
            groups.append(dict(params=[p], lr=lr * 0.1, weight_decay=wd * 0.))
        elif norm:
            groups.append(dict(params=[p], lr=lr, weight_decay=wd * 0.))
        elif leaf == 'bias':
            groups.append(dict(params=[p], lr=lr * 2., weight_decay=wd))
        else:
            groups.append(dict(params=[p], lr=lr, weight_decay=wd))
    return groups


def _mmcv_rate(base, it, total):
    """CosineAnnealingLrUpdaterHook.get_lr(base) then LrUpdaterHook.get_warmup_lr, as mmcv writes them."""
    r = 1e-3 + 0.5 * (base - 1e-3) * (1 + math.cos(math.pi * it / total))
    if it < 4:
        r = r * (1 - (1 - it / 4) * (1 - 0.1))
    return r


def test_sgd_paramwise_matches_torch_sgd_over_hand_built_groups(tmp_path):
    z, tr, m, data, cfg = _setup(tmp_path)
    lr, wd = tr['lr'], tr['weight_decay']
    cfg['optimizer'] = dict(type='SGD', lr=lr, momentum=0.9, weight_decay=wd, nesterov=True, paramwise_cfg=PW)
    cfg['lr_config'] = LR_CFG
    cfg['checkpoint_config'] = None
    mk = lambda **kw: (lambda mod: torch.optim.SGD(_hand_groups(mod, lr, wd), lr=lr, momentum=0.9, weight_decay=wd,
                                                   nesterov=True, **kw))
    m64, _ = _reference_run(copy.deepcopy(m), data, cfg, mk(), torch.float64, _mmcv_rate)
    m32, o32 = _reference_run(copy.deepcopy(m), data, cfg, mk(foreach=False), torch.float32, _mmcv_rate)
    p0 = {k: p.detach().clone() for k, p in m.named_parameters()}
    engine = D.TrainEngine(m, optimizer=cfg['optimizer'], use_graph=False)
    opt = engine.opt
    assert isinstance(opt, D.FlatSGD) and opt.table is not None
    bases = opt.group_base_lrs
    assert sorted(set(bases)) == sorted({lr, lr * 2., lr * 0.1}) and bases[0] == lr
    runner = EpochRunner(m, engine, _BatchSource(data, torch.device('cpu')), cfg)
    seen, set_lr = [], opt.set_lr
    opt.set_lr = lambda rates: (seen.append(list(rates)), set_lr(rates))[1]
    with D.kernels.use_ops(torch_ops):
        runner.run()
    assert runner.iter == 6 and len(seen) == 6
    for it, rates in enumerate(seen):                          # exactly mmcv's numbers: not proportional to lr_mult
        assert rates == [_mmcv_rate(b, it, 6) for b in bases], it
        assert runner.log[it]['lr'] == _mmcv_rate(lr, it, 6)    # mmcv logs group 0
    assert seen[5][bases.index(lr * 0.1)] / seen[5][0] != pytest.approx(0.1, rel=1e-3)
    P64, P32 = dict(m64.named_parameters()), dict(m32.named_parameters())
    rule = {r.name: r for r in opt.rules}
    worst = (0.0, 0.0)
    for k, p in m.named_parameters():
        a, b = rule_sides(p, P32[k], P64[k], rule[k].lr)
        assert a <= 2 * b + 6 * 2.0 ** -23, (k, a, b)
        worst = max(worst, (a, b))
    print(f'error rule SGD paramwise train loop, worst parameter: ours {worst[0]:.3e}  ref32 {worst[1]:.3e}')
    for k in (k for k in p0 if 'conv2_se' in k):               # torch skips a .grad of None: no decay either
        assert torch.equal(dict(m.named_parameters())[k], p0[k]), k
    # the checkpoint lists what torch's own optimizer lists
    sd, tsd = opt.state_dict(), o32.state_dict()
    assert sorted(sd['state']) == sorted(tsd['state'])
    for a, b in zip(sd['param_groups'], tsd['param_groups']):
        assert a['params'] == b['params'] and a['weight_decay'] == b['weight_decay'] and a['lr'] == b['lr']
        assert a['initial_lr'] == b['initial_lr']
    del opt.set_lr                                             # (the recorder)
    with pytest.raises(ValueError, match='one rate per group'):
        opt.set_lr(0.05)


# ---- checkpoints in torch's layout, both ways ---------------------------------------------------------------------------

def _pair():
    torch.manual_seed(0)
    net, ref = Hand(), Hand()
    ref.load_state_dict(net.state_dict())
    return net, ref, torch.randn(5, 3, 4, 4)


def _torch_groups(mod, rules):
    by = {id(r.param): r for r in rules}
    return [dict(params=[p], lr=by[id(p)].lr, weight_decay=by[id(p)].weight_decay) for p in mod.parameters()]


@pytest.mark.parametrize('kind', ['SGD', 'Adam', 'AdamW'])
def test_state_dict_round_trip_with_torch(kind):
    net, ref, x = _pair()
    pw = dict(norm_decay_mult=0., bias_lr_mult=2., custom_keys={'alpha': dict(lr_mult=0.1)})
    extra = dict(momentum=0.9, nesterov=True) if kind == 'SGD' else dict(betas=(0.8, 0.99), eps=1e-6)
    cfg = dict(type=kind, lr=0.01, weight_decay=0.02, paramwise_cfg=pw, **extra)
    opt = build_optimizer(D.FlatParams(net), cfg)
    rules_ref = param_rules(ref, 0.01, 0.02, pw)
    mk = lambda mod, rules, **kw: getattr(torch.optim, kind)(_torch_groups(mod, rules), lr=0.01, weight_decay=0.02,
                                                             **extra, **kw)
    topt = mk(ref, rules_ref, foreach=False)
    assert opt.state_dict()['state'] == {}
    for _ in range(2):
        for mod, o in ((net, opt), (ref, topt)):
            o.zero_grad()
            mod(x).backward()
            o.step()
    sd = opt.state_dict()
    assert 1 not in sd['state'] and len(sd['param_groups']) == 9            # slot 1 = `frozen`: a group, no state
    assert all('initial_lr' in g for g in sd['param_groups'])
    # ours -> torch: a fresh torch optimizer over a copy of our model continues like ours
    cont = copy.deepcopy(net)
    for p in cont.parameters():
        p.grad = None
    c64 = copy.deepcopy(cont).double()
    t32, t64 = mk(cont, param_rules(cont, 0.01, 0.02, pw), foreach=False), mk(c64, param_rules(c64, 0.01, 0.02, pw))
    t32.load_state_dict(copy.deepcopy(sd))
    sd64 = copy.deepcopy(sd)
    for st in sd64['state'].values():
        for k in st:
            st[k] = st[k].double()
    t64.load_state_dict(sd64)
    # torch -> ours: a fresh flat optimizer takes torch's dict
    net2 = copy.deepcopy(net)
    opt2 = build_optimizer(D.FlatParams(net2), cfg)
    opt2.load_state_dict(copy.deepcopy(t32.state_dict()))
    if kind != 'SGD':
        assert opt2.steps == 2 and torch.equal(opt2.m, opt.m) and torch.equal(opt2.v, opt.v)
        sd_int = copy.deepcopy(sd)
        for st in sd_int['state'].values():
            st['step'] = 2                                     # an int is accepted as well as a tensor
        opt2.load_state_dict(sd_int)
        assert opt2.steps == 2
    else:
        assert torch.equal(opt2.buf, opt.buf)
    for mod, o, xx in ((net, opt, x), (net2, opt2, x), (cont, t32, x), (c64, t64, x.double())):
        o.zero_grad()
        mod(xx).backward()
        o.step()
    assert torch.equal(net2.alpha, net.alpha) and torch.equal(opt2.flat.flat_p, opt.flat.flat_p)
    P32, P64 = dict(cont.named_parameters()), dict(c64.named_parameters())
    rule = {r.name: r for r in opt.rules}
    for k, p in net.named_parameters():
        check_rule(f'{kind} after reload {k}', p, P32[k], P64[k], rule[k].lr, 1)
    assert torch.equal(net.frozen, torch.ones(2))


def test_load_state_dict_refuses_rates_that_split_a_group():
    """Two tensors of one device group with different saved rates: written under another paramwise_cfg."""
    net, _, _ = _pair()
    opt = build_optimizer(D.FlatParams(net), dict(type='AdamW', lr=0.01, weight_decay=0.02,
                                                  paramwise_cfg=dict(bias_lr_mult=2.)))
    sd = opt.state_dict()
    opt.load_state_dict(copy.deepcopy(sd))
    names = [k for k, _ in net.named_parameters()]
    sd['param_groups'][names.index('conv.weight')]['lr'] = 0.5          # conv.weight and dw.weight share a group
    with pytest.raises(ValueError, match='conv.weight|dw.weight'):
        opt.load_state_dict(sd)


def test_sgd_without_paramwise_cfg_is_the_plain_flat_sgd():
    """The shipped configs: no group table, the launches and the bits of FlatSGD as it was constructed before."""
    torch.manual_seed(0)
    a_net = nn.Sequential(nn.Linear(5, 4), nn.Linear(4, 3))
    b_net = copy.deepcopy(a_net)
    x = torch.randn(6, 5)
    a = build_optimizer(D.FlatParams(a_net), dict(type='SGD', lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True),
                        grad_clip=dict(max_norm=0.5))
    b = D.FlatSGD(D.FlatParams(b_net), lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True, capturable=True,
                  grad_clip=dict(max_norm=0.5))
    assert type(a) is D.FlatSGD and a.table is None and not hasattr(a, 'rules') and not a.flat.grad_observers
    assert a.group_base_lrs is None and b.group_base_lrs is None
    for it in range(3):
        for mod, o in ((a_net, a), (b_net, b)):
            o.set_lr(0.1 / (it + 1))
            o.zero_grad()
            mod(x).square().sum().backward()
            o.step()
    assert torch.equal(a.flat.flat_p, b.flat.flat_p) and torch.equal(a.buf, b.buf) and torch.equal(a.grad_norm, b.grad_norm)
    assert a.state_dict()['param_groups'] == b.state_dict()['param_groups']
    eng = D.TrainEngine(make_model(3), optimizer=dict(type='SGD', lr=0.1, momentum=0.9), use_graph=False)
    assert type(eng.opt) is D.FlatSGD and eng.opt.table is None


def test_gradient_pattern_is_fixed_at_the_first_step():
    m = make_model(3)
    eng = D.TrainEngine(m, optimizer=dict(type='Adam', lr=1e-3), use_graph=False)
    b = batch_for(0)
    with D.kernels.use_ops(torch_ops):
        eng.step(b['keypoint'], b['label'])
    live = list(eng.opt.table.live)
    assert not all(live) and any(live)
    flat = eng.flat
    flat.zero_grad()
    for p, alive in zip(flat.params, live):
        p.grad = torch.zeros_like(p) if alive else None
    flat.collect_grads()                                       # the same pattern: fine
    flat.zero_grad()
    for p in flat.params:
        p.grad = torch.zeros_like(p)
    with pytest.raises(RuntimeError, match='receive a gradient changed'):
        flat.collect_grads()


# ---- two ranks ----------------------------------------------------------------------------------------------------------

def _adamw_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(1)
    model = make_model(seed=7 + rank)
    eng = D.TrainEngine(model, optimizer=dict(type='AdamW', lr=1e-3, weight_decay=0.01,
                                              paramwise_cfg=dict(norm_decay_mult=0.)),
                        use_graph=False, grad_clip=dict(max_norm=1e-3))
    b = batch_for(rank)
    norms, local = [], []
    with D.kernels.use_ops(torch_ops):
        for _ in range(2):
            logs = eng.step(b['keypoint'], b['label'], lr=[1e-3] * len(eng.opt.group_base_lrs))
            norms.append(float(logs['grad_norm']))
            local.append(float(logs['loss']))
    torch.save(dict(p=eng.flat.flat_p.clone(), m=eng.opt.m.clone(), v=eng.opt.v.clone(), norms=norms, local=local,
                    steps=eng.opt.steps), os.path.join(out_dir, f'r{rank}.pt'))
    dist.destroy_process_group()


def test_two_ranks_adamw_with_clip_end_alike(tmp_path):
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_adamw_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = [torch.load(tmp_path / f'r{r}.pt', weights_only=False) for r in range(2)]
    assert r0['local'] != r1['local']
    assert r0['norms'] == r1['norms'] and all(n > 1e-3 for n in r0['norms'])
    assert torch.equal(r0['p'], r1['p']) and torch.equal(r0['m'], r1['m']) and torch.equal(r0['v'], r1['v'])
    assert r0['steps'] == r1['steps'] == 2


# ---- the C ABI: argument checks before any launch -----------------------------------------------------------------------

NEW = ('dsgcn_optim_chunks', 'dsgcn_optim_table', 'dsgcn_sgd_group_step', 'dsgcn_sgd_group_step_clip', 'dsgcn_adam_step',
       'dsgcn_adam_step_clip')


def test_new_entry_points_are_declared_and_bound():
    from test_native_abi import declared_symbols
    assert set(NEW) <= set(declared_symbols()) and set(NEW) <= set(native.SIGNATURES)


def test_optim_table_is_checked_and_filled_on_the_host():
    lib = native.lib()
    assert [lib.dsgcn_optim_chunks(n) for n in (1, 4095, 4096, 4097, 1376950)] == [1, 1, 2, 2, 337]
    assert lib.dsgcn_optim_chunks(0) == -1 and lib.dsgcn_optim_chunks(-3) == -1 and lib.dsgcn_optim_chunks(2 ** 31) == -2

    def table(ends, group, wd, n, groups=None):
        ends, group = np.array(ends, dtype=np.int32), np.array(group, dtype=np.int32)
        wd = np.array(wd, dtype=np.float64)
        first = np.full(max(n, 1) // 4096 + 2, -7, dtype=np.int32)
        rc = lib.dsgcn_optim_table(ends.ctypes.data, group.ctypes.data, len(ends), wd.ctypes.data,
                                   len(wd) if groups is None else groups, n, first.ctypes.data)
        return rc, first.tolist()
    assert table([1, 2, 4096, 4097, 9000], [0, 1, -1, 0, 1], [0., 5e-4], 9000) == (0, [0, 3, 4, 4])
    assert table([3], [0], [0.], 3) == (0, [0, 0])
    assert table([4096], [0], [0.], 4096) == (0, [0, 0, 0])
    for bad in (dict(ends=[1, 1, 5]), dict(ends=[2, 1, 5]), dict(ends=[1, 2, 4]), dict(ends=[0, 2, 5]),
                dict(group=[0, 2, 0]), dict(group=[0, -2, 0]), dict(wd=[0., -1e-4]), dict(wd=[0., float('nan')]),
                dict(wd=[0., float('inf')]), dict(n=0), dict(groups=0)):
        a = dict(dict(ends=[1, 2, 5], group=[0, 1, -1], wd=[0., 1e-4], n=5), **bad)
        assert table(**a)[0] == -1, bad
    assert table([5], [0], [0.] * 257, 5)[0] == -2
    P = 4096
    assert lib.dsgcn_optim_table(None, P, 1, P, 1, 5, P) == -1 and lib.dsgcn_optim_table(P, P, 1, P, 1, 5, None) == -1


def test_update_entry_points_reject_bad_arguments_without_gpu():
    lib = native.lib()
    P = 4096                                              # any aligned non-NULL address: rejected before it is touched
    tab = dict(ends=P, group=P, first=P, ntens=2, lr=P, wd=P, groups=2)
    clip = dict(partial=P, rows=1, norm_type=2, max_norm=1.0, out=P)

    def sgd(clipped, **kw):
        a = dict(dict(p=P, g=P, buf=P, mom=0.9, nesterov=1, n=8, **tab, **clip), **kw)
        head = (a['p'], a['g'], a['buf'], a['ends'], a['group'], a['first'], a['ntens'], a['lr'], a['wd'], a['groups'])
        if clipped:
            return lib.dsgcn_sgd_group_step_clip(*head, a['partial'], a['rows'], a['norm_type'], a['max_norm'], a['out'],
                                                 a['mom'], a['nesterov'], a['n'], None)
        return lib.dsgcn_sgd_group_step(*head, a['mom'], a['nesterov'], a['n'], None)

    def adam(clipped, **kw):
        a = dict(dict(p=P, g=P, m=P, v=P, step=P, b1=0.9, b2=0.999, eps=1e-8, decoupled=1, n=8, **tab, **clip), **kw)
        head = (a['p'], a['g'], a['m'], a['v'], a['step'], a['ends'], a['group'], a['first'], a['ntens'], a['lr'], a['wd'],
                a['groups'])
        tail = (a['b1'], a['b2'], a['eps'], a['decoupled'], a['n'], None)
        if clipped:
            return lib.dsgcn_adam_step_clip(*head, a['partial'], a['rows'], a['norm_type'], a['max_norm'], a['out'], *tail)
        return lib.dsgcn_adam_step(*head, *tail)

    nan = float('nan')
    common = [dict(p=None), dict(g=None), dict(ends=None), dict(group=None), dict(first=None), dict(lr=None), dict(wd=None),
              dict(p=P + 4), dict(g=P + 8), dict(ends=P + 2), dict(lr=P + 4), dict(wd=P + 4), dict(n=0), dict(n=-1),
              dict(ntens=0), dict(ntens=9), dict(groups=0), dict(groups=-1)]
    clipbad = [dict(partial=None), dict(out=None), dict(rows=0), dict(norm_type=1), dict(norm_type=3), dict(max_norm=-1.0),
               dict(max_norm=nan), dict(partial=P + 4)]
    for clipped in (False, True):
        for bad in common + (clipbad if clipped else []):
            assert sgd(clipped, **bad) == -1, (clipped, bad)
            assert adam(clipped, **bad) == -1, (clipped, bad)
        assert sgd(clipped, groups=257) == -2 and adam(clipped, groups=257) == -2
        assert sgd(clipped, n=2 ** 31) == -2 and adam(clipped, n=2 ** 31) == -2
        for bad in (dict(buf=None), dict(mom=-0.1), dict(mom=nan), dict(buf=P + 4)):
            assert sgd(clipped, **bad) == -1, bad
        for bad in (dict(m=None), dict(v=None), dict(step=None), dict(m=P + 4), dict(v=P + 4), dict(step=P + 2), dict(b1=1.0),
                    dict(b1=-0.1), dict(b2=1.0), dict(b2=nan), dict(eps=-1e-8), dict(eps=nan)):
            assert adam(clipped, **bad) == -1, bad
