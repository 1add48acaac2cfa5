"""CPU: gradient clipping by total norm (mmcv ``optimizer_config.grad_clip`` = torch.nn.utils.clip_grad_norm_ before the
optimizer step) on FlatSGD's torch path, mmcv's LR warm-up in the epoch loop, both through ``train_model``, the 2-rank
gloo path, and the argument checks of the three C entry points (no launch)."""
import math
import os
import socket
import types

import pytest
import torch

import dsgcn_amd as D
import torch_ops
from dsgcn_amd import native
from dsgcn_amd.apis import EpochRunner, train_model
from test_data_parallel import batch_for, make_model
from test_train_loop import _setup

INF = float('inf')


def _two_linear():
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(5, 4), torch.nn.Linear(4, 3))
    ref = torch.nn.Sequential(torch.nn.Linear(5, 4), torch.nn.Linear(4, 3))
    ref.load_state_dict(net.state_dict())
    return net, ref, torch.randn(6, 5)


def _measured_norm(norm_type):
    net, _, x = _two_linear()
    net(x).square().sum().backward()
    return float(torch.nn.utils.clip_grad_norm_(net.parameters(), 1e30, norm_type=norm_type))


@pytest.mark.parametrize('capturable', [True, False])
@pytest.mark.parametrize('scale', [0.5, 2.0])          # max_norm below / above the norm of the first gradient
@pytest.mark.parametrize('norm_type', [2, INF])
def test_flat_sgd_clip_matches_torch(norm_type, scale, capturable):
    """FlatSGD(grad_clip=...) == clip_grad_norm_ + torch.optim.SGD on a copy: three steps with a changing rate."""
    max_norm = scale * _measured_norm(norm_type)
    net, ref, x = _two_linear()
    flat = D.FlatParams(net)
    opt = D.FlatSGD(flat, lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True, capturable=capturable,
                    grad_clip=dict(max_norm=max_norm, norm_type=norm_type))
    topt = torch.optim.SGD(ref.parameters(), lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True)
    norm_ptr = opt.grad_norm.data_ptr()                      # allocated by the constructor, never re-homed
    clipped = []
    for it in range(3):
        lr = D.cosine_lr(0.1, it, 4)
        opt.set_lr(lr)
        topt.param_groups[0]['lr'] = lr
        opt.zero_grad()
        net(x).square().sum().backward()
        opt.step()
        topt.zero_grad()
        ref(x).square().sum().backward()
        total = torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm, norm_type=norm_type)
        topt.step()
        clipped.append(float(total) > max_norm)
        assert abs(float(opt.grad_norm) - float(total)) <= 1e-6 * float(total), (it, float(opt.grad_norm), float(total))
        # clip_grad_norm_ leaves the clipped values in .grad; the flat buffer holds them too
        for a, b in zip(net.parameters(), ref.parameters()):
            assert torch.allclose(a.grad, b.grad, rtol=1e-6, atol=1e-7)
    assert opt.grad_norm.data_ptr() == norm_ptr and flat.check_views()
    assert clipped[0] == (scale < 1)
    for a, b in zip(net.parameters(), ref.parameters()):
        assert torch.allclose(a, b, atol=1e-6)
    # no optimizer state is added: the checkpoint layout is torch SGD's
    assert set(opt.state_dict()) == {'state', 'param_groups'}
    assert set(opt.state_dict()['state'][0]) == {'momentum_buffer'}


def test_grad_clip_none_is_the_plain_step():
    net, ref, x = _two_linear()
    a = D.FlatSGD(D.FlatParams(net), lr=0.1, capturable=True, grad_clip=None)
    b = D.FlatSGD(D.FlatParams(ref), lr=0.1, capturable=True)
    assert a.clip is None and a.grad_norm is None and a.clip_partial is None
    for model, o in ((net, a), (ref, b)):
        o.zero_grad()
        model(x).square().sum().backward()
        o.step()
    assert torch.equal(a.flat.flat_p, b.flat.flat_p)


def test_grad_clip_arguments():
    net, _, _ = _two_linear()
    flat = D.FlatParams(net)
    for nt, code in ((2, 2), (2.0, 2), (INF, 0), ('inf', 0)):
        assert D.FlatSGD(flat, grad_clip=dict(max_norm=1.0, norm_type=nt)).clip == (1.0, code)
    assert D.FlatSGD(flat, grad_clip=dict(max_norm=45)).clip == (45.0, 2)       # norm_type defaults to 2
    with pytest.raises(NotImplementedError, match='norm_type'):
        D.FlatSGD(flat, grad_clip=dict(max_norm=1.0, norm_type=3))
    with pytest.raises(NotImplementedError, match='norm_type'):
        D.FlatSGD(flat, grad_clip=dict(max_norm=1.0, norm_type='fro'))
    with pytest.raises(ValueError, match='max_norm'):
        D.FlatSGD(flat, grad_clip=dict(norm_type=2))
    with pytest.raises(NotImplementedError, match='norm_type'):
        D.TrainEngine(net, grad_clip=dict(max_norm=1.0, norm_type=1))


# ---- warm-up ------------------------------------------------------------------------------------------------------------

BASE, SAMPLES, BATCH, EPOCHS = 0.1, 12, 4, 3          # 3 iterations per epoch, 9 in all


def _runner(lr_config):
    engine = types.SimpleNamespace(opt=types.SimpleNamespace(base_lr=BASE))
    cfg = dict(data=dict(videos_per_gpu=BATCH), total_epochs=EPOCHS, lr_config=lr_config)
    return EpochRunner(None, engine, list(range(SAMPLES)), cfg)


def _rates(runner):
    out = []
    for it in range(runner.max_iters):
        runner.iter, runner.epoch = it, it // runner.iters_per_epoch
        out.append(runner.current_lr())
    return out


def _regular(policy, it, max_iters, ipe):
    if policy == 'CosineAnnealing':
        return 0.0 + 0.5 * (BASE - 0.0) * (1 + math.cos(math.pi * it / max_iters))
    return BASE * 0.1 ** ((it // ipe) // 2)                  # step=2: x0.1 from epoch 2 on


def _table(policy, mode, warmup_iters, ratio, max_iters=9, ipe=3):
    rows = []
    for it in range(max_iters):
        r = _regular(policy, it, max_iters, ipe)
        if it < warmup_iters:
            if mode == 'constant':
                r = r * ratio
            elif mode == 'linear':
                r = r * (1 - (1 - it / warmup_iters) * (1 - ratio))
            else:
                r = r * ratio ** (1 - it / warmup_iters)
        rows.append(r)
    return rows


POLICIES = {'CosineAnnealing': dict(policy='CosineAnnealing', min_lr=0, by_epoch=False), 'step': dict(policy='step', step=2)}


@pytest.mark.parametrize('policy', ['CosineAnnealing', 'step'])
@pytest.mark.parametrize('mode', ['constant', 'linear', 'exp'])
def test_warmup_rates_follow_mmcv(policy, mode):
    runner = _runner(dict(POLICIES[policy], warmup=mode, warmup_iters=4, warmup_ratio=0.1))
    assert runner.iters_per_epoch == 3 and runner.max_iters == 9
    got, want = _rates(runner), _table(policy, mode, 4, 0.1)
    assert got == want                                       # the same Python-float expressions: exact
    plain = _rates(_runner(dict(POLICIES[policy])))
    assert got[4:] == plain[4:]                              # iteration warmup_iters carries the regular rate
    assert all(a < b for a, b in zip(got[:4], plain[:4]))
    if mode == 'constant':
        assert got[0] == plain[0] * 0.1
    # warmup_ratio defaults to 0.1
    assert _rates(_runner(dict(POLICIES[policy], warmup=mode, warmup_iters=4))) == want


@pytest.mark.parametrize('policy', ['CosineAnnealing', 'step'])
def test_warmup_by_epoch(policy):
    """warmup_by_epoch: warmup_iters counts epochs, mmcv converts with the epoch length (3 iterations here)."""
    runner = _runner(dict(POLICIES[policy], warmup='linear', warmup_iters=2, warmup_ratio=0.25, warmup_by_epoch=True))
    assert runner.warmup_iters == 6
    assert _rates(runner) == _table(policy, 'linear', 6, 0.25)


def test_warmup_arguments():
    with pytest.raises(ValueError, match='warming up'):
        _runner(dict(POLICIES['step'], warmup='cosine', warmup_iters=4))
    with pytest.raises(ValueError):
        _runner(dict(POLICIES['step'], warmup='linear', warmup_iters=0))
    assert _runner(dict(POLICIES['step'], warmup=None)).warmup is None


# ---- both options through train_model -----------------------------------------------------------------------------------

def _clip_cfg(cfg):
    cfg['optimizer_config'] = dict(grad_clip=dict(max_norm=45, norm_type=2))
    cfg['lr_config'] = dict(policy='CosineAnnealing', min_lr=0, by_epoch=False, warmup='linear', warmup_iters=4,
                            warmup_ratio=0.1)
    return cfg


def test_train_model_with_grad_clip_and_warmup_cpu(tmp_path):
    """The reference's commented-in schedule line (grad_clip=dict(max_norm=45, norm_type=2)) plus a linear warm-up on the
    tiny dataset: the run logs a finite grad_norm per interval and walks the warm-up table; a run resumed from the
    checkpoint of epoch 1 (iteration 3 of a 4-iteration warm-up) continues the table and ends at the same weights."""
    z, tr, m, data, cfg = _setup(tmp_path)
    with D.kernels.use_ops(torch_ops):
        runner = train_model(m, data, _clip_cfg(cfg), device='cpu', use_graph=False)
    assert runner.iter == 6 and len(runner.log) == 6
    assert all(math.isfinite(r['grad_norm']) and r['grad_norm'] > 0 for r in runner.log)
    want = []
    for it in range(6):
        r = 0.0 + 0.5 * (tr['lr'] - 0.0) * (1 + math.cos(math.pi * it / 6))
        want.append(r * (1 - (1 - it / 4) * (1 - 0.1)) if it < 4 else r)
    assert [r['lr'] for r in runner.log] == want
    final = {k: v.clone() for k, v in m.state_dict().items()}
    _, _, m2, data2, cfg2 = _setup(tmp_path / 'second', resume_from=str(tmp_path / 'epoch_1.pth'))
    with D.kernels.use_ops(torch_ops):
        r2 = train_model(m2, data2, _clip_cfg(cfg2), device='cpu', use_graph=False)
    assert r2.iter == 6 and [r['lr'] for r in r2.log] == want[3:]
    assert [r['grad_norm'] for r in r2.log] == [r['grad_norm'] for r in runner.log[3:]]
    for k, v in m2.state_dict().items():
        assert torch.equal(v, final[k]), k


def test_train_model_clip_changes_the_run_cpu(tmp_path):
    """A max_norm far below the gradient norm: every step is clipped, so the weights differ from the unclipped run."""
    z, tr, m, data, cfg = _setup(tmp_path, total_epochs=1)
    cfg['optimizer_config'] = dict(grad_clip=dict(max_norm=1e-3, norm_type='inf'))
    cfg['checkpoint_config'] = None
    with D.kernels.use_ops(torch_ops):
        runner = train_model(m, data, cfg, device='cpu', use_graph=False)
    assert all(r['grad_norm'] > 1e-3 for r in runner.log)
    _, _, m2, data2, cfg2 = _setup(tmp_path / 'b', total_epochs=1)
    cfg2['checkpoint_config'] = None
    with D.kernels.use_ops(torch_ops):
        r2 = train_model(m2, data2, cfg2, device='cpu', use_graph=False)
    assert 'grad_norm' not in r2.log[0]
    assert not torch.equal(runner.engine.flat.flat_p, r2.engine.flat.flat_p)
    # (the first loss is computed before any update: the two runs start alike)
    assert [r['loss'] for r in runner.log][0] == [r['loss'] for r in r2.log][0]


# ---- two ranks ----------------------------------------------------------------------------------------------------------

def _clip_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(1)
    model = make_model(seed=7 + rank)                    # the wrap-time broadcast makes the replicas equal
    eng = D.TrainEngine(model, lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True, use_graph=False,
                        grad_clip=dict(max_norm=1e-3))
    b = batch_for(rank)                                  # another batch per rank: the local gradients differ
    norms, local = [], []
    with D.kernels.use_ops(torch_ops):
        for _ in range(2):
            logs = eng.step(b['keypoint'], b['label'], lr=0.1)
            norms.append(float(logs['grad_norm']))
            local.append(float(logs['loss']))
    torch.save(dict(p=eng.flat.flat_p.clone(), g=eng.flat.flat_g.clone(), norms=norms, local=local),
               os.path.join(out_dir, f'r{rank}.pt'))
    dist.destroy_process_group()


def test_two_ranks_clip_the_averaged_gradient_alike(tmp_path):
    """Clipping runs after the all-reduce on a buffer every rank holds alike, in a fixed order: the same grad_norm and
    bit-identical parameters on both ranks after two clipped steps, without a second collective."""
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_clip_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = [torch.load(tmp_path / f'r{r}.pt', weights_only=False) for r in range(2)]
    assert r0['local'] != r1['local']                    # the ranks did see different batches
    assert r0['norms'] == r1['norms'] and all(n > 1e-3 for n in r0['norms'])
    assert torch.equal(r0['p'], r1['p']) and torch.equal(r0['g'], r1['g'])
    # the buffer both hold is the clipped one: its norm is max_norm (up to the 1e-6 of the coefficient's denominator)
    assert float(r0['g'].double().norm()) == pytest.approx(1e-3, rel=1e-2)


# ---- the C ABI: argument checks before any launch -----------------------------------------------------------------------

def test_clip_entry_points_reject_bad_arguments_without_gpu():
    lib = native.lib()
    assert lib.dsgcn_grad_norm_rows(0) == -1 and lib.dsgcn_grad_norm_rows(-5) == -1
    # fixed by n alone: one row per 8192-element slice
    assert [lib.dsgcn_grad_norm_rows(n) for n in (1, 8192, 8193, 1376950)] == [1, 1, 2, 169]
    P = 4096                                              # any aligned non-NULL address: rejected before it is touched
    assert lib.dsgcn_grad_norm_partials(None, 8, 2, P, None) == -1
    assert lib.dsgcn_grad_norm_partials(P, 8, 2, None, None) == -1
    assert lib.dsgcn_grad_norm_partials(P, 0, 2, P, None) == -1
    assert lib.dsgcn_grad_norm_partials(P, 8, 1, P, None) == -1
    assert lib.dsgcn_grad_norm_partials(P, 8, 3, P, None) == -1
    assert lib.dsgcn_grad_norm_partials(P + 4, 8, 2, P, None) == -1         # g not 16-byte aligned
    good = dict(p=P, g=P, buf=P, lr=P, partial=P, rows=1, norm_type=2, max_norm=1.0, out=P, mom=0.9, wd=5e-4, nesterov=1, n=8)

    def call(**kw):
        a = dict(good, **kw)
        return lib.dsgcn_sgd_step_clip(a['p'], a['g'], a['buf'], a['lr'], a['partial'], a['rows'], a['norm_type'], a['max_norm'],
                                       a['out'], a['mom'], a['wd'], a['nesterov'], a['n'], None)
    for bad in (dict(p=None), dict(g=None), dict(lr=None), dict(partial=None), dict(out=None), dict(buf=None), dict(n=0),
                dict(n=-1), dict(rows=0), dict(norm_type=1), dict(norm_type=3), dict(max_norm=-1.0),
                dict(max_norm=float('nan')), dict(p=P + 4)):
        assert call(**bad) == -1, bad
