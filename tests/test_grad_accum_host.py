"""CPU: gradient accumulation (mmcv GradientCumulativeOptimizerHook) on TrainEngine's torch path — k micro-batches on one
device are the reference's k ranks —, its tail rule, its per-micro-iteration state, the config key in ``train_model`` and
the two new C entry points (symbols and argument checks, no launch)."""
import ctypes
import logging
import math
import os

import pytest
import torch

import dsgcn_amd as D
import torch_ops
from dsgcn_amd import native
from dsgcn_amd.apis import parse_optimizer_config, train_model
from grad_accum_fp64 import SGD, grouped, host_statement, micro_batches, reduced_model, running_stats
from test_train_loop import _setup


def _engine(k, **kw):
    return D.TrainEngine(reduced_model(), use_graph=False, accumulate=k, **dict(SGD, **kw))


def _assert_equals_statement(eng, want):
    for name, p in eng.model.named_parameters():
        assert torch.equal(p.detach(), want['p'][name]), name
    for (name, _), (off, n) in zip(eng.model.named_parameters(), eng.flat.slices):
        assert torch.equal(eng.opt.buf[off:off + n], want['buf'][name].reshape(-1)), name


def test_two_micro_batches_are_two_virtual_ranks():
    """k = 2, two 2-clip micro-batches: parameters and momentum after the two calls are those of the hand-written loop —
    two passes under their own batch statistics, (g1 + g2) * 0.5, one torch.optim.SGD(nesterov=True) step.  Same
    operations in the same order: equal, not close."""
    batches = micro_batches(2)
    eng = _engine(2)
    p0 = eng.flat.flat_p.clone()
    with D.kernels.use_ops(torch_ops):
        eng.step(*batches[0])
        assert torch.equal(eng.flat.flat_p, p0) and eng.pending == 1 and not eng.opt.buf.any()    # no update yet
        eng.step(*batches[1])
    assert eng.pending == 0 and not eng.opt.acc.any() and not torch.equal(eng.flat.flat_p, p0)
    want = host_statement(batches, [[0, 1]])
    _assert_equals_statement(eng, want)
    # ... and it is not the 4-clip batch (other BatchNorm statistics) nor an update per call
    big = D.TrainEngine(reduced_model(), use_graph=False, **SGD)
    each = D.TrainEngine(reduced_model(), use_graph=False, **SGD)
    with D.kernels.use_ops(torch_ops):
        big.step(torch.cat([batches[0][0], batches[1][0]]), torch.cat([batches[0][1], batches[1][1]]))
        each.step(*batches[0])
        each.step(*batches[1])
    assert not torch.equal(big.flat.flat_p, eng.flat.flat_p) and not torch.equal(each.flat.flat_p, eng.flat.flat_p)


def test_accumulation_is_the_two_rank_data_parallel_recipe():
    """test_data_parallel.py's recipe — rank r's batch on rank 0's weights, gradients summed by the collective and scaled
    by 1 / world (FlatDataParallel.allreduce_grads over gloo), FlatSGD step, twice — stated in one process, against
    accumulate=2 over the same four batches."""
    from test_data_parallel import batch_for, make_model
    torch.set_num_threads(1)
    world = 2
    model = make_model(seed=7)
    flat = D.FlatParams(model, gather=True)
    opt = D.FlatSGD(flat, **SGD)
    with D.kernels.use_ops(torch_ops):
        for _ in range(2):
            local = []
            for r in range(world):
                opt.zero_grad()
                b = batch_for(r)
                model.train_step(b, None, sync_log_vars=False)['loss'].backward()
                flat.collect_grads()
                local.append(flat.flat_g.clone())
            flat.flat_g.copy_(local[0] + local[1])          # all_reduce(SUM)
            flat.flat_g.mul_(1.0 / world)
            opt.step()
        eng = D.TrainEngine(make_model(seed=7), use_graph=False, accumulate=world, **SGD)
        for _ in range(2):
            for r in range(world):
                b = batch_for(r)
                eng.step(b['keypoint'], b['label'])
    assert eng.iter == 4
    assert torch.equal(eng.flat.flat_p, flat.flat_p) and torch.equal(eng.opt.buf, opt.buf)


def test_tail_group_is_divided_by_its_own_length():
    """k = 4, 6 iterations: one full group, then flush(2) updates on (g5 + g6) * 0.5."""
    batches = micro_batches(6)
    eng = _engine(4)
    with D.kernels.use_ops(torch_ops):
        for b in batches:
            eng.step(*b)
        assert eng.pending == 2
        with pytest.raises(ValueError, match='holds 2'):
            eng.flush(3)
        eng.flush(2)
    assert eng.pending == 0 and eng.iter == 6 and not eng.opt.acc.any()
    groups = grouped(6, 4)
    assert groups == [[0, 1, 2, 3], [4, 5]]
    want = host_statement(batches, groups)
    _assert_equals_statement(eng, want)
    with pytest.raises(ValueError, match='holds 0'):
        eng.flush()
    with pytest.raises(RuntimeError, match='accumulate=1'):
        D.TrainEngine(reduced_model(), use_graph=False, **SGD).flush()


def test_micro_iterations_carry_their_own_state():
    """engine.iter counts micro-iterations; the rate of the stepping call is the one applied; BatchNorm running statistics
    move on every micro-iteration (k times per update); grad_norm is refreshed by updates only, and the clip acts on the
    averaged gradient."""
    k = 3
    batches = micro_batches(6)
    lrs = [0.5, 0.4, 0.03, 0.2, 0.1, 0.07]
    clip = dict(max_norm=1e-3)
    eng, clipped = _engine(k), _engine(k, grad_clip=clip)
    stats, norms = [running_stats(eng.model)], []
    with D.kernels.use_ops(torch_ops):
        for i, b in enumerate(batches):
            p_before = eng.flat.flat_p.clone()
            logs = eng.step(*b, lr=lrs[i])
            assert set(logs) >= {'loss', 'top1_acc'} and 'grad_norm' not in logs and math.isfinite(float(logs['loss']))
            assert eng.iter == i + 1 and eng.pending == (i + 1) % k
            assert torch.equal(eng.flat.flat_p, p_before) == ((i + 1) % k != 0)
            stats.append(running_stats(eng.model))
            norms.append(float(clipped.step(*b, lr=lrs[i])['grad_norm']))
    for a, b in zip(stats, stats[1:]):                     # every call is a training-mode forward of its own
        assert not torch.equal(a['backbone.data_bn.running_mean'], b['backbone.data_bn.running_mean'])
        assert all(int(b[name]) == int(a[name]) + 1 for name in a if name.endswith('num_batches_tracked'))
    assert int(stats[-1]['backbone.data_bn.num_batches_tracked']) == int(stats[0]['backbone.data_bn.num_batches_tracked']) + 6
    # rates 0.03 and 0.07, those of calls 3 and 6: equal to the statement with them, different from one with call 1's
    _assert_equals_statement(eng, host_statement(batches, grouped(6, k), lrs=lrs))
    other = host_statement(batches, grouped(6, k), lrs=[lrs[0]] * 6)
    assert any(not torch.equal(p.detach(), other['p'][name]) for name, p in eng.model.named_parameters())
    # grad_norm: 0 until the first update, then the last update's; every update clipped (the norm of the mean > max_norm)
    assert norms[0] == norms[1] == 0.0 and norms[2] == norms[3] == norms[4] > 1e-3 and norms[5] not in (0.0, norms[2])
    want = host_statement(batches, grouped(6, k), lrs=lrs, grad_clip=clip)
    total = math.sqrt(sum(float(g.double().square().sum()) for g in want['mean'].values()))
    assert norms[5] == pytest.approx(total, rel=1e-6)
    for name, p in clipped.model.named_parameters():
        assert torch.allclose(p.detach(), want['p'][name], rtol=0, atol=1e-6), name
    with pytest.raises(ValueError, match='accumulate'):
        _engine(0)
    with pytest.raises(ValueError, match='accumulate'):
        _engine(2.0)


# ---- train_model ---------------------------------------------------------------------------------------------------------

def test_optimizer_config_types():
    assert parse_optimizer_config(None) == (None, 1)
    assert parse_optimizer_config(dict(grad_clip=None)) == (None, 1)
    assert parse_optimizer_config(dict(type='OptimizerHook', grad_clip=dict(max_norm=45))) == (dict(max_norm=45), 1)
    assert parse_optimizer_config(dict(type='GradientCumulativeOptimizerHook')) == (None, 1)
    assert parse_optimizer_config(dict(type='GradientCumulativeOptimizerHook', cumulative_iters=8,
                                       grad_clip=dict(max_norm=45))) == (dict(max_norm=45), 8)
    with pytest.raises(NotImplementedError, match='Fp16OptimizerHook'):
        parse_optimizer_config(dict(type='Fp16OptimizerHook', loss_scale=512.0))
    with pytest.raises(ValueError, match='cumulative_iters'):
        parse_optimizer_config(dict(type='GradientCumulativeOptimizerHook', cumulative_iters=0))


def _run(tmp_path, optimizer_config, logger=None, **extra):
    z, tr, m, data, cfg = _setup(tmp_path, **extra)
    if optimizer_config is None:
        del cfg['optimizer_config']
    else:
        cfg['optimizer_config'] = optimizer_config
    with D.kernels.use_ops(torch_ops):
        runner = train_model(m, data, cfg, device='cpu', use_graph=False, logger=logger)
    return runner, tr


def test_train_model_unknown_hook_type_raises(tmp_path):
    with pytest.raises(NotImplementedError, match='GradientCumulativeFp16OptimizerHook'):
        _run(tmp_path, dict(type='GradientCumulativeFp16OptimizerHook', cumulative_iters=2))


def test_train_model_cumulative_iters_one_is_no_key_at_all(tmp_path):
    a, _ = _run(tmp_path / 'a', None)
    b, _ = _run(tmp_path / 'b', dict(type='GradientCumulativeOptimizerHook', cumulative_iters=1))
    c, _ = _run(tmp_path / 'c', dict(type='OptimizerHook', grad_clip=None))
    for r in (b, c):
        assert r.engine.accumulate == 1 and r.engine.opt.acc is None
        assert [x['loss'] for x in r.log] == [x['loss'] for x in a.log]
        assert torch.equal(r.engine.flat.flat_p, a.engine.flat.flat_p) and torch.equal(r.engine.opt.buf, a.engine.opt.buf)


def test_train_model_accumulates_and_closes_groups_at_epoch_ends(tmp_path):
    """3 iterations per epoch, 2 epochs, cumulative_iters=2: updates after iterations 2, 3 (the epoch ends inside a group:
    a short group of one, one log line), 5 and 6 (the tail).  The schedule and the log count the 6 micro-iterations; the
    checkpoint of epoch 1 resumes to the same weights with no accumulator state."""
    records = []
    handler = logging.Handler()
    handler.emit = lambda rec: records.append(rec.getMessage())
    logger = logging.getLogger('grad_accum_host')
    logger.setLevel(logging.INFO)
    logger.addHandler(handler)
    try:
        runner, tr = _run(tmp_path, dict(type='GradientCumulativeOptimizerHook', cumulative_iters=2), logger=logger)
    finally:
        logger.removeHandler(handler)
    assert runner.engine.accumulate == 2 and runner.engine.pending == 0
    assert runner.iter == runner.engine.iter == 6 and len(runner.log) == 6
    assert [r['lr'] for r in runner.log] == [D.cosine_lr(tr['lr'], it, 6) for it in range(6)]
    notes = [r for r in records if 'ends inside a group' in r]
    assert len(notes) == 2 and 'Epoch [1]' in notes[0] and 'Epoch [2]' in notes[1]
    # the same loop by hand over the engine: the sampler's batches, an update after calls 2, 3, 5 and 6
    z, _, m, data, cfg = _setup(tmp_path / 'hand')
    eng = D.TrainEngine(m, use_graph=False, accumulate=2, lr=tr['lr'], momentum=tr['momentum'],
                        weight_decay=tr['weight_decay'], nesterov=True)
    from dsgcn_amd.apis import epoch_indices
    it = 0
    with D.kernels.use_ops(torch_ops):
        for epoch in range(2):
            order = epoch_indices(len(data), epoch, tr['seed'], 0, 1)
            for b in range(3):
                idx = order[b * tr['batch']:(b + 1) * tr['batch']]
                kp = torch.stack([torch.as_tensor(data[i]['keypoint'], dtype=torch.float32) for i in idx])
                lb = torch.tensor([data[i]['label'] for i in idx], dtype=torch.int64).view(-1, 1)
                eng.step(kp, lb, lr=D.cosine_lr(tr['lr'], it, 6))
                it += 1
            assert eng.pending == 1
            eng.flush(1)
    assert torch.equal(eng.flat.flat_p, runner.engine.flat.flat_p) and torch.equal(eng.opt.buf, runner.engine.opt.buf)
    # resume from the end of epoch 1: nothing but the usual checkpoint is needed
    final = {k: v.clone() for k, v in runner.model.state_dict().items()}
    z2, _, m2, data2, cfg2 = _setup(tmp_path / 'second', resume_from=str(tmp_path / 'epoch_1.pth'))
    cfg2['optimizer_config'] = dict(type='GradientCumulativeOptimizerHook', cumulative_iters=2)
    with D.kernels.use_ops(torch_ops):
        r2 = train_model(m2, data2, cfg2, device='cpu', use_graph=False)
    assert r2.iter == 6 and [r['lr'] for r in r2.log] == [r['lr'] for r in runner.log[3:]]
    for k, v in m2.state_dict().items():
        assert torch.equal(v, final[k]), k


# ---- the C ABI -----------------------------------------------------------------------------------------------------------

def test_accum_symbols_are_exported_and_reject_bad_arguments_without_gpu():
    if not os.path.exists(native.LIB_PATH):
        pytest.skip('libdsgcn.so is not built')
    handle = ctypes.CDLL(native.LIB_PATH)
    for name in ('dsgcn_grad_accum', 'dsgcn_grad_accum_finish'):
        assert hasattr(handle, name), name
        assert name in native.SIGNATURES
    lib = native.lib()
    A, G, F = 4096, 8192, 16384                            # any non-NULL addresses: rejected before they are touched
    assert lib.dsgcn_grad_accum(None, G, 8, None) == -1
    assert lib.dsgcn_grad_accum(A, None, 8, None) == -1
    assert lib.dsgcn_grad_accum(A, G, 0, None) == -1
    assert lib.dsgcn_grad_accum(A, G, -4, None) == -1
    assert lib.dsgcn_grad_accum(A + 2, G, 8, None) == -1                       # not a float address
    assert lib.dsgcn_grad_accum(A, A + 16, 8, None) == -1                      # overlapping ranges
    assert lib.dsgcn_grad_accum_finish(None, G, F, 8, None) == -1
    assert lib.dsgcn_grad_accum_finish(A, None, F, 8, None) == -1
    assert lib.dsgcn_grad_accum_finish(A, G, None, 8, None) == -1
    assert lib.dsgcn_grad_accum_finish(A, G, F, 0, None) == -1
    assert lib.dsgcn_grad_accum_finish(A, G, F + 1, 8, None) == -1
    assert lib.dsgcn_grad_accum_finish(G, G, F, 8, None) == -1
