"""mmcv's EMAHook through ``train_model`` on the CPU (the host loop over tests/torch_ops.py; the EMA update and the swap
as torch ops): the momentum formula, the buffers' names and state, the epoch-boundary swap as seen in the checkpoints and by
the evaluator, resume, the config errors, two ranks over gloo, and the argument checks of the two C entry points.

The comparisons against the fp64 recurrence use the bound of tests/ema_common.py (4 k 2^-24 B) and first make sure that the
recurrence with any one update left out would miss it tenfold.

``test_model`` runs on the GPU only (``InferEngine`` has no CPU path), so here the evaluator's scores are compared with the
scores of a FRESH model that ``load_checkpoint(strict=False)`` filled from ``epoch_1.pth`` — what ``test_model`` does before
it builds its engine; tests/test_ema_gpu.py makes the comparison with ``test_model`` itself."""
import ctypes
import logging
import os

import numpy as np
import pytest
import torch

import dsgcn_amd as D
import torch_ops
from dsgcn_amd import native
from dsgcn_amd.apis import EvalLoop, parse_custom_hooks, train_model
from dsgcn_amd.ema import FlatEMA, buffer_name
from ema_common import HOOK, check_epoch_file, fixture_model, flat_of, recorded, setup


# ---- 1: the momentum ---------------------------------------------------------------------------------------------------

def test_ema_momentum_formula():
    for s in range(301):
        want = min(0.5, (1 + s) / (100 + s))
        assert D.ema_momentum(s, 0.5, 1, 100) == want
        assert (want < 0.5) == (s < 98)                       # the warm-up branch is live below s = 98
        full = 0.9 ** 3
        assert abs(full - 0.729) < 1e-15
        want3 = min(full, (1 + s) / (100 + s)) if s % 3 == 0 else 0.0
        assert D.ema_momentum(s, 0.9, 3, 100) == want3
        assert D.ema_momentum(s) == min(0.0002, (1 + s) / (100 + s)) == 0.0002      # the defaults: M at every s
    assert D.ema_momentum(297, 0.9, 3, 100) == 0.9 ** 3 and D.ema_momentum(298, 0.9, 3, 100) == 0.0


# ---- 2: names and state ------------------------------------------------------------------------------------------------

def test_buffers_ride_in_the_state_dict():
    _, m = fixture_model()
    before = set(m.state_dict())
    flat = D.FlatParams(m, gather=True)
    ema = FlatEMA(flat, momentum=0.5, warm_up=4)
    sd = m.state_dict()
    params = dict(m.named_parameters())
    assert set(sd) - before == {buffer_name(k) for k in params} and len(set(sd) - before) == len(params)
    assert buffer_name('backbone.gcn.0.tcn.bn.weight') == 'ema_backbone_gcn_0_tcn_bn_weight'
    for k, p in params.items():
        assert torch.equal(sd[buffer_name(k)], p.detach()), k
    assert ema.flat_e.numel() == flat.flat_p.numel() and torch.equal(ema.flat_e, flat.flat_p)
    # a round trip through load_state_dict: in place (the flat buffer keeps its address and sees the loaded values)
    g = torch.Generator().manual_seed(3)
    new = {k: (torch.randn(v.shape, generator=g) if k.startswith('ema_') else v.clone()) for k, v in sd.items()}
    ptr = ema.flat_e.data_ptr()
    res = m.load_state_dict(new, strict=True)
    assert not res.missing_keys and not res.unexpected_keys and ema.flat_e.data_ptr() == ptr
    for (off, n), p in zip(flat.slices, flat.params):
        name = next(k for k, q in params.items() if q is p)
        assert torch.equal(ema.flat_e[off:off + n], new[buffer_name(name)].reshape(-1)), name
    for k, v in m.state_dict().items():
        assert torch.equal(v, new[k]), k
    with pytest.raises(ValueError, match='already has'):
        FlatEMA(flat)
    # update and swap as torch ops: m = 0 leaves the buffer alone, m = 1 copies, twice swapped is the identity
    e0, p0 = ema.flat_e.clone(), flat.flat_p.clone()
    ema.interval = 2
    ema.update(1)
    assert ema.m == 0.0 and torch.equal(ema.flat_e, e0)
    ema.update(2)
    assert ema.m == 0.25 and not torch.equal(ema.flat_e, e0)  # min(0.5 ** 2, 3 / 6)
    assert float((ema.flat_e.double() - (1 - ema.m) * e0.double() - ema.m * p0.double()).abs().max()) <= \
        4 * 2.0 ** -24 * max(float(e0.abs().max()), float(p0.abs().max()))
    ema.flat_e.copy_(e0)
    ema.swap()
    assert ema.swapped and torch.equal(ema.flat_e, p0) and torch.equal(flat.flat_p, e0)
    ema.swap()
    assert not ema.swapped and torch.equal(ema.flat_e, e0) and torch.equal(flat.flat_p, p0)


# ---- 3-5: the run ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def ema_run(tmp_path_factory):
    """ONE run of the fixture with the hook (2 epochs of 3 iterations, validation after each) and one without."""
    work = tmp_path_factory.mktemp('ema')
    m, data, cfg = setup(work / 'hook', custom_hooks=[dict(HOOK, priority=49)],
                         evaluation=dict(interval=1, metrics=['top_k_accuracy']))
    with D.kernels.use_ops(torch_ops), recorded() as rec:
        runner = train_model(m, data, cfg, device='cpu', use_graph=False, validate=True, val_dataset=data)
    p0 = torch.empty_like(runner.engine.flat.flat_p)
    z, fresh = fixture_model()
    for (off, n), p in zip(runner.engine.flat.slices, runner.engine.flat.params):
        name = next(k for k, q in m.named_parameters() if q is p)
        p0[off:off + n] = dict(fresh.named_parameters())[name].detach().reshape(-1)
    m2, data2, cfg2 = setup(work / 'plain')
    with D.kernels.use_ops(torch_ops):
        plain = train_model(m2, data2, cfg2, device='cpu', use_graph=False)
    return dict(work=work, runner=runner, model=m, data=data, rec=rec, p0=p0, plain=plain)


def test_epoch_checkpoint_holds_ema_under_the_parameter_names(ema_run, tmp_path):
    r = ema_run
    sd1 = check_epoch_file(r['work'] / 'hook' / 'epoch_1.pth', r['runner'].engine, r['p0'], r['rec']['steps'], 3)
    # the second epoch continues from the first one's average (iterations 3..5)
    check_epoch_file(r['work'] / 'hook' / 'epoch_2.pth', r['runner'].engine, flat_of(sd1, r['runner'].engine),
                     r['rec']['steps'], 6, first=3)
    # the run without the hook: no ema_* key; its weights are the hook run's RAW weights (the average never leaks into
    # training), and a run through custom_hooks=[] writes the same file
    plain1 = torch.load(r['work'] / 'plain' / 'epoch_1.pth', weights_only=False)['state_dict']
    assert not any(k.startswith('ema_') for k in plain1)
    for k, p in r['model'].named_parameters():
        assert torch.equal(plain1[k], sd1[buffer_name(k)]), k
    assert sum(not torch.equal(plain1[k], sd1[k]) for k, _ in r['model'].named_parameters()) > 100
    m3, data3, cfg3 = setup(tmp_path, custom_hooks=[])
    with D.kernels.use_ops(torch_ops):
        train_model(m3, data3, cfg3, device='cpu', use_graph=False)
    empty1 = torch.load(tmp_path / 'epoch_1.pth', weights_only=False)['state_dict']
    assert list(empty1) == list(plain1)
    for k in plain1:
        assert torch.equal(empty1[k], plain1[k]), k


def test_validation_scores_the_checkpointed_weights(ema_run):
    r = ema_run
    assert len(r['rec']['scores']) == 2 and [x['epoch'] for x in r['runner'].evaluator.results] == [1, 2]
    _, fresh = fixture_model()
    ck = D.load_checkpoint(fresh, str(r['work'] / 'hook' / 'epoch_1.pth'), strict=False)
    assert ck['unexpected_keys'] and all(k.startswith('ema_') for k in ck['unexpected_keys']) and not ck['missing_keys']
    loop = EvalLoop(r['data'], batch_size=8, device='cpu', metrics=['top_k_accuracy'], save_best=None)
    with D.kernels.use_ops(torch_ops):
        scores = np.stack(loop.predict(fresh, 0, 1))
    assert np.array_equal(scores, r['rec']['scores'][0])
    vals = loop.evaluate(scores, loop.labels())
    assert vals['top1_acc'] == r['runner'].evaluator.results[0]['top1_acc']
    # and not the raw weights': those score differently
    _, raw = fixture_model()
    sd = torch.load(r['work'] / 'plain' / 'epoch_1.pth', weights_only=False)['state_dict']
    raw.load_state_dict(sd)
    with D.kernels.use_ops(torch_ops):
        assert not np.array_equal(np.stack(loop.predict(raw, 0, 1)), scores)


def test_resume_continues_the_average(ema_run, tmp_path):
    r = ema_run
    # the hook's own resume_from stands in for the run's
    m, data, cfg = setup(tmp_path, custom_hooks=[dict(HOOK, resume_from=str(r['work'] / 'hook' / 'epoch_1.pth'))])
    with D.kernels.use_ops(torch_ops), recorded() as rec:
        runner = train_model(m, data, cfg, device='cpu', use_graph=False)
    assert runner.epoch == 2 and runner.iter == 6 and [s[2] for s in rec['steps']] == [3, 4, 5]
    assert rec['steps'][0][1] == D.ema_momentum(3, 0.5, 1, 4) == 0.5 and runner.engine.iter == 3
    for a, b in zip(rec['steps'], r['rec']['steps'][3:]):
        assert torch.equal(a[0], b[0]) and a[1] == b[1]               # trained on the RAW weights the first run trained on
    final = r['model'].state_dict()
    for k, v in m.state_dict().items():
        assert torch.equal(v, final[k]), k
    # at the end the model holds the average and the buffers the raw weights
    ema = runner.engine.ema
    assert ema.swapped and torch.equal(ema.flat_e, rec['steps'][-1][0])
    assert not torch.equal(runner.engine.flat.flat_p, ema.flat_e)
    ck1 = torch.load(r['work'] / 'hook' / 'epoch_1.pth', weights_only=False)
    sd1 = ck1['state_dict']
    assert ck1['meta']['ema_swapped'] is True
    # a file that says the RAW weights lie under the parameter names (saved with the model unswapped) resumes unswapped
    ck1['meta']['ema_swapped'] = False
    torch.save(ck1, tmp_path / 'unswapped.pth')
    m5, data5, cfg5 = setup(tmp_path / 'u', total_epochs=1, custom_hooks=[HOOK])
    from dsgcn_amd.apis import EpochRunner, _BatchSource
    eng5 = D.TrainEngine(m5, optimizer=cfg5['optimizer'], use_graph=False, ema=dict(momentum=0.5, warm_up=4))
    r5 = EpochRunner(m5, eng5, _BatchSource(data5, 'cpu'), cfg5)
    r5.resume(str(tmp_path / 'unswapped.pth'))
    assert not eng5.ema.swapped and eng5.ema_iter == r5.iter == 3
    r5.resume(str(r['work'] / 'hook' / 'epoch_1.pth'))
    assert eng5.ema.swapped
    check_epoch_file(tmp_path / 'epoch_2.pth', runner.engine, flat_of(sd1, runner.engine), r['rec']['steps'], 6, first=3)


# ---- 6: the config errors ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('hook, key', [
    (dict(momentum=0.0), 'momentum'), (dict(momentum=1.0), 'momentum'), (dict(momentum=1.5), 'momentum'),
    (dict(momentum=-0.1), 'momentum'), (dict(interval=0), 'interval'), (dict(interval=-2), 'interval'),
    (dict(interval=1.5), 'interval'), (dict(interval=True), 'interval'), (dict(warm_up=-1), 'warm_up'),
    (dict(decay=0.99), 'decay'), (dict(momentun=0.1), 'momentun')])
def test_config_errors_name_the_key(tmp_path, hook, key):
    m, data, cfg = setup(tmp_path, custom_hooks=[dict(type='EMAHook', **hook)])
    with pytest.raises(ValueError, match=key):
        train_model(m, data, cfg, device='cpu', use_graph=False)
    with pytest.raises(ValueError, match=key):
        D.TrainEngine(m, ema=hook, use_graph=False)
    assert not any(k.startswith('ema_') for k in m.state_dict())


def test_two_ema_hooks_raise_and_other_hooks_stay_ignored(tmp_path, caplog):
    m, data, cfg = setup(tmp_path, custom_hooks=[dict(type='EMAHook'), dict(type='EMAHook', momentum=0.1)])
    with pytest.raises(ValueError, match='EMAHook'):
        train_model(m, data, cfg, device='cpu', use_graph=False)
    log = logging.getLogger('test_ema_host')
    with caplog.at_level(logging.WARNING, logger='test_ema_host'):
        assert parse_custom_hooks([dict(type='SyncBuffersHook', momentum=7)], log) == (None, None)
    assert 'SyncBuffersHook' in caplog.text
    got = parse_custom_hooks([dict(type='SyncBuffersHook'), dict(type='EMAHook', interval=2, priority='NORMAL')], None)
    assert got == (dict(type='EMAHook', interval=2, priority='NORMAL'), dict(momentum=0.0002, interval=2, warm_up=100))
    assert parse_custom_hooks(None) == (None, None) and parse_custom_hooks([]) == (None, None)


# ---- 7: two ranks ----------------------------------------------------------------------------------------------------------

def _dp_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(1)
    m, data, cfg = setup(os.path.join(out_dir, f'w{rank}'), total_epochs=1, custom_hooks=[HOOK])
    cfg['data']['videos_per_gpu'] = 4
    if rank == 1:                                   # a rank that starts from other weights: the wrap-time broadcast fixes it
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.01)
    with D.kernels.use_ops(torch_ops):
        runner = train_model(m, data, cfg, device='cpu', use_graph=False)
    eng = runner.engine
    torch.save(dict(p=eng.flat.flat_p.clone(), e=eng.ema.flat_e.clone(), swapped=eng.ema.swapped, iters=runner.iter),
               os.path.join(out_dir, f'r{rank}.pt'))
    dist.destroy_process_group()


def test_two_ranks_keep_equal_averages_gloo(tmp_path):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = [torch.load(tmp_path / f'r{r}.pt', weights_only=False) for r in range(2)]
    assert r0['iters'] == r1['iters'] == 3 and r0['swapped'] and r1['swapped']
    assert torch.equal(r0['e'], r1['e']) and torch.equal(r0['p'], r1['p'])
    assert not torch.equal(r0['e'], r0['p'])


# ---- 10: the entry points reject bad arguments before any launch ----------------------------------------------------------

def test_argument_rejection_without_gpu():
    lib = native.lib()
    L, V = ctypes.c_longlong, ctypes.c_void_p
    assert native.SIGNATURES['dsgcn_ema_update'] == [V, V, L, V, V]
    assert native.SIGNATURES['dsgcn_ema_swap'] == [V, V, L, V]
    a, b, h = 0x10000, 0x20000, 0x30000                  # never dereferenced: every call below returns before a launch
    bad = -1
    assert lib.dsgcn_ema_update(None, b, 4, h, None) == bad
    assert lib.dsgcn_ema_update(a, None, 4, h, None) == bad
    assert lib.dsgcn_ema_update(a, b, 4, None, None) == bad
    assert lib.dsgcn_ema_update(a, b, -1, h, None) == bad
    assert lib.dsgcn_ema_update(a, b, 4, h + 4, None) == bad            # hyper: 8-byte aligned
    assert lib.dsgcn_ema_update(a + 2, b, 4, h, None) == bad            # the buffers: 4-byte aligned
    assert lib.dsgcn_ema_update(a, a + 8, 4, h, None) == bad            # overlapping
    assert lib.dsgcn_ema_update(a, b, 0, h, None) == 0                  # nothing to do: no launch
    assert lib.dsgcn_ema_swap(None, b, 4, None) == bad
    assert lib.dsgcn_ema_swap(a, None, 4, None) == bad
    assert lib.dsgcn_ema_swap(a, b, -1, None) == bad
    assert lib.dsgcn_ema_swap(a, b + 1, 4, None) == bad
    assert lib.dsgcn_ema_swap(a, a, 4, None) == bad
    assert lib.dsgcn_ema_swap(a, b, 0, None) == 0
