"""-m gpu: the EMA launches (csrc/ema.hip) against fp64, eager and replayed; ``TrainEngine(ema=...)`` on the reduced
DS-STGCN with and without accumulation; an ``InferEngine`` across a swap; and ``train_model`` with the EMAHook on the
product path.  Every comparison against the fp64 recurrence uses the bound of tests/ema_common.py (4 k 2^-24 B) and first
makes sure that leaving one update out of the recurrence would miss it tenfold."""
import json

import numpy as np
import pytest
import torch

import dsgcn_amd as D
from dsgcn_amd import native
from ema_common import (HOOK, bound, check_epoch_file, check_not_vacuous, fixture_model, flat_of, recorded, recurrence, setup)

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 255, 256, 1023, 1025, 65537, 1376950]      # the last: the flat buffer of the headline model
MS = [0.5, 0.0, 0.25, 1.0, 0.1, 0.729]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _update(e, p, hyper):
    native.check(native.lib().dsgcn_ema_update(e.data_ptr(), p.data_ptr(), e.numel(), hyper.data_ptr(), _stream()),
                 'dsgcn_ema_update')


def _inputs(n):
    g = torch.Generator().manual_seed(n)
    e0 = torch.randn(n, generator=g).cuda()
    ps = [torch.randn(n, generator=g).cuda() for _ in MS]
    return e0, ps


def _eager(e0, ps):
    hyper = torch.zeros(1, dtype=torch.float64, device='cuda')
    e = e0.clone()
    out = []
    for p, m in zip(ps, MS):
        hyper.fill_(m)
        _update(e, p, hyper)
        out.append(e.clone())
    return out


@pytest.mark.parametrize('n', SIZES)
def test_update_against_fp64(n):
    e0, ps = _inputs(n)
    got = _eager(e0, ps)
    # after every update: the fp64 recurrence so far within the bound — and that update left out would miss it tenfold
    # (the m = 0 update changes nothing by definition: it is held to bit-equality instead)
    for j in range(len(MS)):
        tol = bound(e0, ps[:j + 1])
        want = recurrence(e0, ps[:j + 1], MS[:j + 1])
        err = float((got[j].double() - want).abs().max())
        print(f'n = {n}, update {j} (m = {MS[j]}): worst error {err:.3e}, bound {tol:.3e}')
        assert err <= tol, (j, err, tol)
        if MS[j] > 0:
            rel_tol = tol * n ** 0.5 / float(want.norm())
            rel = float((recurrence(e0, ps[:j + 1], MS[:j + 1], skip=j) - want).norm() / want.norm())
            assert rel > 10 * rel_tol, (j, rel, rel_tol)
    assert torch.equal(got[1], got[0])                         # m = 0: bit-unchanged
    assert torch.equal(got[3], ps[3])                          # m = 1: bit-equal to p
    again = _eager(e0, ps)
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    # one captured launch, replayed with the device scalar (and p) rewritten between the replays
    hyper = torch.zeros(1, dtype=torch.float64, device='cuda')
    e, p = e0.clone(), torch.zeros_like(e0)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        _update(e, p, hyper)
    e.copy_(e0)
    for j, m in enumerate(MS):
        p.copy_(ps[j])
        hyper.fill_(m)
        graph.replay()
        assert torch.equal(e, got[j]), j


def test_update_leaves_ema_alone_at_zero_whatever_p_holds():
    n = 1025
    e0 = torch.randn(n).cuda()
    e0[::7] = float('nan')
    e0[1::7] = -0.0
    p = torch.full((n,), float('inf')).cuda()
    hyper = torch.zeros(1, dtype=torch.float64, device='cuda')
    e = e0.clone()
    _update(e, p, hyper)
    assert torch.equal(e.view(torch.int32), e0.view(torch.int32))
    # buffers at other distances from a 16-byte boundary: the head / tail path, and the all-scalar path
    base_e, base_p = torch.randn(n + 8).cuda(), torch.randn(n + 8).cuda()
    hyper.fill_(0.25)
    for oe, op in ((1, 1), (3, 3), (1, 2), (0, 3)):
        e, q = base_e[oe:oe + n].clone(), base_p[op:op + n]
        buf = base_e.clone()
        view = buf[oe:oe + n]
        _update(view, q, hyper)
        want = recurrence(e, [q], [0.25])
        assert float((view.double() - want).abs().max()) <= bound(e, [q])
        assert torch.equal(buf[:oe], base_e[:oe]) and torch.equal(buf[oe + n:], base_e[oe + n:])     # nothing outside


@pytest.mark.parametrize('n', SIZES)
def test_swap(n):
    g = torch.Generator().manual_seed(n + 1)
    a0, b0 = torch.randn(n, generator=g).cuda(), torch.randn(n, generator=g).cuda()
    a, b = a0.clone(), b0.clone()
    lib = native.lib()
    native.check(lib.dsgcn_ema_swap(a.data_ptr(), b.data_ptr(), n, _stream()), 'dsgcn_ema_swap')
    assert torch.equal(a, b0) and torch.equal(b, a0)
    native.check(lib.dsgcn_ema_swap(a.data_ptr(), b.data_ptr(), n, _stream()), 'dsgcn_ema_swap')
    assert torch.equal(a, a0) and torch.equal(b, b0)


# ---- the engine --------------------------------------------------------------------------------------------------------

def _batches():
    z, _ = fixture_model()
    x, y = torch.from_numpy(z['x']).float(), torch.from_numpy(z['label']).long().view(-1, 1)
    return [(x[i:i + 4].cuda(), y[i:i + 4].cuda()) for i in range(0, 24, 4)]


def _engine_run(use_graph, accumulate):
    _, m = fixture_model()
    m = m.cuda().train()
    eng = D.TrainEngine(m, lr=0.01, use_graph=use_graph, warmup_eager=2, ema=dict(momentum=0.5, warm_up=4),
                        accumulate=accumulate)
    # lr = 0.01 is the fixture's rate.  On its own it does not make every update visible over SIX of them: the trace of
    # update 0 is halved by each later one (left out, the recurrence moves by 7.5e-6 in relative L2 on this fixture, below
    # ten times the bound), and with accumulate = 2 the first micro-iteration finds p == ema, so its update changes
    # nothing at all.  So the average starts 0.01 * randn away from the weights: every update then moves it by more than
    # the condition asks, the first micro-iteration's included, and the weights it averages still move at the fixture's rate.
    noise = torch.randn(eng.ema.flat_e.numel(), generator=torch.Generator().manual_seed(7)).cuda()
    eng.ema.flat_e.add_(noise, alpha=0.01)
    e0 = eng.ema.flat_e.clone().cpu()
    snaps, ms = [], []
    batches = _batches()
    for kp, lb in batches:
        eng.step(kp, lb, lr=0.01)
        snaps.append(eng.flat.flat_p.clone().cpu())
        ms.append(eng.ema.m)
    torch.cuda.synchronize()
    return eng, e0, snaps, ms, batches


@pytest.mark.parametrize('accumulate', [1, 2])
def test_engine_keeps_the_average_eager_and_replayed(accumulate):
    eng, e0, snaps, ms, batches = _engine_run(True, accumulate)
    assert eng.capture_error is None and eng.graphed(*batches[0])
    if accumulate == 1:
        assert eng._seen[next(iter(eng._seen))] == 2            # two eager steps, then four replays
    else:
        assert sorted(eng._seen.values()) == [2, 2]             # per kind: two eager calls, the third one replayed
        assert torch.equal(snaps[0], snaps[1]) is False and torch.equal(snaps[1], snaps[2])      # a micro-iteration leaves p
    assert ms == [D.ema_momentum(s, 0.5, 1, 4) for s in range(6)] and eng.ema_iter == 6
    tol = bound(e0, snaps)
    want = check_not_vacuous(e0, snaps, ms, tol)
    err = float((eng.ema.flat_e.cpu().double() - want).abs().max())
    print(f'accumulate = {accumulate}: worst error after 6 updates {err:.3e}, bound {tol:.3e}')
    assert err <= tol, (err, tol)
    ref, e0r, snaps_r, _, _ = _engine_run(False, accumulate)
    assert not ref._graphs and torch.equal(e0r, e0)
    for a, b in zip(snaps, snaps_r):
        assert torch.equal(a, b)
    assert torch.equal(eng.ema.flat_e, ref.ema.flat_e)
    if accumulate == 2:
        before = eng.ema.flat_e.clone()
        eng.step(*batches[0], lr=0.01)                          # one more micro-iteration: moves the average ...
        moved = eng.ema.flat_e.clone()
        assert not torch.equal(moved, before)
        eng.flush()                                             # ... and closing the short group does not
        assert torch.equal(eng.ema.flat_e, moved)


def test_infer_engine_follows_the_swap():
    eng, _, _, _, batches = _engine_run(False, 1)
    m = eng.model
    x = batches[0][0]
    infer = D.InferEngine(m, use_graph=True, warmup_eager=1)
    infer(x)
    raw = infer(x)
    assert infer.graphed(x) and infer.replays == 1
    eng.ema.swap()
    got = infer(x)
    assert infer.replays == 2 and eng.ema.swapped
    fresh = D.InferEngine(m, use_graph=False)(x)
    assert torch.equal(got, fresh) and not torch.equal(got, raw)
    eng.ema.swap()
    assert torch.equal(infer(x), raw)


# ---- the loop ----------------------------------------------------------------------------------------------------------

def test_train_model_with_the_hook_gpu(tmp_path):
    m, data, cfg = setup(tmp_path / 'hook', custom_hooks=[HOOK], evaluation=dict(interval=1, metrics=['top_k_accuracy']))
    _, fresh = fixture_model()
    with recorded() as rec:
        runner = D.train_model(m, data, cfg, device='cuda', use_graph=True, validate=True, val_dataset=data)
    eng = runner.engine
    assert eng.capture_error is None and len(eng._graphs) == 1 and eng.ema.swapped
    p0 = flat_of(dict(fresh.named_parameters()), eng)
    sd1 = check_epoch_file(tmp_path / 'hook' / 'epoch_1.pth', eng, p0, rec['steps'], 3)
    check_epoch_file(tmp_path / 'hook' / 'epoch_2.pth', eng, flat_of(sd1, eng), rec['steps'], 6, first=3)
    # without the hook: no ema_* key, and the weights are the hook run's raw weights, bit for bit
    m2, data2, cfg2 = setup(tmp_path / 'plain', custom_hooks=[])
    D.train_model(m2, data2, cfg2, device='cuda', use_graph=True)
    plain1 = torch.load(tmp_path / 'plain' / 'epoch_1.pth', weights_only=False)['state_dict']
    assert not any(k.startswith('ema_') for k in plain1)
    for k, _ in m2.named_parameters():
        assert torch.equal(plain1[k], sd1['ema_' + k.replace('.', '_')]), k
    # the evaluator scored what epoch_1.pth holds under the parameter names: test_model on that file, no further option
    _, m3 = fixture_model()
    res = D.test_model(m3, data, D.Config(dict(data=dict(test_dataloader=dict(videos_per_gpu=8)))),
                       checkpoint=str(tmp_path / 'hook' / 'epoch_1.pth'), metrics=['top_k_accuracy'])
    # (the evaluator of train_model runs forward_test, test_model the captured InferEngine with its one-launch head: with
    # equal weights the two agree to 1e-6 of a video's scores, tests/test_infer_gpu.py::test_test_model_end_to_end; the raw
    # weights of the same epoch score 4e-3 away)
    got, want = np.stack(res['results']).astype(np.float64), rec['scores'][0].astype(np.float64)
    errs = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)
    print(f'test_model(epoch_1.pth) against the evaluator: worst relative error {errs.max():.2e}')
    assert errs.max() < 1e-6
    assert res['metrics']['top1_acc'] == runner.evaluator.results[0]['top1_acc']
    _, m4 = fixture_model()
    raw = D.test_model(m4, data, D.Config(dict(data=dict(test_dataloader=dict(videos_per_gpu=8)))),
                       checkpoint=str(tmp_path / 'plain' / 'epoch_1.pth'), metrics=['top_k_accuracy'])
    off = np.stack(raw['results']).astype(np.float64)
    assert (np.linalg.norm(off - want, axis=1) / np.linalg.norm(want, axis=1)).min() > 1e-4
    assert json.dumps(sorted(k for k in sd1 if k.startswith('ema_'))) == \
        json.dumps(sorted('ema_' + k.replace('.', '_') for k, _ in m.named_parameters()))
