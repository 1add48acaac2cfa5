"""-m gpu: the test pass — the one-launch test-time head (csrc/head_test.hip), ``InferEngine`` (captured multi-clip inference)
and ``test_model`` — against fp64, against the reference's own eval fixtures and against ``forward_test``."""
import gc
import os
import pickle

import numpy as np
import pytest
import torch

import dsgcn_amd as D
from dsgcn_amd import kernels as K
from bench import ds_cfg
from test_kernels_gpu import rel as trel
from test_model_gpu import R2_CONFIGS, _load_running, _r2_model
from test_oracle_golden import GOLD, load, rel

pytestmark = pytest.mark.gpu
DEV = 'cuda'


# ---- 1. the kernel against fp64 ------------------------------------------------------------------------------------
def head_test_fp64(feat, w, b, N, clips, M, mode):
    """simple_head.py:88-98 + recognizergcn.py's average_clips, restated in fp64 on the host."""
    feat, w = feat.double().cpu(), w.double().cpu()
    pooled = feat.view(N * clips, M, -1).mean(1)
    score = pooled @ w.t() + (b.double().cpu() if b is not None else 0.0)
    score = score.view(N, clips, -1)
    if mode == 'prob':
        return torch.softmax(score, dim=2).mean(1), score
    if mode == 'score':
        return score.mean(1), score
    return score, score


@pytest.mark.parametrize('mode', ['prob', 'score', None])
@pytest.mark.parametrize('bias', [True, False])
@pytest.mark.parametrize('N,clips,M,C,Kc', [(2, 10, 2, 256, 60), (16, 10, 2, 256, 60), (3, 1, 2, 256, 120), (4, 10, 2, 256, 400),
                                            (5, 3, 1, 64, 7), (64, 10, 2, 256, 60), (2, 4, 2, 30, 5), (2, 3, 2, 516, 9)])
def test_head_test_vs_fp64(N, clips, M, C, Kc, bias, mode):
    """out and clip_score to 2e-6 of their norm (the bar check_head_loss holds dsgcn_head_loss_fwd to, same rel); a second
    launch is bit-identical.  (2,4,2,30,5): C not a multiple of 4 (scalar loads); (2,3,2,516,9): more than one channel chunk."""
    g = torch.Generator().manual_seed(N * 31 + Kc + clips)
    feat = torch.randn(N * clips * M, C, generator=g)
    w = torch.randn(Kc, C, generator=g) * 0.2
    b = torch.randn(Kc, generator=g) * 0.1 if bias else None
    dev = [t.to(DEV) if t is not None else None for t in (feat, w, b)]
    out, cs = K.head_test(*dev, N, clips, M, mode, want_clip_scores=True)
    want, want_cs = head_test_fp64(feat, w, b, N, clips, M, mode)
    assert out.shape == want.shape and cs.shape == (N, clips, Kc) and out.dtype == torch.float32
    e_out, e_cs = trel(out, want), trel(cs, want_cs)
    print(f'head_test {(N, clips, M, C, Kc)} bias={bias} mode={mode}: out {e_out:.2e} clip_score {e_cs:.2e}')
    assert e_out < 2e-6 and e_cs < 2e-6, (e_out, e_cs)
    out2, cs2 = K.head_test(*dev, N, clips, M, mode, want_clip_scores=True)
    assert torch.equal(out, out2) and torch.equal(cs, cs2)
    assert torch.equal(K.head_test(*dev, N, clips, M, mode), out)           # without the per-clip scores: same result


@pytest.mark.parametrize('mode', ['prob', 'score', None])
def test_head_test_nan_poisons_only_its_video(mode):
    N, clips, M, C, Kc = 4, 10, 2, 256, 60
    g = torch.Generator().manual_seed(3)
    feat = torch.randn(N * clips * M, C, generator=g)
    w, b = torch.randn(Kc, C, generator=g) * 0.2, torch.randn(Kc, generator=g) * 0.1
    clean = K.head_test(feat.to(DEV), w.to(DEV), b.to(DEV), N, clips, M, mode)
    bad = feat.clone()
    bad[((2 * clips + 7) * M + 1), 100] = float('nan')                       # video 2, clip 7, person 1
    out = K.head_test(bad.to(DEV), w.to(DEV), b.to(DEV), N, clips, M, mode)
    if mode is None:
        assert torch.isnan(out[2, 7]).all()                                  # that clip's scores
        keep = torch.ones(N, clips, dtype=torch.bool)
        keep[2, 7] = False
        assert torch.equal(out[keep.to(DEV)], clean[keep.to(DEV)])
    else:
        assert torch.isnan(out[2]).all()
        assert torch.equal(out[[0, 1, 3]], clean[[0, 1, 3]])


# ---- 2. the engine against the reference's eval fixtures ----------------------------------------------------------------
def _eval_setup(name):
    from closed_form import EVAL_LIVEN, eval_clips
    m, cfg, T, V = _r2_model(name, EVAL_LIVEN.get(name, 0.5))
    z = load(f'eval_{name}.npz')
    _load_running(m, z)
    return m.cuda().eval(), z, eval_clips(name, T, V).cuda()


def _replayed(eng, x):
    """Call until the graph for x's shape is the one answering (warm-up calls, the capture), then once more."""
    for _ in range(eng.warmup_eager + 1):
        eng(x)
    before = eng.replays
    out = eng(x)
    assert eng.capture_error is None and eng.graphed(x) and eng.replays == before + 1
    return out


@pytest.mark.parametrize('name', list(R2_CONFIGS))
def test_engine_vs_reference_fixture(name):
    """The bars of test_eval_mode_vs_reference_fixture, unchanged, for the REPLAYED engine: probabilities to 1e-5 and
    per-clip scores (average_clips=None) to 1e-4 of the reference's fp64 outputs."""
    m, z, x = _eval_setup(name)
    eng = D.InferEngine(m)
    assert eng.fused_head
    probs = _replayed(eng, x)
    assert probs.is_cuda and tuple(probs.shape) == z['probs64'].shape
    e = rel(probs.cpu(), z['probs64'])
    print(f'engine {name}: probs {e:.2e}')
    assert e < 1e-5
    m.test_cfg['average_clips'] = None
    scores = _replayed(eng, x)
    assert tuple(scores.shape) == z['scores64_clips'].shape
    e = rel(scores.cpu(), z['scores64_clips'])
    print(f'engine {name}: clip scores {e:.2e}')
    assert e < 1e-4
    assert not m.training


# ---- 3. replay == eager -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['dsstgcn_ntu60', 'ctrgcn_ntu60'])
def test_replay_is_the_eager_engine(name):
    m, z, x = _eval_setup(name)
    eager = D.InferEngine(m, use_graph=False)
    want = eager(x)
    assert eager.replays == 0 and eager.eager_calls == 1 and not eager.graphed(x)
    eng = D.InferEngine(m, warmup_eager=1)
    got = _replayed(eng, x)
    assert eng.eager_calls == 1 and eng.replays == 2 and len(eng._graphs) == 1
    assert torch.equal(got, want), rel(got.cpu(), want.cpu())
    m.train()                                       # the engine switches to eval for the call and puts the mode back
    again = eng(x)
    assert m.training and torch.equal(again, want)


# ---- 4. weights move under a captured graph -----------------------------------------------------------------------------
def test_replay_sees_weights_changed_in_place():
    """The captured graph rebuilds the bf16 weight images of the wide convs from the parameters of the moment: after a
    TrainEngine step (raw-pointer SGD on the flat buffer, BatchNorm buffers moved) and after load_state_dict, a replay
    equals a freshly built engine on the new weights, bit for bit."""
    torch.manual_seed(0)
    np.random.seed(0)
    m = D.build_model(ds_cfg(60)).cuda()
    train = D.TrainEngine(m, lr=0.1, use_graph=False)                 # (flattens the parameters: before the capture)
    g = torch.Generator().manual_seed(5)
    xt = torch.randn(4, 1, 2, 32, 25, 3, generator=g).cuda()         # 32 frames: stages 2 and 3 take the wide-conv form
    yt = torch.randint(0, 60, (4, 1), generator=g).cuda()
    x = torch.randn(2, 3, 2, 32, 25, 3, generator=g).cuda()
    m.train()
    train.step(xt, yt)
    images_global = set(K._wsplit_state['jobs'])                      # the process-wide table (TrainEngine prunes it as it goes)
    eng = D.InferEngine(m)
    before = _replayed(eng, x).clone()
    m.train()
    train.step(xt, yt)
    got = _replayed(eng, x)
    want = D.InferEngine(m, use_graph=False)(x)
    assert not torch.equal(got, before)                               # the step did move the output
    assert torch.equal(got, want), rel(got.cpu(), want.cpu())
    assert set(K._wsplit_state['jobs']) <= images_global              # the engines keep their images to themselves
    # another state, loaded in place
    torch.manual_seed(1)
    other = D.build_model(ds_cfg(60))
    with torch.no_grad():
        for p in other.parameters():
            p.add_(torch.randn_like(p) * 0.01)
    m.load_state_dict(other.state_dict())
    replays = eng.replays
    got = eng(x)
    assert eng.replays == replays + 1
    want = D.InferEngine(m, use_graph=False)(x)
    assert torch.equal(got, want), rel(got.cpu(), want.cpu())


# ---- 5. fuse_conv_bn ----------------------------------------------------------------------------------------------------
def test_engine_on_a_fused_model():
    m, z, x = _eval_setup('dsstgcn_ntu60')
    D.fuse_conv_bn(m)
    eng = D.InferEngine(m)                                            # built after the fold
    e = rel(_replayed(eng, x).cpu(), z['probs64'])
    print(f'engine fused: probs {e:.2e}')
    assert e < 1e-5
    m.test_cfg['average_clips'] = None
    e = rel(_replayed(eng, x).cpu(), z['scores64_clips'])
    print(f'engine fused: clip scores {e:.2e}')
    assert e < 1e-4


# ---- 6. max_views -------------------------------------------------------------------------------------------------------
def test_max_views_chunks_whole_videos():
    """5 videos x 10 clips with max_views=20 (chunks of 2, 2 and 1 videos: two shapes, two graphs) against the undivided
    batch: eval-mode BatchNorm makes videos independent, and no kernel's summation order depends on the batch size —
    bit-identical."""
    m, z, x2 = _eval_setup('dsstgcn_ntu60')
    g = torch.Generator().manual_seed(11)
    x = torch.cat([x2, x2.flip(0), x2[:1]]) + 0.01 * torch.randn(5, *x2.shape[1:], generator=g).cuda()
    whole = D.InferEngine(m)
    want = _replayed(whole, x)
    eng = D.InferEngine(m, max_views=20)
    assert eng._chunks(5, 10) == [(0, 2), (2, 4), (4, 5)]
    for _ in range(2):
        eng(x)
    got = eng(x)
    assert len(eng._graphs) == 2 and eng.capture_error is None
    print(f'max_views: chunked vs whole rel {rel(got.cpu(), want.cpu()):.2e}')
    assert got.shape == want.shape and torch.equal(got, want)
    assert D.InferEngine(m, max_views=5)._chunks(3, 10) == [(0, 1), (1, 2), (2, 3)]        # a video is never split


# ---- 7. test_model end to end -------------------------------------------------------------------------------------------
def _reduced_ds(classes=12):
    import json
    with open(os.path.join(GOLD, 'model_reduced_cfg.json')) as f:
        cfg = json.load(f)
    cfg['backbone']['tcn_ms_cfg'] = [tuple(c) if isinstance(c, list) else c for c in cfg['backbone']['tcn_ms_cfg']]
    cfg['cls_head']['num_classes'] = classes
    torch.manual_seed(0)
    np.random.seed(0)
    m = D.build_model(cfg)
    from closed_form import liven32
    liven32(m, 1, 0.5)
    return m


def test_test_model_end_to_end(tmp_path):
    """Seven videos of unequal length through the shipped test pipeline (configs/dsstgcn/ntu60_xsub_3dkp/j.py:29-37 with
    num_clips=10; clip_len 16 to stay small), batch size 3 (3 + 3 + 1): the results equal forward_test's on the same
    batches to 1e-6, the file reloads, the metrics are there and numpy's RNG state is left alone."""
    from pipeline_cases import raw_clips
    anns = [dict(frame_dir=f'clip{i}', label=(5 * i) % 12, keypoint=k, total_frames=k.shape[1])
            for i, k in enumerate(raw_clips())]
    pipe = [dict(type='PreNormalize3D', align_spine=False), dict(type='GenSkeFeat', feats=['j']),
            dict(type='UniformSample', clip_len=16, num_clips=10, test_mode=True), dict(type='PoseDecode'),
            dict(type='FormatGCNInput'), dict(type='Collect', keys=['keypoint', 'label'], meta_keys=[]),
            dict(type='ToTensor', keys=['keypoint'])]
    store, batcher = D.SkeletonStore(anns), D.SkeletonBatcher(pipe)
    from closed_form import fill_running
    m = _reduced_ds()
    fill_running(m)                                                    # running statistics off their 0 / 1 start
    m = m.cuda().train()
    cfg = D.Config(dict(data=dict(videos_per_gpu=16, test_dataloader=dict(videos_per_gpu=3)), work_dir=str(tmp_path)))
    out = str(tmp_path / 'res' / 'result.pkl')
    np.random.seed(77)
    state = np.random.get_state()
    res = D.test_model(m, (store, batcher), cfg, out=out)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    assert m.training                                                  # the mode it came in
    m.eval()
    want = []
    for idx in ([0, 1, 2], [3, 4, 5], [6]):
        kp, _ = batcher(store, idx)
        assert kp.shape[1:] == (10, 2, 16, 25, 3)
        want.extend(m(keypoint=kp, return_loss=False))
    assert len(res['results']) == 7
    for i, (a, b) in enumerate(zip(res['results'], want)):
        assert a.shape == (12,) and a.dtype == np.float32
        e = rel(a, b)
        print(f'test_model video {i}: {e:.2e}')
        assert e < 1e-6, (i, e)
    assert list(res['metrics']) == ['top1_acc', 'top5_acc', 'mean_class_accuracy']
    labels = [a['label'] for a in anns]
    assert res['metrics']['top1_acc'] == float(D.top_k_accuracy(np.stack(res['results']), labels, (1,))[0])
    with open(out, 'rb') as f:
        back = pickle.load(f)
    assert len(back) == 7 and all(np.array_equal(a, b) for a, b in zip(back, res['results']))
    # the four-stream workflow ends in the package
    ens = D.ensemble_results([out, res['results']], labels=labels)
    assert ens['metrics']['top1_acc'] == res['metrics']['top1_acc']
    # --average-clips score, EvalLoop(engine=...)
    res_s = D.test_model(m, (store, batcher), cfg, average_clips='score', use_graph=False)
    assert m.test_cfg['average_clips'] == 'prob' and not np.allclose(np.stack(res_s['results']), np.stack(res['results']))
    loop = D.EvalLoop((store, batcher), batch_size=3, engine=D.InferEngine(m), device=DEV)
    part = loop.predict(m, 0, 1)
    assert len(part) == 7 and all(rel(a, b) < 1e-6 for a, b in zip(part, want))
    # checkpoint=None takes <work_dir>/latest.pth when it is there
    D.save_checkpoint(m, os.path.join(str(tmp_path), 'latest.pth'))
    fresh = _reduced_ds()
    res_c = D.test_model(fresh, (store, batcher), cfg)
    assert all(np.array_equal(a, b) for a, b in zip(res_c['results'], res['results']))


# ---- 8. no stray syncs --------------------------------------------------------------------------------------------------
def test_replayed_call_does_not_synchronise():
    """A replayed eng(x) neither copies to the host nor waits for the device.  Which check ran is printed: torch's sync
    debug mode ('error') when this build honours it (a deliberate .item() raises under it), else a torch.profiler trace
    of the call without hipMemcpy* / hipStreamSynchronize / hipDeviceSynchronize entries."""
    m = _reduced_ds().cuda().eval()
    x = torch.randn(3, 10, 2, 16, 25, 3, device=DEV)
    eng = D.InferEngine(m)
    _replayed(eng, x)
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    honoured = False
    torch.cuda.set_sync_debug_mode('error')
    try:
        try:
            probe.item()
        except RuntimeError:
            honoured = True
        if honoured:
            out = eng(x)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if honoured:
        print('no-sync check: torch.cuda.set_sync_debug_mode("error")')
    else:
        print('no-sync check: torch.profiler CPU-activity trace')
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU]) as prof:
            out = eng(x)
        names = {e.name for e in prof.events()}
        bad = [n for n in names if n.startswith('hipMemcpy') or n in ('hipStreamSynchronize', 'hipDeviceSynchronize')]
        assert not bad, bad
    assert out.is_cuda and out.shape == (3, 12) and eng.graphed(x)


# ---- engines come and go ------------------------------------------------------------------------------------------------
def test_engines_built_and_dropped_leave_memory_flat():
    """Every engine keeps its weight images and graphs to itself: after it is dropped the allocator is back where it was
    (within one engine's footprint), and the process-wide image table a TrainEngine uses never saw them."""
    m = D.build_model(ds_cfg(60)).cuda().eval()
    x = torch.randn(1, 2, 2, 32, 25, 3, device=DEV)
    table = set(K._wsplit_state['jobs'])

    def one():
        eng = D.InferEngine(m)
        _replayed(eng, x)
        assert len(eng._images) > 0                                    # the wide convs did build images — in ITS table
        torch.cuda.synchronize()
        used = torch.cuda.memory_allocated()
        del eng
        gc.collect()
        torch.cuda.synchronize()
        return used

    base = torch.cuda.memory_allocated()
    footprint = one() - base
    after = [torch.cuda.memory_allocated()]
    for _ in range(4):
        one()
        after.append(torch.cuda.memory_allocated())
    print(f'engine footprint {footprint / 2**20:.1f} MiB; allocated after each drop (MiB over base): '
          f'{[round((a - base) / 2**20, 2) for a in after]}')
    assert footprint > 0 and after[-1] - base <= footprint
    assert set(K._wsplit_state['jobs']) == table
