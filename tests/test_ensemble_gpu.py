"""GPU: the multi-stream test pass bit for bit against the single-stream path — the input launch against the existing
batcher, the ensemble head against S head launches + ``ensemble_results``, EnsembleEngine and test_ensemble against
InferEngine / test_model + ``ensemble_results``.  Every comparison is torch.equal / np.array_equal: the shared device
functions and the fixed summation order leave no rounding to allow for."""
import numpy as np
import pytest
import torch

import dsgcn_amd as D
from dsgcn_amd import kernels_infer, native

import ensemble_cases as EC

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# ---- 1. the input launch ------------------------------------------------------------------------------------------------
_single = {}          # (case, feature) -> the existing batcher's output, made once


def _case(name):
    if name not in _single:
        anns, pipe = EC.INPUT_CASES[name]
        store = D.SkeletonStore(anns())
        idx = list(range(len(store)))
        _single[name] = (store, idx, pipe, {})
    return _single[name]


def _reference(name, feat):
    store, idx, pipe, done = _case(name)
    if feat not in done:
        out, label = D.SkeletonBatcher(pipe(feat))(store, idx)
        done[feat] = (out.clone(), label.clone())
    return done[feat]


@pytest.mark.parametrize('feats', EC.FEATURE_LISTS, ids='-'.join)
@pytest.mark.parametrize('name', list(EC.INPUT_CASES))
def test_stream_launch_equals_single_launches(name, feats):
    store, idx, pipe, _ = _case(name)
    sb = D.StreamBatcher([pipe(f) for f in feats])
    outs, label = sb(store, idx)
    assert len(outs) == len(feats)
    persons = 5 if name == 'k400_compact' else 2
    for f, out in zip(feats, outs):
        want, want_label = _reference(name, f)
        assert out.shape == want.shape == (len(idx), 2, persons, EC.CLIP_LEN, store.V, store.C)
        assert torch.equal(out, want), (name, f, (out - want).abs().max().item())
        assert torch.equal(label, want_label)
    if len(feats) > 1:                               # the streams are different tensors with different contents
        assert outs[0].data_ptr() != outs[1].data_ptr() and not torch.equal(outs[0], outs[1])


def test_cases_cover_what_they_claim():
    """The plans behind the cases above: a missing successor frame, the fp16 flag, the compact-box flag, an empty slot."""
    store, idx, pipe, _ = _case('ntu3d_zero')
    plan = D.StreamBatcher([pipe('j'), pipe('bm')]).plan(store, idx)
    assert (plan['f1'] == -1).any() and set(plan['M']) == {1, 2} and set(plan['T']) == {5, 40}
    store, idx, pipe, _ = _case('coco_fp16')
    assert (D.StreamBatcher([pipe('b')]).plan(store, idx)['flags'] & 4).all()
    store, idx, pipe, _ = _case('coco_fp32')
    assert not (D.StreamBatcher([pipe('b')]).plan(store, idx)['flags'] & 4).any()
    store, idx, pipe, _ = _case('k400_compact')
    plan = D.StreamBatcher([pipe('jm')]).plan(store, idx)
    assert (plan['flags'] & 8).any() and plan['M'].min() == 1 and plan['M'].max() < 5


# ---- 2. the head --------------------------------------------------------------------------------------------------------
WEIGHTS = {1: (0.7,), 2: (1, 1), 3: (0.3, 0.7, 0.11), 4: (2, 2, 1, 1)}
SHAPES = [(1, 1, 1, 4, 2, 1), (3, 10, 2, 256, 60, 4), (2, 3, 5, 64, 2, 4), (2, 23, 2, 256, 400, 2), (2, 2, 2, 6, 7, 3)]


def _head_inputs(N, clips, M, C, K, S, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * S + K)
    feats = [torch.randn(N * clips * M, C, generator=g).to(DEV) for _ in range(S)]
    heads = [((torch.randn(K, C, generator=g) * 0.3).to(DEV), (torch.randn(K, generator=g) * 0.1).to(DEV) if s % 2 == 0 else None)
             for s in range(S)]
    return feats, heads


def _head_reference(feats, heads, weights, N, clips, M, mode):
    rows = [kernels_infer.head_test(f, w, b, N, clips, M, mode).cpu().numpy() for f, (w, b) in zip(feats, heads)]
    return np.stack(rows), EC.host_sum(rows, weights)


def _wt(weights):
    return torch.tensor([float(w) for w in weights], dtype=torch.float32, device=DEV)


@pytest.mark.parametrize('mode', ['prob', 'score'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_head_ensemble_equals_head_launches_and_host_sum(shape, mode):
    N, clips, M, C, K, S = shape
    feats, heads = _head_inputs(*shape)
    for weights in [WEIGHTS[S]] + ([(0.3, 0.7, 0.11, 1.9)] if S == 4 else []):
        want_streams, want = _head_reference(feats, heads, weights, N, clips, M, mode)
        out, so = kernels_infer.head_ensemble(feats, heads, _wt(weights), N, clips, M, mode, want_streams=True)
        assert out.shape == (N, K) and so.shape == (S, N, K)
        assert np.array_equal(so.cpu().numpy(), want_streams), np.abs(so.cpu().numpy() - want_streams).max()
        assert np.array_equal(out.cpu().numpy(), want), np.abs(out.cpu().numpy() - want).max()
        again = kernels_infer.head_ensemble(feats, heads, _wt(weights), N, clips, M, mode)          # no stream_out
        assert torch.equal(again, out)                                                               # two launches, equal bits


def test_head_ensemble_takes_each_streams_own_load_width():
    """A weight that is not 16-byte aligned makes dsgcn_head_test_fwd read it by single floats (another summation order):
    the ensemble launch decides per stream, as that launch would."""
    N, clips, M, C, K, S = 2, 2, 2, 8, 5, 2
    feats, heads = _head_inputs(N, clips, M, C, K, S)
    buf = torch.zeros(K * C + 1, device=DEV)
    buf[1:] = heads[1][0].reshape(-1)
    shifted = buf[1:].view(K, C)
    assert shifted.data_ptr() % 16 == 4
    heads[1] = (shifted, heads[1][1])
    want_streams, want = _head_reference(feats, heads, (1, 1), N, clips, M, 'prob')
    out, so = kernels_infer.head_ensemble(feats, heads, _wt((1, 1)), N, clips, M, 'prob', want_streams=True)
    assert np.array_equal(so.cpu().numpy(), want_streams) and np.array_equal(out.cpu().numpy(), want)


def test_head_ensemble_lds_limit_raises_before_the_launch():
    feats, heads = _head_inputs(2, 24, 2, 256, 400, 2)
    assert not kernels_infer.head_ensemble_fits(24, 256, 400) and kernels_infer.head_ensemble_fits(23, 256, 400)
    with pytest.raises(native.DsgcnError, match='LDS'):
        kernels_infer.head_ensemble(feats, heads, _wt((1, 1)), 2, 24, 2, 'prob')
    torch.cuda.synchronize()


@pytest.mark.parametrize('mode', ['prob', 'score'])
def test_head_ensemble_nan_poisons_only_its_rows(mode):
    N, clips, M, C, K, S = 3, 4, 2, 64, 9, 3
    feats, heads = _head_inputs(N, clips, M, C, K, S)
    w = _wt(WEIGHTS[3])
    clean, clean_s = kernels_infer.head_ensemble(feats, heads, w, N, clips, M, mode, want_streams=True)
    feats[1] = feats[1].clone()
    feats[1][1 * clips * M + 3, 5] = float('nan')                    # video 1 of stream 1
    out, so = kernels_infer.head_ensemble(feats, heads, w, N, clips, M, mode, want_streams=True)
    assert torch.isnan(out[1]).all() and torch.isnan(so[1, 1]).all()
    keep = torch.ones(S, N, dtype=torch.bool)
    keep[1, 1] = False
    assert torch.equal(so[keep.to(DEV)], clean_s[keep.to(DEV)])
    assert torch.equal(out[[0, 2]], clean[[0, 2]])


# ---- 3. engine and pass -------------------------------------------------------------------------------------------------
FOUR = (2, 2, 1, 1)


@pytest.fixture(scope='module')
def streams():
    """Four reduced-width DS-STGCN models, 3 videos x 2 clips x 2 persons of T = 16, V = 25 per stream, and what four
    InferEngines + ensemble_results make of them (second call of each engine: a replay)."""
    models = [EC.reduced_model(11 + s).to(DEV).eval() for s in range(4)]
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(3, 2, 2, 16, 25, 3, generator=g).to(DEV) for _ in range(4)]
    rows = []
    for m, x in zip(models, xs):
        eng = D.InferEngine(m)
        eng(x)
        rows.append(eng(x).cpu().numpy())
        assert eng.graphed(x)
    return dict(models=models, xs=xs, rows=np.stack(rows), total=EC.host_sum(rows, FOUR))


def test_engine_equals_four_infer_engines(streams):
    eng = D.EnsembleEngine(streams['models'], FOUR)
    eager = eng(streams['xs'])
    eager_s = eng.stream_scores
    assert not eng.graphed(streams['xs']) and eng.eager_calls == 1
    out = eng(streams['xs'])
    assert eng.capture_error is None and eng.graphed(streams['xs']) and eng.replays == 1
    assert out.is_cuda and out.shape == (3, 12) and eng.stream_scores.shape == (4, 3, 12)
    assert torch.equal(out, eager) and torch.equal(eng.stream_scores, eager_s)          # eager step == replayed step
    assert np.array_equal(eng.stream_scores.cpu().numpy(), streams['rows'])
    assert np.array_equal(out.cpu().numpy(), streams['total'])
    # the result is a copy: the next replay does not rewrite it; new weights are followed by the replay
    eng.set_weights((1, 1, 1, 1))
    other = eng(streams['xs'])
    assert eng.replays == 2 and np.array_equal(out.cpu().numpy(), streams['total'])
    assert np.array_equal(other.cpu().numpy(), EC.host_sum(list(streams['rows']), (1, 1, 1, 1)))


def test_replay_sees_a_head_weight_changed_in_place(streams):
    models, xs = streams['models'], streams['xs']
    eng = D.EnsembleEngine(models, FOUR)
    eng(xs), eng(xs)
    assert eng.graphed(xs)
    w = models[2].cls_head.fc_cls.weight
    with torch.no_grad():
        w.mul_(2.0)
    try:
        out = eng(xs)
        assert eng.replays == 2
        rows = list(streams['rows'])
        rows[2] = D.InferEngine(models[2], use_graph=False)(xs[2]).cpu().numpy()
        assert not np.array_equal(rows[2], streams['rows'][2])
        assert np.array_equal(eng.stream_scores.cpu().numpy(), np.stack(rows))
        assert np.array_equal(out.cpu().numpy(), EC.host_sum(rows, FOUR))
    finally:
        with torch.no_grad():
            w.mul_(0.5)                               # (exact: the models are shared)


def test_max_views_gives_the_same_rows(streams):
    eng = D.EnsembleEngine(streams['models'], FOUR, max_views=2)      # one video (2 clips) per forward
    assert eng._chunks(3, 2) == [(0, 1), (1, 2), (2, 3)]
    for _ in range(2):
        out = eng(streams['xs'])
        assert np.array_equal(out.cpu().numpy(), streams['total'])
        assert np.array_equal(eng.stream_scores.cpu().numpy(), streams['rows'])
    assert eng.replays >= 3


def test_concurrent_equals_sequential(streams):
    eng = D.EnsembleEngine(streams['models'], FOUR, concurrent=True)
    eager = eng(streams['xs'])
    assert np.array_equal(eager.cpu().numpy(), streams['total'])
    out = eng(streams['xs'])
    assert eng.capture_error is None and eng.graphed(streams['xs']) and eng.replays == 1
    assert np.array_equal(out.cpu().numpy(), streams['total'])
    assert np.array_equal(eng.stream_scores.cpu().numpy(), streams['rows'])


def test_engine_refuses_what_has_no_weighted_sum(streams):
    models = streams['models']
    with pytest.raises(ValueError, match='stream weights'):
        D.EnsembleEngine(models, (1, 1))
    other = EC.reduced_model(3, classes=7).to(DEV)
    with pytest.raises(ValueError, match='classes'):
        D.EnsembleEngine(models[:1] + [other], (1, 1))
    models[1].test_cfg['average_clips'] = 'score'
    try:
        with pytest.raises(ValueError, match='average_clips'):
            D.EnsembleEngine(models, FOUR)
    finally:
        models[1].test_cfg['average_clips'] = 'prob'
    models[3].test_cfg['feat_ext'] = True
    try:
        with pytest.raises(ValueError, match='feat_ext'):
            D.EnsembleEngine(models, FOUR)
    finally:
        del models[3].test_cfg['feat_ext']


def test_test_ensemble_equals_four_test_model_runs(streams, tmp_path):
    """Five videos of unequal length, batches of 2 + 2 + 1: results, stream results, metrics and files against four
    ``test_model`` runs + ``ensemble_results``."""
    from pipeline_cases import raw_clips
    anns = [dict(frame_dir=f'clip{i}', label=(5 * i) % 12, keypoint=k, total_frames=k.shape[1])
            for i, k in enumerate(raw_clips()[:5])]
    assert len({a['total_frames'] for a in anns}) == 5
    feats = ['j', 'b', 'jm', 'bm']

    def pipe(f):
        return EC.pipe_3d(f, clip_len=16, num_clips=2, align_spine=False)
    store = D.SkeletonStore(anns)
    cfg = D.Config(dict(data=dict(test_dataloader=dict(videos_per_gpu=2)), work_dir=str(tmp_path)))
    models = streams['models']
    labels = [a['label'] for a in anns]
    singles, files = [], []
    for s, f in enumerate(feats):
        files.append(str(tmp_path / f'{f}.pkl'))
        singles.append(D.test_model(models[s], (store, D.SkeletonBatcher(pipe(f))), cfg, out=files[-1]))
    want = D.ensemble_results(files, FOUR, labels=labels)

    np.random.seed(77)
    state = np.random.get_state()
    outs = [str(tmp_path / 'ens' / f'{f}.pkl') for f in feats]
    res = D.test_ensemble(models, (store, D.StreamBatcher([pipe(f) for f in feats])), cfg, weights='2:2:1:1',
                          out=str(tmp_path / 'ens' / 'sum.pkl'), stream_out=outs)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    assert not any(m.training for m in models)
    assert len(res['results']) == 5 and all(r.shape == (12,) and r.dtype == np.float32 for r in res['results'])
    assert np.array_equal(np.stack(res['results']), np.stack(want['results']))
    assert dict(res['metrics']) == dict(want['metrics']) and list(res['metrics']) == list(want['metrics'])
    for s in range(4):
        assert np.array_equal(np.stack(res['stream_results'][s]), np.stack(singles[s]['results'])), feats[s]
        assert dict(res['stream_metrics'][s]) == dict(singles[s]['metrics'])
        back, single_file = D.load_results(outs[s]), D.load_results(files[s])
        assert len(back) == 5 and all(np.array_equal(a, b) for a, b in zip(back, single_file))
    back = D.load_results(str(tmp_path / 'ens' / 'sum.pkl'))
    assert all(np.array_equal(a, b) for a, b in zip(back, want['results']))
    with pytest.raises(ValueError, match='3 weights for 4 streams'):
        D.test_ensemble(models, (store, D.StreamBatcher([pipe(f) for f in feats])), cfg, weights='1:1:1')
