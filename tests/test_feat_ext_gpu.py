"""-m gpu: feature / score-map extraction at test time — the one-launch kernel (csrc/featext.hip, ``kernels.feat_ext``)
against the reference's own runs (tests/golden/featext.npz, tests/feat_ext_cases.py), then ``RecognizerGCN.forward_test``,
``InferEngine`` and ``test_model`` over it.

Bars.  float16: the fp32 result rounded to nearest even, bit for bit, everywhere; where every mean is exact in fp32 (the
'exact' and 'inf' cases) the float16 result IS the reference's, bit for bit.  fp32: error(a) = max|a - ref64| / max|ref64|
at most twice the reference's own fp32 error (one fp32 ulp of max|ref64| where that error is 0).  Every run prints both
errors; profiles/feat_ext/README.md keeps the observed ratios."""
import json
import os

import numpy as np
import pytest
import torch

import dsgcn_amd as D
import feat_ext_cases as F
from dsgcn_amd import kernels as K
from test_feat_ext_host import feat_ext_argument_checks
from test_oracle_golden import GOLD, load, rel, sd_of

pytestmark = pytest.mark.gpu
DEV = 'cuda'
Z = load('featext.npz')


def bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def half_of(out32):
    with np.errstate(over='ignore'):
        return out32.cpu().numpy().astype(np.float16)


def check_run(out16, out32, k, tag, exact=False):
    """shape, the rounding identity, the 2x rule (and, exact: the reference's float16 bits); -> error / bar"""
    want16 = F.ref16(Z, k)
    assert out16.dtype == torch.float16 and out32.dtype == torch.float32
    assert tuple(out16.shape) == tuple(out32.shape) == want16.shape, (tag, tuple(out16.shape), want16.shape)
    assert same_bits(out16.cpu().numpy(), half_of(out32)), tag
    e_got, e_ref, bar = F.errors(out32.cpu().numpy(), Z, k)
    print(f'feat_ext {tag}: error {e_got:.2e}  reference fp32 {e_ref:.2e}  bar {bar:.2e}  ratio to the bar {e_got / bar:.2f}')
    if exact:
        assert same_bits(out16.cpu().numpy(), want16), tag
        assert e_got == 0, tag
    assert e_got <= bar, (tag, e_got, e_ref)
    return e_got / bar


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------
def _case(name):
    c = F.CASES[name]
    x = torch.from_numpy(F.case_x(Z, name)).to(DEV).flatten(0, 2)              # (videos*clips*M, C, T, V)
    w = torch.from_numpy(Z[name + '_w']).to(DEV) if name + '_w' in Z else None
    b = torch.from_numpy(Z[name + '_b']).to(DEV) if name + '_b' in Z else None
    return c, x, w, b


@pytest.mark.parametrize('name', list(F.CASES))
def test_kernel_case(name):
    """Every (mode, pool_opt) run of a case: all 16 masks ('all'), the tile / vector / class-round boundaries, plane-mean
    input, no bias, whole-plane reductions, the exact and the out-of-range cases.  Two launches give the same bits; the
    float16-only launch gives the float16 of the two-output one."""
    c, x, w, b = _case(name)
    sizes = (c['videos'], c['clips'], c['M'])
    for mode, pool in F.runs(name):
        ww, bb = (w, b) if mode == 'score' else (None, None)
        out16, out32 = K.feat_ext(x, *sizes, pool, ww, bb, want_fp32=True)
        check_run(out16, out32, F.key(name, mode, pool), f'{name} {mode} {pool}', exact=name in F.EXACT)
        again16, again32 = K.feat_ext(x, *sizes, pool, ww, bb, want_fp32=True)
        assert same_bits(again16, out16) and same_bits(again32, out32), (name, mode, pool)
        only16 = K.feat_ext(x, *sizes, K.parse_pool_opt(pool), ww, bb)
        assert same_bits(only16, out16), (name, mode, pool)
    if name == 'inf':
        got = K.feat_ext(x, *sizes, 'none').cpu().numpy()
        want = Z[F.key('inf', 'feat', 'none') + '_r16']
        assert np.isinf(got).sum() == 6 and np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(got, want)


def test_plane_mean_input_forms():
    """(R, C), (N, M, C) and (R, C, 1, 1) are one input; pooling an axis of extent 1 is the identity."""
    c, x, w, b = _case('planes')
    sizes = (c['videos'], c['clips'], c['M'])
    a = K.feat_ext(x, *sizes, 'nm', w, b)
    assert same_bits(K.feat_ext(x[:, :, 0, 0], *sizes, 'nm', w, b), a)
    assert same_bits(K.feat_ext(x[:, :, 0, 0].reshape(c['videos'] * c['clips'], c['M'], -1), *sizes, 'nm', w, b), a)
    assert same_bits(K.feat_ext(x, *sizes, 'nmtv', w, b), a)
    with pytest.raises(ValueError):
        K.feat_ext(x, c['videos'], c['clips'], c['M'] + 1, 'nm', w, b)
    with pytest.raises(ValueError):
        K.feat_ext(x, *sizes, 'nm', w[:, :-1].contiguous(), b)
    with pytest.raises(RuntimeError):
        K.feat_ext(x.cpu(), *sizes, 'nm')                                       # no CPU path


def test_argument_checks():
    feat_ext_argument_checks()


# ---- 2. the model -------------------------------------------------------------------------------------------------------
def _model(name, **test_cfg):
    z = load(name + '.npz')
    with open(os.path.join(GOLD, name + '_cfg.json')) as f:
        cfg = json.load(f)
    if 'tcn_ms_cfg' in cfg['backbone']:
        cfg['backbone']['tcn_ms_cfg'] = [tuple(c) if isinstance(c, list) else c for c in cfg['backbone']['tcn_ms_cfg']]
    cfg['test_cfg'] = test_cfg
    m = D.build_model(cfg)
    m.load_state_dict(sd_of(z, 'sd_', torch.float32))
    return m.to(DEV).eval()


def _cfg_of(mode, pool):
    return {('score_ext' if mode == 'score' else 'feat_ext'): True, 'pool_opt': pool}


X1 = torch.from_numpy(Z['model_x'])                                             # (1, 3, 2, 16, 25, 3)


def _videos(n):
    g = torch.Generator().manual_seed(21)
    return torch.cat([X1] + [X1 + 0.3 * torch.randn(X1.shape, generator=g) for _ in range(n - 1)]).to(DEV)


def _replayed(eng, x):
    for _ in range(eng.warmup_eager + 1):
        eng(x)
    before = eng.replays
    out = eng(x)
    assert eng.capture_error is None and eng.graphed(x) and eng.replays == before + 1
    return out


@pytest.mark.parametrize('name', F.MODELS)
def test_forward_test_vs_reference(name):
    """model(keypoint, return_loss=False) returns the reference's array — shape, leading axis in score mode, float16 — and
    its fp32 value meets the 2x rule against the reference's fp64 run of the same model."""
    m = _model(name)
    x = X1.to(DEV)
    for mode, pool in F.MODEL_RUNS:
        m.test_cfg.update(score_ext=False, feat_ext=False)
        m.test_cfg.update(_cfg_of(mode, pool))
        k = F.key(name, mode, pool)
        got = m(keypoint=x, return_loss=False)
        assert isinstance(got, np.ndarray) and got.dtype == np.float16 and got.shape == F.ref16(Z, k).shape
        out16, out32 = m.forward_extract(x, want_fp32=True)
        lead = out16 if mode == 'score' else out16[0]
        assert same_bits(lead.cpu().numpy(), got)
        view = (lambda t: t) if mode == 'score' else (lambda t: t[0])
        check_run(view(out16), view(out32), k, f'{name} {mode} {pool}')
    with pytest.raises(AssertionError):                                        # the reference's call convention: bs == 1
        m(keypoint=_videos(2), return_loss=False)


@pytest.mark.parametrize('mode,pool', F.MODEL_RUNS)
def test_engine_eager_replayed_and_forward_test_agree(mode, pool):
    m = _model('model_reduced', **_cfg_of(mode, pool))
    x = X1.to(DEV)
    want = m(keypoint=x, return_loss=False)
    eager = D.InferEngine(m, use_graph=False)(x)
    eng = D.InferEngine(m)
    got = _replayed(eng, x)
    assert got.is_cuda and got.dtype == torch.float16 and same_bits(got, eager)
    assert same_bits((got if mode == 'score' else got[0]).cpu().numpy(), want)
    # the extraction config is part of the graph key: another pool_opt is another graph, not a stale replay
    m.test_cfg['pool_opt'] = 'm'
    assert not eng.graphed(x)
    other = eng(x)
    assert other.shape != got.shape and same_bits(other, D.InferEngine(m, use_graph=False)(x))
    m.test_cfg['pool_opt'] = pool
    assert eng.graphed(x) and same_bits(eng(x), got)


@pytest.mark.parametrize('mode,pool', [('feat', 'nmtv'), ('feat', 't'), ('score', 'nm'), ('score', 'none')])
def test_batch_of_videos_and_max_views(mode, pool):
    """3 videos in one call == three single-video calls, bit for bit (pooling never crosses videos); chunks of whole
    videos (max_views) == the undivided call."""
    m = _model('model_reduced', **_cfg_of(mode, pool))
    x = _videos(3)
    whole = _replayed(D.InferEngine(m), x)
    assert whole.shape[0] == 3
    single = D.InferEngine(m, use_graph=False)
    for i in range(3):
        assert same_bits(single(x[i:i + 1])[0], whole[i]), i
        want = m(keypoint=x[i:i + 1], return_loss=False)
        assert same_bits((whole[i:i + 1] if mode == 'score' else whole[i]).cpu().numpy(), want)
    eng = D.InferEngine(m, max_views=2 * F.MODEL_CLIPS)
    assert eng._chunks(3, F.MODEL_CLIPS) == [(0, 2), (2, 3)]
    for _ in range(2):
        eng(x)
    got = eng(x)
    assert len(eng._graphs) == 2 and eng.capture_error is None and same_bits(got, whole)


def test_scores_are_untouched_when_the_keys_are_unset():
    """Same model, no extraction keys: the engine scores as forward_test does (the bar of test_test_model_end_to_end), and
    setting then clearing the keys leaves the captured scoring graph answering with the same bits."""
    m = _model('model_reduced')
    x = _videos(3)
    want = m(keypoint=x, return_loss=False)
    assert want.dtype == np.float32 and want.shape == (3, 12)
    eng = D.InferEngine(m)
    got = _replayed(eng, x)
    assert got.dtype == torch.float32 and rel(got.cpu().numpy(), want) < 1e-6
    m.test_cfg.update(feat_ext=True, pool_opt='tv')
    assert eng(x).dtype == torch.float16
    m.test_cfg.update(feat_ext=False)
    assert eng.graphed(x) and same_bits(eng(x), got)


def test_pooled_shortcut_skips_the_activation():
    """With 't' and 'v' both pooled the backbone is asked for plane means (pool=True), from the engine and from
    forward_test, in both modes: the activation is never written.  With either axis kept it is the whole activation."""
    m = _model('model_reduced', feat_ext=True, pool_opt='mtv')
    calls = []
    real = m.backbone.forward

    def spy(x, pool=False):
        calls.append(pool)
        return real(x, pool=pool)

    m.backbone.forward = spy
    x = _videos(2)
    out = D.InferEngine(m, use_graph=False)(x)
    assert calls == [True] and tuple(out.shape) == (2, F.MODEL_CLIPS, 1, 32, 1, 1)
    m.test_cfg.update(feat_ext=False, score_ext=True, pool_opt='vt')
    D.InferEngine(m, use_graph=False)(x)
    m(keypoint=x[:1], return_loss=False)
    assert calls == [True, True, True]
    m.test_cfg['pool_opt'] = 'nmt'                                             # joints kept: the whole activation
    out = D.InferEngine(m, use_graph=False)(x)
    assert calls[-1] is False and tuple(out.shape) == (2, 1, 1, 12, 1, 25)


@pytest.mark.parametrize('mode,pool', [('feat', 'tv'), ('score', 'nm')])
def test_test_model_returns_one_array_per_video(tmp_path, mode, pool):
    m = _model('model_reduced', **_cfg_of(mode, pool))
    x = _videos(5).cpu()
    data = [dict(keypoint=x[i].numpy(), label=i) for i in range(5)]
    cfg = D.Config(dict(data=dict(test_dataloader=dict(videos_per_gpu=2)), work_dir=str(tmp_path)))
    out = str(tmp_path / 'maps.pkl')
    res = D.test_model(m, data, cfg, out=out)
    assert res['metrics'] is None and len(res['results']) == 5
    back = D.load_results(out)
    for i, (a, b) in enumerate(zip(res['results'], back)):
        want = m(keypoint=x[i:i + 1].to(DEV), return_loss=False)
        assert a.dtype == b.dtype == np.float16 and same_bits(a, want) and same_bits(b, want), i
    assert res['results'][0].shape == ((F.MODEL_CLIPS, F.MODEL_M, 32, 1, 1) if mode == 'feat' else (1, 1, 1, 12, 8, 25))
    with pytest.raises(ValueError, match='pkl'):
        D.test_model(m, data, cfg, out=str(tmp_path / 'maps.json'))
