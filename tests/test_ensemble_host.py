"""CPU: the multi-stream test pass — exports and bindings of dsgcn_skeleton_prep_streams / dsgcn_head_ensemble_fwd, their
argument rejection, StreamBatcher's pipeline comparison and plan, the stream-weight strings."""
import ctypes

import numpy as np
import pytest

import dsgcn_amd as D
from dsgcn_amd import kernels_infer, native

import ensemble_cases as EC
import pipeline_cases as PC

NEW = ('dsgcn_skeleton_prep_streams', 'dsgcn_head_ensemble_fwd')


def test_symbols_exported_and_bound():
    lib = native.lib()
    for name in NEW:
        assert name in native.SIGNATURES
        assert hasattr(lib, name)


def _table(n, value=64):
    return (ctypes.c_void_p * n)(*([value] * n))


def test_skeleton_prep_streams_rejects_without_gpu():
    lib = native.lib()
    p = 64                                      # any non-NULL address: a rejected call reads none of them
    sizes = (1, 1, 2, 8, 25, 3)
    assert lib.dsgcn_skeleton_prep_streams(None, None, None, None, None, None, None, None, None, None, None, *sizes,
                                           1, 0, 0, 0, None) == -1
    assert lib.dsgcn_skeleton_prep_streams(p, p, p, p, p, p, p, p, p, p, None, *sizes, 1, 0, 0, 0, None) == -1
    assert lib.dsgcn_skeleton_prep_streams(p, p, p, p, p, p, p, p, p, p, _table(4), *sizes, 5, 0, 0, 0, None) == -1
    assert lib.dsgcn_skeleton_prep_streams(p, p, p, p, p, p, p, p, p, p, _table(4), *sizes, 0, 0, 0, 0, None) == -1
    assert lib.dsgcn_skeleton_prep_streams(p, p, p, p, p, p, p, p, p, p, _table(4, None), *sizes, 2, 4, 0, 0, None) == -1
    assert lib.dsgcn_skeleton_prep_streams(p, p, p, p, p, p, p, p, p, p, _table(4), 1, 1, 2, 8, 25, 4, 2, 4, 0, 0,
                                           None) == -1                                                  # C = 4


def test_head_ensemble_rejects_without_gpu():
    lib = native.lib()
    p = 64
    t = _table(9)
    ok = (2, 2, 2, 8, 5)                        # N, clips, M, C, K
    assert lib.dsgcn_head_ensemble_fwd(None, None, None, None, 2, *ok, 0, None, None, None) == -1
    assert lib.dsgcn_head_ensemble_fwd(t, t, t, p, 0, *ok, 0, p, p, None) == -1
    assert lib.dsgcn_head_ensemble_fwd(t, t, t, p, 9, *ok, 0, p, p, None) == -1
    assert lib.dsgcn_head_ensemble_fwd(t, t, t, p, 2, *ok, 2, p, p, None) == -1                         # per-clip mode
    assert lib.dsgcn_head_ensemble_fwd(t, t, t, p, 2, *ok, 0, p, None, None) == -1                      # no out
    assert lib.dsgcn_head_ensemble_fwd(t, _table(9, None), t, p, 2, *ok, 0, p, p, None) == -1           # w[s] NULL
    assert lib.dsgcn_head_ensemble_fwd(t, t, t, p, 2, 2, 0, 2, 8, 5, 0, p, p, None) == -1               # clips = 0
    assert lib.dsgcn_head_ensemble_fwd(t, t, None, p, 2, 2, 24, 2, 256, 400, 0, p, p, None) == -2       # LDS, no launch


@pytest.mark.parametrize('clips,C,K', [(1, 4, 2), (10, 256, 60), (23, 256, 400), (24, 256, 400), (60, 256, 0), (61, 256, 0),
                                       (10, 1024, 512), (10, 1024, 513)])
def test_head_ensemble_fits_is_head_test_fits(clips, C, K):
    assert kernels_infer.head_ensemble_fits(clips, C, K) == kernels_infer.head_test_fits(clips, C, K)
    assert kernels_infer.head_ensemble_fits(clips, C, K) == (clips * (C + K) * 4 <= 60 * 1024)


def test_head_ensemble_per_clip_mode_is_a_value_error():
    with pytest.raises(ValueError, match='per-clip'):
        kernels_infer.head_ensemble([], [], None, 1, 1, 1, average_clips=None)


def test_pipeline_mismatch_names_the_key():
    four = [EC.pipe_3d(f) for f in ('j', 'b', 'jm', 'bm')]
    assert D.StreamBatcher(four).feats == ['j', 'b', 'jm', 'bm']
    with pytest.raises(ValueError, match=r'UniformSample\.clip_len: 60 != 100'):
        D.StreamBatcher([EC.pipe_3d('j', clip_len=60)] + [EC.pipe_3d(f, clip_len=100) for f in ('b', 'jm', 'bm')])
    with pytest.raises(ValueError, match=r'PreNormalize3D\.align_spine'):
        D.StreamBatcher([EC.pipe_3d('j'), EC.pipe_3d('b', align_spine=False)])
    two = EC.pipe_3d('j')
    two[1] = dict(type='GenSkeFeat', feats=['j', 'b'])
    with pytest.raises(ValueError, match=r'GenSkeFeat\.feats'):
        D.StreamBatcher([EC.pipe_3d('b'), two])
    with pytest.raises(ValueError, match=r'GenSkeFeat\.dataset'):
        D.StreamBatcher([EC.pipe_2d('j'),
                         [dict(t, dataset='openpose') if t['type'] == 'GenSkeFeat' else t for t in EC.pipe_2d('b')]])
    with pytest.raises(ValueError, match='1 to 4'):
        D.StreamBatcher([])
    # a list where the other pipeline has a tuple is the same argument
    same = EC.pipe_3d('b')
    same[0] = dict(type='PreNormalize3D', zaxis=(0, 1))
    first = EC.pipe_3d('j')
    first[0] = dict(type='PreNormalize3D', zaxis=[0, 1])
    assert len(D.StreamBatcher([first, same])) == 2


def test_stream_weight_strings():
    assert D.parse_stream_weights('2:2:1:1') == (2.0, 2.0, 1.0, 1.0)
    assert D.parse_stream_weights('0.3:0.7:0.11', 3) == (0.3, 0.7, 0.11)
    assert D.parse_stream_weights('four', 4) == (2.0, 2.0, 1.0, 1.0) and D.parse_stream_weights('two') == (1.0, 1.0)
    assert D.parse_stream_weights([1, 2.5], 2) == (1.0, 2.5)
    assert D.STREAM_WEIGHTS == {'two': (1, 1), 'four': (2, 2, 1, 1)}
    with pytest.raises(ValueError, match='4 weights for 2 streams'):
        D.parse_stream_weights('2:2:1:1', 2)
    with pytest.raises(ValueError):
        D.parse_stream_weights('2:x')
    with pytest.raises(ValueError, match='2 weights for 4 streams'):
        D.test_ensemble([None] * 4, None, {}, weights=(1, 1))


def _state_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize('train', [True, False])
def test_stream_plan_draws_like_the_single_plan(train):
    """S = 4: numpy's RNG is consumed once per clip, not once per stream — same state afterwards, same decisions."""
    key = 'train_j' if train else 'test10_seeded'
    def pipe(f):
        return [dict(t, feats=[f]) if t['type'] == 'GenSkeFeat' else dict(t) for t in PC.pipelines()[key]]
    store = D.SkeletonStore(PC.annotations(), plan_only=True)
    idx = [0, 1, 2, 3, 4, 5, 6, 3]
    np.random.seed(31)
    p1 = D.SkeletonBatcher(pipe('j')).plan(store, idx)
    s1 = np.random.get_state()
    np.random.seed(31)
    p4 = D.StreamBatcher([pipe(f) for f in ('j', 'b', 'jm', 'bm')]).plan(store, idx)
    s4 = np.random.get_state()
    assert _state_equal(s1, s4)
    assert sorted(p1) == sorted(p4)
    for k in p1:
        assert np.array_equal(p1[k], p4[k]), k
    if train:                                       # (the draws were real: another seed gives other frames)
        np.random.seed(32)
        assert not np.array_equal(D.SkeletonBatcher(pipe('j')).plan(store, idx)['f0'], p1['f0'])
