"""CPU: the host side of the test pass (dsgcn_amd.test_model and friends) — argument rejection of the test-time head, the
result files and their ensemble, the rank sharding of a pass, the batch-size rule.  No GPU."""
import os
import sys

import numpy as np
import pytest

import dsgcn_amd as D
from dsgcn_amd import native
from dsgcn_amd.recognizers import interleave_parts
from dsgcn_amd.testing import test_batch_size as resolve_batch_size

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_head_test_rejects_bad_arguments_without_gpu():
    """NULL pointers / bad sizes / a bad mode / nothing to write are refused before any launch (DSGCN_EINVAL = -1); the
    pointers below are never dereferenced (every call fails its checks first)."""
    f = native.lib().dsgcn_head_test_fwd
    p = 4096                                                    # a non-NULL stand-in: the checks only compare with NULL
    ok = dict(feat=p, w=p, b=None, N=2, clips=10, M=2, C=256, K=60, mode=0, clip_score=None, out=p)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a['feat'], a['w'], a['b'], a['N'], a['clips'], a['M'], a['C'], a['K'], a['mode'], a['clip_score'], a['out'],
                 None)

    assert call(feat=None) == -1 and call(w=None) == -1
    for size in ('N', 'clips', 'M', 'C', 'K'):
        assert call(**{size: 0}) == -1 and call(**{size: -3}) == -1, size
    assert call(mode=3) == -1 and call(mode=-1) == -1
    assert call(out=None, clip_score=None) == -1                # both outputs NULL
    assert call(mode=2, out=p, clip_score=None) == -1           # mode 2 writes clip_score only
    assert call(clips=24, K=400) == -2                          # 24 * (256 + 400) floats: above the stated LDS limit


def test_head_test_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import codeobj_report
    native.build()
    ks = {k: v for k, v in codeobj_report.kernels(native.LIB_PATH).items() if k.startswith('k_head_test')}
    assert sorted(ks) == ['k_head_test<false>', 'k_head_test<true>']
    for name, k in ks.items():
        assert k.get('scratch_instructions', 0) == 0 and k.get('vgpr_spill_count', 0) == 0, (name, k)
        assert k.get('sgpr_spill_count', 0) == 0 and k.get('private_segment_fixed_size', 0) == 0, (name, k)


def _scores(seed, n=23, classes=7):
    return list(np.random.default_rng(seed).standard_normal((n, classes)).astype(np.float32))


@pytest.mark.parametrize('suffix', ['.pkl', '.json'])
def test_dump_and_ensemble_round_trip(tmp_path, suffix):
    sets = [_scores(s) for s in range(4)]                       # j, b, jm, bm
    labels = np.random.default_rng(9).integers(0, 7, 23)
    files = [D.dump_results(s, str(tmp_path / 'sub' / f'r{i}{suffix}')) for i, s in enumerate(sets)]
    for f, s in zip(files, sets):
        back = D.load_results(f)
        assert len(back) == 23 and all(b.dtype == np.float32 and np.array_equal(b, a) for a, b in zip(s, back))
    # unweighted: the plain sum, from files and from lists alike
    want = np.stack(sets[0]) + np.stack(sets[1]) + np.stack(sets[2]) + np.stack(sets[3])
    got = D.ensemble_results(files)
    assert got['metrics'] is None and np.allclose(np.stack(got['results']), want, rtol=0, atol=1e-6)
    assert np.array_equal(np.stack(D.ensemble_results(sets)['results']), np.stack(got['results']))
    # weights honoured, metrics = those of the summed scores
    w = [2.0, 1.0, 0.5, 0.0]
    got = D.ensemble_results([files[0], sets[1], files[2], sets[3]], weights=w, labels=labels)
    want = sum(np.stack(s) * np.float32(x) for s, x in zip(sets, w))
    assert np.allclose(np.stack(got['results']), want, rtol=0, atol=1e-6)
    top1, top5 = D.top_k_accuracy(want, labels, (1, 5))
    assert list(got['metrics']) == ['top1_acc', 'top5_acc', 'mean_class_accuracy']
    assert got['metrics']['top1_acc'] == float(top1) and got['metrics']['top5_acc'] == float(top5)
    assert got['metrics']['mean_class_accuracy'] == float(D.mean_class_accuracy(want, labels)[0])
    with pytest.raises(ValueError):
        D.ensemble_results(files, weights=[1, 2])
    with pytest.raises(ValueError):
        D.dump_results(sets[0], str(tmp_path / 'r.txt'))


@pytest.mark.parametrize('world', [1, 2, 3])
@pytest.mark.parametrize('n', [7, 9, 4])
def test_rank_sharding_reassembles_dataset_order(world, n):
    """What test_model does per rank (epoch_indices(shuffle=False): samples rank, rank + world, ..., wrapped to equal
    lengths) and what gather_results does with the parts (interleave, cut to the dataset length)."""
    parts = [[('score of', i) for i in D.epoch_indices(n, 0, 0, r, world, shuffle=False)] for r in range(world)]
    assert len({len(p) for p in parts}) == 1                    # every rank runs the same number of samples
    assert interleave_parts(parts, n) == [('score of', i) for i in range(n)]


def test_gather_results_without_process_group_is_the_identity_cut():
    assert D.gather_results([3, 1, 2, 9], 3) == [3, 1, 2]


def test_batch_size_resolution_order():
    assert resolve_batch_size(dict(data=dict(videos_per_gpu=16, test_dataloader=dict(videos_per_gpu=4)))) == 4
    assert resolve_batch_size(dict(data=dict(videos_per_gpu=16, test_dataloader=dict(workers_per_gpu=2)))) == 16
    assert resolve_batch_size(dict(data=dict(videos_per_gpu=16, val_dataloader=dict(videos_per_gpu=2)))) == 16
    assert resolve_batch_size(dict(data=dict(test=dict()))) == 1
    assert resolve_batch_size(dict()) == 1
    assert resolve_batch_size(D.Config(dict(data=dict(videos_per_gpu=8)))) == 8


def test_public_names():
    for name in ('InferEngine', 'test_model', 'dump_results', 'ensemble_results', 'EvalLoop'):
        assert hasattr(D, name), name
    assert 'dsgcn_head_test_fwd' in native.SIGNATURES
    import inspect
    assert inspect.signature(D.EvalLoop.__init__).parameters['engine'].default is None
