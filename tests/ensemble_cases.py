"""Shared cases of tests/test_ensemble_host.py and tests/test_ensemble_gpu.py: synthetic annotations in the style of
tests/golden/pipeline_cases.py, the single-feature pipelines of a multi-stream test pass, and four small models."""
import json
import os

import numpy as np
import torch

import pipeline_cases as PC

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CLIP_LEN = 8
FEATURE_LISTS = [['j', 'b', 'jm', 'bm'], ['b', 'jm'], ['j']]      # all four; two, out of code order; S = 1

_TAIL = [dict(type='Collect', keys=['keypoint', 'label'], meta_keys=[]), dict(type='ToTensor', keys=['keypoint'])]


def annotations_3d():
    """One and two persons, 5 raw frames (shorter than the clip: repeated frames, the last one without a successor) and
    40 raw frames."""
    rng = np.random.RandomState(515)
    out = []
    for i, (M, T) in enumerate([(2, 40), (1, 5), (1, 40), (2, 5)]):
        base = rng.randn(1, 1, 25, 3).astype(np.float32) * 0.4 + np.array([0.2, 0.1, 3.0], dtype=np.float32)
        kp = (base + np.cumsum(rng.randn(M, T, 1, 3).astype(np.float32) * 0.02, axis=1)
              + rng.randn(M, T, 25, 3).astype(np.float32) * 0.05).astype(np.float32)
        out.append(dict(frame_dir=f'e{i}', label=(7 * i) % 12, keypoint=kp, total_frames=T))
    return out


def pipe_3d(feat, mode='zero', clip_len=CLIP_LEN, num_clips=2, **norm):
    return [dict(type='PreNormalize3D', **norm), dict(type='GenSkeFeat', feats=[feat]),
            dict(type='UniformSample', clip_len=clip_len, num_clips=num_clips, test_mode=True), dict(type='PoseDecode'),
            dict(type='FormatGCNInput', num_person=2, mode=mode)] + _TAIL


def annotations_2d(dtype):
    """The coco clips of pipeline_cases stored in ``dtype`` (fp16: the reference's feature arithmetic rounds to fp16)."""
    return [a for a in PC.annotations_2d() if a['keypoint'].dtype == dtype]


def pipe_2d(feat):
    return [dict(type='PreNormalize2D', img_shape=(1080, 1920)), dict(type='GenSkeFeat', dataset='coco', feats=[feat]),
            dict(type='UniformSample', clip_len=CLIP_LEN, num_clips=2, test_mode=True), dict(type='PoseDecode'),
            dict(type='FormatGCNInput', num_person=2)] + _TAIL


def pipe_k400(feat):
    """The compressed-pose order: features of the SAMPLED frames, five person slots (clip 1 fills one of them)."""
    return [dict(type='DecompressPose', squeeze=True, max_person=10),
            dict(type='UniformSampleFrames', clip_len=CLIP_LEN, num_clips=2, test_mode=True), dict(type='PoseDecode'),
            dict(type='PoseCompact', hw_ratio=1., allow_imgpad=True), dict(type='GenSkeFeat', dataset='coco', feats=[feat]),
            dict(type='FormatGCNInput', num_person=5)] + _TAIL


# name -> (annotations, feature -> pipeline)
INPUT_CASES = {
    'ntu3d_zero': (annotations_3d, lambda f: pipe_3d(f, 'zero')),
    'ntu3d_loop': (annotations_3d, lambda f: pipe_3d(f, 'loop')),
    'coco_fp16': (lambda: annotations_2d(np.float16), pipe_2d),
    'coco_fp32': (lambda: annotations_2d(np.float32), pipe_2d),
    'k400_compact': (PC.annotations_k400, pipe_k400),
}


def reduced_model(seed, classes=12):
    """DS-STGCN at the widths of tests/golden/model_reduced_cfg.json, live dynamic-adjacency parameters and running
    statistics off their start values; ``seed`` decides every parameter."""
    import dsgcn_amd as D
    from closed_form import fill_running, liven32
    with open(os.path.join(GOLD, 'model_reduced_cfg.json')) as f:
        cfg = json.load(f)
    cfg['backbone']['tcn_ms_cfg'] = [tuple(c) if isinstance(c, list) else c for c in cfg['backbone']['tcn_ms_cfg']]
    cfg['cls_head']['num_classes'] = classes
    torch.manual_seed(seed)
    np.random.seed(seed)
    m = D.build_model(cfg)
    liven32(m, seed + 1, 0.5)
    fill_running(m)
    return m


def host_sum(stream_rows, weights):
    """``ensemble_results``' fp32 sum of S (N, K) arrays -> (N, K)."""
    import dsgcn_amd as D
    return np.stack(D.ensemble_results([list(r) for r in stream_rows], weights)['results'])
