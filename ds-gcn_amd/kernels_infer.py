"""The ops of the test pass: the front of the one-launch test-time head (csrc/head_test.hip, ``dsgcn_head_test_fwd``) and
the switch that gives an ``infer.InferEngine`` a weight-image table of its own.  ``dsgcn_amd.kernels`` re-exports them.
Checked against fp64 by tests/test_infer_gpu.py."""
import contextlib

import torch

from . import native
from . import kernels as _K

HEAD_TEST_MODES = {'prob': 0, 'score': 1, None: 2}


def head_test_fits(clips, C, K):
    """dsgcn_head_test_fwd keeps a video's pooled features and scores in LDS (include/dsgcn.h states the limit)."""
    return int(clips) * (int(C) + int(K)) * 4 <= 60 * 1024


def head_test(feat, weight, bias, videos, clips, persons, average_clips='prob', want_clip_scores=False):
    """The test-time head in ONE launch (csrc/head_test.hip): person mean + Linear + ``average_clips`` over the clips.
    feat (videos*clips*persons, C) plane means -> (videos, K) for 'prob' / 'score', (videos, clips, K) for None.
    ``want_clip_scores``: -> (result, clip scores (videos, clips, K)).  No gradient."""
    _K._require_cuda(feat, weight)
    if average_clips not in HEAD_TEST_MODES:
        raise ValueError(f'{average_clips} is not supported. Supported: ["score", "prob", None]')
    mode = HEAD_TEST_MODES[average_clips]
    feat, weight, bias = _K._f32c(feat.detach()), _K._f32c(weight.detach()), _K._f32c(None if bias is None else bias.detach())
    N, Q, M = int(videos), int(clips), int(persons)
    R, C = feat.shape
    K = weight.shape[0]
    if R != N * Q * M or weight.shape[1] != C:
        raise ValueError(f'head_test: feat {tuple(feat.shape)}, weight {tuple(weight.shape)}, {N} videos x {Q} clips x '
                         f'{M} persons do not fit together')
    shape = (N, Q, K) if mode == 2 else (N, K)
    out = torch.empty(shape, device=feat.device, dtype=torch.float32)
    cs = out if mode == 2 else (torch.empty((N, Q, K), device=feat.device, dtype=torch.float32) if want_clip_scores else None)
    rc = native.lib().dsgcn_head_test_fwd(_K._ptr(feat), _K._ptr(weight), _K._ptr(bias), N, Q, M, C, K, mode, _K._ptr(cs),
                                          None if mode == 2 else _K._ptr(out), _K._stream())
    native.check(rc, 'dsgcn_head_test_fwd')
    return (out, cs) if want_clip_scores else out


@contextlib.contextmanager
def private_weight_images(jobs):
    """Run a forward OUTSIDE a training step with the weight-image table ``jobs`` (a dict the caller owns) in place of the
    process-wide one: the images it builds — and the pins a hipGraph capture puts on them — belong to the caller and die
    with it, and a TrainEngine in the same process never sees them in its per-step rebuild (nor the other way round).
    Outside a step every image is split on the spot (``_wsplit_image``, ``_StepBuilt.get``), so a captured forward
    carries the launches that rebuild its images from the weights of the moment."""
    st = _K._wsplit_state
    saved = st['jobs'], st['in_step']
    st['jobs'], st['in_step'] = jobs, False
    try:
        yield jobs
    finally:
        st['jobs'], st['in_step'] = saved
