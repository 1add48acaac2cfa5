"""The ops of the test pass: the front of the one-launch test-time head (csrc/head_test.hip, ``dsgcn_head_test_fwd``), the
feature / score-map extraction (csrc/featext.hip, ``dsgcn_feat_ext_fwd``) and the switch that gives an
``infer.InferEngine`` a weight-image table of its own.  ``dsgcn_amd.kernels`` re-exports them.
Checked against fp64 by tests/test_infer_gpu.py and tests/test_feat_ext_gpu.py."""
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


POOL_BITS = dict(n=1, m=2, t=4, v=8)      # dsgcn_feat_ext_fwd's pool_mask


def parse_pool_opt(pool_opt):
    """``test_cfg['pool_opt']`` -> pool_mask.  'none': 0; 'all': nmtv (the reference's evident intent: its line 74 compares
    where it means to assign); otherwise letters of n m t v as a SET — the means commute up to fp32 rounding, a repeated
    letter counts once.  Anything else: AssertionError, like the reference's ``assert digit in dim_idx``."""
    assert isinstance(pool_opt, str), f'pool_opt {pool_opt!r} is not a string'
    if pool_opt == 'none':
        return 0
    if pool_opt == 'all':
        return 15
    mask = 0
    for letter in pool_opt:
        assert letter in POOL_BITS, f'pool_opt {pool_opt!r}: {letter!r} is none of n, m, t, v'
        mask |= POOL_BITS[letter]
    return mask


def feat_ext_shape(videos, clips, persons, channels, T, V, pool, num_classes=None):
    """Shape of ``feat_ext``'s result from the sizes alone (no GPU): (videos, n', m', C | K, t', v'), a pooled axis having
    extent 1.  pool: a pool_opt string or a mask.  num_classes: K in score mode, None in feature mode."""
    mask = parse_pool_opt(pool) if isinstance(pool, str) else int(pool)
    if mask & ~15:
        raise ValueError(f'feat_ext: pool mask {mask} has bits outside n m t v')
    return (int(videos), 1 if mask & 1 else int(clips), 1 if mask & 2 else int(persons),
            int(channels if num_classes is None else num_classes), 1 if mask & 4 else int(T), 1 if mask & 8 else int(V))


def feat_ext(x, videos, clips, persons, pool, weight=None, bias=None, want_fp32=False):
    """Feature / score-map extraction in ONE launch (csrc/featext.hip): the mean over the axes of ``pool`` (a pool_opt
    string or a mask; 'n' = the clips of one video) and, with ``weight`` (K, C), the Linear at every remaining position.
    x (videos*clips*persons, C, T, V) — the backbone's (N, M, C, T, V) activation, N = videos*clips, is taken as it comes —
    or plane means (videos*clips*persons, C).  -> float16 (videos, n', m', C | K, t', v');  ``want_fp32``: -> (float16,
    float32), the float16 being the float32 rounded to nearest even.  No gradient."""
    _K._require_cuda(x)
    mask = parse_pool_opt(pool) if isinstance(pool, str) else int(pool)
    N, Q, M = int(videos), int(clips), int(persons)
    x = _K._f32c(x.detach())
    if x.dim() == 5:
        x = x.flatten(0, 1)
    elif x.dim() == 3:
        x = x.flatten(0, 1)[:, :, None, None]
    elif x.dim() == 2:
        x = x[:, :, None, None]
    if x.dim() != 4 or x.shape[0] != N * Q * M:
        raise ValueError(f'feat_ext: x {tuple(x.shape)} is not {N} videos x {Q} clips x {M} persons of (C, T, V) planes')
    C, T, V = x.shape[1:]
    K = None
    if weight is not None:
        _K._require_cuda(weight)
        weight, bias = _K._f32c(weight.detach()), _K._f32c(None if bias is None else bias.detach())
        K = weight.shape[0]
        if weight.dim() != 2 or weight.shape[1] != C or (bias is not None and tuple(bias.shape) != (K,)):
            raise ValueError(f'feat_ext: weight {tuple(weight.shape)} / bias do not fit {C} channels')
    shape = feat_ext_shape(N, Q, M, C, T, V, mask, K)
    out16 = torch.empty(shape, device=x.device, dtype=torch.float16)
    out32 = torch.empty(shape, device=x.device, dtype=torch.float32) if want_fp32 else None
    rc = native.lib().dsgcn_feat_ext_fwd(_K._ptr(x), _K._ptr(weight), _K._ptr(bias), N, Q, M, C, T, V, K or 0, mask,
                                         _K._ptr(out32), _K._ptr(out16), _K._stream())
    native.check(rc, 'dsgcn_feat_ext_fwd')
    return (out16, out32) if want_fp32 else out16


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
