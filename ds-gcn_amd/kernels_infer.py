"""The ops of the test pass: the front of the one-launch test-time head (csrc/head_test.hip, ``dsgcn_head_test_fwd``), of
the multi-stream head (csrc/head_ensemble.hip, ``dsgcn_head_ensemble_fwd``), the
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


ENSEMBLE_MAX = 8          # dsgcn_head_ensemble_fwd: streams per launch


def head_ensemble_fits(clips, C, K):
    """dsgcn_head_ensemble_fwd passes the streams through the same LDS one after another: ``head_test_fits``' limit,
    whatever the number of streams."""
    return head_test_fits(clips, C, K)


def head_ensemble(feats, weights_and_biases, stream_weights, videos, clips, persons, average_clips='prob',
                  want_streams=False):
    """The test-time heads of S models and their weighted sum in ONE launch (csrc/head_ensemble.hip).
    feats: S tensors (videos*clips*persons, C) of plane means;  weights_and_biases: S pairs (weight (K, C), bias (K) |
    None), one C and one K for all;  stream_weights: (S,) float32 DEVICE tensor (read by the launch: a captured graph
    follows its contents).  -> (videos, K): ((0 + w_0 p_0) + w_1 p_1) + ... in fp32, p_s being ``head_test``'s result for
    stream s bit for bit — ``ensemble_results`` of the S result sets.  ``want_streams``: -> (sum, (S, videos, K) p_s).
    ``average_clips`` 'prob' | 'score'; the per-clip mode (None) has no weighted sum: ValueError.  No gradient."""
    import ctypes
    if average_clips not in ('prob', 'score'):
        raise ValueError(f'head_ensemble: average_clips={average_clips!r}: "prob" or "score" (a weighted sum of per-clip '
                         'score lists is not defined)')
    S = len(feats)
    if not 1 <= S <= ENSEMBLE_MAX:
        raise ValueError(f'head_ensemble: {S} streams; 1 to {ENSEMBLE_MAX} fit one launch')
    if len(weights_and_biases) != S or stream_weights.numel() != S:
        raise ValueError(f'head_ensemble: {S} feature tensors, {len(weights_and_biases)} heads, '
                         f'{stream_weights.numel()} stream weights')
    N, Q, M = int(videos), int(clips), int(persons)
    keep, fp, wp, bp = [], [], [], []
    C = K = None
    for f, (w, b) in zip(feats, weights_and_biases):
        _K._require_cuda(f, w, b)
        f, w, b = _K._f32c(f.detach()), _K._f32c(w.detach()), _K._f32c(None if b is None else b.detach())
        if C is None:
            C, K = f.shape[1], w.shape[0]
        if tuple(f.shape) != (N * Q * M, C) or tuple(w.shape) != (K, C) or (b is not None and tuple(b.shape) != (K,)):
            raise ValueError(f'head_ensemble: feat {tuple(f.shape)}, weight {tuple(w.shape)}, {N} videos x {Q} clips x '
                             f'{M} persons, {C} channels and {K} classes do not fit together')
        keep += [f, w, b]
        fp.append(_K._ptr(f)); wp.append(_K._ptr(w)); bp.append(_K._ptr(b))
    _K._require_cuda(stream_weights)
    if stream_weights.dtype != torch.float32 or not stream_weights.is_contiguous():
        raise ValueError('head_ensemble: stream_weights is a contiguous float32 tensor on the device')
    if not head_ensemble_fits(Q, C, K):
        raise native.DsgcnError(f'dsgcn_head_ensemble_fwd: {Q} clips x ({C} channels + {K} classes) floats exceed the 60 KB '
                                'of LDS a video may take')
    out = torch.empty((N, K), device=stream_weights.device, dtype=torch.float32)
    so = torch.empty((S, N, K), device=stream_weights.device, dtype=torch.float32) if want_streams else None
    table = ctypes.c_void_p * S
    rc = native.lib().dsgcn_head_ensemble_fwd(table(*fp), table(*wp), table(*bp), _K._ptr(stream_weights), S, N, Q, M, C, K,
                                              HEAD_TEST_MODES[average_clips], _K._ptr(so), _K._ptr(out), _K._stream())
    native.check(rc, 'dsgcn_head_ensemble_fwd')
    del keep
    return (out, so) if want_streams else out


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


GRAPH_MODES = ('ctr', 'ahat')


def parse_graph_ext(value):
    """``test_cfg['graph_ext']`` -> None (False / absent), 'ctr' (True or 'ctr': ``A + alpha tanh(D)``, what the
    reference's hook rebuilds, core/hooks/feature_hook.py:74-110) or 'ahat' (the adjacency the layer aggregates with, the
    ``beta softmax`` term included).  Anything else: ValueError."""
    if value is False or value is None:
        return None
    if value is True:
        return 'ctr'
    if isinstance(value, str) and value in GRAPH_MODES:
        return value
    raise ValueError(f"test_cfg['graph_ext'] = {value!r}: one of False, True, 'ctr', 'ahat'")


def graph_pool(ahat, group, K, out, layer):
    """Per-video mean of one layer's adjacency over person-samples and channels (csrc/graphpool.hip), written into the
    caller's buffer: ahat (videos*group, K*mid, V, V) -> out[:, layer] of out (videos, L, K, V, V) float32.  ahat is read in
    place; at most two launches (the partial planes of the first live in a scratch tensor of this call).  No gradient."""
    _K._require_cuda(ahat, out)
    a = ahat.detach()
    if a.dtype != torch.float32 or not a.is_contiguous():
        raise ValueError('graph_pool: ahat is a contiguous float32 tensor (the kernel reads it where it lies)')
    n, KM, V, V2 = a.shape
    group, K, layer = int(group), int(K), int(layer)
    if V != V2 or group < 1 or n % group or K < 1 or KM % K:
        raise ValueError(f'graph_pool: ahat {tuple(a.shape)} is not (videos x {group} person-samples, {K} subsets x mid, V, V)')
    videos, mid = n // group, KM // K
    if (out.dim() != 5 or out.dtype != torch.float32 or not out.is_contiguous() or out.shape[0] != videos
            or tuple(out.shape[2:]) != (K, V, V) or not 0 <= layer < out.shape[1]):
        raise ValueError(f'graph_pool: out {tuple(out.shape)} is not a contiguous float32 ({videos}, L, {K}, {V}, {V}) '
                         f'buffer with a layer {layer}')
    lib = native.lib()
    splits = lib.dsgcn_graph_pool_splits(videos, group, K, mid, V)
    if splits < 0:
        native.check(splits, 'dsgcn_graph_pool')
    ws = torch.empty(videos * K * splits * V * V, device=a.device, dtype=torch.float32) if splits > 1 else None
    rc = lib.dsgcn_graph_pool(_K._ptr(a), _K._ptr(out), _K._ptr(ws), videos, group, K, mid, V, out.shape[1], layer,
                              _K._stream())
    native.check(rc, 'dsgcn_graph_pool')
    return out


class GraphCollector:
    """What ``graph_collect`` yields: the layer counter and the buffer the taps fill."""

    def __init__(self, group, mode, out):
        if mode not in GRAPH_MODES:
            raise ValueError(f'graph_collect: mode {mode!r}: one of {GRAPH_MODES}')
        self.group, self.mode, self.out = int(group), mode, out
        self.layer = 0

    def tap(self, unit, xbar, ahat):
        if self.layer >= self.out.shape[1]:
            raise RuntimeError(f'graph_collect: the buffer holds {self.out.shape[1]} layers and one more unit taps')
        if self.mode == 'ctr':
            # one more adjacency of the same unit with a zero beta: `+ 0 * softmax` is exact, so this is A + alpha tanh(D)
            # in the K-B kernels' own arithmetic; the layer's own Ahat is not touched
            ahat = unit.adjacency(xbar, beta=torch.zeros_like(unit.beta))
        _K.ops().graph_pool(ahat, self.group, unit.num_subsets, self.out, self.layer)
        self.layer += 1


_graph = None          # the active GraphCollector: the units' tap is `if _graph is not None`


@contextlib.contextmanager
def graph_collect(group, mode, out):
    """Collect the per-video learned adjacency of every dynamic-adjacency unit that runs inside the block: unit number l
    (in call order) fills ``out[:, l]`` of ``out`` (videos, L, K, V, V) float32 with the mean over the ``group`` consecutive
    person-samples of each video and over the channels of ``A + alpha tanh(D)`` (mode 'ctr') or of its whole Ahat
    ('ahat').  Evaluation only: eval-mode units under ``torch.no_grad()``."""
    global _graph
    if torch.is_grad_enabled():
        raise RuntimeError('graph_collect: graphs are collected under torch.no_grad() (a test-time pass)')
    if _graph is not None:
        raise RuntimeError('graph_collect: a collection is already active')
    _graph = GraphCollector(group, mode, out)
    try:
        yield _graph
    finally:
        _graph = None


def graph_tap(unit, xbar, ahat):
    """Called by every dynamic-adjacency unit right after ``adjacency()``: nothing unless a ``graph_collect`` is active."""
    if _graph is not None:
        if unit.training:
            raise RuntimeError('graph_collect: graphs are collected in eval mode')
        _graph.tap(unit, xbar, ahat)


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
