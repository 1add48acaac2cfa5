"""K-B for ``dggcn`` at any number of subsets: the autograd function and the ``dynadj``-style front of the plain
dynamic-adjacency kernels (csrc/dynadj_plain.hip, ``dsgcn_dynplain_*``).  ``dsgcn_amd.kernels`` re-exports
``dynadj_plain``; the helpers (K-C ``pwconv``, stacked weights, ordered column sums) are that module's.  Checked at full
batch against fp64 by tests/test_dggcn_plain_gpu.py."""
import torch

from . import native
from . import kernels as _K
from .kernels import _f32c, _ptr

MAX_SUBSETS, MAX_MID, MAX_JOINTS = 16, 64, 32      # csrc/dynadj_plain.hip: MAXK, MAXM, MAXV


def check_range(who, K, mid, V):
    """NotImplementedError naming the value that lies outside what the plain K-B implements."""
    if not 1 <= K <= MAX_SUBSETS:
        raise NotImplementedError(f'{who}: num_subsets (A.size(0)) = {K}: the plain K-B implements 1 <= K <= {MAX_SUBSETS}')
    if not 1 <= mid <= MAX_MID:
        raise NotImplementedError(f'{who}: mid_channels = {mid}: the plain K-B implements 1 <= mid <= {MAX_MID}')
    if not 1 <= V <= MAX_JOINTS:
        raise NotImplementedError(f'{who}: {V} joints: the plain K-B implements V <= {MAX_JOINTS}')


class _PlainAdj(torch.autograd.Function):
    """proj (n, 2*K*mid, ld) rows [conv1 | conv2] (ld >= V: padded joint stride) -> Ahat (n, K*mid, V, V): the plain K-B
    (csrc/dynadj_plain.hip), one launch each way."""

    @staticmethod
    def forward(ctx, proj, A, alpha, beta, defer_ok):
        _K._require_cuda(proj, A)
        proj, A, alpha, beta = [_f32c(t) for t in (proj, A, alpha, beta)]
        n, R, ld = proj.shape
        K, V = A.shape[0], A.shape[-1]
        mid = R // (2 * K)
        assert R == 2 * K * mid and alpha.numel() == K and beta.numel() == K, (R, K, alpha.shape, beta.shape)
        ahat = torch.empty((n, K * mid, V, V), device=proj.device, dtype=torch.float32)
        rc = native.lib().dsgcn_dynplain_fwd(_ptr(proj), _ptr(A), _ptr(alpha), _ptr(beta), _ptr(ahat), n, K,
                                             mid, V, ld, _K._stream())
        native.check(rc, 'dsgcn_dynplain_fwd')
        ctx.save_for_backward(proj, alpha, beta)
        ctx.dims = (n, K, mid, V, ld)
        ctx.defer_ok = defer_ok
        return ahat

    @staticmethod
    def backward(ctx, dahat):
        proj, alpha, beta = ctx.saved_tensors
        n, K, mid, V, ld = ctx.dims
        dahat = _f32c(dahat)
        lib = native.lib()
        dproj = torch.empty_like(proj)
        pstride = lib.dsgcn_dynplain_partial_stride(K, V)
        ppar = torch.empty((n, pstride), device=proj.device, dtype=torch.float32)      # per-sample parameter partials
        rc = lib.dsgcn_dynplain_bwd(_ptr(proj), _ptr(alpha), _ptr(beta), _ptr(dahat), _ptr(dproj),
                                    _ptr(ppar), pstride, n, K, mid, V, ld, _K._stream())
        native.check(rc, 'dsgcn_dynplain_bwd')
        red = _K.param_colsum(ppar, bool(ctx.defer_ok))                                # ordered sum over samples: deterministic
        o = K * V * V
        return dproj, red[:o].view(K, V, V), red[o:o + K], red[o + K:o + 2 * K], None


def dynadj_plain(xbar, A, alpha, beta, w1, b1, w2, b2, single_use=True):
    """Dynamic adjacency of ``dggcn`` for K = A.shape[0] subsets: Ahat (n, K*mid, V, V) from xbar (n, Ci, V or 32).
    conv1 / conv2 (``w1`` / ``w2`` (K*mid, Ci)) are one K-C launch on xbar padded to 32 joints (as in ``dynadj``); the rest
    is one plain K-B launch each way.  ``alpha`` / ``beta`` hold K values (a unit without subset_wise passes
    ``alpha[0].expand(K)``: autograd adds the K sums).  Parameter partials are ordered column sums."""
    K, V = A.shape[0], A.shape[-1]
    mid = w1.shape[0] // K
    if w1.shape[0] != K * mid or w2.shape[0] != K * mid:
        raise ValueError(f'dynadj_plain: {w1.shape[0]} / {w2.shape[0]} projection rows for {K} subsets')
    check_range('dynadj_plain', K, mid, V)
    proj = _K._kb_projections(xbar, V, [w1, w2], [b1, b2])
    defer_ok = bool(single_use) and _K._leafish(A, alpha, beta)
    return _PlainAdj.apply(proj, A, alpha, beta, defer_ok)
