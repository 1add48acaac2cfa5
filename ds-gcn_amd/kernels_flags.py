"""K-B for the ``dgphgcn1`` ablation arms: the autograd function and the ``dynadj``-style front of the flag-specialised
dynamic-adjacency kernels (csrc/dynadj_flags.hip, ``dsgcn_dynflag_*``).  ``dsgcn_amd.kernels`` re-exports ``dynadj_flags``;
the helpers (K-C ``pwconv``, stacked weights, ordered column sums) are that module's.  Checked at full batch against fp64
for every compile-time instantiation by tests/test_dgphgcn1_flags_gpu.py."""
import torch

from . import native
from . import kernels as _K
from .kernels import _f32c, _ptr


class _FlagAdj(torch.autograd.Function):
    """proj (n, R, ld) [conv1 | conv2 | conv1_se], pq (n, E*mid, 2, 32) or None, ada_linears (wa, ba) or None -> Ahat
    (n, 3*mid, V, V): the flag-specialised K-B (csrc/dynadj_flags.hip), one launch each way."""

    @staticmethod
    def forward(ctx, proj, pq, be, wa, ba, A, alpha, beta, node_type, edge_type, mid, P, E, flags, defer_ok):
        _K._require_cuda(proj, A)
        proj, pq, be, wa, ba, A, alpha, beta = [_f32c(t) for t in (proj, pq, be, wa, ba, A, alpha, beta)]
        n, R, ld = proj.shape
        V = A.shape[-1]
        assert A.shape[0] == 3 and alpha.numel() == 3 and beta.numel() == 3
        assert R == (6 * mid if not flags & 3 else 4 * mid + mid * P), (R, mid, P, flags)
        assert node_type.dtype == torch.int32 and edge_type.dtype == torch.int32
        assert node_type.numel() == V and edge_type.numel() == V * V
        if flags & 4:
            assert tuple(pq.shape) == (n, E * mid, 2, 32) and be.numel() == E * mid
        if flags & 8:
            assert wa.numel() == 9 * E and ba.numel() == 3 * E
        ahat = torch.empty((n, 3 * mid, V, V), device=proj.device, dtype=torch.float32)
        rc = native.lib().dsgcn_dynflag_fwd(_ptr(proj), _ptr(pq), _ptr(be), _ptr(wa), _ptr(ba), _ptr(A), _ptr(alpha),
                                            _ptr(beta), _ptr(node_type), _ptr(edge_type), _ptr(ahat), n, mid, V, ld, P, E,
                                            flags, _K._stream())
        native.check(rc, 'dsgcn_dynflag_fwd')
        ctx.save_for_backward(proj, pq, be, wa, ba, alpha, beta, node_type, edge_type)
        ctx.dims = (n, mid, V, ld, P, E, flags)
        ctx.defer_ok = defer_ok
        return ahat

    @staticmethod
    def backward(ctx, dahat):
        proj, pq, be, wa, ba, alpha, beta, node_type, edge_type = ctx.saved_tensors
        n, mid, V, ld, P, E, flags = ctx.dims
        dahat = _f32c(dahat)
        lib = native.lib()
        dd = torch.empty_like(dahat)
        dproj = torch.empty_like(proj)
        dpq = torch.empty_like(pq) if pq is not None else None
        pstride = lib.dsgcn_dynflag_partial_stride(mid, V, E, flags)
        ppar = torch.empty((n, pstride), device=proj.device, dtype=torch.float32)
        rc = lib.dsgcn_dynflag_bwd(_ptr(proj), _ptr(pq), _ptr(be), _ptr(wa), _ptr(ba), _ptr(alpha), _ptr(beta),
                                   _ptr(node_type), _ptr(edge_type), _ptr(dahat), _ptr(dd), _ptr(dproj), _ptr(dpq),
                                   _ptr(ppar), pstride, n, mid, V, ld, P, E, flags, _K._stream())
        native.check(rc, 'dsgcn_dynflag_bwd')
        per_subset = bool(flags & 16)
        # scalar alpha / beta: the three per-subset sums are added below, so they are needed now (no deferred sum)
        red = _K.param_colsum(ppar, bool(ctx.defer_ok) and per_subset)             # ordered sum over samples: deterministic
        o = 3 * V * V
        dA, dalpha, dbeta = red[:o].view(3, V, V), red[o:o + 3], red[o + 3:o + 6]
        if not per_subset:                         # alpha[0] / beta[0] scale every subset; entries 1: get an exact zero
            ab = torch.zeros(2, 3, device=proj.device, dtype=torch.float32)
            ab[:, 0] = red[o:o + 6].view(2, 3).sum(1)
            dalpha, dbeta = ab[0], ab[1]
        o += 6
        dbe = dwa = dba = None
        if flags & 4:
            dbe = red[o:o + E * mid]
            o += E * mid
        if flags & 8:
            dwa, dba = red[o:o + 9 * E].view(3 * E, 3), red[o + 9 * E:o + 12 * E]
        return dproj, dpq, dbe, dwa, dba, dA, dalpha, dbeta, None, None, None, None, None, None, None


def dynadj_flags(xbar, A, alpha, beta, w1, b1, w2, b2, wse, bse, we, be, wa, ba, node_type, edge_type, P, E, subset_wise,
                 single_use=True):
    """Dynamic adjacency of ``dgphgcn1`` outside its shipped flag set.  conv1 / conv2 (/ conv1_se: ``wse`` (mid*P rows) or
    None = decompose off) are one K-C launch on xbar padded to 32 joints (as in ``dynadj``); the edge linear of subset 1
    (``we`` (E*mid, mid), ``be``; None: no edge attention — no product, no partials) is one K-C launch over [x1_1 | x2_1]
    viewed as a (n, mid, 2, 32) clip; ``wa`` (3E, 3) / ``ba``: ada_linears, the class mix of the Gram (None: off).  The
    rest is one flag-specialised K-B launch each way; parameter partials are ordered column sums."""
    sem = 0 if wse is None else (2 if P > 1 else 1)
    mid = w1.shape[0] // (3 if sem == 0 else 2)
    if we is not None and sem == 0:
        raise ValueError('dynadj_flags: the edge linear needs the decomposed layout')
    proj = _K._kb_projections(xbar, A.shape[-1], [w1, w2] + ([wse] if sem else []), [b1, b2] + ([bse] if sem else []))
    pq = None
    flags = sem | (16 if subset_wise else 0)
    if we is not None:
        x12 = torch.stack([proj[:, mid:2 * mid, :32], proj[:, 3 * mid:4 * mid, :32]], 2)
        pq = _K.pwconv(x12, None, None, None, False, we, None, 1, False)[0]
        flags |= 4
    if wa is not None:
        flags |= 8
    live = [t for t in (A, alpha, beta, be, wa, ba) if t is not None]
    defer_ok = bool(single_use) and _K._leafish(*live)
    return _FlagAdj.apply(proj, pq, be if we is not None else None, wa, ba, A, alpha, beta, node_type, edge_type, mid,
                          P if sem == 2 else 1, E, flags, defer_ok)
