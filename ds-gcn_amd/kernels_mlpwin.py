"""``dgmsmlp``'s temporal stage: the autograd function of the mlp-window kernel (csrc/mlpwin.hip, ``dsgcn_mlpwin_*``), the
window stage around it with its staged form, and the op ``temporal_dgmlp``.  ``dsgcn_amd.kernels`` re-exports them; the
helpers (branch_act, tapconv, dwcausal, K-C ``pwconv``, ``fuse_out``, combine, ordered column sums) are that module's, reached
at call time.  Checked against fp64 by tests/test_dgmsmlp_gpu.py."""
import torch

from . import native
from . import kernels as _K


def _mlpwin_tables(branch_cfg, widths, add_tcn, merge_after):
    """ms_cfg-style branch list -> window tables of csrc/mlpwin.hip: (types, c0s, widths, dils, adds)."""
    types, c0s, bcs, dils, adds = [], [], [], [], []
    c0 = 0
    for cfg, bc in zip(branch_cfg, widths):
        mlp = not isinstance(cfg, str) and cfg[0] != 'max'
        types.append(0 if mlp else 1)
        dils.append(int(cfg[1]) if mlp else 1)
        adds.append((2 if merge_after else 1) if (mlp and add_tcn) else 0)
        c0s.append(c0)
        bcs.append(int(bc))
        c0 += int(bc)
    return types, c0s, bcs, dils, adds


def mlpwin_supported(n, C, T, V1, stride, KM, tables):
    """Does csrc/mlpwin.hip take this shape (dsgcn_mlpwin_supported)?  Asked before anything launches."""
    types, c0s, bcs, dils, adds = tables
    if len(types) > 8:
        return False
    ia = _K._int_array
    return native.lib().dsgcn_mlpwin_supported(n, C, T, V1, int(stride), int(KM), len(types), ia(types), ia(c0s), ia(bcs),
                                               ia(dils), ia(adds)) == 1


class _MlpWin(torch.autograd.Function):
    """The mlp windows of dgmsmlp over h (n,C,T,V1) and o (n,C,T',V1) -> u (n,C,T',V1): depthwise causal taps, the
    windows' bc x bc conv1 on the fp32 MFMA, the addend before / after it, copies of the other windows — one HIP launch per
    direction (csrc/mlpwin.hip).  w1b1: one conv1 weight per window, then one bias per window (None for copy windows)."""

    @staticmethod
    def forward(ctx, h, o, dw_w, dw_b, stride, types, c0s, bcs, dils, adds, *w1b1):
        _K._require_cuda(h, dw_w)
        ctx.defer_ok = _K._leafish(dw_w, dw_b, *w1b1)
        h, o, dw_w, dw_b = _K._f32c(h), _K._f32c(o), _K._f32c(dw_w), _K._f32c(dw_b)
        n, C, T, V1 = h.shape
        nwin = len(types)
        w1s = [None if t is None else _K._f32c(t.reshape(t.shape[0], -1)) for t in w1b1[:nwin]]
        b1s = [_K._f32c(t) for t in w1b1[nwin:]]
        KM = dw_w.shape[1]
        Tout = (T + stride - 1) // stride
        u = torch.empty((n, C, Tout, V1), device=h.device, dtype=torch.float32)
        tabs = (_K._int_array(types), _K._int_array(c0s), _K._int_array(bcs), _K._int_array(dils), _K._int_array(adds))
        ptr = _K._ptr
        rc = native.lib().dsgcn_mlpwin_fwd(ptr(h), ptr(o), ptr(u), ptr(dw_w), ptr(dw_b), n, C, T, V1, stride, KM, nwin,
                                           *tabs, _K._ptr_array(w1s), _K._ptr_array(b1s), _K._stream())
        native.check(rc, 'dsgcn_mlpwin_fwd')
        ctx.save_for_backward(h, o if 1 in adds else None, dw_w, dw_b, *[w for w in w1s if w is not None])
        ctx.cfg = (stride, tuple(types), tuple(c0s), tuple(bcs), tuple(dils), tuple(adds), o is not None, dw_b is not None,
                   tuple(None if t is None else tuple(t.shape) for t in w1b1[:nwin]), tuple(b is not None for b in b1s))
        return u

    @staticmethod
    def backward(ctx, du):
        h, o, dw_w, dw_b, *wsaved = ctx.saved_tensors
        stride, types, c0s, bcs, dils, adds, has_o, has_tb, wshapes, has_b1 = ctx.cfg
        n, C, T, V1 = h.shape
        nwin = len(types)
        KM = dw_w.shape[1]
        du = _K._f32c(du)
        lib = native.lib()
        it = iter(wsaved)
        w1s = [next(it) if t == 0 else None for t in types]
        tabs = (_K._int_array(types), _K._int_array(c0s), _K._int_array(bcs), _K._int_array(dils), _K._int_array(adds))
        pstride = lib.dsgcn_mlpwin_partial_stride(C, KM, nwin, tabs[0], tabs[2])
        dh = torch.empty_like(h)
        do = torch.empty_like(du)
        gbuf = torch.empty_like(du) if any(t == 0 and a != 1 for t, a in zip(types, adds)) else None
        part = torch.empty((n, pstride), device=h.device, dtype=torch.float32)
        ptr = _K._ptr
        rc = lib.dsgcn_mlpwin_bwd(ptr(h), ptr(o), ptr(du), ptr(dw_w), ptr(dw_b), ptr(dh), ptr(do), ptr(gbuf), ptr(part), n, C,
                                  T, V1, stride, KM, nwin, *tabs, _K._ptr_array(w1s), pstride, _K._stream())
        native.check(rc, 'dsgcn_mlpwin_bwd')
        red = _K.param_colsum(part, ctx.defer_ok)
        d_tw = red[:C * KM].view(C, KM)
        d_tb = red[C * KM:C * KM + C] if has_tb else None
        dws, dbs = [], []
        off = C * KM + C
        for t, bc, shp, hb in zip(types, bcs, wshapes, has_b1):
            if t != 0:
                dws.append(None)
                dbs.append(None)
                continue
            dws.append(red[off:off + bc * bc].view(shp))
            dbs.append(red[off + bc * bc:off + bc * bc + bc] if hb else None)
            off += bc * bc + bc
        return (dh, do if has_o else None, d_tw, d_tb, None, None, None, None, None, None, *dws, *dbs)


def dgmlp_windows(h, branch_cfg, widths, conv_w, conv_b, dw_w, dw_b, dw_dil, w1s, b1s, merge_after, stride):
    """The window stage of ``temporal_dgmlp`` (everything between branch_act and combine): h (n,C,T,V1) activated ->
    u (n,C,T',V1).  tapconv for the alpha-scaled dilated convs / max-pool / strided copy, then the mlp windows as one launch
    (csrc/mlpwin.hip) or — under DSGCN_MLPWIN=0, outside its range, and by default where a backward is recorded (kernels.MLPWIN)
    — dwcausal -> block-diagonal 1x1 -> add."""
    n, C, T, V1 = h.shape
    stride = int(stride)
    add_tcn = bool(conv_w)
    mlp = [not isinstance(c, str) and c[0] != 'max' for c in branch_cfg]
    none = [None] * sum(mlp)
    KT, types, c0s, bcs, dils, ws, bs = _K._branch_tables(branch_cfg, widths, conv_w if add_tcn else none,
                                                          conv_b if add_tcn else none)
    if add_tcn:
        o = _K._TapBranches.apply(h, stride, KT, C, types, c0s, c0s, bcs, bcs, dils, *ws, *bs)
    else:
        # the mlp windows have no addend: tapconv runs the other windows only, and nothing of o or dh is left unwritten
        keep = [i for i, t in enumerate(types) if t != 0]
        pick = lambda l: [l[i] for i in keep]       # noqa: E731
        o = None
        if keep:
            o = _K._TapBranchesZero.apply(h, stride, KT, C, pick(types), pick(c0s), pick(c0s), pick(bcs), pick(bcs),
                                          pick(dils), *pick(ws), *pick(bs))
    tabs = _mlpwin_tables(branch_cfg, widths, add_tcn, merge_after)
    use = _K.MLPWIN not in ('0', False) and mlpwin_supported(n, C, T, V1, stride, dw_w.shape[1], tabs)
    if use and _K.MLPWIN == 'auto':      # the kernel where no backward is recorded (kernels.MLPWIN)
        use = not (torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (h, dw_w, dw_b, *w1s, *b1s)))
    if use:
        w1it, b1it = iter(w1s), iter(b1s)
        w1_all = [next(w1it) if m else None for m in mlp]
        b1_all = [next(b1it) if m else None for m in mlp]
        u = _MlpWin.apply(h, o, dw_w, dw_b, stride, *tabs, *w1_all, *b1_all)
    else:
        dw = _K._DwCausal.apply(h, dw_w, dw_b, dw_dil, stride)
        before = add_tcn and not merge_after
        blocks, biases = [], []
        w1it, b1it = iter(w1s), iter(b1s)
        for m, bc in zip(mlp, widths):
            if m:
                blocks.append(next(w1it).reshape(bc, bc))
                biases.append(next(b1it))
            else:      # identity blocks pass the other windows through a mix that follows the add, zero blocks leave them to it
                blocks.append(torch.eye(bc, device=h.device, dtype=h.dtype) if before else h.new_zeros(bc, bc))
                biases.append(h.new_zeros(bc))
        pw_w, pw_b = torch.block_diag(*blocks), torch.cat(biases)
        if o is None:
            u = _K.pwconv(dw, None, None, None, False, pw_w, pw_b, 1, False)[0]
        elif before:
            u = _K.pwconv(_K.fuse_out(dw, None, o, None, 0, False)[0], None, None, None, False, pw_w, pw_b, 1, False)[0]
        else:
            u = _K.fuse_out(_K.pwconv(dw, None, None, None, False, pw_w, pw_b, 1, False)[0], None, o, None, 0, False)[0]
    return u


def temporal_dgmlp(z, zaug, scale, shift, n_act, branch_cfg, widths, conv_w, conv_b, dw_w, dw_b, dw_dil, w1s, b1s,
                   add_coeff, merge_after, stride, gamma=None, beta=None, eps=1e-5, want_bn=False):
    """dgmsmlp's temporal stage (tcn.py:432-523 with unitmlp 525-614) after the stacked branch conv with the global-joint
    column: h = BN+ReLU of (z | zaug) on channels < n_act (V+1 columns), then per mlp window
    conv1(dw(h)) + alpha * tconv(h)  (merge_after),  conv1(dw(h) + alpha * tconv(h))  or, without add_tcn,  conv1(dw(h)),
    beside the (3,1) max-pool and the strided pass-through windows; then  f = u[..., :V] + u[..., V] * add_coeff  and the
    train-mode BN of f (transform.0) as a deferred affine.
    conv_w / conv_b: the (k,1) dilated convs ALREADY scaled by their window's alpha, one per mlp window (empty or None:
    no add_tcn);  dw_w (C, KM), dw_b (C), dw_dil (C) int32: depthwise taps by channel (dil 0 outside the mlp windows);
    w1s / b1s: conv1 of every mlp window, in order.  -> (f, scale, shift, mean, var)
    The mlp windows run as one launch per direction (csrc/mlpwin.hip) or as the staged form dwcausal -> block-diagonal 1x1
    -> add: see ``dgmlp_windows`` and ``kernels.MLPWIN``."""
    _K._require_cuda(z)
    n, C, T, V = z.shape
    stride = int(stride)
    coeff = add_coeff if add_coeff.shape[0] == V else add_coeff[:V].contiguous()
    h = _K._BranchAct.apply(z, zaug, scale, shift, n_act)
    u = dgmlp_windows(h, branch_cfg, widths, conv_w, conv_b, dw_w, dw_b, dw_dil, w1s, b1s, merge_after, stride)
    bn = _K.BNCtx() if want_bn else None
    out = _K._TmsCombine.apply(u, coeff, gamma, beta, float(eps), bool(want_bn), bn)
    if want_bn:
        _K._bn_attach(out[1], bn, out[3], out[4], gamma, eps, float(u.shape[0] * u.shape[2] * (u.shape[3] - 1)),
                      u.shape[1])
    return out
