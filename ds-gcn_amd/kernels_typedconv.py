"""Position-typed 1x1 conv (csrc/typedconv.hip, ``dsgcn_typedconv_*``): ``y[n, o, pos] = W[type(pos)] x[n, :, pos] + b[type(pos)]``
with ``type(pos) = table[pos % L]`` — the primitive under CTRHGC's ``target_specific`` (node-typed: L = V) and
``full_channels`` (edge-typed: L = V*V) arms.  ``dsgcn_amd.kernels`` re-exports ``typed_conv`` and ``typed_plan``.
fp32 MFMA at both matmul precision levels; the weight gradient adds its per-split partials in order (``kernels.colsum``):
no float atomics, the same bits every run.  Checked against fp64 by tests/test_ctrhgcn_flags_gpu.py."""
import numpy as np
import torch

from . import native
from . import kernels as _K
from .kernels import _ptr

MAX_TYPES = 16          # include/dsgcn.h: DSGCN_TYPED_MAX_TYPES
MAX_PERIOD = 1024       # include/dsgcn.h: DSGCN_TYPED_MAX_PERIOD
TILE = 32
N_OFF = 17


class TypedPlan:
    """The sorted-by-type tile plan of one table (include/dsgcn.h, dsgcn_typedconv_fwd): ``tensor`` int32 (a module keeps
    it as a non-persistent buffer and hands the moved tensor back through ``on``), the period ``L``, ``chunk`` (the whole
    number of periods the permutation covers) and ``ntiles``."""
    __slots__ = ('tensor', 'L', 'chunk', 'ntiles', 'P')

    def __init__(self, tensor, L, chunk, ntiles, P):
        self.tensor, self.L, self.chunk, self.ntiles, self.P = tensor, L, chunk, ntiles, P

    def on(self, tensor):
        return TypedPlan(tensor, self.L, self.chunk, self.ntiles, self.P)


def typed_plan(table, P):
    """table: L integers in [0, P) (the type of each position of one period) -> TypedPlan on the CPU.  The chunk is as many
    whole periods as fit 1024 positions (tiles of a type fill up across periods: 25 joints of 5 types would leave most
    of every 32-column tile empty); inside a type the positions ascend, so a tile whose first position lies outside a
    short plane is skipped whole."""
    t = np.asarray(torch.as_tensor(table).detach().cpu()).reshape(-1).astype(np.int64)
    L, P = int(t.size), int(P)
    if P > MAX_TYPES:
        raise NotImplementedError(f'typed_conv: P = {P} position types (at most {MAX_TYPES})')
    if L > MAX_PERIOD:
        raise NotImplementedError(f'typed_conv: L = {L} positions per period (at most {MAX_PERIOD})')
    if L < 1 or P < 1 or t.min() < 0 or t.max() >= P:
        raise ValueError(f'typed_conv: the table must hold L >= 1 types in [0, {P})')
    G = max(1, MAX_PERIOD // L)
    types = np.tile(t, G)
    tile_off, tile_type, perm = [0], [], []
    for p in range(P):
        idx = np.nonzero(types == p)[0]
        nt = -(-idx.size // TILE)
        perm.extend(idx.tolist())
        perm.extend([-1] * (nt * TILE - idx.size))
        tile_type.extend([p] * nt)
        tile_off.append(tile_off[-1] + nt)
    tile_off.extend([tile_off[-1]] * (N_OFF - len(tile_off)))
    return TypedPlan(torch.tensor(tile_off + tile_type + perm, dtype=torch.int32), L, G * L, len(tile_type), P)


class _TypedConv(torch.autograd.Function):
    """x (n, Ci, T, V), W (P, Co, Ci), b (P, Co) -> y (n, Co, T, V): one launch each for the forward, the data gradient
    and the weight gradient (+ the ordered sum of its partial rows)."""

    @staticmethod
    def forward(ctx, x, W, b, plan):
        _K._require_cuda(x, W, b, plan.tensor)
        x, W, b = _K._f32c(x), _K._f32c(W), _K._f32c(b)      # (looked up at call time: tests/layout_cases.py)
        n, Ci, T, V = x.shape
        P, Co, _ = W.shape
        if W.shape[2] != Ci or tuple(b.shape) != (P, Co) or P != plan.P:
            raise ValueError(f'typed_conv: x {tuple(x.shape)}, W {tuple(W.shape)}, b {tuple(b.shape)}, P = {plan.P}, '
                             f'L = {plan.L}')
        if plan.tensor.dtype != torch.int32 or plan.tensor.numel() != N_OFF + (TILE + 1) * plan.ntiles:
            raise ValueError('typed_conv: not a typed_plan tensor')
        y = torch.empty((n, Co, T, V), device=x.device, dtype=torch.float32)
        rc = native.lib().dsgcn_typedconv_fwd(_ptr(x), _ptr(W), _ptr(b), _ptr(plan.tensor), plan.ntiles, _ptr(y), n, Ci, Co,
                                              T * V, plan.L, plan.chunk, P, _K._stream())
        native.check(rc, 'dsgcn_typedconv_fwd')
        ctx.save_for_backward(x, W, plan.tensor)
        ctx.plan = plan
        return y

    @staticmethod
    def backward(ctx, dy):
        x, W, pt = ctx.saved_tensors
        plan = ctx.plan
        n, Ci, T, V = x.shape
        P, Co, _ = W.shape
        dy = _K._f32c(dy)
        lib = native.lib()
        dx = dW = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            rc = lib.dsgcn_typedconv_dgrad(_ptr(dy), _ptr(W), _ptr(pt), plan.ntiles, _ptr(dx), n, Ci, Co, T * V, plan.L,
                                           plan.chunk, P, _K._stream())
            native.check(rc, 'dsgcn_typedconv_dgrad')
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            rows = lib.dsgcn_typedconv_wgrad_rows(n, Ci, Co, P)
            if rows <= 0:
                native.check(rows or -1, 'dsgcn_typedconv_wgrad_rows')
            part = torch.empty((rows, P * Co * Ci + P * Co), device=x.device, dtype=torch.float32)
            rc = lib.dsgcn_typedconv_wgrad(_ptr(x), _ptr(dy), _ptr(pt), plan.ntiles, _ptr(part), n, Ci, Co, T * V, plan.L,
                                           plan.chunk, P, _K._stream())
            native.check(rc, 'dsgcn_typedconv_wgrad')
            red = part[0] if rows == 1 else _K.colsum(part)           # the splits added in order, fp64 accumulation
            dW, db = red[:P * Co * Ci].view(P, Co, Ci), red[P * Co * Ci:].view(P, Co)
        return dx, dW, db, None


def typed_conv(x, W, b, table, P, plan=None):
    """y[n, o, t, v] = sum_c W[type][o][c] x[n, c, t, v] + b[type][o] with type = table[(t*V + v) % L].
    x (n, Ci, T, V); W (P, Co, Ci); b (P, Co); table: int32 device tensor of L entries in [0, P).
    plan: the ``TypedPlan`` of the table, built once by its owner (``typed_plan``); without it the plan is built here from
    the table (a device-to-host copy: test and tool use)."""
    if plan is None:
        plan = typed_plan(table, P)
        plan = plan.on(plan.tensor.to(x.device))
    return _TypedConv.apply(x, W, b, plan)
