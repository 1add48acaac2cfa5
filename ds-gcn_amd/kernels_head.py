"""The head of the training step for the loss options beyond unit-weight hard-label cross entropy: the autograd function
and front of csrc/head_target.hip (``dsgcn_head_target_fwd/bwd``).  ``dsgcn_amd.kernels`` re-exports ``head_target``;
``kernels.head_loss`` (csrc/head.hip) stays the path of the default loss.  Checked against fp64 by
tests/test_head_target_gpu.py."""
import torch

from . import native
from . import kernels as _K
from .kernels import _f32c, _ptr


class _HeadTarget(torch.autograd.Function):
    """_HeadLoss for the other loss options (csrc/head_target.hip).  mode 0: target (N) int64, 1: (N, K) soft labels,
    2: (N, K) multi-hot labels; class_weight (K) or None.  -> (loss scalar, acc (2) fp64 [mode 0; else an empty tensor],
    score (N, K)); only the loss is differentiable.  Two launches forward, one backward."""

    @staticmethod
    def forward(ctx, feat, weight, bias, target, M, mode, class_weight, loss_weight):
        _K._require_cuda(feat, weight, target, class_weight)
        feat, weight, bias, class_weight = _f32c(feat), _f32c(weight), _f32c(bias), _f32c(class_weight)
        R, C = feat.shape
        K = weight.shape[0]
        if mode not in (0, 1, 2):
            raise ValueError(f'head_target: mode {mode} (0 hard labels, 1 soft labels, 2 binary cross entropy)')
        if R % M or weight.shape[1] != C or (class_weight is not None and class_weight.shape != (K,)):
            raise ValueError(f'head_target: feat {tuple(feat.shape)}, weight {tuple(weight.shape)}, class_weight '
                             f'{None if class_weight is None else tuple(class_weight.shape)}, {M} persons do not fit together')
        N = R // M
        if mode == 0:
            if target.is_floating_point() or target.numel() != N:
                raise ValueError(f'head_target: mode 0 takes {N} integer labels, got {tuple(target.shape)} {target.dtype}')
            target = target.to(torch.int64).contiguous()
        else:
            if target.shape != (N, K):
                raise ValueError(f'head_target: mode {mode} takes ({N}, {K}) float targets, got {tuple(target.shape)}')
            target = _f32c(target)
        dev = feat.device
        pooled = torch.empty((N, C), device=dev, dtype=torch.float32)
        score = torch.empty((N, K), device=dev, dtype=torch.float32)
        dscore = torch.empty((N, K), device=dev, dtype=torch.float32)
        clip = torch.empty((N, 4), device=dev, dtype=torch.float32)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        den = torch.empty(1, device=dev, dtype=torch.float32)
        acc = torch.empty(2 if mode == 0 else 0, device=dev, dtype=torch.float64)
        rc = native.lib().dsgcn_head_target_fwd(_ptr(feat), _ptr(weight), _ptr(bias), _ptr(class_weight), _ptr(target), mode,
                                                N, M, C, K, float(loss_weight), _ptr(pooled), _ptr(score), _ptr(dscore),
                                                _ptr(clip), _ptr(loss), _ptr(den), _ptr(acc) if mode == 0 else None,
                                                _K._stream())
        native.check(rc, 'dsgcn_head_target_fwd')
        ctx.save_for_backward(dscore, pooled, weight, den)
        ctx.dims = (N, M, C, K, float(loss_weight), bias is not None)
        ctx.mark_non_differentiable(acc, score)
        ctx.set_materialize_grads(False)
        return loss, acc, score

    @staticmethod
    def backward(ctx, gloss, _gacc, _gscore):
        if gloss is None:
            return (None,) * 8
        dscore, pooled, weight, den = ctx.saved_tensors
        N, M, C, K, lw, has_bias = ctx.dims
        dev = dscore.device
        gloss = _f32c(gloss)
        dfeat = torch.empty((N * M, C), device=dev, dtype=torch.float32)
        dw = torch.empty((K, C), device=dev, dtype=torch.float32)
        db = torch.empty(K, device=dev, dtype=torch.float32)
        rc = native.lib().dsgcn_head_target_bwd(_ptr(dscore), _ptr(pooled), _ptr(weight), _ptr(gloss), _ptr(den), N, M, C, K,
                                                lw, _ptr(dfeat), _ptr(dw), _ptr(db), _K._stream())
        native.check(rc, 'dsgcn_head_target_bwd')
        return dfeat, dw, (db if has_bias else None), None, None, None, None, None


def head_target(feat, weight, bias, target, persons, mode, class_weight=None, loss_weight=1.0):
    """Person mean + Linear + one of the weighted / soft-label / multi-label losses (times loss_weight).  mode 0: hard
    labels, F.cross_entropy(weight=class_weight), + top-1 / top-5 accuracy;  mode 1: (N, K) soft labels, cross entropy
    with the reference's weighted mean;  mode 2: (N, K) multi-hot labels, binary cross entropy with logits.
    -> (loss 0-dim fp32, acc (2,) fp64 or None [modes 1, 2], score (N, K))."""
    loss, acc, score = _HeadTarget.apply(feat, weight, bias, target, int(persons), int(mode), class_weight,
                                         float(loss_weight))
    return loss, (acc if int(mode) == 0 else None), score
