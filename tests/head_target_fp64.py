"""``kernels.head_target`` in plain torch ops (any dtype, any device): the fp64 truth of tests/test_head_target_gpu.py and
the CPU seam (``kernels.use_ops``) of tests/test_head_target_host.py — tests/torch_ops.py plus that one function.  Written
from the loss definitions (F.cross_entropy(weight=), the reference's soft-label reduction, F.binary_cross_entropy_with_
logits(weight=)); tests/test_head_target_host.py pins it to the reference's fp64 outputs (tests/golden/headloss.npz)."""
import types

import numpy as np
import torch
import torch.nn.functional as F

# head.hip's bar (tests/test_kernels_gpu.py::check_head_loss): error against fp64 relative to the norm
HEAD_LOSS_BAR = 2e-6


def head_target(feat, weight, bias, target, persons, mode, class_weight=None, loss_weight=1.0):
    N = feat.shape[0] // persons
    score = F.linear(feat.reshape(N, persons, -1).mean(1), weight, bias)
    cw = None if class_weight is None else class_weight.to(score.dtype)
    acc = None
    if mode == 0:
        loss = F.cross_entropy(score, target, weight=cw)
        with torch.no_grad():
            sl = score.gather(1, target.view(-1, 1))
            idx = torch.arange(score.shape[1], device=score.device)[None]
            rank = ((score > sl) | ((score == sl) & (idx > target.view(-1, 1)))).sum(1)
            acc = torch.stack([(rank < 1).double().mean(), (rank < 5).double().mean()])
    elif mode == 1:
        q = target.to(score.dtype)
        lsm = F.log_softmax(score, 1)
        if cw is None:
            loss = -(q * lsm).sum(1).mean()
        else:
            loss = -(q * lsm * cw[None]).sum() / (q * cw[None]).sum()
    elif mode == 2:
        loss = F.binary_cross_entropy_with_logits(score, target.to(score.dtype), weight=cw)
    else:
        raise ValueError(mode)
    return loss * loss_weight, acc, score.detach()


def cpu_ops(calls=None):
    """tests/torch_ops.py plus ``head_target``; with `calls` (a list) the names of the head ops called are appended."""
    import torch_ops
    ns = types.SimpleNamespace(**{k: v for k, v in vars(torch_ops).items() if not k.startswith('__')})

    def rec(name, fn):
        def wrapped(*a, **kw):
            if calls is not None:
                calls.append(name)
            return fn(*a, **kw)
        return wrapped
    ns.head_loss = rec('head_loss', torch_ops.head_loss)
    ns.head_target = rec('head_target', head_target)
    return ns


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ---- the fixture (tests/golden/headloss.npz, written by tests/golden/gen_golden_headloss.py) ---------------------------

def fixture():
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'headloss.npz')
    with np.load(path) as f:
        return {k: f[k] for k in f.files}


def fixture_case(z, name):
    """-> (head config dict, tensors by name) of one case."""
    import json
    tag = name + '_'
    cfg = json.loads(str(z[tag + 'cfg']))
    t = {k[len(tag):]: (v if v.dtype.kind == 'U' else torch.from_numpy(np.array(v))) for k, v in z.items()
         if k.startswith(tag) and k != tag + 'cfg'}
    return cfg, t
