"""Shared pieces of the gradient-accumulation tests: the reduced DS-STGCN of tests/golden/model_reduced_cfg.json, a fixed
list of 2-clip micro-batches, the hand-written statement of an accumulated run (k forward/backward passes, each under its
own BatchNorm statistics, gradients summed in call order and scaled by fp32(1 / count), one torch.optim.SGD step) and the
numpy statement of the two kernels."""
import functools
import json
import os

import numpy as np
import torch

import dsgcn_amd as D
import torch_ops
from test_oracle_golden import GOLD, load, sd_of

SGD = dict(lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True)


@functools.lru_cache(maxsize=None)
def _golden():
    z = load('model_reduced.npz')
    with open(os.path.join(GOLD, 'model_reduced_cfg.json')) as f:
        cfg = json.load(f)
    cfg['backbone']['tcn_ms_cfg'] = [tuple(c) if isinstance(c, list) else c for c in cfg['backbone']['tcn_ms_cfg']]
    return z, cfg


def reduced_model():
    """A fresh copy of the golden reduced DS-STGCN (CPU, training mode)."""
    z, cfg = _golden()
    m = D.build_model(cfg)
    m.load_state_dict(sd_of(z, 'sd_', torch.float32))
    return m.train()


@functools.lru_cache(maxsize=None)
def micro_batches(count, clips=2):
    """``count`` different (keypoint, label) micro-batches of ``clips`` clips in the golden input's layout; never modified."""
    z, cfg = _golden()
    shape = (clips,) + tuple(z['x'].shape[1:])
    classes = cfg['cls_head']['num_classes']
    gen = torch.Generator().manual_seed(20)
    return tuple((torch.randn(shape, generator=gen), torch.randint(0, classes, (clips, 1), generator=gen))
                 for _ in range(count))


def grouped(n_iters, k):
    """mmcv's grouping of ``n_iters`` iterations: full groups of k, then the ``n_iters % k`` left over as one short group."""
    idx = list(range(n_iters))
    return [idx[i:i + k] for i in range(0, n_iters, k)]


def host_statement(batches, groups, lrs=None, sgd=SGD, grad_clip=None):
    """The hand-written loop on the CPU with the torch statements of the ops (tests/torch_ops.py).
    -> dict(model, p (named parameters), buf (momentum per name), mean (the last group's averaged gradient per name),
            micro (the last group's micro-gradients))."""
    m = reduced_model()
    opt = torch.optim.SGD(m.parameters(), **sgd)
    names = [k for k, _ in m.named_parameters()]
    mean = micro = None
    with D.kernels.use_ops(torch_ops):
        for group in groups:
            total, micro = None, []
            for i in group:
                kp, lb = batches[i]
                for p in m.parameters():
                    p.grad = None
                m.train_step(dict(keypoint=kp, label=lb), None, sync_log_vars=False)['loss'].backward()
                g = [torch.zeros_like(p) if p.grad is None else p.grad.detach().clone() for p in m.parameters()]
                micro.append(g)
                total = [torch.zeros_like(x) + x for x in g] if total is None else [t + x for t, x in zip(total, g)]
            factor = torch.tensor(1.0 / len(group), dtype=torch.float32)
            mean = [t * factor for t in total]
            for p, g in zip(m.parameters(), mean):
                p.grad = g.clone()
            if grad_clip is not None:
                torch.nn.utils.clip_grad_norm_(m.parameters(), **grad_clip)
            if lrs is not None:
                opt.param_groups[0]['lr'] = lrs[group[-1]]            # the rate of the stepping call
            opt.step()
    return dict(model=m, p={k: p.detach().clone() for k, p in m.named_parameters()},
                buf={k: opt.state[p]['momentum_buffer'].clone() for k, p in m.named_parameters()},
                mean=dict(zip(names, mean)), micro=[dict(zip(names, g)) for g in micro])


def flat_of(engine, per_name):
    """A dict of per-parameter tensors laid out as the engine's flat buffers."""
    out = torch.empty(engine.flat.numel, dtype=torch.float64)
    for (k, _), (off, n) in zip(engine.model.named_parameters(), engine.flat.slices):
        out[off:off + n] = per_name[k].detach().double().cpu().reshape(-1)
    return out


def running_stats(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if 'running' in k or 'num_batches' in k}


# ---- the kernels -------------------------------------------------------------------------------------------------------

def accum_ref(acc, g):
    """acc + g: an fp32 add is the exact sum rounded once, and the fp64 sum of two fp32 values IS the exact sum while their
    exponents lie less than 29 apart (the test data: normal deviates and sums of a few of them)."""
    return (acc.astype(np.float64) + g.astype(np.float64)).astype(np.float32)


def finish_ref(acc, g, factor):
    """(acc + g) * fp32(factor), each operation rounded to fp32 (the product of two fp32 values is exact in fp64)."""
    s = accum_ref(acc, g)
    return (s.astype(np.float64) * np.float64(np.float32(factor))).astype(np.float32)
