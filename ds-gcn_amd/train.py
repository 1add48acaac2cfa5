"""Optimizer / schedule used by the reference's shipped configs (configs/_init_/lr_schedual.py:11-27):
SGD(lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True) on ALL parameters (mmcv's default
constructor applies weight decay to BN/alpha/beta/A as well, quirk Q10), cosine annealing per iteration."""
import math

import torch

from . import kernels, native


class FlatSGD:
    """Nesterov SGD over ``FlatParams`` buffers: a handful of elementwise launches per step regardless of
    the 604 parameter tensors.  Matches torch.optim.SGD(nesterov=True, dampening=0) update-for-update.

    ``capturable=True`` keeps the learning rate in a one-element device tensor (``set_lr`` fills it): a ``step()`` captured
    in a hipGraph then follows the per-iteration schedule on replay instead of freezing the rate of the capture.  The
    momentum buffer is allocated once and only ever written in place (``load_state_dict`` included), so a captured
    ``step()`` keeps updating the live buffer after a resume.

    ``grad_clip``: mmcv's ``optimizer_config.grad_clip`` dict (``max_norm``, ``norm_type`` 2 or inf) — ``step()`` then clips
    the flat gradient by its total norm first, the way ``torch.nn.utils.clip_grad_norm_`` does before ``optimizer.step()``
    (the flat buffer has no padding: its elements are exactly the parameters' elements).  ``flat_g`` holds the clipped
    gradient afterwards and ``grad_norm`` (one device float, allocated here) the total norm BEFORE clipping.  On the device
    that is two launches (csrc/clip.hip) in place of ``dsgcn_sgd_step``; clipping adds no optimizer state.

    ``accumulate=k > 1``: mmcv's ``GradientCumulativeOptimizerHook(cumulative_iters=k)`` — k backward passes per update.
    ``accum_add()`` adds the flat gradient to ``acc`` (a buffer of its own, allocated here); ``accum_finish()`` leaves
    ``(acc + g) * (1 / k)`` in the flat gradient and ``acc`` at zero, and ``step()`` follows as ever.  One launch each
    (csrc/accum.hip); off the fused path the same two operations with torch ops.  ``acc`` is no optimizer state: it is
    empty between groups and not part of ``state_dict()``."""

    def __init__(self, flat, lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True, capturable=False, grad_clip=None,
                 accumulate=1):
        self.flat = flat
        self.lr = lr
        self.base_lr = lr
        self.momentum = momentum
        self.weight_decay = weight_decay
        self.nesterov = nesterov
        self.buf = None
        self.capturable = capturable
        self.lr_t = torch.full((1,), float(lr), device=flat.flat_p.device, dtype=flat.flat_p.dtype) if capturable else None
        if capturable and momentum:
            self.buf = torch.zeros_like(flat.flat_p)       # torch's first step sets buf = g; momentum * 0 + g is the same value
        self.clip = parse_grad_clip(grad_clip)             # None | (max_norm, 2 or 0 = inf)
        self.grad_norm = self.clip_partial = None
        if self.clip is not None:
            # both workspaces here, never inside step(): an allocation inside a captured step is replayed as garbage
            dev = flat.flat_p.device
            self.grad_norm = torch.zeros(1, device=dev, dtype=torch.float32)
            if capturable and dev.type == 'cuda' and flat.flat_p.dtype == torch.float32:
                rows = native.lib().dsgcn_grad_norm_rows(flat.flat_p.numel())
                native.check(min(rows, 0), 'dsgcn_grad_norm_rows')
                self.clip_partial = torch.zeros(rows, device=dev, dtype=torch.float64)
        if isinstance(accumulate, bool) or not isinstance(accumulate, int) or accumulate < 1:
            raise ValueError(f'accumulate must be an integer >= 1, got {accumulate!r}')
        self.accumulate = accumulate
        self.acc = self.acc_factor = self.acc_tail_factor = None
        if accumulate > 1:
            # here for the same reason as the clip's workspaces; the factors are device floats so that a captured
            # accum_finish() and an eager one for a short last group read theirs the same way
            self.acc = torch.zeros_like(flat.flat_g)
            self.acc_factor = torch.full((1,), 1.0 / accumulate, device=flat.flat_g.device, dtype=flat.flat_g.dtype)
            self.acc_tail_factor = torch.ones_like(self.acc_factor)

    def set_lr(self, lr):
        self.lr = float(lr)
        if self.lr_t is not None:
            self.lr_t.fill_(self.lr)

    def _fused(self):
        p = self.flat.flat_p
        return self.capturable and p.is_cuda and p.dtype == torch.float32 and kernels.FUSED_ENDS

    @torch.no_grad()
    def step(self):
        p, g = self.flat.flat_p, self.flat.flat_g
        if self.clip is not None and self._fused():
            # norm partials, then clip + update in one launch (csrc/clip.hip): one extra read of the flat gradient
            max_norm, norm_type = self.clip
            st = torch.cuda.current_stream().cuda_stream
            rc = native.lib().dsgcn_grad_norm_partials(g.data_ptr(), g.numel(), norm_type, self.clip_partial.data_ptr(), st)
            native.check(rc, 'dsgcn_grad_norm_partials')
            rc = native.lib().dsgcn_sgd_step_clip(p.data_ptr(), g.data_ptr(), self.buf.data_ptr() if self.momentum else None,
                                                  self.lr_t.data_ptr(), self.clip_partial.data_ptr(),
                                                  self.clip_partial.numel(), norm_type, max_norm, self.grad_norm.data_ptr(),
                                                  float(self.momentum), float(self.weight_decay),
                                                  int(bool(self.nesterov)), p.numel(), st)
            native.check(rc, 'dsgcn_sgd_step_clip')
            return
        if self.clip is not None:
            # the same arithmetic with torch ops: fp64 sum of squares (max |g|), fp32 total, fp32 coefficient
            max_norm, norm_type = self.clip
            total = (g.abs().max() if norm_type == 0 else g.double().square().sum().sqrt()).to(torch.float32)
            coef = max_norm / (total + 1e-6)
            coef = torch.where(coef < 1.0, coef, torch.ones_like(coef))
            g.mul_(coef.to(g.dtype))
            self.grad_norm.copy_(total.reshape(1))
        if self._fused():
            # one launch (csrc/head.hip k_sgd) instead of five elementwise passes over the flat buffers
            rc = native.lib().dsgcn_sgd_step(p.data_ptr(), g.data_ptr(), self.buf.data_ptr() if self.momentum else None,
                                             self.lr_t.data_ptr(), float(self.momentum), float(self.weight_decay),
                                             int(bool(self.nesterov)), p.numel(),
                                             torch.cuda.current_stream().cuda_stream)
            native.check(rc, 'dsgcn_sgd_step')
            return
        if self.weight_decay:
            g = g.add(p, alpha=self.weight_decay)
        if self.momentum:
            if self.buf is None:
                self.buf = g.clone()
            else:
                self.buf.mul_(self.momentum).add_(g)
            g = g.add(self.buf, alpha=self.momentum) if self.nesterov else self.buf
        if self.capturable:
            p.addcmul_(g, self.lr_t, value=-1.0)
        else:
            p.add_(g, alpha=-self.lr)

    def _accum_ready(self):
        if self.acc is None:
            raise RuntimeError('FlatSGD was built with accumulate=1: there is no accumulation buffer')
        return self.flat.flat_g

    @torch.no_grad()
    def accum_add(self):
        """acc += flat gradient (a micro-iteration: no update follows)."""
        g = self._accum_ready()
        if self._fused():
            rc = native.lib().dsgcn_grad_accum(self.acc.data_ptr(), g.data_ptr(), g.numel(),
                                               torch.cuda.current_stream().cuda_stream)
            native.check(rc, 'dsgcn_grad_accum')
            return
        self.acc.add_(g)

    @torch.no_grad()
    def accum_finish(self, count=None):
        """flat gradient = (acc + flat gradient) * (1 / count), acc = 0.  count None: the group is full (1 / accumulate, the
        only form a captured step uses); an int: a short last group of that many gradients (mmcv divides the tail of a run
        by its own length)."""
        g = self._accum_ready()
        factor = self.acc_factor
        if count is not None:
            if not 1 <= int(count) <= self.accumulate:
                raise ValueError(f'accum_finish: a group holds 1..{self.accumulate} gradients, got {count}')
            factor = self.acc_tail_factor
            factor.fill_(1.0 / int(count))
        if self._fused():
            rc = native.lib().dsgcn_grad_accum_finish(self.acc.data_ptr(), g.data_ptr(), factor.data_ptr(), g.numel(),
                                                      torch.cuda.current_stream().cuda_stream)
            native.check(rc, 'dsgcn_grad_accum_finish')
            return
        g.add_(self.acc).mul_(factor)
        self.acc.zero_()

    def zero_grad(self):
        self.flat.zero_grad()

    def state_dict(self):
        """torch.optim.SGD's layout — ``{'state': {i: {'momentum_buffer': tensor}}, 'param_groups': [{...}]}`` with one
        entry per parameter tensor in ``module.parameters()`` order — so the ``optimizer`` entry of a checkpoint is
        interchangeable with the reference's (mmcv saves ``optimizer.state_dict()`` of a torch SGD).  CPU tensors."""
        state = {}
        if self.buf is not None and (not self.capturable or bool(self.buf.any())):     # all-zero = no step taken yet
            for i, (p, (off, n)) in enumerate(zip(self.flat.params, self.flat.slices)):
                state[i] = {'momentum_buffer': self.buf[off:off + n].view(p.shape).detach().cpu().clone()}
        group = dict(lr=self.lr, momentum=self.momentum, dampening=0, weight_decay=self.weight_decay,
                     nesterov=self.nesterov, maximize=False, foreach=None, differentiable=False, fused=None,
                     initial_lr=self.base_lr, params=list(range(len(self.flat.params))))
        return {'state': state, 'param_groups': [group]}

    def load_state_dict(self, sd):
        """Accepts the torch SGD layout (this class's own checkpoints and the reference's)."""
        groups = sd['param_groups']
        if len(groups) != 1 or len(groups[0]['params']) != len(self.flat.params):
            raise ValueError('FlatSGD.load_state_dict: expected one param group over '
                             f'{len(self.flat.params)} tensors, got {[len(g["params"]) for g in groups]}')
        g = groups[0]
        self.set_lr(g['lr'])
        self.base_lr = g.get('initial_lr', self.base_lr)
        self.momentum = g.get('momentum', self.momentum)
        self.weight_decay = g.get('weight_decay', self.weight_decay)
        self.nesterov = g.get('nesterov', self.nesterov)
        state = sd.get('state', {})
        if not state:
            if self.capturable and self.buf is not None:
                self.buf.zero_()
            else:
                self.buf = None
            return
        # in place when the buffer exists: a hipGraph captured around step() holds its address
        buf = self.buf if self.buf is not None else torch.zeros_like(self.flat.flat_p)
        buf.zero_()
        for i, pid in enumerate(g['params']):
            mb = state.get(pid, state.get(str(pid), {})).get('momentum_buffer')
            if mb is not None:
                off, n = self.flat.slices[i]
                buf[off:off + n].copy_(mb.reshape(-1))
        self.buf = buf


def parse_grad_clip(grad_clip):
    """mmcv's ``optimizer_config.grad_clip`` (the keyword arguments of ``torch.nn.utils.clip_grad_norm_``) ->
    ``None`` or ``(max_norm, norm_type)`` with ``norm_type`` 2 or 0 (= inf, the C ABI's code)."""
    if grad_clip is None:
        return None
    cfg = dict(grad_clip)
    if 'max_norm' not in cfg:
        raise ValueError(f'grad_clip needs max_norm (got {sorted(cfg)})')
    max_norm = float(cfg.pop('max_norm'))
    if not max_norm >= 0.0:
        raise ValueError(f'grad_clip max_norm must be >= 0, got {max_norm}')
    norm_type = cfg.pop('norm_type', 2)
    if cfg:
        raise NotImplementedError(f'grad_clip options {sorted(cfg)} are not supported (max_norm, norm_type)')
    if isinstance(norm_type, str):
        if norm_type != 'inf':
            raise NotImplementedError(f'grad_clip norm_type {norm_type!r}: 2 and inf are implemented')
        norm_type = math.inf
    norm_type = float(norm_type)
    if norm_type == 2.0:
        return max_norm, 2
    if norm_type == math.inf:
        return max_norm, 0
    raise NotImplementedError(f'grad_clip norm_type {norm_type!r}: 2 and inf are implemented')


def warmup_lr(regular_lr, cur_iter, warmup, warmup_iters, warmup_ratio=0.1):
    """mmcv LrUpdaterHook.get_warmup_lr for ``cur_iter < warmup_iters`` (from ``warmup_iters`` on the caller keeps the
    regular rate): constant ``r * ratio``; linear ``r * (1 - (1 - cur/iters) * (1 - ratio))``; exp
    ``r * ratio ** (1 - cur/iters)``."""
    if warmup == 'constant':
        return regular_lr * warmup_ratio
    if warmup == 'linear':
        return regular_lr * (1 - (1 - cur_iter / warmup_iters) * (1 - warmup_ratio))
    if warmup == 'exp':
        return regular_lr * warmup_ratio ** (1 - cur_iter / warmup_iters)
    raise ValueError(f'"{warmup}" is not a supported type for warming up, valid types are "constant", "linear" and "exp"')


def cosine_lr(base_lr, it, total_iters, min_lr=0.0):
    """mmcv CosineAnnealingLrUpdaterHook(by_epoch=False)."""
    return min_lr + 0.5 * (base_lr - min_lr) * (1 + math.cos(math.pi * it / max(total_iters, 1)))


def step_lr(base_lr, progress, step, gamma=0.1, min_lr=None):
    """mmcv StepLrUpdaterHook.get_lr: ``progress`` = the 0-based epoch about to run (by_epoch=True); ``step`` an int
    (decay every ``step`` epochs) or a list of milestones (configs/stgcn/stgcn_vanilla_ntu60_xsub_3dkp/j.py:35)."""
    if isinstance(step, int):
        exp = progress // step
    else:
        exp = len(step)
        for i, s in enumerate(step):
            if progress < s:
                exp = i
                break
    lr = base_lr * gamma ** exp
    if min_lr is not None:
        lr = max(lr, min_lr)
    return lr
