"""Optimizer / schedule used by the reference's shipped configs (configs/_init_/lr_schedual.py:11-27):
SGD(lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True) on ALL parameters (mmcv's default
constructor applies weight decay to BN/alpha/beta/A as well, quirk Q10), cosine annealing per iteration."""
import math

import numpy as np
import torch

from . import kernels, native


SKIP = -1          # include/dsgcn.h DSGCN_OPTIM_SKIP: the group id of a tensor the update leaves alone
MAX_GROUPS = 256   # what csrc/optim.hip implements


class GroupTable:
    """Where the parameter tensors of a ``FlatParams`` lie in the flat buffers and which (rate, weight decay) group each
    belongs to — what the grouped update kernels (csrc/optim.hip) look up per element.

    ``lrs`` / ``wds``: one value per tensor of ``flat.params``.  Tensors with an equal (initial rate, weight decay) share
    one group, numbered in order of first appearance (group 0 is the first parameter's, whose rate mmcv logs).  The table
    goes to the device once, here; ``lr_t`` (fp64, one rate per group) is what ``set_lr`` rewrites every iteration and
    ``wd_t`` is constant.  ``fix_live(pattern)`` moves the tensors that receive no gradient to the SKIP group: in place,
    outside any capture, once."""

    def __init__(self, flat, lrs, wds):
        self.flat = flat
        pairs, self.tensor_group = [], []
        for lr, wd in zip(lrs, wds):
            pair = (float(lr), float(wd))
            if pair not in pairs:
                pairs.append(pair)
            self.tensor_group.append(pairs.index(pair))
        if len(pairs) > MAX_GROUPS:
            raise NotImplementedError(f'{len(pairs)} distinct (lr, weight_decay) pairs: the update kernels take {MAX_GROUPS}')
        self.base_lrs = [lr for lr, _ in pairs]
        self.lrs = list(self.base_lrs)
        self.wds = [wd for _, wd in pairs]
        if any(not wd >= 0.0 for wd in self.wds):
            raise ValueError(f'Invalid weight_decay value: {min(self.wds)}')
        self.live = None                                   # per tensor of flat.params, once known
        # rows of the table: the non-empty tensors in the order they lie in the buffer (flat_groups() may reorder them)
        self.rows = sorted((i for i, (_, n) in enumerate(flat.slices) if n > 0), key=lambda i: flat.slices[i][0])
        dev = flat.flat_p.device
        n = flat.flat_p.numel()
        self.ends = np.array([flat.slices[i][0] + flat.slices[i][1] for i in self.rows], dtype=np.int32)
        self.chunks = native.lib().dsgcn_optim_chunks(n)
        native.check(min(self.chunks, 0), 'dsgcn_optim_chunks')
        host = self._host_table()
        self.tab = torch.from_numpy(host).to(dev)          # int32: ends | group | first
        self.lr_t = torch.tensor(self.lrs, dtype=torch.float64, device=dev)
        self.wd_t = torch.tensor(self.wds, dtype=torch.float64, device=dev)

    def _host_table(self):
        """ends | group | first as one int32 array; dsgcn_optim_table checks it and fills ``first`` on the host."""
        k = len(self.rows)
        live = self.live or [True] * len(self.tensor_group)
        host = np.zeros(2 * k + self.chunks + 1, dtype=np.int32)
        host[:k] = self.ends
        host[k:2 * k] = [self.tensor_group[i] if live[i] else SKIP for i in self.rows]
        wd = np.array(self.wds, dtype=np.float64)
        rc = native.lib().dsgcn_optim_table(host[:k].ctypes.data, host[k:2 * k].ctypes.data, k, wd.ctypes.data, len(self.wds),
                                            self.flat.flat_p.numel(), host[2 * k:].ctypes.data)
        native.check(rc, 'dsgcn_optim_table')
        return host

    def fix_live(self, pattern):
        self.live = [bool(v) for v in pattern]
        self.tab.copy_(torch.from_numpy(self._host_table()))

    def set_lrs(self, lrs):
        """One fill per group (a single one when all rates are equal): the value travels in the launch's arguments, so the
        host neither waits for the device nor keeps a staging buffer alive until the copy has run."""
        lrs = [float(v) for v in lrs]
        if len(lrs) != len(self.base_lrs):
            raise ValueError(f'set_lr: {len(self.base_lrs)} group(s), got {len(lrs)} rate(s)')
        self.lrs = lrs
        if len(set(lrs)) == 1:
            self.lr_t.fill_(lrs[0])
        else:
            for g, v in enumerate(lrs):
                self.lr_t[g].fill_(v)

    def pointers(self):
        """(ends, group, first, ntens, lr, wd, groups): the table arguments of the update entry points."""
        k, base = len(self.rows), self.tab.data_ptr()
        return base, base + 4 * k, base + 8 * k, k, self.lr_t.data_ptr(), self.wd_t.data_ptr(), len(self.wds)

    def tensors(self):
        """(offset, length, rate, weight decay) of every tensor the update touches, for the torch-op path."""
        for i, (off, cnt) in enumerate(self.flat.slices):
            if cnt and (self.live is None or self.live[i]):
                g = self.tensor_group[i]
                yield off, cnt, self.lrs[g], self.wds[g]


class _FlatOptimizer:
    """What FlatSGD and FlatAdam share: the clip's and the accumulator's workspaces (allocated at construction, never
    inside a step that may be captured), ``accum_add`` / ``accum_finish`` / ``zero_grad``, and the bookkeeping of parameters
    that never receive a gradient."""

    def _setup(self, flat, capturable, grad_clip, accumulate):
        self.flat = flat
        self.capturable = capturable
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

    def _fused(self):
        """Whether the update runs as HIP launches: fp32 buffers on the GPU, unless DSGCN_FUSED_ENDS=0 switches the fused
        kernels off — then, as on the CPU, every path of these classes runs the same update with torch ops."""
        p = self.flat.flat_p
        return self.capturable and p.is_cuda and p.dtype == torch.float32 and kernels.FUSED_ENDS

    def _clip_torch(self, g):
        """clip_grad_norm_ with torch ops, the device kernels' arithmetic: fp64 sum of squares (max |g|), fp32 total, fp32
        coefficient."""
        max_norm, norm_type = self.clip
        total = (g.abs().max() if norm_type == 0 else g.double().square().sum().sqrt()).to(torch.float32)
        coef = max_norm / (total + 1e-6)
        coef = torch.where(coef < 1.0, coef, torch.ones_like(coef))
        g.mul_(coef.to(g.dtype))
        self.grad_norm.copy_(total.reshape(1))

    def _norm_partials(self, g, st):
        rc = native.lib().dsgcn_grad_norm_partials(g.data_ptr(), g.numel(), self.clip[1], self.clip_partial.data_ptr(), st)
        native.check(rc, 'dsgcn_grad_norm_partials')

    def _accum_ready(self):
        if self.acc is None:
            raise RuntimeError(f'{type(self).__name__} was built with accumulate=1: there is no accumulation buffer')
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

    # ---- a momentum (SGD) / beta1 (Adam) that follows a schedule ----------------------------------------------------------
    def _setup_hyper(self, scheduled, value):
        """scheduled_momentum: the value lives in ``hyper_t`` (one fp64 device element, allocated here and only ever written
        in place), the update launches are the ``*_hyper`` forms that read it there, and ``set_momentum`` rewrites it — so a
        ``step()`` captured in a hipGraph follows a momentum schedule as it follows the rates.  ``initial_momentum`` is the
        schedule's base (mmcv's momentum hooks keep it in the param groups)."""
        self.scheduled_momentum = bool(scheduled)
        self.hyper_t = self.initial_momentum = None
        if self.scheduled_momentum:
            self.initial_momentum = check_momentum(value)
            self.hyper_t = torch.full((1,), self.initial_momentum, device=self.flat.flat_p.device, dtype=torch.float64)

    def set_momentum(self, value):
        """The momentum (FlatSGD) / beta1 (FlatAdam) of the next ``step()``: validated, then one in-place fill — like
        ``set_lr`` the value travels in the launch's arguments, no staging buffer, no sync."""
        if not self.scheduled_momentum:
            raise RuntimeError(f'{type(self).__name__}.set_momentum: build the optimizer with scheduled_momentum=True — the '
                               'update launches of this one take the value as an argument, a captured step would keep it')
        value = check_momentum(value)
        self._store_momentum(value)
        self.hyper_t.fill_(value)


    # ---- per-tensor groups and parameters without a gradient (FlatAdam; FlatSGD with a group table) --------------------
    def _setup_groups(self, rules, paramwise, default_wd):
        """rules: paramwise.param_rules() over flat.module (every parameter, frozen ones included)."""
        by_id = {id(r.param): k for k, r in enumerate(rules)}
        self.rules = rules
        self.paramwise = bool(paramwise)
        self.default_wd = default_wd
        self.param_ids = [by_id[id(p)] for p in self.flat.params]         # slot of each flat tensor in parameters() order
        wd_of = lambda r: default_wd if r.weight_decay is None else r.weight_decay
        self.table = GroupTable(self.flat, [rules[k].lr for k in self.param_ids], [wd_of(rules[k]) for k in self.param_ids])
        self.base_lr = self.lr = self.table.base_lrs[0]
        self._live_fixed = False
        self.flat.grad_observers.append(self._observe_grads)

    @property
    def group_base_lrs(self):
        """The initial rate of every device group: the schedule is evaluated once per entry (``set_lr`` takes the list).
        None for an optimizer without a group table (plain FlatSGD: one rate)."""
        return None if self.table is None else list(self.table.base_lrs)

    def set_lr(self, lr):
        """One rate per group (the order of ``group_base_lrs``).  A scalar is taken for every group only when all groups
        share one initial rate: otherwise mmcv's per-group ``get_lr(initial_lr)`` is not one number."""
        if isinstance(lr, (list, tuple)):
            lrs = [float(v) for v in lr]
        elif len(set(self.table.base_lrs)) == 1:
            lrs = [float(lr)] * len(self.table.base_lrs)
        else:
            raise ValueError(f'set_lr({lr!r}): the groups start from different rates {sorted(set(self.table.base_lrs))} — '
                             'pass one rate per group (group_base_lrs gives their initial rates)')
        self.table.set_lrs(lrs)
        self.lr = lrs[0]

    def _observe_grads(self, pattern):
        """Called by FlatParams.collect_grads with ``p.grad is not None`` per tensor.  torch skips a parameter without a
        gradient (no decay, no moments, no state entry), so such tensors go to the SKIP group — fixed at the first call,
        which must be an eager one (the table is rewritten by a host copy), and checked on every later one."""
        pattern = tuple(pattern)
        if not self._live_fixed:
            if self.flat.flat_p.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f'{type(self).__name__}: the first step must run eagerly — which parameters receive a '
                                   'gradient is written into the group table there, outside any capture')
            self.table.fix_live(pattern)
            self._live_fixed = True
        elif pattern != tuple(self.table.live):
            changed = [self.rules[self.param_ids[i]].name for i, (a, b) in enumerate(zip(pattern, self.table.live)) if a != b]
            raise RuntimeError(f'{type(self).__name__}: the set of parameters that receive a gradient changed '
                               f'({changed[:4]}{"..." if len(changed) > 4 else ""}); it is fixed at the first step')

    def _live(self, i):
        return self.table.live is None or self.table.live[i]

    def _torch_groups(self, extra):
        """torch's ``param_groups``: one group over all parameters, or one per parameter tensor under paramwise_cfg (frozen
        ones included: a slot without state).  extra: the optimizer's other hyper-parameters."""
        slot_group = {k: self.table.tensor_group[i] for i, k in enumerate(self.param_ids)}
        if not self.paramwise:
            return [dict(extra, lr=self.table.lrs[0], weight_decay=self.table.wds[0], initial_lr=self.table.base_lrs[0],
                         params=list(range(len(self.rules))))]
        groups = []
        for k, r in enumerate(self.rules):
            g = slot_group.get(k)
            if g is None:       # frozen: mmcv leaves it the optimizer's defaults; never updated, its rate is never read
                wd = self.default_wd if r.weight_decay is None else r.weight_decay
                groups.append(dict(extra, lr=r.lr, weight_decay=wd, initial_lr=r.lr, params=[k]))
            else:
                groups.append(dict(extra, lr=self.table.lrs[g], weight_decay=self.table.wds[g],
                                   initial_lr=self.table.base_lrs[g], params=[k]))
        return groups

    def _load_groups(self, groups):
        """The per-group rates of a checkpoint -> the device table, in place.  -> {slot: saved parameter id}."""
        ids = [pid for g in groups for pid in g['params']]
        if len(ids) != len(self.rules) or len(groups) not in (1, len(self.rules)):
            raise ValueError(f'{type(self).__name__}.load_state_dict: expected {len(self.rules)} parameters in 1 or '
                             f'{len(self.rules)} param groups, got {[len(g["params"]) for g in groups]}')
        group_of_slot = {}
        for g in groups:
            for pid in g['params']:
                group_of_slot[len(group_of_slot)] = g
        lrs, bases = list(self.table.lrs), list(self.table.base_lrs)
        seen = {}
        for i, k in enumerate(self.param_ids):
            dg = self.table.tensor_group[i]
            pair = (float(group_of_slot[k]['lr']), float(group_of_slot[k].get('initial_lr', bases[dg])))
            if seen.setdefault(dg, pair) != pair:
                raise ValueError(f'{type(self).__name__}.load_state_dict: {self.rules[k].name} carries (lr, initial_lr) = '
                                 f'{pair}, other tensors of its group {seen[dg]}: the checkpoint was written under another '
                                 'paramwise_cfg')
            lrs[dg], bases[dg] = pair
        self.table.base_lrs = bases
        self.base_lr = bases[0]
        self.set_lr(lrs)
        return dict(enumerate(ids))


class FlatSGD(_FlatOptimizer):
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
    empty between groups and not part of ``state_dict()``.

    ``rules`` (``paramwise.param_rules``: one (lr, weight_decay) per parameter tensor, mmcv's ``paramwise_cfg``): the update
    is the grouped kernel of csrc/optim.hip — the same arithmetic with the rate and the decay looked up per element — and
    tensors that never receive a gradient are left alone, as torch leaves a ``.grad`` of None.  ``lr`` / ``weight_decay``
    are then the rules'; ``set_lr`` takes one rate per group.  Without ``rules`` nothing changes: one rate, one decay, the
    launches ``dsgcn_sgd_step`` / ``dsgcn_sgd_step_clip``."""


    def __init__(self, flat, lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True, capturable=False, grad_clip=None,
                 accumulate=1, rules=None, paramwise=True, scheduled_momentum=False):
        """scheduled_momentum: see ``_setup_hyper`` / ``set_momentum``.  Implies ``capturable``; the momentum buffer exists
        from the start whatever the first value (a schedule may pass through 0 and leave it again: at 0 the buffer is left
        alone, as torch leaves it)."""
        if scheduled_momentum:
            capturable = True
        self.lr = lr
        self.base_lr = lr
        self.momentum = momentum
        self.weight_decay = weight_decay
        self.nesterov = nesterov
        self.buf = None
        self.table = None
        if rules is not None:
            capturable = True                              # the grouped path keeps its rates on the device (GroupTable.lr_t)
        self.lr_t = None
        if capturable and rules is None:
            self.lr_t = torch.full((1,), float(lr), device=flat.flat_p.device, dtype=flat.flat_p.dtype)
        if capturable and (momentum or scheduled_momentum):
            self.buf = torch.zeros_like(flat.flat_p)       # torch's first step sets buf = g; momentum * 0 + g is the same value
        self._setup(flat, capturable, grad_clip, accumulate)
        self._setup_hyper(scheduled_momentum, momentum)
        if rules is not None:
            if not momentum >= 0.0:
                raise ValueError(f'Invalid momentum value: {momentum}')
            self._setup_groups(rules, paramwise, default_wd=0.0)

    def set_lr(self, lr):
        if self.table is not None:
            return _FlatOptimizer.set_lr(self, lr)
        self.lr = float(lr)
        if self.lr_t is not None:
            self.lr_t.fill_(self.lr)

    def _store_momentum(self, value):
        self.momentum = value

    @torch.no_grad()
    def _step_grouped(self):
        p, g, t = self.flat.flat_p, self.flat.flat_g, self.table
        if self._fused():
            st = torch.cuda.current_stream().cuda_stream
            if self.scheduled_momentum:
                return self._step_grouped_hyper(p, g, t, st)
            buf = self.buf.data_ptr() if self.momentum else None
            if self.clip is not None:
                self._norm_partials(g, st)
                rc = native.lib().dsgcn_sgd_group_step_clip(p.data_ptr(), g.data_ptr(), buf, *t.pointers(),
                                                            self.clip_partial.data_ptr(), self.clip_partial.numel(),
                                                            self.clip[1], self.clip[0], self.grad_norm.data_ptr(),
                                                            float(self.momentum), int(bool(self.nesterov)), p.numel(), st)
                native.check(rc, 'dsgcn_sgd_group_step_clip')
            else:
                rc = native.lib().dsgcn_sgd_group_step(p.data_ptr(), g.data_ptr(), buf, *t.pointers(), float(self.momentum),
                                                       int(bool(self.nesterov)), p.numel(), st)
                native.check(rc, 'dsgcn_sgd_group_step')
            return
        if self.clip is not None:
            self._clip_torch(g)
        # torch.optim.SGD's single-tensor sequence on the views, tensor by tensor: the same bits as torch on the CPU
        for off, n, lr, wd in t.tensors():
            pv, d = p[off:off + n], g[off:off + n]
            if wd != 0:
                d = d.add(pv, alpha=wd)
            if self.momentum:
                bv = self.buf[off:off + n]
                bv.mul_(self.momentum).add_(d)                  # (buf starts at zero: torch's first step sets buf = d)
                d = d.add(bv, alpha=self.momentum) if self.nesterov else bv
            pv.add_(d, alpha=-lr)

    def _step_grouped_hyper(self, p, g, t, st):
        """The grouped launches with the momentum read from ``hyper_t`` (csrc/optim.hip, the DEV forms)."""
        hyper, nesterov = self.hyper_t.data_ptr(), int(bool(self.nesterov))
        if self.clip is not None:
            self._norm_partials(g, st)
            rc = native.lib().dsgcn_sgd_group_step_clip_hyper(p.data_ptr(), g.data_ptr(), self.buf.data_ptr(), *t.pointers(),
                                                              self.clip_partial.data_ptr(), self.clip_partial.numel(),
                                                              self.clip[1], self.clip[0], self.grad_norm.data_ptr(), hyper,
                                                              nesterov, p.numel(), st)
            native.check(rc, 'dsgcn_sgd_group_step_clip_hyper')
        else:
            rc = native.lib().dsgcn_sgd_group_step_hyper(p.data_ptr(), g.data_ptr(), self.buf.data_ptr(), *t.pointers(), hyper,
                                                         nesterov, p.numel(), st)
            native.check(rc, 'dsgcn_sgd_group_step_hyper')

    def _step_hyper(self, p, g):
        """``dsgcn_sgd_step[_clip]`` with the momentum read from ``hyper_t`` (k_sgd_hyper / k_sgd_clip_hyper)."""
        st = torch.cuda.current_stream().cuda_stream
        if self.clip is not None:
            max_norm, norm_type = self.clip
            self._norm_partials(g, st)
            rc = native.lib().dsgcn_sgd_step_clip_hyper(p.data_ptr(), g.data_ptr(), self.buf.data_ptr(), self.lr_t.data_ptr(),
                                                        self.clip_partial.data_ptr(), self.clip_partial.numel(), norm_type,
                                                        max_norm, self.grad_norm.data_ptr(), self.hyper_t.data_ptr(),
                                                        float(self.weight_decay), int(bool(self.nesterov)), p.numel(), st)
            native.check(rc, 'dsgcn_sgd_step_clip_hyper')
        else:
            rc = native.lib().dsgcn_sgd_step_hyper(p.data_ptr(), g.data_ptr(), self.buf.data_ptr(), self.lr_t.data_ptr(),
                                                   self.hyper_t.data_ptr(), float(self.weight_decay),
                                                   int(bool(self.nesterov)), p.numel(), st)
            native.check(rc, 'dsgcn_sgd_step_hyper')

    @torch.no_grad()
    def step(self):
        if self.table is not None:
            return self._step_grouped()
        p, g = self.flat.flat_p, self.flat.flat_g
        if self.scheduled_momentum and self._fused():
            return self._step_hyper(p, g)
        if self.clip is not None and self._fused():
            # norm partials, then clip + update in one launch (csrc/clip.hip): one extra read of the flat gradient
            max_norm, norm_type = self.clip
            st = torch.cuda.current_stream().cuda_stream
            self._norm_partials(g, st)
            rc = native.lib().dsgcn_sgd_step_clip(p.data_ptr(), g.data_ptr(), self.buf.data_ptr() if self.momentum else None,
                                                  self.lr_t.data_ptr(), self.clip_partial.data_ptr(),
                                                  self.clip_partial.numel(), norm_type, max_norm, self.grad_norm.data_ptr(),
                                                  float(self.momentum), float(self.weight_decay),
                                                  int(bool(self.nesterov)), p.numel(), st)
            native.check(rc, 'dsgcn_sgd_step_clip')
            return
        if self.clip is not None:
            self._clip_torch(g)
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

    def state_dict(self):
        """torch.optim.SGD's layout — ``{'state': {i: {'momentum_buffer': tensor}}, 'param_groups': [{...}]}`` with one
        entry per parameter tensor in ``module.parameters()`` order — so the ``optimizer`` entry of a checkpoint is
        interchangeable with the reference's (mmcv saves ``optimizer.state_dict()`` of a torch SGD).  CPU tensors."""
        if self.table is not None:
            return self._state_dict_grouped()
        state = {}
        if self.buf is not None and (not self.capturable or bool(self.buf.any())):     # all-zero = no step taken yet
            for i, (p, (off, n)) in enumerate(zip(self.flat.params, self.flat.slices)):
                state[i] = {'momentum_buffer': self.buf[off:off + n].view(p.shape).detach().cpu().clone()}
        group = dict(lr=self.lr, momentum=self.momentum, dampening=0, weight_decay=self.weight_decay,
                     nesterov=self.nesterov, maximize=False, foreach=None, differentiable=False, fused=None,
                     initial_lr=self.base_lr, params=list(range(len(self.flat.params))))
        if self.scheduled_momentum:
            group['initial_momentum'] = self.initial_momentum
        return {'state': state, 'param_groups': [group]}

    def load_state_dict(self, sd):
        """Accepts the torch SGD layout (this class's own checkpoints and the reference's)."""
        if self.table is not None:
            return self._load_state_dict_grouped(sd)
        groups = sd['param_groups']
        if len(groups) != 1 or len(groups[0]['params']) != len(self.flat.params):
            raise ValueError('FlatSGD.load_state_dict: expected one param group over '
                             f'{len(self.flat.params)} tensors, got {[len(g["params"]) for g in groups]}')
        g = groups[0]
        self.set_lr(g['lr'])
        self.base_lr = g.get('initial_lr', self.base_lr)
        self._load_momentum(g.get('momentum', self.momentum))
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

    def _load_momentum(self, value):
        """A checkpoint's current momentum: to the device too when it is scheduled (the schedule's base, ``initial_momentum``,
        always comes from the config)."""
        if self.scheduled_momentum:
            self.set_momentum(value)
        else:
            self.momentum = value

    def _state_dict_grouped(self):
        """The same layout with the parameters numbered over ALL of ``parameters()`` and, under paramwise_cfg, one param
        group per tensor; a tensor that never received a gradient has no state entry."""
        state = {}
        if self.buf is not None and bool(self.buf.any()):
            for i, (p, (off, n)) in enumerate(zip(self.flat.params, self.flat.slices)):
                if self._live(i):
                    state[self.param_ids[i]] = {'momentum_buffer': self.buf[off:off + n].view(p.shape).detach().cpu().clone()}
        extra = dict(momentum=self.momentum, dampening=0, nesterov=self.nesterov, maximize=False, foreach=None,
                     differentiable=False, fused=None)
        if self.scheduled_momentum:
            extra['initial_momentum'] = self.initial_momentum
        return {'state': state, 'param_groups': self._torch_groups(extra)}

    def _load_state_dict_grouped(self, sd):
        saved = self._load_groups(sd['param_groups'])
        g0 = sd['param_groups'][0]
        self._load_momentum(g0.get('momentum', self.momentum))
        self.nesterov = g0.get('nesterov', self.nesterov)
        state = sd.get('state', {})
        if self.buf is not None:
            self.buf.zero_()                               # in place: a captured step holds its address
            for i, k in enumerate(self.param_ids):
                mb = state.get(saved[k], state.get(str(saved[k]), {})).get('momentum_buffer')
                if mb is not None:
                    off, n = self.flat.slices[i]
                    self.buf[off:off + n].copy_(mb.reshape(-1))


class FlatAdam(_FlatOptimizer):
    """torch.optim.Adam / AdamW (``decoupled=True``) over ``FlatParams`` buffers, ``amsgrad=False, maximize=False``, in
    torch's single-tensor order; one launch per update (csrc/optim.hip), two with ``grad_clip``.

    Always ``capturable``: ``m``, ``v``, the per-group rates and the step count live in device memory allocated here and are
    only ever written in place (``load_state_dict`` included), and the update launch advances the step count itself, so a
    ``step()`` captured in a hipGraph follows the schedule and counts on with every replay.  ``step_t`` holds one int32
    counter per workgroup of the launch, all equal (no workgroup reads what another one writes); ``steps`` reads it.

    ``rules``: ``paramwise.param_rules`` — one (lr, weight_decay) per parameter tensor; default one group.  ``set_lr`` takes
    one rate per group (``group_base_lrs``).  A tensor that never receives a gradient (the dead ``conv2_se`` tensors) is left
    untouched and has no state, as in torch: under Adam with L2 decay it would otherwise walk at rate lr per step.  Which
    tensors those are is read at the first ``FlatParams.collect_grads``, which must run eagerly.
    ``grad_clip`` / ``accumulate`` / ``accum_*``: as in ``FlatSGD``.  ``state_dict`` has torch's layout (``step`` a float
    tensor, ``exp_avg``, ``exp_avg_sq``; every param group carries ``initial_lr``)."""

    def __init__(self, flat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=None, decoupled=False, grad_clip=None,
                 accumulate=1, rules=None, paramwise=None, scheduled_momentum=False):
        """scheduled_momentum: beta1 follows a schedule (``_setup_hyper`` / ``set_momentum``); torch's behaviour when a param
        group's ``betas[0]`` changes between steps, bias correction ``1 - beta1 ** t`` with the current value included."""
        from .paramwise import param_rules
        default_wd = 1e-2 if decoupled else 0.0            # torch.optim.AdamW / Adam
        if not 0.0 <= lr:
            raise ValueError(f'Invalid learning rate: {lr}')
        if not 0.0 <= eps:
            raise ValueError(f'Invalid epsilon value: {eps}')
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f'Invalid beta parameter at index 0: {betas[0]}')
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f'Invalid beta parameter at index 1: {betas[1]}')
        self.betas = (float(betas[0]), float(betas[1]))
        self.eps = float(eps)
        self.decoupled = bool(decoupled)
        self._setup(flat, True, grad_clip, accumulate)
        self._setup_hyper(scheduled_momentum, self.betas[0])
        if rules is None:
            rules = param_rules(flat.module, lr, weight_decay)
        self._setup_groups(rules, bool(paramwise), default_wd)
        self.weight_decay = self.table.wds[0]
        self.m = torch.zeros_like(flat.flat_p)
        self.v = torch.zeros_like(flat.flat_p)
        self.step_t = torch.zeros(self.table.chunks, dtype=torch.int32, device=flat.flat_p.device)

    @property
    def steps(self):
        """Updates taken so far (one host read)."""
        return int(self.step_t[0])

    def _store_momentum(self, value):
        self.betas = (value, self.betas[1])

    @torch.no_grad()
    def step(self):
        p, g, t = self.flat.flat_p, self.flat.flat_g, self.table
        if self._fused():
            st = torch.cuda.current_stream().cuda_stream
            head = (p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.step_t.data_ptr()) + t.pointers()
            tail = (self.betas[0], self.betas[1], self.eps, int(self.decoupled), p.numel(), st)
            if self.scheduled_momentum:                    # beta1 read from hyper_t (csrc/optim.hip, the DEV forms)
                tail = (self.hyper_t.data_ptr(),) + tail[1:]
                if self.clip is not None:
                    self._norm_partials(g, st)
                    rc = native.lib().dsgcn_adam_step_clip_hyper(*head, self.clip_partial.data_ptr(),
                                                                 self.clip_partial.numel(), self.clip[1], self.clip[0],
                                                                 self.grad_norm.data_ptr(), *tail)
                    native.check(rc, 'dsgcn_adam_step_clip_hyper')
                else:
                    native.check(native.lib().dsgcn_adam_step_hyper(*head, *tail), 'dsgcn_adam_step_hyper')
                return
            if self.clip is not None:
                self._norm_partials(g, st)
                rc = native.lib().dsgcn_adam_step_clip(*head, self.clip_partial.data_ptr(), self.clip_partial.numel(),
                                                       self.clip[1], self.clip[0], self.grad_norm.data_ptr(), *tail)
                native.check(rc, 'dsgcn_adam_step_clip')
            else:
                native.check(native.lib().dsgcn_adam_step(*head, *tail), 'dsgcn_adam_step')
            return
        if self.clip is not None:
            self._clip_torch(g)
        self.step_t.add_(1)
        b1, b2 = self.betas
        bc1, bc2 = 1 - b1 ** self.steps, 1 - b2 ** self.steps
        # torch/optim/adam.py _single_tensor_adam on the views, tensor by tensor: the same bits as torch on the CPU
        bc2_sqrt = bc2 ** 0.5
        for off, n, lr, wd in t.tensors():
            pv, d, mv, vv = p[off:off + n], g[off:off + n], self.m[off:off + n], self.v[off:off + n]
            if self.decoupled:
                pv.mul_(1 - lr * wd)
            elif wd != 0:
                d = d.add(pv, alpha=wd)
            mv.lerp_(d, 1 - b1)
            vv.mul_(b2).addcmul_(d, d, value=1 - b2)
            denom = (vv.sqrt() / bc2_sqrt).add_(self.eps)
            pv.addcdiv_(mv, denom, value=-(lr / bc1))

    def state_dict(self):
        state = {}
        steps = self.steps
        if steps:
            for i, (p, (off, n)) in enumerate(zip(self.flat.params, self.flat.slices)):
                if self._live(i):
                    state[self.param_ids[i]] = {'step': torch.tensor(float(steps)),
                                                'exp_avg': self.m[off:off + n].view(p.shape).detach().cpu().clone(),
                                                'exp_avg_sq': self.v[off:off + n].view(p.shape).detach().cpu().clone()}
        extra = dict(betas=self.betas, eps=self.eps, amsgrad=False, maximize=False, foreach=None, capturable=False,
                     differentiable=False, fused=None, decoupled_weight_decay=self.decoupled)
        if self.scheduled_momentum:
            extra['initial_momentum'] = self.initial_momentum
        return {'state': state, 'param_groups': self._torch_groups(extra)}

    def load_state_dict(self, sd):
        """Accepts torch.optim.Adam / AdamW's layout (this class's own checkpoints and the reference's); ``step`` an int or
        a tensor.  Everything is restored in place: a captured ``step()`` holds the addresses."""
        saved = self._load_groups(sd['param_groups'])
        g0 = sd['param_groups'][0]
        self.betas = tuple(float(b) for b in g0.get('betas', self.betas))
        if self.scheduled_momentum:
            self.set_momentum(self.betas[0])               # the current value, on the device too
        self.eps = float(g0.get('eps', self.eps))
        state = sd.get('state', {})
        self.m.zero_()
        self.v.zero_()
        steps = set()
        for i, k in enumerate(self.param_ids):
            st = state.get(saved[k], state.get(str(saved[k])))
            if st:
                off, n = self.flat.slices[i]
                self.m[off:off + n].copy_(st['exp_avg'].reshape(-1))
                self.v[off:off + n].copy_(st['exp_avg_sq'].reshape(-1))
                steps.add(int(st['step']))
        if len(steps) > 1:
            raise ValueError(f'FlatAdam.load_state_dict: the parameters carry different step counts {sorted(steps)}')
        self.step_t.fill_(steps.pop() if steps else 0)


def build_optimizer(flat, cfg, grad_clip=None, accumulate=1, scheduled_momentum=False):
    """mmcv's ``build_optimizer(model, cfg)`` over a ``FlatParams``: ``cfg = dict(type='SGD' | 'Adam' | 'AdamW', ...,
    paramwise_cfg=...)`` with torch's defaults for absent keys.  SGD without ``paramwise_cfg`` is the plain ``FlatSGD``.
    scheduled_momentum: the run has a ``momentum_config`` — momentum / beta1 live on the device (``set_momentum``)."""
    from .paramwise import param_rules
    cfg = dict(cfg)
    kind = cfg.pop('type', 'SGD')
    ctor = cfg.pop('constructor', 'DefaultOptimizerConstructor')
    if ctor != 'DefaultOptimizerConstructor':
        raise NotImplementedError(f'optimizer constructor {ctor!r}: DefaultOptimizerConstructor is implemented')
    paramwise_cfg = cfg.pop('paramwise_cfg', None)
    for key in ('foreach', 'fused', 'differentiable', 'capturable'):      # how torch runs the update, not what it computes
        cfg.pop(key, None)
    if cfg.pop('maximize', False):
        raise NotImplementedError('optimizer maximize=True is not supported')
    base_wd = cfg.pop('weight_decay', None)
    if kind == 'SGD':
        if cfg.pop('dampening', 0) != 0:
            raise NotImplementedError('optimizer dampening != 0 is not supported')
        lr, momentum, nesterov = cfg.pop('lr', 1e-3), cfg.pop('momentum', 0), cfg.pop('nesterov', False)
        if cfg:
            raise NotImplementedError(f'SGD options {sorted(cfg)} are not supported')
        if nesterov and momentum <= 0:
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')
        if paramwise_cfg is None:
            return FlatSGD(flat, lr=lr, momentum=momentum, weight_decay=base_wd or 0, nesterov=nesterov, capturable=True,
                           grad_clip=grad_clip, accumulate=accumulate, scheduled_momentum=scheduled_momentum)
        rules = param_rules(flat.module, lr, base_wd, paramwise_cfg)
        return FlatSGD(flat, lr=lr, momentum=momentum, weight_decay=base_wd or 0, nesterov=nesterov, capturable=True,
                       grad_clip=grad_clip, accumulate=accumulate, rules=rules, paramwise=True,
                       scheduled_momentum=scheduled_momentum)
    if kind in ('Adam', 'AdamW'):
        if cfg.pop('amsgrad', False):
            raise NotImplementedError('optimizer amsgrad=True is not supported')
        lr, betas, eps = cfg.pop('lr', 1e-3), cfg.pop('betas', (0.9, 0.999)), cfg.pop('eps', 1e-8)
        if cfg.pop('decoupled_weight_decay', kind == 'AdamW') != (kind == 'AdamW'):
            raise NotImplementedError("optimizer decoupled_weight_decay: choose type='Adam' or type='AdamW' instead")
        if cfg:
            raise NotImplementedError(f'{kind} options {sorted(cfg)} are not supported')
        rules = param_rules(flat.module, lr, base_wd, paramwise_cfg)
        return FlatAdam(flat, lr=lr, betas=betas, eps=eps, weight_decay=base_wd, decoupled=kind == 'AdamW',
                        grad_clip=grad_clip, accumulate=accumulate, rules=rules, paramwise=paramwise_cfg is not None,
                        scheduled_momentum=scheduled_momentum)
    raise NotImplementedError(f'optimizer type {kind!r}: SGD, Adam and AdamW are implemented')


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


# ---- mmcv's other rate policies and its two momentum policies: pure functions of the run's position -----------------------
# `progress` is runner.iter or runner.epoch (by_epoch), `max_progress` max_iters or max_epochs.

def cos_anneal(start, end, factor, weight=1):
    """mmcv annealing_cos: from ``start`` (factor 0) to ``end`` (factor 1) along half a cosine."""
    return end + 0.5 * weight * (start - end) * (math.cos(math.pi * factor) + 1)


def lin_anneal(start, end, factor):
    """mmcv annealing_linear."""
    return (end - start) * factor + start


ANNEAL = {'cos': cos_anneal, 'linear': lin_anneal}


def anneal_target(base, min_lr=None, min_lr_ratio=None):
    """The floor of the cosine policies: ``min_lr``, or ``base * min_lr_ratio`` — exactly one of the two (mmcv asserts it)."""
    if (min_lr is None) == (min_lr_ratio is None):
        raise ValueError('exactly one of min_lr and min_lr_ratio must be given')
    return base * min_lr_ratio if min_lr_ratio is not None else min_lr


def exp_lr(base, progress, gamma):
    """mmcv ExpLrUpdaterHook."""
    return base * gamma ** progress


def poly_lr(base, progress, max_progress, power=1., min_lr=0.):
    """mmcv PolyLrUpdaterHook."""
    coeff = (1 - progress / max_progress) ** power
    return (base - min_lr) * coeff + min_lr


def inv_lr(base, progress, gamma, power=1.):
    """mmcv InvLrUpdaterHook."""
    return base * (1 + gamma * progress) ** (-power)


def cosine_restart_lr(base, progress, periods, restart_weights=(1,), min_lr=None, min_lr_ratio=None):
    """mmcv CosineRestartLrUpdaterHook: period i runs from cum[i - 1] to cum[i] and anneals from
    ``target + restart_weights[i] * (base - target)`` down to the target."""
    target = anneal_target(base, min_lr, min_lr_ratio)
    cum = 0
    for i, period in enumerate(periods):
        start, cum = cum, cum + period
        if progress < cum:
            alpha = min((progress - start) / period, 1)
            return cos_anneal(base, target, alpha, restart_weights[i])
    raise ValueError(f'Current iteration {progress} exceeds cumulative_periods {cum}')


def cyclic_value(base, it, max_iters, target_ratio=(10, 1e-4), cyclic_times=1, step_ratio_up=0.4, anneal='cos'):
    """mmcv CyclicLrUpdaterHook / CyclicMomentumUpdaterHook (by iteration): ``cyclic_times`` cycles of
    ``L = max_iters // cyclic_times`` iterations, each ``base -> base * target_ratio[0]`` over the first
    ``int(step_ratio_up * L)`` iterations and ``-> base * target_ratio[1]`` over the rest."""
    length = max_iters // cyclic_times
    up = int(step_ratio_up * length)
    c = it % length
    fn = ANNEAL[anneal]
    if c < up:
        return fn(base, base * target_ratio[0], c / up)
    return fn(base * target_ratio[0], base * target_ratio[1], (c - up) / (length - up))


def onecycle_value(values, it, total_steps, pct_start=0.3, anneal='cos', three_phase=False):
    """The phase walk mmcv's OneCycleLrUpdaterHook and OneCycleMomentumUpdaterHook share (torch's OneCycleLR).  values:
    the phase end points, ``(v0, v1, v2)`` for two phases (v0 -> v1 until ``pct_start * S - 1``, v1 -> v2 until ``S - 1``),
    ``(v0, v1, v2, v3)`` for three (the middle one ends at ``2 * pct_start * S - 2``)."""
    ends = [float(pct_start * total_steps) - 1]
    if three_phase:
        ends.append(float(2 * pct_start * total_steps) - 2)
    ends.append(total_steps - 1)
    fn = ANNEAL[anneal]
    start = 0
    for i, end in enumerate(ends):
        if it <= end:
            return fn(values[i], values[i + 1], (it - start) / (end - start))
        start = end
    raise ValueError(f'iteration {it} lies beyond the {total_steps} steps of the cycle')


def onecycle_lr_values(base, div_factor=25, final_div_factor=1e4, three_phase=False):
    """Phase end points of the OneCycle rate for a group whose initial rate is ``base`` (= max_lr / div_factor)."""
    if three_phase:
        return base * 1, base * div_factor, base * 1, base * (1 / final_div_factor)
    return base * 1, base * div_factor, base * (1 / final_div_factor)


def onecycle_momentum_values(base_momentum=0.85, max_momentum=0.95, three_phase=False):
    """Phase end points of the OneCycle momentum: max -> base -> max, and with three phases max held to the end."""
    if three_phase:
        return max_momentum, base_momentum, max_momentum, max_momentum
    return max_momentum, base_momentum, max_momentum


def check_momentum(value, what='momentum'):
    """A scheduled momentum / beta1 must lie in [0, 1): the update kernels read it from device memory and use it as it is."""
    value = float(value)
    if not 0.0 <= value < 1.0:
        raise ValueError(f'{what} {value!r} is outside [0, 1)')
    return value
