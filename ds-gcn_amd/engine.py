"""One optimisation step of a recognizer on one GPU of a data-parallel job, the MI355X way.

The reference's step (mmcv runner over torch DDP: pyskl/core/local_runner/epoch_based_sparse_runner.py:26-52 with
OptimizerHook and CosineAnnealingLrUpdaterHook, pyskl/apis/train.py:94-134) is ~2 k eager launches, four host syncs for
the log scalars and a bucketed NCCL all-reduce.  Here:

    graph A (hipGraph replay): zero-grad + forward + backward + pack gradients into the flat buffer
    one RCCL all-reduce of the flat gradient buffer (N > 1; between the graphs, never captured)
    graph B (hipGraph replay): SGD-nesterov update on the flat buffers, rate read from a device scalar; with
                               ``grad_clip`` the total-norm clip of the averaged gradient rides in the same graph; with
                               ``ema`` (mmcv's EMAHook) the weight average's one launch is its last node

With ``accumulate=k > 1`` (mmcv GradientCumulativeOptimizerHook) a call of ``step()`` is one micro-iteration: graph A ends
in ``acc += g`` on k - 1 calls out of k (graph M, no exchange, no update) and in ``g = (acc + g) / k, acc = 0`` on the k-th
(graph S), which the exchange and graph B follow unchanged.

``bench.py`` times exactly this object, ``apis.train_model`` drives it epoch by epoch.
"""
import torch
import torch.distributed as dist

from . import kernels
from .data_parallel import FlatDataParallel, FlatParams
from .ema import FlatEMA, parse_ema
from .train import FlatAdam, FlatSGD, build_optimizer


class TrainEngine:

    def __init__(self, model, lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True, process_group=None, use_graph=True,
                 warmup_eager=2, strict_graph=False, extra_allreduce=False, grad_clip=None, accumulate=1, optimizer=None,
                 matmul_precision=None, scheduled_momentum=False, ema=None):
        """optimizer: mmcv's ``optimizer`` dict (``type`` 'SGD' | 'Adam' | 'AdamW', ..., ``paramwise_cfg``; see
        ``train.build_optimizer``) or a ``FlatSGD`` / ``FlatAdam`` built over ``FlatParams(model, gather=True)`` — in place of
        the keywords lr / momentum / weight_decay / nesterov (and, for a built one, of grad_clip / accumulate, which it
        carries).  FlatAdam and FlatSGD with per-tensor groups skip the parameters that receive no gradient and learn
        which ones those are at the first step, which must therefore be eager: ``warmup_eager=0`` raises.
        grad_clip: mmcv's ``optimizer_config.grad_clip`` dict (``max_norm``, ``norm_type`` 2 or inf) or None.  The clip
        runs with the update, AFTER the all-reduce (the reference's order: backward, DDP average, clip_grads, step): every
        rank holds the same averaged buffer and the norm is reduced in a fixed order, so every rank applies the same
        coefficient without a second collective.  ``step()`` then also returns ``grad_norm`` (before clipping).
        strict_graph: a failed capture raises instead of falling back to eager launches (multi-GPU runs: ranks must not
        silently differ).  extra_allreduce: issue the gradient all-reduce even at world size 1 (measurement of the N > 1
        call sequence under a 1-rank RCCL group).
        accumulate: mmcv's ``GradientCumulativeOptimizerHook.cumulative_iters``.  With k > 1 every ``step()`` is one
        micro-iteration — forward, backward (its own BatchNorm statistics, its own dropout masks), gradient added to the
        accumulator — and every k-th one also averages the k gradients, exchanges, clips and updates, at the rate passed
        on THAT call: k micro-batches on one GPU are the reference's k ranks.  ``flush()`` closes a short last group.
        scheduled_momentum: the optimizer built here keeps its momentum (SGD) / beta1 (Adam) in device memory and
        ``step(..., momentum=...)`` rewrites it: graph B follows a momentum schedule as it follows the rate (a built
        optimizer carries its own flag).
        matmul_precision: 'highest' | 'high' (``kernels.set_matmul_precision``) or None = the process level at this moment.
        Fixed here: every eager step, capture and replay of this engine runs under it, whatever the process level is set
        to later and whatever level another engine of the process uses.
        ema: None, or mmcv's ``EMAHook`` options ``dict(momentum=0.0002, interval=1, warm_up=100)`` (``ema.parse_ema``).
        The engine then keeps an exponential moving average of the weights (``self.ema``, a ``FlatEMA``; its buffers ride
        in the model's ``state_dict()`` under mmcv's ``ema_*`` names) and every ``step()`` — a micro-iteration included, as
        mmcv's ``after_train_iter`` runs on each — ends with ONE more launch, behind the update: inside graph B where there
        is one, a plain launch behind graph A on a micro-iteration.  Its ``m`` is a device scalar set from ``ema_iter``
        before the replay: no re-capture, no sync.  ``flush()`` leaves the average alone.  Data-parallel runs need no
        collective for it: every rank averages the same weights.  With None the engine launches what it always did."""
        self.model = model
        self.matmul_precision = kernels.get_matmul_precision() if matmul_precision is None else matmul_precision
        kernels.matmul_precision(self.matmul_precision)        # (ValueError for an unknown name)
        if isinstance(optimizer, (FlatSGD, FlatAdam)):
            if optimizer.flat.module is not model or not optimizer.flat.gather or not optimizer.capturable:
                raise ValueError('TrainEngine(optimizer=...): build it with capturable=True over FlatParams(model, gather=True)')
            self.flat = optimizer.flat
        else:
            self.flat = FlatParams(model, gather=True)
        self.dp = FlatDataParallel(self.flat, process_group)
        # the averaged copy starts from the weights every rank holds AFTER the wrap-time broadcast, and its buffers are
        # registered after it: they are no part of that broadcast (nor of any later collective)
        self.ema = None if ema is None else FlatEMA(self.flat, **parse_ema(ema, 'TrainEngine(ema=...)'))
        self.ema_iter = 0          # the runner's iteration the next step() is (a resumed run sets it; `iter` starts at 0)
        if isinstance(optimizer, (FlatSGD, FlatAdam)):
            self.opt = optimizer
        elif optimizer is not None:
            self.opt = build_optimizer(self.flat, optimizer, grad_clip=grad_clip, accumulate=accumulate,
                                       scheduled_momentum=scheduled_momentum)
        else:
            self.opt = FlatSGD(self.flat, lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov,
                               capturable=True, grad_clip=grad_clip, accumulate=accumulate,
                               scheduled_momentum=scheduled_momentum)
        if getattr(self.opt, 'table', None) is not None and bool(use_graph) and warmup_eager < 1:
            raise ValueError(f'{type(self.opt).__name__} with per-tensor groups needs warmup_eager >= 1: the first step runs '
                             'eagerly, the parameters that receive no gradient are marked there')
        self.accumulate = self.opt.accumulate
        self.pending = 0           # gradients in the accumulator: micro-iterations since the last update
        self.use_graph = bool(use_graph) and self.flat.flat_p.is_cuda
        self.strict_graph = strict_graph
        self.extra_allreduce = extra_allreduce
        self.warmup_eager = warmup_eager
        # batch shape [+ 'micro' | 'step' with accumulate > 1] -> (graph A, graph B or None, static keypoint, static label,
        # static outputs)
        self._graphs = {}
        self._seen = {}            # the same key -> eager steps taken
        self.capture_error = None
        self._seed = None
        self.iter = 0

    # ---- pieces --------------------------------------------------------------------------------------------
    def _fwd_bwd(self, keypoint, label, kind=None):
        """kind: None (accumulate == 1) | 'micro' | 'step' — what follows the gradient collection."""
        self.opt.zero_grad()
        kernels.reset_leaf_uses()
        try:
            out = self.model.train_step(dict(keypoint=keypoint, label=label), None, sync_log_vars=False)
            loss = out['loss']
            if self._seed is None or self._seed.dtype != loss.dtype or self._seed.device != loss.device:
                self._seed = torch.ones((), dtype=loss.dtype, device=loss.device)  # (backward() fills a fresh one per step)
            if self.flat.flat_p.is_cuda:
                # parameter-gradient partial rows are summed by ONE launch at the end of the backward (kernels.param_colsum)
                with kernels.deferred_param_sums(self.flat):
                    loss.backward(self._seed)
            else:
                loss.backward(self._seed)
            self.flat.collect_grads()
            if kind == 'micro':
                self.opt.accum_add()
            elif kind == 'step':
                self.opt.accum_finish()
            kernels.dropout_step_advance()       # (fused dropout: the next step draws other masks; no-op without it)
        finally:
            # the update that follows rewrites the weights through raw pointers: cached weight images are stale from here
            kernels.end_step()
        return {k: v.detach() for k, v in out['log_vars'].items()}

    def _exchange(self):
        self.dp.allreduce_grads()
        if self.extra_allreduce and self.dp.world == 1 and dist.is_available() and dist.is_initialized():
            dist.all_reduce(self.flat.flat_g)

    def _capture(self, keypoint, label, kind=None):
        # no extra warm-up pass here: the eager steps that precede the capture (warmup_eager) already ran this shape —
        # allocator pools, the pinned pointer table of dsgcn_pack, the momentum buffer — and a pass that is not a real
        # step would move the BatchNorm running statistics once too often
        skp, slb = keypoint.clone(), label.clone()
        torch.cuda.synchronize()
        g_a = torch.cuda.CUDAGraph()
        # thread_local: the RCCL watchdog thread polls its events while we capture (N > 1); neither graph holds a collective
        with torch.cuda.graph(g_a, capture_error_mode='thread_local'):
            logs = self._fwd_bwd(skp, slb, kind)
        g_b = None
        if kind != 'micro':
            g_b = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g_b, capture_error_mode='thread_local'):
                self.opt.step()
                if self.ema is not None:
                    self.ema.launch()
        torch.cuda.synchronize()
        return g_a, g_b, skp, slb, self._with_grad_norm(logs, static=True)

    def _with_grad_norm(self, logs, static=False):
        """The optimizer's one-float norm as a log scalar: the static tensor itself beside a replayed graph's other static
        outputs, a copy of it after an eager step (whose other log tensors are fresh every step too)."""
        if self.opt.grad_norm is None:
            return logs
        return dict(logs, grad_norm=self.opt.grad_norm[0] if static else self.opt.grad_norm[0].clone())

    # ---- the step ------------------------------------------------------------------------------------------
    def step(self, keypoint, label, lr=None, momentum=None, ema_iter=None):
        """-> dict of detached DEVICE scalars (loss, loss_cls, top1_acc, top5_acc; grad_norm with grad_clip): no host
        sync here.  With accumulate > 1: one micro-iteration; grad_norm is the one of the last update.
        momentum: the momentum (SGD) / beta1 (Adam) of this iteration, for an optimizer with ``scheduled_momentum``.  As
        mmcv's momentum hooks do it is set before every iteration and the update sees the last one: under accumulation
        the value given at the stepping call.
        ema_iter: with ``ema``, the runner's iteration this call is (mmcv's ``runner.iter`` before its increment: it enters
        the warm-up of ``m`` and the ``interval`` gating); None: ``self.ema_iter``, which counts on from the last call."""
        with kernels.matmul_precision(self.matmul_precision):
            return self._step(keypoint, label, lr, momentum, ema_iter)

    def _step(self, keypoint, label, lr, momentum=None, ema_iter=None):
        if self.ema is not None:
            if self.ema.swapped:
                raise RuntimeError('TrainEngine.step: the model holds the averaged weights (ema.swapped): swap() them back '
                                   'before training on')
            if ema_iter is not None:
                self.ema_iter = int(ema_iter)
            self.ema.set_iter(self.ema_iter)       # one fill of the device scalar, ahead of whatever reads it below
        if lr is not None:
            self.opt.set_lr(lr)
        if momentum is not None:
            self.opt.set_momentum(momentum)
        key = (tuple(keypoint.shape), tuple(label.shape))
        kind = None
        if self.accumulate > 1:
            # a micro-iteration and a stepping iteration are two captures per batch shape, each after eager calls of its own
            kind = 'step' if self.pending + 1 == self.accumulate else 'micro'
            key = key + (kind,)
        if self.use_graph and key not in self._graphs and self._seen.get(key, 0) >= self.warmup_eager:
            try:
                self._graphs[key] = self._capture(keypoint, label, kind)
            except Exception as exc:       # noqa: BLE001 — report and fall back (or raise) below
                self.capture_error = f'{type(exc).__name__}: {exc}'
                if self.strict_graph:
                    raise
                self.use_graph = False
        if self.use_graph and key in self._graphs:
            g_a, g_b, skp, slb, logs = self._graphs[key]
            skp.copy_(keypoint)
            slb.copy_(label)
            g_a.replay()
            if kind != 'micro':
                self._exchange()
                g_b.replay()                       # (with ema: the average's launch is its last node)
            elif self.ema is not None:
                self.ema.launch()
        else:
            logs = self._fwd_bwd(keypoint, label, kind)
            if kind != 'micro':
                self._exchange()
                self.opt.step()
            if self.ema is not None:
                self.ema.launch()
            logs = self._with_grad_norm(logs)
            self._seen[key] = self._seen.get(key, 0) + 1
        if kind is not None:
            self.pending = self.pending + 1 if kind == 'micro' else 0
        self.iter += 1
        if self.ema is not None:
            self.ema_iter += 1
        return logs

    def flush(self, remainder=None, lr=None, momentum=None):
        """Close a short group early: average the ``remainder`` gradients in the accumulator (all of them; None = however
        many there are), exchange, clip and update — mmcv's rule for the last ``max_iters % k`` iterations of a run, which
        it divides by their own count.  The rate (the momentum) is ``lr`` (``momentum``) or the one of the last call.  Eager launches (once per run or
        epoch); no forward runs, so no BatchNorm statistic and no dropout counter moves.  -> {} or {'grad_norm': ...}."""
        if self.accumulate == 1:
            raise RuntimeError('flush(): this engine does not accumulate (accumulate=1)')
        if remainder is None:
            remainder = self.pending
        if remainder != self.pending or remainder < 1:
            raise ValueError(f'flush({remainder}): the accumulator holds {self.pending} gradient(s)')
        if lr is not None:
            self.opt.set_lr(lr)
        if momentum is not None:
            self.opt.set_momentum(momentum)
        self.flat.flat_g.zero_()                   # the group's gradients are all in the accumulator already
        self.opt.accum_finish(remainder)
        self._exchange()
        self.opt.step()
        self.pending = 0
        return self._with_grad_norm({})

    def graphed(self, keypoint, label):
        key = (tuple(keypoint.shape), tuple(label.shape))
        if self.accumulate > 1:
            return all(key + (kind,) in self._graphs for kind in ('micro', 'step'))
        return key in self._graphs
