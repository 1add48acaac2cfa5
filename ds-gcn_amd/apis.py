"""``train_model`` behind the reference's entry point (pyskl/apis/train.py:52-223) for the skeleton configs.

What the reference assembles out of mmcv parts — ``MMDistributedDataParallel`` (train.py:94-102), ``build_optimizers``,
``EpochBasedSparseRunner`` (core/local_runner/epoch_based_sparse_runner.py:26-105), ``OptimizerHook``,
``CosineAnnealingLrUpdaterHook(by_epoch=False)``, ``CheckpointHook(interval)``, ``DistSamplerSeedHook``, the text logger and
resume / load_from (train.py:153-157) — is one loop here over ``engine.TrainEngine`` (two hipGraph replays + one RCCL
all-reduce per iteration):

    for epoch:  order = DistributedSampler(seed + epoch)            # datasets/samplers/distributed_sampler.py:27-43
        for batch in order:  lr = cosine(iter / max_iters)           # before_train_iter
                             engine.step(batch, lr)                  # train_step + backward + all-reduce + SGD
                             log every `interval` (ONE packed all-reduce + ONE host read)
        checkpoint every `checkpoint_config.interval` epochs         # epoch_{n}.pth + latest.pth, mmcv layout

Batches come from the HIP input pipeline when the dataset is a (``SkeletonStore``, ``SkeletonBatcher``) pair — clips
resident in HBM, host decisions, one launch per batch — or from any map-style dataset whose items are
``dict(keypoint=(clips, M, T, V, C), label=int)`` (the output of the reference-style ``Compose`` pipelines).

``validate=True`` registers the counterpart of the reference's ``DistEvalHook`` (train.py:134-147 over mmcv's EvalHook):
every ``evaluation.interval`` epochs the val split goes through ``forward_test`` rank-sharded in dataset order, the parts
are gathered (``gather_results``), rank 0 computes ``evaluation.metrics`` (top-k / mean-class accuracy) and keeps
``best_<key>_epoch_<n>.pth`` (``save_best='auto'``: the first metric returned).  ``lr_config`` policies: mmcv's
``CosineAnnealing`` (the DS-GCN configs: by iteration), ``step`` (configs/stgcn/stgcn_vanilla_ntu60_xsub_3dkp/j.py:35: by
epoch), ``fixed``, ``Exp``, ``Poly``, ``Inv``, ``CosineRestart``, each by epoch or by iteration, and ``Cyclic`` / ``OneCycle`` by
iteration (the alternatives configs/_init_/lr_schedual.py names); each with mmcv's ``warmup`` ('constant' / 'linear' /
'exp', ``warmup_iters``, ``warmup_ratio``, ``warmup_by_epoch``).  ``momentum_config`` policies ``cyclic`` / ``OneCycle`` schedule
the momentum (SGD) or beta1 (Adam, AdamW): the value lives in device memory, so the update's hipGraph follows it.
``optimizer_config.grad_clip=dict(max_norm=..., norm_type=2 | inf)`` (configs/_init_/lr_schedual.py:24) clips the averaged
gradient by its total norm inside the update's hipGraph; ``grad_norm`` (before clipping) joins the log scalars.
``optimizer_config=dict(type='GradientCumulativeOptimizerHook', cumulative_iters=k)`` makes every iteration a
micro-iteration and every k-th one an update on the mean of the k gradients (``TrainEngine(accumulate=k)``): the schedule
and the log count micro-iterations as mmcv's ``runner.iter`` does, the last ``max_iters % k`` iterations form a short group
divided by their own count, and a group that an epoch end cuts short is closed there (checkpoints hold no accumulator).

``optimizer=dict(type='SGD' | 'Adam' | 'AdamW', ..., paramwise_cfg=...)`` is mmcv's ``build_optimizer`` (``train.build_optimizer``,
``paramwise.py``): per-tensor rates and weight decays, the schedule evaluated once per distinct initial rate.

``custom_hooks=[dict(type='EMAHook', momentum=0.0002, interval=1, warm_up=100)]`` is mmcv's ``EMAHook`` (``ema.py``): an
exponential moving average of the weights, one launch behind every iteration's update, swapped under the model from the
end of an epoch to the start of the next — validation and the epoch checkpoints see the averaged weights, the raw ones
ride along as ``ema_*`` buffers.  Other custom hooks are ignored (the logger names them).

Not reproduced: TensorBoard logging, multi-optimizer configs.
"""
import math
import os
import time
from collections import OrderedDict

import numpy as np
import torch
import torch.distributed as dist

from .checkpoint import find_resume, load_checkpoint, resume, save_checkpoint
from .engine import TrainEngine
from .evaluation import mean_class_accuracy, top_k_accuracy
from .recognizers import gather_results, reduce_log_vars
from .train import (ANNEAL, anneal_target, check_momentum, cosine_lr, cosine_restart_lr, cyclic_value, exp_lr, inv_lr,
                    onecycle_lr_values, onecycle_momentum_values, onecycle_value, poly_lr, step_lr, warmup_lr)


def _rank_world():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def _get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def epoch_indices(n, epoch, seed, rank, world, shuffle=True):
    """The reference's ``DistributedSampler.__iter__``: a permutation seeded with ``epoch + seed``, padded by wrapping to a
    multiple of the world size, every ``world``-th element from ``rank``."""
    if shuffle:
        g = torch.Generator()
        g.manual_seed(epoch + (seed if seed is not None else 0))
        idx = torch.randperm(n, generator=g).tolist()
    else:
        idx = list(range(n))
    total = int(math.ceil(n / world)) * world
    idx += idx[:total - len(idx)]
    return idx[rank:total:world]


class _BatchSource:
    """index list -> (keypoint (B, clips, M, T, V, C) float32, label (B, 1) int64) on the device.

    With the resident (``SkeletonStore``, ``SkeletonBatcher``) pair the host half of a batch (``plan``: RNG draws + index
    gathers) is made ONE BATCH AHEAD on a feeder thread while the device runs the current step: ``batch(idx, nxt)`` hands
    back the batch for ``idx`` and starts the plan for ``nxt``.  One worker, one plan at a time, in loop order: numpy's
    global RNG is consumed in exactly the order of the unthreaded loop."""

    def __init__(self, dataset, device, prefetch=True):
        self.device = device
        self.store = self.batcher = None
        self._pool = self._pending = self._pending_key = None
        if isinstance(dataset, (tuple, list)) and len(dataset) == 2 and hasattr(dataset[1], 'plan'):
            self.store, self.batcher = dataset
            self.n = len(self.store)
            if hasattr(self.batcher, 'prepare'):
                self.batcher.prepare(self.store)          # the per-clip decisions, once (first epoch at full rate)
            if prefetch:
                from concurrent.futures import ThreadPoolExecutor
                self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix='dsgcn-feeder')
        else:
            self.dataset = dataset
            self.n = len(dataset)

    def __len__(self):
        return self.n

    def _plan(self, indices):
        key = tuple(indices)
        if self._pending is not None:
            fut, pkey = self._pending, self._pending_key
            self._pending = self._pending_key = None
            plan = fut.result()                           # (also orders the RNG: the feeder has finished its draws)
            if pkey == key:
                return plan
            raise RuntimeError('_BatchSource: the batch asked for is not the one announced as next')
        return self.batcher.plan(self.store, indices)

    def batch(self, indices, next_indices=None):
        if self.store is not None:
            plan = self._plan(indices)
            if self._pool is not None and next_indices is not None and len(next_indices):
                nxt = list(next_indices)
                self._pending_key = tuple(nxt)
                self._pending = self._pool.submit(self.batcher.plan, self.store, nxt)
            return self.batcher.run(self.store, plan)
        items = [self.dataset[i] for i in indices]
        kp = torch.stack([torch.as_tensor(np.asarray(it['keypoint']), dtype=torch.float32) for it in items])
        lb = torch.as_tensor([int(np.asarray(it['label']).reshape(-1)[0]) for it in items], dtype=torch.int64).view(-1, 1)
        return kp.to(self.device, non_blocking=True), lb.to(self.device, non_blocking=True)


# ``lr_config`` / ``momentum_config``: mmcv's policies and the options each takes; anything else raises, naming it
_LR_COMMON = ('policy', 'by_epoch', 'warmup', 'warmup_iters', 'warmup_ratio', 'warmup_by_epoch')
_LR_OPTIONS = {
    'CosineAnnealing': ('min_lr', 'min_lr_ratio'),
    'Step': ('step', 'gamma', 'min_lr'),
    'Fixed': (),
    'Exp': ('gamma',),
    'Poly': ('power', 'min_lr'),
    'Inv': ('gamma', 'power'),
    'CosineRestart': ('periods', 'restart_weights', 'min_lr', 'min_lr_ratio'),
    'Cyclic': ('target_ratio', 'cyclic_times', 'step_ratio_up', 'anneal_strategy'),
    'OneCycle': ('max_lr', 'total_steps', 'pct_start', 'anneal_strategy', 'div_factor', 'final_div_factor', 'three_phase'),
}
_BY_ITER_ONLY = ('Cyclic', 'OneCycle')
_MOMENTUM_OPTIONS = {
    'Cyclic': ('target_ratio', 'cyclic_times', 'step_ratio_up'),
    'OneCycle': ('base_momentum', 'max_momentum', 'pct_start', 'anneal_strategy', 'three_phase'),
}


def _policy_name(name):
    """mmcv's hook lookup: a lower-case name is title-cased ('step' -> 'Step', 'cyclic' -> 'Cyclic'), any other is taken
    as written."""
    return name.title() if isinstance(name, str) and name == name.lower() else name


def _check_options(what, cfg, policy, table, common):
    if policy not in table:
        raise NotImplementedError(f'{what} policy {cfg.get("policy")!r}: {", ".join(sorted(table))} are implemented')
    extra = sorted(set(cfg) - set(common) - set(table[policy]))
    if extra:
        raise NotImplementedError(f'{what} policy {policy!r}: option(s) {extra} are not supported '
                                  f'({", ".join(table[policy]) or "none"})')


def _check_cycle(what, cfg, max_iters):
    """The arguments the Cyclic / OneCycle pairs share, checked where mmcv asserts them."""
    if cfg.get('anneal_strategy', 'cos') not in ANNEAL:
        raise ValueError(f'{what}: anneal_strategy must be one of "cos" or "linear", instead got {cfg["anneal_strategy"]!r}')
    if cfg.get('policy') == 'Cyclic':
        ratio = cfg.get('target_ratio')
        if ratio is not None and (not isinstance(ratio, (tuple, list)) or len(ratio) != 2):
            raise ValueError(f'{what}: target_ratio must be a pair, got {ratio!r}')
        times = cfg.get('cyclic_times', 1)
        if isinstance(times, bool) or not isinstance(times, int) or not 1 <= times <= max(max_iters, 1):
            raise ValueError(f'{what}: cyclic_times must be an integer in 1..max_iters ({max_iters}), got {times!r}')
        if not 0 <= cfg.get('step_ratio_up', 0.4) < 1.0:
            raise ValueError(f'{what}: step_ratio_up must be in range [0,1), got {cfg["step_ratio_up"]!r}')
    if 'pct_start' in cfg and not 0 <= cfg['pct_start'] <= 1:
        raise ValueError(f'{what}: expected float between 0 and 1 pct_start, but got {cfg["pct_start"]!r}')


class EpochRunner:
    """State of a run (``epoch``, ``iter``, ``max_iters``) + the loop; ``log`` collects one dict per logging interval."""

    def __init__(self, model, engine, source, cfg, work_dir=None, meta=None, logger=None):
        self.model, self.engine, self.source, self.cfg = model, engine, source, cfg
        self.work_dir, self.meta, self.logger = work_dir, dict(meta or {}), logger
        self.epoch = self.iter = 0
        self.rank, self.world = _rank_world()
        data = _get(cfg, 'data', {}) or {}
        loader = dict(data.get('train_dataloader', {}) or {})
        self.batch_size = int(loader.get('videos_per_gpu', data.get('videos_per_gpu', 1)))
        self.shuffle = bool(loader.get('shuffle', True))
        self.drop_last = bool(loader.get('drop_last', False))
        self.seed = _get(cfg, 'seed', None)
        self.max_epochs = int(_get(cfg, 'total_epochs', 1))
        lr_cfg = dict(_get(cfg, 'lr_config', None) or dict(policy='CosineAnnealing', min_lr=0, by_epoch=False))
        self.policy = _policy_name(lr_cfg.get('policy'))
        _check_options('lr_config', lr_cfg, self.policy, _LR_OPTIONS, _LR_COMMON)
        # mmcv's LrUpdaterHook counts epochs unless told otherwise; the Cyclic / OneCycle hooks count iterations only
        self.by_epoch = bool(lr_cfg.get('by_epoch', self.policy not in _BY_ITER_ONLY))
        if self.by_epoch and self.policy in _BY_ITER_ONLY:
            raise NotImplementedError(f'lr_config policy {self.policy!r}: by_epoch=True is not supported (mmcv: only '
                                      'by_epoch=False)')
        # mmcv LrUpdaterHook: warmup None | 'constant' | 'linear' | 'exp' over the first warmup_iters iterations
        # (warmup_by_epoch: warmup_iters counts epochs and is converted below, once iters_per_epoch is known)
        self.warmup = lr_cfg.get('warmup')
        if self.warmup is not None:
            if self.warmup not in ('constant', 'linear', 'exp'):
                raise ValueError(f'"{self.warmup}" is not a supported type for warming up, valid types are "constant", '
                                 '"linear" and "exp"')
            self.warmup_ratio = float(lr_cfg.get('warmup_ratio', 0.1))
            if int(lr_cfg.get('warmup_iters', 0)) <= 0 or not 0 < self.warmup_ratio <= 1.0:
                raise ValueError('lr warm-up needs warmup_iters > 0 and 0 < warmup_ratio <= 1')
        self.lr_cfg = lr_cfg
        self.log_interval = int((_get(cfg, 'log_config', None) or {}).get('interval', 20))
        ck = _get(cfg, 'checkpoint_config', None)          # None = no CheckpointHook (mmcv register_checkpoint_hook)
        self.ckpt_interval = 0 if ck is None else int(dict(ck).get('interval', 1))
        self.log = []
        self.evaluator = None                              # EvalLoop, set by train_model(validate=True)
        per_rank = int(math.ceil(len(source) / self.world))
        self.iters_per_epoch = per_rank // self.batch_size if self.drop_last else int(math.ceil(per_rank / self.batch_size))
        self.max_iters = self.max_epochs * self.iters_per_epoch
        if self.warmup is not None:
            self.warmup_iters = int(lr_cfg['warmup_iters']) * (self.iters_per_epoch if lr_cfg.get('warmup_by_epoch') else 1)
        self._check_lr_policy()
        mom_cfg = _get(cfg, 'momentum_config', None)
        self.momentum_cfg = None if mom_cfg is None else self._parse_momentum(dict(mom_cfg))

    def _check_lr_policy(self):
        """What mmcv's hooks assert in their constructors and ``before_run``, once ``max_iters`` is known."""
        c, policy = self.lr_cfg, self.policy
        if policy in ('CosineAnnealing', 'CosineRestart'):
            anneal_target(1.0, c.get('min_lr'), c.get('min_lr_ratio'))
        if policy == 'Step':
            step = c.get('step')
            if isinstance(step, bool) or not (isinstance(step, int) and step > 0 or isinstance(step, (list, tuple)) and step
                                              and all(isinstance(v, int) and v > 0 for v in step)):
                raise ValueError(f'lr_config step must be a positive int or a list of them, got {step!r}')
        if policy in ('Exp', 'Inv') and 'gamma' not in c:
            raise ValueError(f'lr_config policy {policy!r} needs gamma')
        if policy == 'CosineRestart':
            periods = c.get('periods')
            weights = c.get('restart_weights', [1])
            if not periods or len(periods) != len(weights):
                raise ValueError('lr_config CosineRestart: periods and restart_weights should have the same length, got '
                                 f'{periods!r} and {weights!r}')
            top = self.max_epochs if self.by_epoch else self.max_iters
            if sum(periods) < top:
                raise ValueError(f'lr_config CosineRestart: the periods cover {sum(periods)} of the run\'s {top} '
                                 f'{"epochs" if self.by_epoch else "iterations"}')
        if policy in _BY_ITER_ONLY:
            _check_cycle(f'lr_config {policy}', dict(c, policy=policy), self.max_iters)
        if policy == 'OneCycle':
            max_lr = c.get('max_lr')
            if isinstance(max_lr, (list, tuple)):
                if len(max_lr) != 1:
                    raise NotImplementedError(f'lr_config OneCycle: max_lr with one rate per group ({len(max_lr)} entries) is '
                                              'not supported: a scalar or a one-element list')
                max_lr = max_lr[0]
            if not isinstance(max_lr, (int, float)) or isinstance(max_lr, bool):
                raise ValueError(f'lr_config OneCycle: the type of max_lr must be the one of list or float, got {max_lr!r}')
            steps = c.get('total_steps')
            if steps is not None:
                if isinstance(steps, bool) or not isinstance(steps, int):
                    raise ValueError(f'lr_config OneCycle: total_steps must be an integer, got {steps!r}')
                if steps < self.max_iters:
                    raise ValueError(f'lr_config OneCycle: the total steps must be greater than or equal to max iterations '
                                     f'{self.max_iters} of runner, but total steps is {steps}')
            self.total_steps = self.max_iters if steps is None else steps
            # EVERY group starts from max_lr / div_factor: mmcv overwrites the groups' initial_lr, lr_mult included
            self.onecycle_base = max_lr / c.get('div_factor', 25)

    def _parse_momentum(self, c):
        """``momentum_config``: mmcv's CyclicMomentumUpdaterHook ('cyclic') and OneCycleMomentumUpdaterHook ('OneCycle').  The
        base is the optimizer's momentum (SGD) / betas[0] (Adam, AdamW) of the config; every value the schedule can take
        must lie in [0, 1) — its extremes are evaluated here."""
        policy = _policy_name(c.get('policy'))
        _check_options('momentum_config', c, policy, _MOMENTUM_OPTIONS, ('policy', 'by_epoch'))
        if c.get('by_epoch', False):
            raise NotImplementedError(f'momentum_config policy {policy!r}: by_epoch=True is not supported')
        opt = self.engine.opt
        if not getattr(opt, 'scheduled_momentum', False):
            raise ValueError('momentum_config needs an optimizer built with scheduled_momentum=True (train_model and '
                             'build_optimizer(..., scheduled_momentum=True) do that)')
        base = opt.initial_momentum
        if base == 0 and not hasattr(opt, 'betas'):
            raise ValueError('momentum_config on SGD with momentum=0: there is no momentum to schedule')
        c['policy'] = policy
        _check_cycle(f'momentum_config {policy}', c, self.max_iters)
        if policy == 'Cyclic':
            ratio = c.setdefault('target_ratio', (0.85 / 0.95, 1))
            extremes = [base, base * ratio[0], base * ratio[1]]
        else:
            extremes = [c.setdefault('base_momentum', 0.85), c.setdefault('max_momentum', 0.95)]
        for v in extremes:
            check_momentum(v, f'momentum_config {policy}: scheduled momentum')
        c['base'] = base
        return c

    def current_momentum(self):
        """The momentum / beta1 of iteration ``self.iter`` under ``momentum_config`` (None without one): a pure function of
        the iteration, so a resumed run continues the schedule with no state of its own."""
        c = self.momentum_cfg
        if c is None:
            return None
        if c['policy'] == 'Cyclic':
            return cyclic_value(c['base'], self.iter, self.max_iters, c['target_ratio'], c.get('cyclic_times', 1),
                                c.get('step_ratio_up', 0.4), 'cos')
        three = bool(c.get('three_phase', False))
        return onecycle_value(onecycle_momentum_values(c['base_momentum'], c['max_momentum'], three), self.iter,
                              self.max_iters, c.get('pct_start', 0.3), c.get('anneal_strategy', 'cos'), three)

    def current_lr(self, base=None):
        """The rate of iteration ``self.iter`` for a group whose initial rate is ``base`` (default: the optimizer's
        ``base_lr``, group 0's — the one mmcv logs): the policy's regular rate, scaled by the warm-up rule during the first
        ``warmup_iters`` iterations (counted from the start of the run: a resumed run continues where it stopped)."""
        lr = self.regular_lr(base)
        if self.warmup is not None and self.iter < self.warmup_iters:
            lr = warmup_lr(lr, self.iter, self.warmup, self.warmup_iters, self.warmup_ratio)
        return lr

    def current_lrs(self):
        """None for an optimizer with one rate; else one rate per group of the optimizer: mmcv's LrUpdaterHook applies
        ``get_lr(initial_lr)`` and then the warm-up to every param group, which with ``min_lr != 0`` (cosine, or the step
        policy's floor) is not proportional to the groups' ``lr_mult`` — so the schedule is evaluated per initial rate."""
        opt = self.engine.opt
        bases = opt.group_base_lrs if hasattr(type(opt), 'group_base_lrs') else None     # (absent on a stand-in optimizer)
        if bases is None:
            return None
        by_base = {b: self.current_lr(b) for b in set(bases)}
        return [by_base[b] for b in bases]

    def regular_lr(self, base=None):
        c, policy = self.lr_cfg, self.policy
        if policy == 'OneCycle':                          # one base for every group, whatever its initial rate
            three = bool(c.get('three_phase', False))
            values = onecycle_lr_values(self.onecycle_base, c.get('div_factor', 25), c.get('final_div_factor', 1e4), three)
            return onecycle_value(values, self.iter, self.total_steps, c.get('pct_start', 0.3),
                                  c.get('anneal_strategy', 'cos'), three)
        if base is None:
            base = self.engine.opt.base_lr
        # mmcv's LrUpdaterHook: by_epoch policies are set before each epoch from runner.epoch, the others from runner.iter
        progress, top = (self.epoch, self.max_epochs) if self.by_epoch else (self.iter, self.max_iters)
        if policy == 'CosineAnnealing':
            return cosine_lr(base, progress, top, anneal_target(base, c.get('min_lr'), c.get('min_lr_ratio')))
        if policy == 'Step':
            return step_lr(base, progress, c['step'], float(c.get('gamma', 0.1)), c.get('min_lr', None))
        if policy == 'Exp':
            return exp_lr(base, progress, c['gamma'])
        if policy == 'Poly':
            return poly_lr(base, progress, top, c.get('power', 1.), c.get('min_lr', 0.))
        if policy == 'Inv':
            return inv_lr(base, progress, c['gamma'], c.get('power', 1.))
        if policy == 'CosineRestart':
            return cosine_restart_lr(base, progress, c['periods'], c.get('restart_weights', [1]), c.get('min_lr'),
                                     c.get('min_lr_ratio'))
        if policy == 'Cyclic':
            return cyclic_value(base, self.iter, self.max_iters, c.get('target_ratio', (10, 1e-4)), c.get('cyclic_times', 1),
                                c.get('step_ratio_up', 0.4), c.get('anneal_strategy', 'cos'))
        return base

    def train_epoch(self):
        self.model.train()
        ema = getattr(self.engine, 'ema', None)
        if ema is not None and ema.swapped:
            # EMAHook.before_train_epoch: the raw weights go back under the model (after an epoch end of this run, or after
            # a resume from an epoch checkpoint, whose parameter entries are the averaged ones).  At the start of a fresh
            # run mmcv swaps too: two equal copies, nothing to exchange here.
            ema.swap()
        order = epoch_indices(len(self.source), self.epoch, self.seed, self.rank, self.world, self.shuffle)
        pending, t0 = [], time.perf_counter()
        for b in range(self.iters_per_epoch):
            idx = order[b * self.batch_size:(b + 1) * self.batch_size]
            nxt = order[(b + 1) * self.batch_size:(b + 2) * self.batch_size] if b + 1 < self.iters_per_epoch else None
            kp, lb = self.source.batch(idx, nxt)
            lr = self.current_lr()                                    # before_train_iter
            lrs = self.current_lrs()                                  # (one rate per group under paramwise_cfg / Adam)
            mom = self.current_momentum()                             # (None without a momentum_config)
            kw = {}                                                   # (a stand-in engine takes the three positionals only)
            if mom is not None:
                kw['momentum'] = mom
            if ema is not None:
                kw['ema_iter'] = self.iter                            # (the run's count: engine.iter restarts on a resume)
            # run_iter + after_train_iter (OptimizerHook; EMAHook)
            logs = self.engine.step(kp, lb, lr if lrs is None else lrs, **kw)
            # a replayed hipGraph hands back the SAME static tensors every iteration: keep this iteration's values
            pending.append(({k: v.clone() for k, v in logs.items()}, len(idx)))
            self.iter += 1
            if (b + 1) % self.log_interval == 0 or b + 1 == self.iters_per_epoch:
                self._flush_log(pending, lr, b + 1, time.perf_counter() - t0, mom)
                pending, t0 = [], time.perf_counter()
        if getattr(self.engine, 'pending', 0):
            # a group never straddles an epoch end: what a checkpoint or a validation pass sees there is a model whose
            # every gradient has been applied, and a resumed run starts with an empty accumulator as this one continues
            short = self.engine.pending
            self.engine.flush(short)
            if self.logger is not None and self.rank == 0:
                self.logger.info('Epoch [%d] ends inside a group of %d accumulated iterations: updated on the mean of the '
                                 'first %d', self.epoch + 1, self.engine.accumulate, short)
        if ema is not None:
            # EMAHook.after_train_epoch at priority 49, ahead of the checkpoint and the evaluation: both see the averaged
            # weights under the parameter names and the raw ones under ema_*
            ema.swap()
        self.epoch += 1
        if self.work_dir and self.ckpt_interval and self.epoch % self.ckpt_interval == 0 and self.rank == 0:
            self.save_checkpoint()
        if self.evaluator is not None:                                # after_train_epoch of the EvalHook
            self.evaluator.after_train_epoch(self)

    def _flush_log(self, pending, lr, inner, dt, momentum=None):
        """The interval's log scalars: sample-weighted means over its iterations, averaged over ranks with ONE collective
        and read back with ONE copy (the reference pays four all-reduces and four ``.item()`` syncs per ITERATION,
        recognizers/base.py:150-156)."""
        if not pending:
            return
        keys = list(pending[0][0])
        w = torch.tensor([n for _, n in pending], dtype=torch.float64, device=pending[0][0][keys[0]].device)
        means = OrderedDict((k, (torch.stack([lv[k].double() for lv, _ in pending]) * w).sum() / w.sum()) for k in keys)
        vals = reduce_log_vars(means)
        rec = dict(epoch=self.epoch + 1, iter=inner, lr=lr, time=dt / max(len(pending), 1), **vals)
        if momentum is not None:                          # (mmcv's text logger prints it once a momentum hook runs)
            rec['momentum'] = momentum
        self.log.append(rec)
        if self.logger is not None and self.rank == 0:
            rate = '%.3e' % lr if momentum is None else '%.3e, momentum: %.4f' % (lr, momentum)
            self.logger.info('Epoch [%d][%d/%d]\tlr: %s, time: %.3f, %s', rec['epoch'], inner, self.iters_per_epoch, rate,
                             rec['time'], ', '.join(f'{k}: {v:.4f}' for k, v in vals.items()))

    def save_checkpoint(self):
        os.makedirs(self.work_dir, exist_ok=True)
        meta = dict(self.meta, epoch=self.epoch, iter=self.iter)
        ema = getattr(self.engine, 'ema', None)
        if ema is not None:
            meta['ema_swapped'] = bool(ema.swapped)        # which of the two sets lies under the parameter names (resume reads it)
        path = os.path.join(self.work_dir, f'epoch_{self.epoch}.pth')
        return save_checkpoint(self.model, path, optimizer=self.engine.opt, meta=meta, create_symlink=True)

    def resume(self, path):
        meta = resume(self.model, self.engine.opt, path)
        self.epoch, self.iter = int(meta.get('epoch', 0)), int(meta.get('iter', 0))
        ema = getattr(self.engine, 'ema', None)
        if ema is not None:
            # both sets were restored in place by the strict load above.  Which one lies under the parameter names is in the
            # file's meta (``save_checkpoint``); a file without the key is taken for an epoch-end checkpoint of a run with
            # the EMAHook, mmcv's included: parameter entries = averaged weights, ema_* = raw weights.  When the model
            # holds the average, the swap at the start of the next epoch puts the raw weights back under training.
            ema.swapped = bool(meta.get('ema_swapped', True))
            self.engine.ema_iter = self.iter
        if meta.get('hook_msgs'):
            self.meta['hook_msgs'] = dict(meta['hook_msgs'])
        if self.evaluator is not None:
            self.evaluator.restore(self.meta)
        return meta

    def run(self):
        while self.epoch < self.max_epochs:
            self.train_epoch()
        return self


def evaluate_scores(scores, labels, metrics=('top_k_accuracy', 'mean_class_accuracy'), metric_options=None):
    """``BaseDataset.evaluate`` (datasets/base.py:111-199) on (n, classes) scores: ``top_k_accuracy`` -> ``top{k}_acc``,
    ``mean_class_accuracy``, ``confusion_matrix``."""
    metric_options = metric_options or dict(top_k_accuracy=dict(topk=(1, 5)))
    out = OrderedDict()
    for metric in metrics:
        if metric == 'top_k_accuracy':
            topk = metric_options.get('top_k_accuracy', {}).get('topk', (1, 5))
            topk = (topk,) if isinstance(topk, int) else tuple(topk)
            for k, acc in zip(topk, top_k_accuracy(scores, labels, topk)):
                out[f'top{k}_acc'] = float(acc)
        elif metric == 'mean_class_accuracy':
            out['mean_class_accuracy'] = float(mean_class_accuracy(scores, labels)[0])
        elif metric == 'confusion_matrix':
            out['confusion_matrix'] = mean_class_accuracy(scores, labels)[1]
        else:
            raise KeyError(f'metric {metric} is not supported')
    return out


class EvalLoop:
    """The reference's ``DistEvalHook`` (pyskl/core/evaluation.py:11-19 over mmcv ``EvalHook`` / ``DistEvalHook``) for the
    epoch-based runner: after every ``interval``-th epoch (from ``start`` on) the val split is scored with ``forward_test``
    — rank r takes samples r, r + world, ... in dataset order (``DistributedSampler(shuffle=False)``), ``videos_per_gpu``
    of the val dataloader per call — the parts are interleaved back (``gather_results``), and rank 0 evaluates
    ``metrics`` the way ``BaseDataset.evaluate`` does (datasets/base.py:111-199: ``top_k_accuracy`` -> ``top{k}_acc``,
    ``mean_class_accuracy``).  ``save_best='auto'`` takes the first key returned; the rule (greater / less) follows the
    key name as in mmcv (``acc`` / ``top`` greater, ``loss`` less); the best checkpoint is ``best_<key>_epoch_<n>.pth`` and
    the previous best file is removed.  ``results`` holds one record per evaluation."""
    greater_keys = ('acc', 'top', 'AR@', 'auc', 'precision', 'mAP@', 'Recall@')
    less_keys = ('loss',)

    def __init__(self, dataset, batch_size=1, interval=1, start=None, metrics='top_k_accuracy',
                 metric_options=None, save_best='auto', rule=None, by_epoch=True, device='cuda',
                 broadcast_bn_buffer=True, engine=None, **unsupported):
        """engine: an ``infer.InferEngine`` over the model that ``predict`` is given — the scores then come from its
        hipGraph replay and stay on the device until the end of the pass (one read-back); ``None``: ``forward_test``."""
        if not by_epoch:
            raise NotImplementedError('evaluation by iteration is not used by the skeleton configs')
        unsupported.pop('key_indicator', None)
        unsupported.pop('gpu_collect', None)
        unsupported.pop('tmpdir', None)
        if unsupported:
            raise NotImplementedError(f'evaluation options {sorted(unsupported)} are not supported')
        self.source = _BatchSource(dataset, device)
        self.batch_size, self.interval, self.start = int(batch_size), int(interval), start
        self.metrics = list(metrics) if isinstance(metrics, (list, tuple)) else [metrics]
        for m in self.metrics:
            if m not in ('top_k_accuracy', 'mean_class_accuracy', 'confusion_matrix'):
                raise KeyError(f'metric {m} is not supported')
        self.metric_options = dict(metric_options or dict(top_k_accuracy=dict(topk=(1, 5))))
        self.save_best, self.rule = save_best, rule
        self.key_indicator = None if save_best in ('auto', None, True) else save_best
        self.best_score = self.best_ckpt = None
        self.broadcast_bn_buffer = bool(broadcast_bn_buffer)
        self.engine = engine
        self.matmul_precision = None      # a level for the eager passes of predict() (train_model sets the run's)
        self.results = []

    def restore(self, meta):
        """After a resume: the best score / file so far ride in the checkpoint's ``meta['hook_msgs']`` (mmcv EvalHook reads
        them back in ``before_run`` / ``_save_ckpt``), so the first evaluation of the resumed run competes with them."""
        msgs = (meta or {}).get('hook_msgs') or {}
        if msgs.get('best_score') is not None:
            self.best_score, self.best_ckpt = msgs['best_score'], msgs.get('best_ckpt')
            self.key_indicator = msgs.get('key_indicator', self.key_indicator)

    @torch.no_grad()
    def sync_bn_buffers(self, model, world):
        """mmcv ``DistEvalHook._do_evaluate`` with ``broadcast_bn_buffer=True`` (its default): BatchNorm running statistics
        evolve rank-locally during training (no per-step buffer sync, pyskl/apis/train.py:98-102), so before a validation
        pass every rank takes rank 0's — the scores then describe the weights AND buffers rank 0 saves.  One packed
        collective for all layers."""
        if world <= 1 or not self.broadcast_bn_buffer:
            return
        bufs = []
        for m in model.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.track_running_stats:
                bufs += [m.running_var, m.running_mean]
        if not bufs:
            return
        packed = torch.cat([b.detach().reshape(-1).float() for b in bufs])
        dist.broadcast(packed, src=0)
        off = 0
        for b in bufs:
            b.copy_(packed[off:off + b.numel()].view_as(b).to(b.dtype))
            off += b.numel()

    def labels(self):
        if self.source.store is not None:
            return [int(v) for v in self.source.store.labels]
        ds = self.source.dataset
        if hasattr(ds, 'video_infos'):
            return [int(np.asarray(a['label']).reshape(-1)[0]) for a in ds.video_infos]
        return [int(np.asarray(ds[i]['label']).reshape(-1)[0]) for i in range(len(ds))]

    @torch.no_grad()
    def predict(self, model, rank, world):
        """This rank's share of the val scores, in its sampler order.  Under ``test_cfg['feat_ext']`` / ``['score_ext']``:
        one float16 array per video, what ``forward_test`` returns for that video alone (mmcv's ``results.extend(result)``
        would split that array on its first axis; not reproduced).  Under ``test_cfg['graph_ext']``: one float32
        ``(L, K, V, V)`` array per video."""
        if self.engine is not None and self.engine.model is not model:
            raise ValueError('EvalLoop(engine=...): the engine was built over another model')
        if self.matmul_precision is not None and self.engine is None:
            from . import kernels
            with kernels.matmul_precision(self.matmul_precision):
                return self._predict(model, rank, world)
        return self._predict(model, rank, world)

    def _predict(self, model, rank, world):
        n = len(self.source)
        order = epoch_indices(n, 0, 0, rank, world, shuffle=False)
        was_training = model.training
        model.eval()
        part, on_device = [], []
        ext = model.extraction() if hasattr(model, 'extraction') else None
        graphs = hasattr(model, 'graph_extraction') and model.graph_extraction() is not None
        # the reference samples val clips in loader worker processes: the test-mode sampler's np.random.seed(255) never
        # touches the TRAINING process's stream.  Here both run in one process, so the stream is put back afterwards.
        rng = np.random.get_state()
        try:
            for b in range(0, len(order), self.batch_size):
                kp, _ = self.source.batch(order[b:b + self.batch_size])
                if self.engine is not None:
                    on_device.append(self.engine(kp))
                elif ext is not None or graphs:                   # forward_test extracts from one video per call
                    part.extend(model(keypoint=kp[i:i + 1], return_loss=False) for i in range(len(kp)))
                else:
                    part.extend(model(keypoint=kp, return_loss=False))
        finally:
            np.random.set_state(rng)
        if on_device:
            rows = torch.cat(on_device).cpu().numpy()             # the pass's one device->host copy
            part.extend((r[None] for r in rows) if ext is not None and ext[0] == 'score' else rows)
        model.train(was_training)
        return part

    def evaluate(self, scores, labels):
        return evaluate_scores(scores, labels, self.metrics, self.metric_options)

    def _better(self, key, value):
        if self.best_score is None:
            return True
        rule = self.rule
        if rule is None:
            low = key.lower()
            if any(k.lower() in low for k in self.greater_keys):
                rule = 'greater'
            elif any(k.lower() in low for k in self.less_keys):
                rule = 'less'
            else:
                raise ValueError(f'Cannot infer the rule for key {key}, thus a specific rule must be specified.')
        return value > self.best_score if rule == 'greater' else value < self.best_score

    def should_run(self, epoch):
        """``epoch`` = completed epochs (mmcv ``_should_evaluate``: every ``interval`` epochs, from ``start`` on)."""
        if self.start is None:
            return epoch % self.interval == 0
        return epoch >= self.start and (epoch - self.start) % self.interval == 0

    def after_train_epoch(self, runner):
        if not self.should_run(runner.epoch):
            return None
        if hasattr(runner.model, 'extraction') and runner.model.extraction() is not None:
            raise ValueError("validation scores classes: test_cfg['feat_ext'] / ['score_ext'] belong to test_model")
        if hasattr(runner.model, 'graph_extraction') and runner.model.graph_extraction() is not None:
            raise ValueError("validation scores classes: test_cfg['graph_ext'] belongs to test_model")
        self.sync_bn_buffers(runner.model, runner.world)
        part = self.predict(runner.model, runner.rank, runner.world)
        scores = gather_results(part, len(self.source))
        rec = None
        if runner.rank == 0:
            vals = self.evaluate(np.stack(scores), self.labels())
            rec = dict(epoch=runner.epoch, **vals)
            self.results.append(rec)
            if runner.logger is not None:
                runner.logger.info('Epoch(val) [%d]\t%s', runner.epoch,
                                   ', '.join(f'{k}: {v:.4f}' for k, v in vals.items() if np.ndim(v) == 0))
            if self.save_best and vals and runner.work_dir:
                key = self.key_indicator or next(iter(vals))
                self.key_indicator = key
                if self._better(key, vals[key]):
                    self.best_score = vals[key]
                    if self.best_ckpt and os.path.isfile(self.best_ckpt):
                        os.remove(self.best_ckpt)
                    os.makedirs(runner.work_dir, exist_ok=True)
                    self.best_ckpt = os.path.join(runner.work_dir, f'best_{key}_epoch_{runner.epoch}.pth')
                    # kept in the runner's meta as mmcv does: every later epoch_N.pth carries it, a resume reads it back
                    runner.meta['hook_msgs'] = dict(best_score=self.best_score, best_ckpt=self.best_ckpt, key_indicator=key)
                    meta = dict(runner.meta, epoch=runner.epoch, iter=runner.iter)
                    save_checkpoint(runner.model, self.best_ckpt, optimizer=runner.engine.opt, meta=meta)
        if runner.world > 1:
            dist.barrier()
        return rec


def parse_optimizer_config(opt_hook):
    """mmcv's ``optimizer_config`` -> (grad_clip, accumulate).  Without ``type`` (or ``OptimizerHook``): an update per
    iteration.  ``GradientCumulativeOptimizerHook``: an update per ``cumulative_iters`` iterations (mmcv's default 1)."""
    opt_hook = dict(opt_hook or {})
    kind = opt_hook.get('type', 'OptimizerHook')
    if kind == 'OptimizerHook':
        return opt_hook.get('grad_clip'), 1
    if kind == 'GradientCumulativeOptimizerHook':
        k = opt_hook.get('cumulative_iters', 1)
        if isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise ValueError(f'cumulative_iters only accepts positive int, but got {k!r} instead.')
        return opt_hook.get('grad_clip'), k
    raise NotImplementedError(f'optimizer_config type {kind!r}: OptimizerHook and GradientCumulativeOptimizerHook are '
                              'implemented')


def parse_custom_hooks(hooks, logger=None):
    """mmcv's ``custom_hooks`` -> (the ``EMAHook`` entry as written — a dict with ``type`` / ``momentum`` / ``interval`` /
    ``warm_up`` / ``resume_from`` / ``priority`` —, its options as ``ema.parse_ema`` validates them: what
    ``TrainEngine(ema=...)`` takes), or (None, None).  More than one EMAHook: ValueError.  Hooks of any other type are not
    implemented and stay ignored; the logger names them once."""
    from .ema import parse_ema
    found, other = [], []
    for hook in hooks or []:
        kind = _get(hook, 'type', None)
        if kind == 'EMAHook':
            found.append(dict(hook))
        else:
            other.append(str(kind))
    if len(found) > 1:
        raise ValueError(f'custom_hooks: {len(found)} entries of type EMAHook; one set of averaged weights is kept')
    if other and logger is not None:
        logger.warning('custom_hooks: %s not implemented, ignored', ', '.join(other))
    if not found:
        return None, None
    return found[0], parse_ema(found[0], 'custom_hooks EMAHook')


def train_model(model, dataset, cfg, distributed=None, validate=False, test=None, timestamp=None, meta=None,
                device='cuda', logger=None, use_graph=True, val_dataset=None, prefetch=True):
    """Train ``model`` on ``dataset`` the way the reference's ``train_model`` does for the skeleton configs; returns the
    ``EpochRunner`` (its ``.log`` holds the interval records, ``.engine`` the optimizer state).

    cfg (``Config`` or dict) keys read: ``data.videos_per_gpu`` / ``data.train_dataloader``, ``optimizer``,
    ``optimizer_config`` (``grad_clip``; ``type`` + ``cumulative_iters``), ``lr_config`` (policy + warm-up),
    ``momentum_config`` ('cyclic' | 'OneCycle': the optimizer then keeps its momentum / beta1 on the device),
    ``custom_hooks`` (the ``EMAHook`` entry: ``parse_custom_hooks``; its ``resume_from`` stands in for an unset ``resume_from``),
    ``total_epochs``, ``checkpoint_config``, ``log_config.interval``, ``work_dir``, ``seed``, ``resume_from`` / ``load_from`` /
    ``auto_resume``, ``matmul_precision`` ('highest' | 'high': the run's training steps and validation passes; absent = the
    process level, ``kernels.set_matmul_precision``); with ``validate=True`` also ``evaluation`` and ``data.val`` / ``data.val_dataloader`` (``val_dataset``
    overrides ``data.val``: a map-style dataset or a (``SkeletonStore``, ``SkeletonBatcher``) pair built for the val
    pipeline).  ``runner.evaluator.results`` holds the evaluation records.  ``prefetch``: plan the next batch of a resident
    store on a feeder thread while the device runs the current step (same RNG stream either way)."""
    if isinstance(dataset, list) and len(dataset) == 1:
        dataset = dataset[0]
    opt_cfg = dict(_get(cfg, 'optimizer', None) or dict(type='SGD', lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True))
    grad_clip, accumulate = parse_optimizer_config(_get(cfg, 'optimizer_config', None))
    ema_hook, ema_cfg = parse_custom_hooks(_get(cfg, 'custom_hooks', None), logger)
    model = model.to(device)
    world = _rank_world()[1]
    # mmcv's build_optimizer(model, cfg.optimizer): SGD | Adam | AdamW with torch's defaults for absent keys, and
    # paramwise_cfg (train.build_optimizer raises for what is not implemented, naming the key)
    engine = TrainEngine(model, optimizer=opt_cfg, use_graph=use_graph, strict_graph=world > 1, grad_clip=grad_clip,
                         accumulate=accumulate, matmul_precision=_get(cfg, 'matmul_precision', None),
                         scheduled_momentum=_get(cfg, 'momentum_config', None) is not None, ema=ema_cfg)
    if logger is not None:
        logger.info('matmul precision: %s', engine.matmul_precision)
        if ema_cfg is not None:
            logger.info('EMA: momentum %g, interval %d, warm_up %g', ema_cfg['momentum'] ** ema_cfg['interval'],
                        ema_cfg['interval'], ema_cfg['warm_up'])
    source = _BatchSource(dataset, next(model.parameters()).device, prefetch=prefetch)
    work_dir = _get(cfg, 'work_dir', None)
    runner = EpochRunner(model, engine, source, cfg, work_dir=work_dir, meta=meta, logger=logger)
    if validate:
        data = _get(cfg, 'data', {}) or {}
        if val_dataset is None:
            from .pipeline import build_dataset
            val_cfg = dict(data['val'])
            val_cfg.setdefault('test_mode', True)
            val_dataset = build_dataset(val_cfg)
        vloader = dict(videos_per_gpu=data.get('videos_per_gpu', 1))
        vloader.update(data.get('val_dataloader', {}) or {})
        eval_cfg = dict(_get(cfg, 'evaluation', None) or {})
        runner.evaluator = EvalLoop(val_dataset, batch_size=vloader['videos_per_gpu'],
                                    device=next(model.parameters()).device, **eval_cfg)
        runner.evaluator.matmul_precision = engine.matmul_precision
    resume_from = _get(cfg, 'resume_from', None)
    if resume_from is None and ema_hook is not None:
        resume_from = ema_hook.get('resume_from')          # the hook's own resume_from acts as the run's when that is unset
    ckpt = find_resume(work_dir, resume_from, bool(_get(cfg, 'auto_resume', False))) if work_dir else resume_from
    if ckpt:
        runner.resume(ckpt)
    elif _get(cfg, 'load_from', None):
        load_checkpoint(model, _get(cfg, 'load_from'), strict=False)
        if engine.ema is not None:
            # mmcv registers the buffers in before_run, after load_from: the average starts from the loaded weights
            engine.ema.reset()
    runner.run()
    if world > 1:
        dist.barrier()
    return runner
