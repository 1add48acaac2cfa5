"""Exponential moving average of the weights: mmcv 1.5's ``EMAHook`` over the flat parameter buffer.

mmcv keeps one buffer per parameter (``'ema_' + name.replace('.', '_')``, registered on the model so that checkpoints carry
them), updates every one of them after every ``interval``-th training iteration

    M   = momentum ** interval
    m   = min(M, (1 + s) / (warm_up + s))          s = runner.iter of the iteration that just ran (0 for the first)
    ema = (1 - m) * ema + m * param

and swaps parameters and buffers at the epoch boundaries, so that validation and the epoch checkpoints see the averaged
weights.  Here the buffers are views of ONE flat buffer laid out like ``FlatParams.flat_p``, the update is one launch over
it (csrc/ema.hip) whose ``m`` lives in device memory — a launch captured in a hipGraph follows the warm-up and the
``interval`` gating (``m = 0``: the buffer is left bit-unchanged) without re-capture — and the swap is one launch that
exchanges the two flat buffers in place: every address a captured graph holds stays valid."""
import torch

from . import kernels, native

EMA_KEYS = ('momentum', 'interval', 'warm_up')
HOOK_KEYS = ('type',) + EMA_KEYS + ('resume_from', 'priority')
DEFAULTS = dict(momentum=0.0002, interval=1, warm_up=100)


def buffer_name(param_name):
    """mmcv's name of the averaged copy of ``param_name``."""
    return 'ema_' + param_name.replace('.', '_')


def parse_ema(cfg, what='ema'):
    """``dict(momentum=, interval=, warm_up=)`` with mmcv's defaults for absent keys (an ``EMAHook`` entry of
    ``custom_hooks`` may also carry ``type``, ``resume_from`` and ``priority``, which are not read here).  ValueError,
    naming the key: an unknown key, ``momentum`` outside (0, 1), ``interval`` not a positive int, ``warm_up`` negative or not
    a number."""
    cfg = dict(cfg)
    for key in cfg:
        if key not in HOOK_KEYS:
            raise ValueError(f'{what}: unknown key {key!r} ({", ".join(HOOK_KEYS)})')
    out = {k: cfg.get(k, DEFAULTS[k]) for k in EMA_KEYS}
    mom, interval, warm_up = out['momentum'], out['interval'], out['warm_up']
    if isinstance(mom, bool) or not isinstance(mom, (int, float)) or not 0.0 < mom < 1.0:
        raise ValueError(f'{what}: momentum must lie in (0, 1), got {mom!r}')
    if isinstance(interval, bool) or not isinstance(interval, int) or interval < 1:
        raise ValueError(f'{what}: interval must be a positive int, got {interval!r}')
    if isinstance(warm_up, bool) or not isinstance(warm_up, (int, float)) or not warm_up >= 0:
        raise ValueError(f'{what}: warm_up must be a number >= 0, got {warm_up!r}')
    out['momentum'] = float(mom)
    return out


def ema_momentum(s, momentum=0.0002, interval=1, warm_up=100):
    """The ``m`` of the update after iteration ``s`` (``runner.iter`` before its increment): 0.0 off the interval, else
    ``min(momentum ** interval, (1 + s) / (warm_up + s))`` (``warm_up = 0`` at ``s = 0``: no warm-up term)."""
    if s % interval != 0:
        return 0.0
    full = momentum ** interval
    if warm_up + s <= 0:
        return full
    return min(full, (1 + s) / (warm_up + s))


class FlatEMA:
    """The averaged copy of a ``FlatParams``: ``flat_e`` (the layout of ``flat.flat_p``), per-parameter views of it
    registered on the model as buffers under mmcv's names — ``state_dict()`` / ``load_state_dict()`` carry them, the latter
    in place — and ``hyper_t``, the fp64 device scalar the update launch reads ``m`` from.  A parameter outside the flat
    buffer (``requires_grad=False``: never updated) gets a plain clone, which no update and no swap needs to touch.

    ``update(s)`` = ``set_iter(s)`` (the host's fill of ``hyper_t``) + ``launch()`` (what a hipGraph may capture);
    ``swap()`` exchanges ``flat_p`` and ``flat_e`` in place and flips ``swapped`` (True: the model holds the averaged
    weights).  On CPU tensors both run as torch ops; on the GPU they are the HIP launches, fp32 only."""

    def __init__(self, flat, momentum=0.0002, interval=1, warm_up=100):
        cfg = parse_ema(dict(momentum=momentum, interval=interval, warm_up=warm_up))
        self.momentum, self.interval, self.warm_up = cfg['momentum'], cfg['interval'], cfg['warm_up']
        self.flat = flat
        p = flat.flat_p
        self.native = p.is_cuda
        if self.native and p.dtype != torch.float32:
            raise NotImplementedError(f'FlatEMA: the update kernel takes fp32 parameters, got {p.dtype}')
        module = flat.module
        names = [(name, buffer_name(name)) for name, _ in module.named_parameters()]
        taken = set(dict(module.named_buffers(recurse=False))) | set(dict(module.named_parameters(recurse=False)))
        for name, bname in names:
            if bname in taken or hasattr(module, bname):
                raise ValueError(f'FlatEMA: the model already has {bname!r} (an EMA is attached to it, or two parameter '
                                 'names map to one buffer name)')
            taken.add(bname)
        self.flat_e = p.detach().clone()
        self.hyper_t = torch.zeros(1, device=p.device, dtype=torch.float64)
        self.m = 0.0
        self.swapped = False
        slot = {id(q): i for i, q in enumerate(flat.params)}
        self.names = []
        for (name, bname), (_, q) in zip(names, module.named_parameters()):
            if id(q) in slot:
                off, n = flat.slices[slot[id(q)]]
                view = self.flat_e[off:off + n].view(q.shape)
            else:
                view = q.detach().clone()
            module.register_buffer(bname, view)
            self.names.append((name, bname))

    def momentum_at(self, s):
        return ema_momentum(int(s), self.momentum, self.interval, self.warm_up)

    def set_iter(self, s):
        """``m`` of the update after iteration ``s`` -> ``hyper_t``: one in-place fill, the value travels in the launch's
        arguments (no staging buffer, no sync)."""
        self.m = self.momentum_at(s)
        self.hyper_t.fill_(self.m)
        return self.m

    @torch.no_grad()
    def launch(self):
        """ema = (1 - m) ema + m p with the ``m`` last set."""
        p, e = self.flat.flat_p, self.flat_e
        if self.native:
            rc = native.lib().dsgcn_ema_update(e.data_ptr(), p.data_ptr(), e.numel(), self.hyper_t.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream)
            native.check(rc, 'dsgcn_ema_update')
            return
        # the kernel's formula with torch ops — m and 1 - m rounded to the buffers' type once, m = 0 leaves ema alone, 1 - m
        # = 0 copies — but not its bits: two rounded products and a rounded sum here, one product and a fused multiply-add
        # there.  Both stay within 4 * 2^-24 * max(|ema|, |p|) of the exact update.
        if self.m == 0.0:
            return
        one = torch.tensor(1.0 - self.m, dtype=e.dtype)
        if float(one) == 0.0:
            e.copy_(p)
        else:
            e.mul_(one).add_(p * torch.tensor(self.m, dtype=e.dtype))

    def update(self, s):
        self.set_iter(s)
        self.launch()

    @torch.no_grad()
    def swap(self):
        """Exchange parameters and averaged copy in place.  The weights change under every cache derived from them: what
        ``kernels.end_step()`` distrusts (the split weight images, the per-step operand buffers) is distrusted from here."""
        p, e = self.flat.flat_p, self.flat_e
        if self.native:
            rc = native.lib().dsgcn_ema_swap(p.data_ptr(), e.data_ptr(), p.numel(), torch.cuda.current_stream().cuda_stream)
            native.check(rc, 'dsgcn_ema_swap')
        else:
            keep = p.clone()
            p.copy_(e)
            e.copy_(keep)
        self.swapped = not self.swapped
        kernels.end_step()

    @torch.no_grad()
    def reset(self):
        """ema = the parameters as they are now (after weights were loaded into a model whose EMA starts afresh)."""
        self.flat_e.copy_(self.flat.flat_p)
        module = self.flat.module
        bufs = dict(module.named_buffers(recurse=False))
        slot = {id(q) for q in self.flat.params}
        for (name, bname), (_, q) in zip(self.names, module.named_parameters()):
            if id(q) not in slot:
                bufs[bname].copy_(q)
        self.swapped = False
