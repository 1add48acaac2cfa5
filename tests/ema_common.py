"""Shared by tests/test_ema_host.py and tests/test_ema_gpu.py: the reduced DS-STGCN run of
tests/golden/trajectory_dsstgcn_reduced.npz under mmcv's EMAHook, the fp64 recurrence it is held to and the bound.

The bound (one statement, used by every comparison): one fp32 update ``ema = (1 - m) ema + m p`` is off by at most
``4 * 2^-24 * max(|ema|, |p|)`` from the exact one — the roundings of m and 1 - m to float, two products, one sum — and
earlier errors are multiplied by 1 - m < 1, so after k updates the elementwise error against the fp64 recurrence is at
most ``4 k 2^-24 B`` with B the largest magnitude among the initial buffer and every p seen."""
import contextlib
import json

import numpy as np
import torch

import dsgcn_amd as D
from dsgcn_amd.apis import EvalLoop
from dsgcn_amd.engine import TrainEngine
from test_oracle_golden import load, sd_of

HOOK = dict(type='EMAHook', momentum=0.5, warm_up=4)


def fixture_model():
    z = load('trajectory_dsstgcn_reduced.npz')
    cfg = json.loads(str(z['cfg']))
    cfg['backbone']['tcn_ms_cfg'] = [tuple(c) if isinstance(c, list) else c for c in cfg['backbone']['tcn_ms_cfg']]
    m = D.build_model(cfg)
    m.load_state_dict(sd_of(z, 'sd_', torch.float32))
    return z, m


def setup(work_dir, total_epochs=2, **extra):
    """-> (model, data, run cfg): 24 clips, batches of 8 -> 3 iterations per epoch, the fixture's SGD and cosine rate."""
    z, m = fixture_model()
    tr = json.loads(str(z['config']))
    data = [dict(keypoint=z['x'][i], label=int(z['label'][i])) for i in range(tr['samples'])]
    cfg = dict(data=dict(videos_per_gpu=tr['batch'], val_dataloader=dict(videos_per_gpu=8)), seed=tr['seed'],
               total_epochs=total_epochs,
               optimizer=dict(type='SGD', lr=tr['lr'], momentum=tr['momentum'], weight_decay=tr['weight_decay'], nesterov=True),
               optimizer_config=dict(grad_clip=None), lr_config=dict(policy='CosineAnnealing', min_lr=0, by_epoch=False),
               checkpoint_config=dict(interval=1), log_config=dict(interval=1), work_dir=str(work_dir), **extra)
    return m, data, cfg


@contextlib.contextmanager
def recorded():
    """Inside: every ``TrainEngine.step`` appends (flat parameters after it, the m it used, the ema_iter it ran as) to
    ``rec['steps']`` and every ``EvalLoop.predict`` its scores to ``rec['scores']``."""
    rec = dict(steps=[], scores=[])
    step, predict = TrainEngine.step, EvalLoop.predict

    def step_rec(self, *a, **k):
        it = k['ema_iter'] if k.get('ema_iter') is not None else self.ema_iter
        out = step(self, *a, **k)
        rec['steps'].append((self.flat.flat_p.detach().clone().cpu(), None if self.ema is None else self.ema.m, it))
        return out

    def predict_rec(self, *a, **k):
        out = predict(self, *a, **k)
        rec['scores'].append(np.stack(out))
        return out

    TrainEngine.step, EvalLoop.predict = step_rec, predict_rec
    try:
        yield rec
    finally:
        TrainEngine.step, EvalLoop.predict = step, predict


def recurrence(e0, ps, ms, skip=None):
    """The fp64 recurrence from e0 over (p, m) pairs; ``skip``: the index of one update to leave out."""
    e = e0.double().clone()
    for j, (p, m) in enumerate(zip(ps, ms)):
        if j != skip:
            e = (1.0 - m) * e + m * p.double()
    return e


def bound(e0, ps, k=None):
    B = max([float(e0.abs().max())] + [float(p.abs().max()) for p in ps])
    return 4 * (len(ps) if k is None else k) * 2.0 ** -24 * B


def check_not_vacuous(e0, ps, ms, tol):
    """The oracle with any single update left out differs from the full one by more than ten times the bound, in relative
    L2 over the buffer — both sides over ||full||: the difference, and an error of ``tol`` in every element.  -> full oracle"""
    full = recurrence(e0, ps, ms)
    norm = float(full.norm())
    rel_tol = tol * full.numel() ** 0.5 / norm
    for j in range(len(ps)):
        rel = float((recurrence(e0, ps, ms, skip=j) - full).norm()) / norm
        print(f'update {j} left out: relative L2 {rel:.3e}; ten times the bound {10 * rel_tol:.3e}')
        assert rel > 10 * rel_tol, (j, rel, rel_tol)
    return full


def flat_names(engine):
    """parameter name -> (offset, length) in the engine's flat buffers"""
    slot = {id(p): s for p, s in zip(engine.flat.params, engine.flat.slices)}
    return {name: slot[id(p)] for name, p in engine.model.named_parameters() if id(p) in slot}


def flat_of(sd, engine):
    """The parameter entries of a state dict in the layout of the engine's flat buffers."""
    names = flat_names(engine)
    out = torch.empty(engine.flat.flat_p.numel(), dtype=torch.float32)
    for name, (off, n) in names.items():
        out[off:off + n] = sd[name].detach().reshape(-1).cpu()
    return out


def check_epoch_file(path, engine, p0, steps, k, first=0):
    """An epoch checkpoint written after ``k`` iterations: ema_* entries = the raw weights after the last of them (bit for
    bit), parameter entries = the fp64 recurrence from ``p0`` (the average before iteration ``first``: the initial weights,
    or the parameter entries of the previous epoch's file) over the raw weights after iterations first..k-1, within the
    bound."""
    sd = torch.load(path, map_location='cpu', weights_only=False)['state_dict']
    names = flat_names(engine)
    ps, ms = [s[0] for s in steps[first:k]], [s[1] for s in steps[first:k]]
    assert [s[2] for s in steps[first:k]] == list(range(first, k))
    assert ms == [D.ema_momentum(s, 0.5, 1, 4) for s in range(first, k)] and min(ms) >= 0.1
    tol = bound(p0, ps)
    want = check_not_vacuous(p0, ps, ms, tol)
    assert sum(key.startswith('ema_') for key in sd) == len(list(engine.model.named_parameters()))
    worst = 0.0
    for name, (off, n) in names.items():
        raw = sd['ema_' + name.replace('.', '_')]
        assert torch.equal(raw.reshape(-1), ps[-1][off:off + n]), name
        err = float((sd[name].reshape(-1).double() - want[off:off + n]).abs().max())
        worst = max(worst, err)
    print(f'EMA after updates {first}..{k - 1}: worst elementwise error {worst:.3e}, bound {tol:.3e}')
    assert worst <= tol, (worst, tol)
    return sd
