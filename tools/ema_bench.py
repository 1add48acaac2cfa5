"""What the weight EMA (mmcv's EMAHook, TrainEngine(ema=...)) costs — the numbers of profiles/ema/README.md.

    python tools/ema_bench.py --kernels    dsgcn_ema_update and dsgcn_ema_swap on the flat buffer of the headline DS-STGCN
                                           model: us per launch, spread
    python tools/ema_bench.py --steps      the headline step (64 clips, hipGraph replay) with ema=None and with the EMA on
    python tools/ema_bench.py --count N [--ema]
                                           N replayed steps of one engine and nothing else after the warm-up marker line:
                                           the target of a `rocprofv3 --kernel-trace --stats` run that counts launches

The pattern of tools/lr_schedules_bench.py: device events around blocks of back-to-back launches / steps on warm buffers,
the two forms ALTERNATING inside one process, five timed blocks each; the figure is the median, spread = max - min."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BLOCKS = 5
EMA = dict(momentum=0.0002, interval=1, warm_up=100)


def timed(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps          # ms


def run_kernels(reps):
    import torch
    import bench
    import dsgcn_amd as D
    from dsgcn_amd import native
    flat = D.FlatParams(bench.build_model().cuda().train(), gather=True)
    lib, st = native.lib(), torch.cuda.current_stream().cuda_stream
    p, e = flat.flat_p, flat.flat_p.clone()
    n = p.numel()
    hyper = torch.full((1,), 0.0002, dtype=torch.float64, device='cuda')
    calls = dict(ema_update=lambda i: lib.dsgcn_ema_update(e.data_ptr(), p.data_ptr(), n, hyper.data_ptr(), st),
                 ema_swap=lambda i: lib.dsgcn_ema_swap(p.data_ptr(), e.data_ptr(), n, st))
    for name, fn in calls.items():
        if fn(0) != 0:
            raise SystemExit(f'{name}: launch failed')
        timed(fn, 20)
        us = [timed(fn, reps) * 1e3 for _ in range(BLOCKS)]
        med = statistics.median(us)
        print(json.dumps(dict(kernel=name, n=n, us=round(med, 2), spread=round(max(us) - min(us), 2),
                              gbps=round(4 * n * (3 if name == 'ema_update' else 4) / med / 1e3, 1))), flush=True)


def engines(which):
    import torch
    import bench
    import dsgcn_amd as D
    g = torch.Generator().manual_seed(1234)
    kp = torch.randn(bench.CLIPS_PER_GPU, 1, bench.M, bench.T, bench.V, bench.C, generator=g).cuda()
    lb = torch.randint(0, bench.CLASSES, (bench.CLIPS_PER_GPU, 1), generator=g).cuda()
    opt = dict(type='SGD', lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True)
    engs = {flag: D.TrainEngine(bench.build_model().cuda().train(), optimizer=opt, use_graph=True, warmup_eager=3,
                                ema=EMA if flag else None) for flag in which}
    return engs, kp, lb


def warm(engs, kp, lb, warmup):
    import torch
    for flag, eng in engs.items():
        for _ in range(warmup):
            eng.step(kp, lb, lr=0.1)
        torch.cuda.synchronize()
        if not eng.graphed(kp, lb):
            raise SystemExit(f'ema={flag}: capture failed: {eng.capture_error}')


def run_steps(steps, warmup):
    engs, kp, lb = engines((False, True))
    warm(engs, kp, lb, warmup)
    ms = {flag: [] for flag in engs}
    for _ in range(BLOCKS):
        for flag, eng in engs.items():
            ms[flag].append(timed(lambda i, eng=eng: eng.step(kp, lb, lr=0.1), steps))
    med = {flag: statistics.median(v) for flag, v in ms.items()}
    print(json.dumps(dict(clips=int(kp.shape[0]), steps_per_block=steps, ms_ema_none=round(med[False], 4),
                          ms_ema_on=round(med[True], 4), spread_ema_none=round(max(ms[False]) - min(ms[False]), 4),
                          spread_ema_on=round(max(ms[True]) - min(ms[True]), 4),
                          difference_us=round((med[True] - med[False]) * 1e3, 2))), flush=True)


def run_count(steps, warmup, ema):
    import torch
    engs, kp, lb = engines((ema,))
    warm(engs, kp, lb, warmup)
    eng = engs[ema]
    for _ in range(steps):
        eng.step(kp, lb, lr=0.1)
    torch.cuda.synchronize()
    print(json.dumps(dict(ema=ema, warmup_steps=warmup, replayed_steps=steps)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--steps', action='store_true')
    ap.add_argument('--count', type=int, default=0, help='replayed steps of ONE engine (under a kernel trace)')
    ap.add_argument('--ema', action='store_true', help='--count: the engine with the EMA on')
    ap.add_argument('--reps', type=int, default=200, help='launches per timed block')
    ap.add_argument('--nsteps', type=int, default=30, help='engine steps per timed block')
    ap.add_argument('--warmup', type=int, default=8)
    args = ap.parse_args()
    import torch
    from dsgcn_amd import native
    native.lib()
    if not torch.cuda.is_available():
        raise SystemExit('ema_bench.py needs the GPU')
    if args.kernels:
        run_kernels(args.reps)
    if args.steps:
        run_steps(args.nsteps, args.warmup)
    if args.count:
        run_count(args.count, args.warmup, args.ema)


if __name__ == '__main__':
    main()
