"""Cost of gradient accumulation on the bench workload (DS-STGCN NTU-60, hipGraphs) — the numbers of
profiles/grad_accum/README.md.  bench.py's model and engine settings; one JSON line per run.
    python tools/grad_accum_bench.py --clips 16 --accumulate 8     ms per micro-iteration, per stepping iteration, clips/s of
                                                                   a whole group (host clock around device synchronises:
                                                                   one after the k - 1 micro-iterations, one after the
                                                                   stepping one; medians over --groups groups)
    python tools/grad_accum_bench.py --clips 128 --accumulate 1    ms per TrainEngine.step as it was before accumulation
                                                                   (accumulate=1 launches nothing new), --groups steps per
                                                                   window, medians over --windows windows
    python tools/grad_accum_bench.py --kernels                     the two kernels alone at the model's flat size: us per
                                                                   launch (events around --steps launches) and the share
                                                                   of 3 * 4n resp. 4 * 4n bytes at 8 TB/s
--root: import bench.py and the package from another checkout (built there); an engine that predates ``accumulate`` is then
built without the argument."""
import argparse
import json
import os
import statistics
import sys
import time

PEAK = 8.0e12                                  # bytes / s, the HBM3E specification


def kernels(args, torch, bench, dsgcn_amd, native, dev):
    model = bench.build_model().to(dev).train()
    n = sum(p.numel() for p in model.parameters() if p.requires_grad)
    acc = torch.zeros(n, device=dev)
    g = torch.randn(n, device=dev)
    f = torch.full((1,), 0.125, device=dev)
    lib, st = native.lib(), torch.cuda.current_stream().cuda_stream
    calls = dict(accum=(lambda: lib.dsgcn_grad_accum(acc.data_ptr(), g.data_ptr(), n, st), 3),
                 finish=(lambda: lib.dsgcn_grad_accum_finish(acc.data_ptr(), g.data_ptr(), f.data_ptr(), n, st), 4))
    out = dict(tag=args.tag, mode='kernels', n=n, launches=args.steps)
    for name, (call, streams) in calls.items():
        for _ in range(20):
            assert call() == 0
        us = []
        for _ in range(args.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.steps):
                call()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / args.steps)
        med = statistics.median(us)
        out[name] = dict(us_per_launch=[round(v, 3) for v in us], median_us=round(med, 3),
                         bytes=streams * 4 * n, share_of_8TBs=round(streams * 4 * n / PEAK * 1e6 / med, 4))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--clips', type=int, default=16)
    ap.add_argument('--accumulate', type=int, default=8)
    ap.add_argument('--groups', type=int, default=20, help='groups (accumulate > 1) or steps (accumulate 1) per window')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=4, help='groups (accumulate > 1) or steps before the first window')
    ap.add_argument('--steps', type=int, default=200, help='--kernels: launches per window')
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--tag', default='')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import bench
    import dsgcn_amd
    from dsgcn_amd import native
    native.lib()
    if not torch.cuda.is_available():
        raise SystemExit('grad_accum_bench.py needs the GPU')
    dev = torch.device('cuda', 0)
    if args.kernels:
        return kernels(args, torch, bench, dsgcn_amd, native, dev)
    k = args.accumulate
    model = bench.build_model().to(dev).train()
    kw = dict(accumulate=k) if k > 1 else {}
    engine = dsgcn_amd.TrainEngine(model, lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True, use_graph=True,
                                   warmup_eager=3, **kw)
    gen = torch.Generator().manual_seed(1234)
    keypoint = torch.randn(args.clips, 1, bench.M, bench.T, bench.V, bench.C, generator=gen).to(dev)
    label = torch.randint(0, bench.CLASSES, (args.clips, 1), generator=gen).to(dev)
    for _ in range(args.warmup * k):
        logs = engine.step(keypoint, label)
    torch.cuda.synchronize()
    if not engine.graphed(keypoint, label):
        raise SystemExit(f'capture failed: {engine.capture_error}')
    out = dict(tag=args.tag, root=os.path.basename(os.path.abspath(args.root)), clips=args.clips, accumulate=k)
    if k == 1:
        ms = []
        for _ in range(args.windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.groups):
                logs = engine.step(keypoint, label)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / args.groups)
        med = statistics.median(ms)
        out.update(steps=args.groups, ms_per_step=[round(v, 4) for v in ms], median_ms=round(med, 4),
                   clips_per_s=round(args.clips / med * 1e3, 1))
    else:
        micro, step, group = [], [], []
        for _ in range(args.windows * args.groups):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(k - 1):
                engine.step(keypoint, label)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            logs = engine.step(keypoint, label)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            micro.append((t1 - t0) * 1e3 / (k - 1))
            step.append((t2 - t1) * 1e3)
            group.append((t2 - t0) * 1e3)
        out.update(groups=len(group), micro_ms=round(statistics.median(micro), 4), stepping_ms=round(statistics.median(step), 4),
                   group_ms=round(statistics.median(group), 4),
                   clips_per_s=round(k * args.clips / statistics.median(group) * 1e3, 1),
                   micro_ms_min_max=[round(min(micro), 4), round(max(micro), 4)],
                   stepping_ms_min_max=[round(min(step), 4), round(max(step), 4)])
    out['loss'] = float(logs['loss'])
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
