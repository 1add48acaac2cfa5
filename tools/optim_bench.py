"""Time per update of the optimizer launches at the flat size of DS-STGCN NTU-60 (1 376 950 elements) — the numbers of
profiles/optim/README.md:
    sgd / sgd_clip              dsgcn_sgd_step, dsgcn_grad_norm_partials + dsgcn_sgd_step_clip     (one rate, one decay)
    group_sgd / group_sgd_clip  dsgcn_sgd_group_step[_clip] over the model's tensor table (paramwise_cfg: 4 groups)
    adam / adam_clip            dsgcn_adam_step[_clip] over the same table (AdamW)
    engine                      bench.py's engine (DS-STGCN, 64 clips, two hipGraphs): ms per step with SGD-nesterov and with
                                AdamW + paramwise_cfg, both in ONE process (--adam-first: the other order)
    python tools/optim_bench.py                 every case, each in a child process of its own under `timeout`
    python tools/optim_bench.py --case adam     one case in this process; one JSON line
The update cases replay a hipGraph of 20 updates (the launches back to back, as they sit in the step's graph B) and report
the median over several windows; the buffers (5.5 MB each) stay in the last-level cache, as they do in the step."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ('sgd', 'sgd_clip', 'group_sgd', 'group_sgd_clip', 'adam', 'adam_clip', 'engine')
PW = dict(norm_decay_mult=0., bias_lr_mult=2., custom_keys={'alpha': dict(lr_mult=0.1, decay_mult=0.)})
PER_GRAPH = 20


def update_case(case, windows, reps):
    import torch
    import bench
    import dsgcn_amd as D
    model = bench.build_model().cuda().train()
    flat = D.FlatParams(model, gather=True)
    clip = dict(max_norm=45, norm_type=2) if case.endswith('_clip') else None
    if case.startswith('sgd'):
        cfg = dict(type='SGD', lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True)
    elif case.startswith('group_sgd'):
        cfg = dict(type='SGD', lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True, paramwise_cfg=PW)
    else:
        cfg = dict(type='AdamW', lr=1e-3, weight_decay=0.01, paramwise_cfg=PW)
    opt = D.build_optimizer(flat, cfg, grad_clip=clip)
    gen = torch.Generator().manual_seed(1)
    grad = (torch.randn(flat.flat_g.numel(), generator=gen) * 1e-3).cuda()
    flat.flat_g.copy_(grad)
    for _ in range(3):
        opt.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(PER_GRAPH):
            opt.step()
    us = []
    for _ in range(windows):
        flat.flat_g.copy_(grad)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            graph.replay()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6 / (reps * PER_GRAPH))
    table = getattr(opt, 'table', None)
    return dict(case=case, n=flat.flat_p.numel(), tensors=len(flat.params), groups=len(table.wds) if table else 1,
                launches_per_update=2 if clip else 1, us_per_update=[round(v, 3) for v in us],
                median_us=round(statistics.median(us), 3))


def engine_case(windows, steps, warmup, adam_first=False):
    import torch
    import bench
    import dsgcn_amd as D
    dev = torch.device('cuda', 0)
    g = torch.Generator().manual_seed(1234)
    keypoint = torch.randn(bench.CLIPS_PER_GPU, 1, bench.M, bench.T, bench.V, bench.C, generator=g).to(dev)
    label = torch.randint(0, bench.CLASSES, (bench.CLIPS_PER_GPU, 1), generator=g).to(dev)
    out = dict(case='engine', steps=steps)
    runs = [('sgd', dict(type='SGD', lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True)),
            ('adamw_paramwise', dict(type='AdamW', lr=1e-3, weight_decay=0.01, paramwise_cfg=PW))]
    out['order'] = 'adamw first' if adam_first else 'sgd first'
    for name, cfg in (runs[::-1] if adam_first else runs):
        engine = D.TrainEngine(bench.build_model().to(dev).train(), optimizer=cfg, use_graph=True, warmup_eager=3)
        for _ in range(warmup):
            engine.step(keypoint, label)
        torch.cuda.synchronize()
        if not engine.graphed(keypoint, label):
            raise SystemExit(f'capture failed: {engine.capture_error}')
        ms = []
        for _ in range(windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                logs = engine.step(keypoint, label)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / steps)
        out[name] = dict(ms_per_step=[round(v, 4) for v in ms], median_ms=round(statistics.median(ms), 4),
                         loss=float(logs['loss']))
        del engine
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', choices=CASES)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--reps', type=int, default=50, help='graph replays (of 20 updates) per window')
    ap.add_argument('--steps', type=int, default=100, help='engine steps per window')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--timeout', type=int, default=240, help='seconds per case')
    ap.add_argument('--adam-first', action='store_true', help='engine case: build and time the AdamW engine before the SGD one')
    args = ap.parse_args()
    if args.case is None:
        # a child per case, each under its own time limit; the first failure ends the run
        for case in CASES:
            cmd = ['timeout', '-k', '10', str(args.timeout), sys.executable, os.path.abspath(__file__), '--case', case,
                   '--windows', str(args.windows), '--reps', str(args.reps), '--steps', str(args.steps),
                   '--warmup', str(args.warmup)]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                raise SystemExit(f'case {case} ended with status {rc}: stopping')
        return
    sys.path.insert(0, ROOT)
    import torch
    from dsgcn_amd import native
    native.lib()
    if not torch.cuda.is_available():
        raise SystemExit('optim_bench.py needs the GPU')
    res = engine_case(args.windows, args.steps, args.warmup, args.adam_first) if args.case == 'engine' else \
        update_case(args.case, args.windows, args.reps)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
