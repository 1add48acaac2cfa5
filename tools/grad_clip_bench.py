"""Step time of the bench workload (DS-STGCN, 64 clips, two hipGraphs) with and without gradient clipping — the numbers of
profiles/grad_clip/README.md.  bench.py's model, batch and engine settings; several timed windows after the warm-up, each
ending in a device synchronise; one JSON line: ms per step of every window, their median, the parameters' sha256 after
the last window and the last grad_norm.
    python tools/grad_clip_bench.py [--max-norm 45] [--norm-type 2] [--steps 100] [--windows 5] [--root OTHER_CHECKOUT]
--root: import bench.py and the package from another checkout (the parent commit, built there) for an A/B on one box; an
engine that predates grad_clip is then built without the argument."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--max-norm', type=float, default=None)
    ap.add_argument('--norm-type', default='2')
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--tag', default='')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import bench
    import dsgcn_amd
    from dsgcn_amd import native
    native.lib()
    if not torch.cuda.is_available():
        raise SystemExit('grad_clip_bench.py needs the GPU')
    dev = torch.device('cuda', 0)
    model = bench.build_model().to(dev).train()
    kw = {}
    if args.max_norm is not None:
        kw['grad_clip'] = dict(max_norm=args.max_norm, norm_type=float(args.norm_type))
    engine = dsgcn_amd.TrainEngine(model, lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True, use_graph=True,
                                   warmup_eager=3, **kw)
    g = torch.Generator().manual_seed(1234)
    keypoint = torch.randn(bench.CLIPS_PER_GPU, 1, bench.M, bench.T, bench.V, bench.C, generator=g).to(dev)
    label = torch.randint(0, bench.CLASSES, (bench.CLIPS_PER_GPU, 1), generator=g).to(dev)
    for _ in range(args.warmup):
        logs = engine.step(keypoint, label)
    torch.cuda.synchronize()
    if not engine.graphed(keypoint, label):
        raise SystemExit(f'capture failed: {engine.capture_error}')
    ms = []
    for _ in range(args.windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            logs = engine.step(keypoint, label)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / args.steps)
    out = dict(tag=args.tag, root=os.path.basename(os.path.abspath(args.root)), max_norm=args.max_norm,
               norm_type=args.norm_type if args.max_norm is not None else None, steps=args.steps,
               ms_per_step=[round(v, 4) for v in ms], median_ms=round(statistics.median(ms), 4),
               param_sha256=hashlib.sha256(engine.flat.flat_p.detach().cpu().numpy().tobytes()).hexdigest()[:16],
               loss=float(logs['loss']), grad_norm=float(logs['grad_norm']) if 'grad_norm' in logs else None)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
