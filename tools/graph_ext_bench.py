#!/usr/bin/env python
"""What the per-video learned adjacency (``test_cfg['graph_ext']``) costs on one MI355X, in one process:

    scoring          InferEngine replay of the scoring pass
    graphs ctr       InferEngine replay under graph_ext='ctr'  (one more K-B per layer with beta = 0, then the pool kernel)
    graphs ahat      InferEngine replay under graph_ext='ahat' (the pool kernel on the layer's own Ahat)
    ... framework    the same two passes with the taps pooled by framework ops (``view(...).mean((1, 3))`` and a copy into
                     the layer slice) instead of csrc/graphpool.hip

DS-STGCN NTU-60 on ``--videos`` x 10 clips x 2 persons at the shipped test clip length; the passes are timed in alternating
rounds with device events (median, quartiles).  Then ``dsgcn_graph_pool`` alone on each layer's Ahat shape (mid 8 / 16 /
32, at ``--videos`` videos and at 1), replayed from a hipGraph: time per call, the launches' splits, and GB/s of the bytes it
must move (Ahat in, graphs out) against the 8 TB/s of the part.  One JSON line on stdout; ``--out FILE`` also writes it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_TBS = 8.0


def spread(v):
    q = statistics.quantiles(v, n=4)
    return dict(median=round(statistics.median(v), 4), q1=round(q[0], 4), q3=round(q[2], 4), min=round(min(v), 4),
                max=round(max(v), 4))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--videos', type=int, default=8)
    ap.add_argument('--clips', type=int, default=10)
    ap.add_argument('--clip-len', type=int, default=60)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import dsgcn_amd as D
    from dsgcn_amd import kernels as K
    from dsgcn_amd import native
    from bench import ds_cfg
    if not torch.cuda.is_available():
        raise SystemExit('graph_ext_bench: needs a GPU (a timing taken elsewhere says nothing)')
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    from closed_form import fill_running, liven32
    np.random.seed(0)
    torch.manual_seed(0)
    model = D.build_model(ds_cfg(60))
    liven32(model, 1, 0.5)
    fill_running(model)
    model = model.cuda().eval()
    x = torch.randn(args.videos, args.clips, 2, args.clip_len, 25, 3, generator=torch.Generator().manual_seed(1)).cuda()

    def framework_pool(ahat, group, Ks, out, layer):
        n, KM, V, _ = ahat.shape
        out[:, layer] = ahat.view(n // group, group, Ks, KM // Ks, V, V).mean((1, 3))
        return out

    hip_pool = K.graph_pool
    passes = (('scoring', False, hip_pool), ('graphs ctr', 'ctr', hip_pool), ('graphs ahat', 'ahat', hip_pool),
              ('graphs ctr, framework pool', 'ctr', framework_pool), ('graphs ahat, framework pool', 'ahat', framework_pool))
    engines, outs = {}, {}

    def run(name, mode, pool):
        model.test_cfg['graph_ext'] = mode
        K.graph_pool = pool                      # the collector reaches the pool through kernels.ops() at call time
        try:
            return engines[name](x)
        finally:
            K.graph_pool = hip_pool
            model.test_cfg['graph_ext'] = False

    for name, mode, pool in passes:
        engines[name] = D.InferEngine(model, strict_graph=True)       # an engine each: their graphs hold their own pool
        for _ in range(3):
            outs[name] = run(name, mode, pool)
        torch.cuda.synchronize()
        assert engines[name].replays >= 2 and engines[name].capture_error is None, name
    diff = {m: float((outs[f'graphs {m}, framework pool'].double() - outs[f'graphs {m}'].double()).norm() /
                     outs[f'graphs {m}'].double().norm()) for m in ('ctr', 'ahat')}

    times = {name: [] for name, _, _ in passes}
    for _ in range(args.repeats):                # alternating: drift of the box lands on all alike
        for name, mode, pool in passes:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            run(name, mode, pool)
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1))

    # the pool kernel alone on every layer shape of the model
    units = model.graph_units()
    group, V, Ks = args.clips * 2, 25, 3
    layers = []
    for videos in (args.videos, 1):
        for mid in sorted({u.mid_channels for u in units}):
            count = sum(u.mid_channels == mid for u in units)
            a = torch.randn(videos * group, Ks * mid, V, V, device='cuda')
            out = torch.empty(videos, 1, Ks, V, V, device='cuda')
            for _ in range(3):
                K.graph_pool(a, group, Ks, out, 0)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                K.graph_pool(a, group, Ks, out, 0)
            for _ in range(10):
                g.replay()
            us = []
            for _ in range(5):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.iters):
                    g.replay()
                t1.record()
                t1.synchronize()
                us.append(t0.elapsed_time(t1) * 1e3 / args.iters)
            t = statistics.median(us)
            nbytes = (a.numel() + out.numel()) * 4
            splits = native.lib().dsgcn_graph_pool_splits(videos, group, Ks, mid, V)
            layers.append(dict(videos=videos, mid=mid, layers_of_this_shape=count, ahat_mb=round(a.numel() * 4 / 2 ** 20, 2),
                               splits=splits, workgroups=videos * Ks * splits, launches=2 if splits > 1 else 1,
                               us=round(t, 2), gb_s=round(nbytes / t / 1e3, 1),
                               pct_of_8tbs=round(nbytes / t / 1e3 / (HBM_TBS * 1e3) * 100, 2)))

    stamp = native.LIB_PATH + '.srchash'
    res = dict(metric='per-video learned adjacency, DS-STGCN NTU-60', videos=args.videos, clips_per_video=args.clips,
               clip_len=args.clip_len, repeats=args.repeats, unit='ms/call', ms={k: spread(v) for k, v in times.items()},
               rel_diff_framework_pool_vs_kernel=diff, pool_kernel=layers, graphs_shape=list(outs['graphs ctr'].shape),
               device=torch.cuda.get_device_name(0),
               kernels_srchash=open(stamp).read().strip() if os.path.exists(stamp) else None)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
