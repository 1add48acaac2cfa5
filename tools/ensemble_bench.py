#!/usr/bin/env python
"""Time the NTU-60 four-stream test pass (joint, bone, joint motion, bone motion; weights 2:2:1:1) three ways on one
MI355X, in one process:

    (a) four_runs    four single-feature SkeletonBatcher launches, four InferEngine replays and four head launches per
                     batch, stream after stream over the whole set, four read-backs, ``ensemble_results`` on the host
    (b) ensemble     StreamBatcher (one plan, one input launch) + EnsembleEngine(concurrent=False): one replay per batch
                     holding the four backbones back to back and the one ensemble-head launch; one read-back
    (c) concurrent   the same with EnsembleEngine(concurrent=True): the backbones as parallel branches of the graph

DS-STGCN at the shipped test shape (10 clips x 2 persons x 100 frames x 25 joints x 3) over a synthetic resident set,
``--videos-per-batch`` 1 and 16.  A block is one whole pass of ``--batches`` batches, host clock around it, ending in the
read-back (a device synchronise).  After a warm-up pass of each way the three alternate for ``--blocks`` blocks; the
median and the extremes of each are reported, and the three results are compared bit for bit.  One JSON line per batch
size on stdout.

``--only WAY --trace-batches N``: no timing — a warm-up pass, then N batches of that way alone, for a kernel trace taken
by an outside profiler (launches per batch = the difference of two such runs over the difference of their N).

The input kernel's requested bytes (loads and stores per output position, from the shapes) are printed with the result:
four single-feature launches read 9 joints per position (j 1, b 2, jm 2, bm 4) and the decisions four times, the stream
launch reads 4 joints and the decisions once."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FEATS = ['j', 'b', 'jm', 'bm']
WEIGHTS = (2, 2, 1, 1)


def pipe(feat, clip_len, clips):
    return [dict(type='PreNormalize3D'), dict(type='GenSkeFeat', feats=[feat]),
            dict(type='UniformSample', clip_len=clip_len, num_clips=clips, test_mode=True), dict(type='PoseDecode'),
            dict(type='FormatGCNInput', num_person=2), dict(type='Collect', keys=['keypoint', 'label'], meta_keys=[]),
            dict(type='ToTensor', keys=['keypoint'])]


def input_bytes(positions, C, V):
    """Bytes the input kernels ask for per batch: (four single launches, one stream launch).  Per output position a
    joint read is C floats; the decisions are f0, f1 (2 ints), M, T, flags (3 ints), offset (8 bytes), centre (3 floats),
    matrix (9 floats) and the joint's parent (1 int); every launch writes C floats per feature."""
    decisions = 4 * (2 + 3 + 3 + 9 + 1) + 8
    joint = 4 * C
    four = positions * (9 * joint + 4 * decisions)
    one = positions * (4 * joint + decisions)
    written = positions * 4 * joint
    return dict(four_launches_read=four, stream_launch_read=one, written_either_way=written)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--videos-per-batch', type=int, nargs='+', default=[1, 16])
    ap.add_argument('--batches', type=int, default=8, help='batches per pass (block)')
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--clips', type=int, default=10)
    ap.add_argument('--clip-len', type=int, default=100)
    ap.add_argument('--only', choices=['four_runs', 'ensemble', 'concurrent'])
    ap.add_argument('--trace-batches', type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch
    import dsgcn_amd as D
    from bench import ds_cfg
    if not torch.cuda.is_available():
        raise SystemExit('ensemble_bench: needs a GPU (a timing taken elsewhere says nothing)')
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    from closed_form import fill_running, liven32
    models = []
    for s in range(4):
        np.random.seed(s)
        torch.manual_seed(s)
        m = D.build_model(ds_cfg(60))
        liven32(m, s + 1, 0.5)
        fill_running(m)
        models.append(m.cuda().eval())

    for per in args.videos_per_batch:
        n = per * (args.trace_batches or args.batches)
        rng = np.random.RandomState(7)
        anns = []
        for i in range(n):
            T = int(rng.randint(60, 140))
            kp = (rng.randn(1, 1, 25, 3) * 0.4 + [0.2, 0.1, 3.0] + np.cumsum(rng.randn(2, T, 1, 3) * 0.02, axis=1)
                  + rng.randn(2, T, 25, 3) * 0.05).astype(np.float32)
            anns.append(dict(frame_dir=f'v{i}', label=i % 60, keypoint=kp, total_frames=T))
        store = D.SkeletonStore(anns)
        batches = [list(range(b, b + per)) for b in range(0, n, per)]
        singles = [D.SkeletonBatcher(pipe(f, args.clip_len, args.clips)) for f in FEATS]
        streams = D.StreamBatcher([pipe(f, args.clip_len, args.clips) for f in FEATS])
        engines = [D.InferEngine(m, strict_graph=True) for m in models]
        seq = D.EnsembleEngine(models, WEIGHTS)
        conc = D.EnsembleEngine(models, WEIGHTS, concurrent=True)

        def four_runs():
            rows = []
            for s in range(4):
                part = [engines[s](singles[s](store, idx)[0]) for idx in batches]
                rows.append(torch.cat(part).cpu().numpy())
            return np.stack(D.ensemble_results([list(r) for r in rows], WEIGHTS)['results'])

        def ensemble(eng=seq):
            part = [eng(streams(store, idx)[0]) for idx in batches]
            return torch.cat(part).cpu().numpy()

        ways = dict(four_runs=four_runs, ensemble=ensemble, concurrent=lambda: ensemble(conc))
        if args.only:
            ways = {args.only: ways[args.only]}
        state = np.random.get_state()
        for _ in range(2):                                   # every shape captured and replayed once
            outs = {k: f() for k, f in ways.items()}
        assert all(e.capture_error is None for e in [seq, conc] + engines)
        if args.only:
            ways[args.only]()
            print(json.dumps(dict(only=args.only, videos_per_batch=per, batches=len(batches), passes=3)))
            continue
        same = {k: bool(np.array_equal(outs[k], outs['four_runs'])) for k in ways}
        times = {k: [] for k in ways}
        for _ in range(args.blocks):                         # alternating: drift of the box lands on all three alike
            for k, f in ways.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                times[k].append((time.perf_counter() - t0) * 1e3 / len(batches))
        np.random.set_state(state)
        positions = per * args.clips * 2 * args.clip_len * 25
        res = dict(metric='four-stream test pass, DS-STGCN NTU-60', videos_per_batch=per, clips=args.clips,
                   clip_len=args.clip_len, batches_per_block=len(batches), blocks=args.blocks, unit='ms/batch',
                   ms={k: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))
                       for k, v in times.items()},
                   equal_to_four_runs=same, replays=dict(ensemble=seq.replays, concurrent=conc.replays),
                   input_kernel_bytes_per_batch=input_bytes(positions, 3, 25), device=torch.cuda.get_device_name(0))
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
