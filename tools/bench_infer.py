#!/usr/bin/env python
"""Time a multi-clip test batch three ways on one MI355X, in one process:

    (a) model(keypoint=x, return_loss=False)      RecognizerGCN.forward_test as it is (eager, host read-back per call)
    (b) InferEngine(model, use_graph=False)(x)    pooled last block + one-launch head, eager launches
    (c) InferEngine(model)(x)                     the same, replayed from its hipGraph

DS-STGCN NTU-60 at the shipped test shape (10 clips x 2 persons x 60 frames x 25 joints x 3), ``--videos`` per call.
After warm-up the three are timed in alternating rounds (``--repeats`` rounds of one call each) with device events; the
median, the quartiles and the extremes of each are reported, (a) including its device->host copy (it is part of the
call).  One JSON line on stdout.  ``--launches`` also counts the kernel launches of (a) and (b) with torch.profiler (one
extra call each, outside the timed rounds); (b)'s launches are the chain (c) replays as ONE graph launch."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(median=round(statistics.median(ms), 4), q1=round(q[0], 4), q3=round(q[2], 4), min=round(min(ms), 4),
                max=round(max(ms), 4))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--videos', type=int, default=16)
    ap.add_argument('--clips', type=int, default=10)
    ap.add_argument('--clip-len', type=int, default=60)
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--launches', action='store_true')
    args = ap.parse_args()
    if args.repeats < 20:
        ap.error('--repeats: at least 20 timed calls each')

    import numpy as np
    import torch
    import dsgcn_amd as D
    from dsgcn_amd import native
    from bench import ds_cfg
    if not torch.cuda.is_available():
        raise SystemExit('bench_infer: needs a GPU (a timing taken elsewhere says nothing)')
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    from closed_form import fill_running, liven32
    np.random.seed(0)
    torch.manual_seed(0)
    model = D.build_model(ds_cfg(60))
    liven32(model, 1, 0.5)
    fill_running(model)
    model = model.cuda().eval()
    x = torch.randn(args.videos, args.clips, 2, args.clip_len, 25, 3, generator=torch.Generator().manual_seed(1)).cuda()

    eager, replay = D.InferEngine(model, use_graph=False), D.InferEngine(model, strict_graph=True)
    ways = dict(forward_test=lambda: model(keypoint=x, return_loss=False), engine_eager=lambda: eager(x),
                engine_replay=lambda: replay(x))
    for _ in range(max(args.warmup, 3)):
        outs = {k: f() for k, f in ways.items()}
    torch.cuda.synchronize()
    assert replay.graphed(x) and replay.capture_error is None
    ref = np.asarray(outs['forward_test'], np.float64)
    diff = {k: float(np.linalg.norm(outs[k].cpu().double().numpy() - ref) / np.linalg.norm(ref))
            for k in ('engine_eager', 'engine_replay')}

    times = {k: [] for k in ways}
    for _ in range(args.repeats):                    # alternating: drift of the box lands on all three alike
        for k, f in ways.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            f()
            t1.record()
            t1.synchronize()
            times[k].append(t0.elapsed_time(t1))

    launches = None
    if args.launches:
        from torch.profiler import ProfilerActivity, profile
        launches = {}
        for k in ('forward_test', 'engine_eager'):
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                ways[k]()
                torch.cuda.synchronize()
            launches[k] = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                              and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower())

    stamp = native.LIB_PATH + '.srchash'
    clips = args.videos * args.clips
    res = dict(metric='multi-clip test batch, DS-STGCN NTU-60', videos=args.videos, clips_per_video=args.clips,
               clip_len=args.clip_len, repeats=args.repeats, unit='ms/call',
               ms={k: spread(v) for k, v in times.items()},
               clips_per_s={k: round(clips / statistics.median(v) * 1e3, 1) for k, v in times.items()},
               speedup_replay_over_forward_test=round(statistics.median(times['forward_test']) /
                                                      statistics.median(times['engine_replay']), 4),
               rel_diff_vs_forward_test=diff, launches=launches, device=torch.cuda.get_device_name(0),
               kernels_srchash=open(stamp).read().strip() if os.path.exists(stamp) else None)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
