"""What matmul precision 'high' buys — the numbers of profiles/precision/README.md.

    python tools/precision_bench.py --kernels      every (shape, direction) of the DS-STGCN NTU-60, ST-GCN and CTR-GCN
                                                   64-clip steps whose query (dsgcn_pwconv_terms / dsgcn_tconv_terms)
                                                   returns 3 at 'high': us at 'highest', us at 'high', ratio, spread
    python tools/precision_bench.py --steps        TrainEngine ms/step of the three models at both levels
    python tools/precision_bench.py --trace-step   a few replayed 'high' DS-STGCN steps and nothing else (the program to put
                                                   after `rocprofv3 --kernel-trace --stats --`)

Device events around blocks of back-to-back launches on warm shapes; the two levels ALTERNATE inside one process (block of
'highest', block of 'high', ...), five timed blocks each; spread = max - min of the five.  The shapes are read off the
library calls of one eager forward of each model (the forward entry points are wrapped for that pass), so the list follows
the models, and the kernels are timed through the C ABI with the operands a training step gives them: forward with an input
affine + ReLU and statistics, data / weight gradient with the BatchNorm terms A0 / B0."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BLOCKS = 5
MODELS = ('ds', 'stgcn', 'ctrgcn')


def build(kind):
    import bench
    import dsgcn_amd as D
    import numpy as np
    import torch
    if kind == 'ds':
        return bench.build_model()
    np.random.seed(0)
    torch.manual_seed(0)
    m = D.build_model(bench.other_cfg(kind))
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith('alpha'):
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
    return m


def batch():
    import bench
    import torch
    g = torch.Generator().manual_seed(1234)
    kp = torch.randn(bench.CLIPS_PER_GPU, 1, bench.M, bench.T, bench.V, bench.C, generator=g).cuda()
    lb = torch.randint(0, bench.CLASSES, (bench.CLIPS_PER_GPU, 1), generator=g).cuda()
    return kp, lb


def step_shapes(kind):
    """{('pw', n, Ci, Co, T, V, stride)} and {('tc', n, Ci, Co, T, V, KT, stride)} of one forward of the model."""
    import torch
    from dsgcn_amd import native
    lib = native.lib()
    seen = set()
    hooks = {'dsgcn_pwconv_fwd_ws': ('pw', 12, 18), 'dsgcn_pwconv_fwd_ws_guest': ('pw', 12, 18), 'dsgcn_tconv_fwd': ('tc', 11, 18)}
    saved = {name: getattr(lib, name) for name in hooks}

    def wrap(name):
        tag, a, b = hooks[name]

        def call(*args):
            seen.add((tag,) + tuple(int(v) for v in args[a:b]))
            return saved[name](*args)
        return call
    try:
        for name in hooks:
            setattr(lib, name, wrap(name))
        m = build(kind).cuda().train()
        kp, lb = batch()
        with torch.no_grad():
            m.train_step(dict(keypoint=kp, label=lb), None)
        torch.cuda.synchronize()
    finally:
        for name, fn in saved.items():
            setattr(lib, name, fn)
    return seen


def time_blocks(launch, reps):
    """us per launch of BLOCKS blocks per level, the levels alternating: {'highest': [...], 'high': [...]}"""
    import torch
    from dsgcn_amd import native
    lib = native.lib()
    out = {0: [], 1: []}
    for level in (0, 1):                             # warm both kernels
        lib.dsgcn_set_matmul_precision(level)
        for _ in range(3):
            launch()
    torch.cuda.synchronize()
    for _ in range(BLOCKS):
        for level in (0, 1):
            lib.dsgcn_set_matmul_precision(level)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                launch()
            e1.record()
            e1.synchronize()
            out[level].append(e0.elapsed_time(e1) * 1e3 / reps)
    lib.dsgcn_set_matmul_precision(0)
    return dict(highest=out[0], high=out[1])


def kernel_cases(shape):
    """-> [(direction, launch)] for the directions whose query says 3 at 'high'."""
    import torch
    from dsgcn_amd import native
    lib = native.lib()
    st = torch.cuda.current_stream().cuda_stream
    tag, n, Ci, Co, T, V = shape[:6]
    KT, stride = (shape[6], shape[7]) if tag == 'tc' else (0, shape[6])
    To = (T + stride - 1) // stride
    lib.dsgcn_set_matmul_precision(1)
    if tag == 'pw':
        dirs = [d for d in range(3) if lib.dsgcn_pwconv_terms(d, n, Ci, Co, T, V, stride) == 3]
    else:
        dirs = [d for d in range(3) if lib.dsgcn_tconv_terms(d, n, Ci, Co, T, V, KT, stride) == 3]
    lib.dsgcn_set_matmul_precision(0)
    if not dirs:
        return []
    g = torch.Generator().manual_seed(Ci + Co)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).cuda()    # noqa: E731
    x, s1, h1 = r(n, Ci, T, V), (torch.rand(Ci, generator=g) + 0.5).cuda(), r(Ci, scale=0.3)
    w = r(Co, Ci, max(KT, 1), 1, scale=(Ci * max(KT, 1)) ** -0.5)
    bias, z, gz = r(Co, scale=0.1), r(n, Co, To, V), r(n, Co, To, V)
    A0, B0 = r(Co, scale=1e-3), r(Co, scale=1e-3)
    zo, dx = torch.empty_like(z), torch.empty_like(x)
    p = lambda t: t.data_ptr()                                                   # noqa: E731
    keep = [x, s1, h1, w, bias, z, gz, A0, B0, zo, dx]
    cases = []
    if tag == 'pw':
        nb = lib.dsgcn_pwconv_wsplit_bytes(n, Ci, Co, T, V, stride)
        ws = torch.empty(max(nb, 4), dtype=torch.uint8, device='cuda')
        native.check(lib.dsgcn_pwconv_wsplit(p(w), Ci, Co, p(ws), st), 'wsplit')
        part = torch.empty(lib.dsgcn_pwconv_partial_rows(n, Ci, Co, T, V, stride, 0), Co, 2, device='cuda')
        ipart = torch.empty(lib.dsgcn_pwconv_ipart_rows(n, Ci, Co, T, V, stride), Ci, 3, device='cuda')
        splits = lib.dsgcn_pwconv_wgrad_splits(n, Ci, Co, T, V, stride)
        pstride = Co * Ci + Co
        wp = torch.empty(splits, pstride, device='cuda')
        keep += [ws, part, ipart, wp]
        fns = {0: lambda: lib.dsgcn_pwconv_fwd_ws(p(x), p(s1), p(h1), None, None, None, 1, p(w), p(bias), p(zo), None, p(part),
                                                   n, Ci, Co, T, V, stride, 0, 1, p(ws), st),
               1: lambda: lib.dsgcn_pwconv_dgrad_ws(p(x), p(s1), p(h1), None, None, None, 1, p(w), p(z), None, p(gz), None,
                                                     p(A0), p(B0), p(dx), None, p(ipart), n, Ci, Co, T, V, stride, 0, p(ws), st),
               2: lambda: lib.dsgcn_pwconv_wgrad(p(x), p(s1), p(h1), None, None, None, 1, p(z), None, p(gz), None, p(A0), p(B0),
                                                  p(wp), p(wp) + 4 * Co * Ci, pstride, n, Ci, Co, T, V, stride, 0, st)}
    else:
        ws = torch.empty(lib.dsgcn_tconv_ws_bytes(n, Ci, Co, T, V, KT, stride), dtype=torch.uint8, device='cuda')
        native.check(lib.dsgcn_tconv_wsplit(p(w), Ci, Co, KT, p(ws), st), 'tsplit')
        part = torch.empty(lib.dsgcn_tconv_rows(0, n, Ci, Co, T, V, KT, stride), Co, 2, device='cuda')
        ipart = torch.empty(lib.dsgcn_tconv_rows(1, n, Ci, Co, T, V, KT, stride), Ci, 3, device='cuda')
        splits = lib.dsgcn_tconv_wgrad_splits(n, Ci, Co, T, V, KT, stride)
        pstride = Co * Ci * KT + Co
        wp = torch.empty(splits, pstride, device='cuda')
        keep += [ws, part, ipart, wp]
        fns = {0: lambda: lib.dsgcn_tconv_fwd(p(x), p(s1), p(h1), None, None, None, 1, p(ws), p(bias), p(zo), p(part), n, Ci, Co,
                                               T, V, KT, stride, st),
               1: lambda: lib.dsgcn_tconv_dgrad(p(x), p(s1), p(h1), None, None, None, 1, p(ws), p(z), p(gz), p(A0), p(B0), p(dx),
                                                 None, p(ipart), n, Ci, Co, T, V, KT, stride, st),
               2: lambda: lib.dsgcn_tconv_wgrad(p(x), p(s1), p(h1), None, None, None, 1, p(z), p(gz), p(A0), p(B0), p(wp),
                                                 p(wp) + 4 * Co * Ci * KT, pstride, n, Ci, Co, T, V, KT, stride, st)}
    for d in dirs:
        def launch(fn=fns[d], keep=keep):
            rc = fn()
            if rc != 0:
                raise SystemExit(f'{shape} direction {d}: status {rc}')
        cases.append((d, launch))
    return cases


def run_kernels(reps):
    shapes = {}
    for kind in MODELS:
        for s in sorted(step_shapes(kind)):
            shapes.setdefault(s, []).append(kind)
    for shape, kinds in sorted(shapes.items()):
        for d, launch in kernel_cases(shape):
            t = time_blocks(launch, reps)
            hi, lo = statistics.median(t['highest']), statistics.median(t['high'])
            print(json.dumps(dict(shape=list(shape), models=kinds, dir=('fwd', 'dgrad', 'wgrad')[d], us_highest=round(hi, 2),
                                  us_high=round(lo, 2), ratio=round(hi / lo, 3),
                                  spread_highest=round(max(t['highest']) - min(t['highest']), 2),
                                  spread_high=round(max(t['high']) - min(t['high']), 2))), flush=True)


def run_steps(steps, warmup):
    import torch
    import dsgcn_amd as D
    kp, lb = batch()
    for kind in MODELS:
        engines = {lv: D.TrainEngine(build(kind).cuda().train(), lr=0.1, use_graph=True, warmup_eager=3, matmul_precision=lv)
                   for lv in D.kernels.MATMUL_PRECISIONS}
        for eng in engines.values():
            for _ in range(warmup):
                eng.step(kp, lb)
            torch.cuda.synchronize()
            if not eng.graphed(kp, lb):
                raise SystemExit(f'{kind}: capture failed: {eng.capture_error}')
        ms = {lv: [] for lv in engines}
        for _ in range(BLOCKS):
            for lv, eng in engines.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(steps):
                    eng.step(kp, lb)
                e1.record()
                e1.synchronize()
                ms[lv].append(e0.elapsed_time(e1) / steps)
        print(json.dumps(dict(model=kind, **{f'ms_{lv}': round(statistics.median(v), 4) for lv, v in ms.items()},
                              **{f'spread_{lv}': round(max(v) - min(v), 4) for lv, v in ms.items()},
                              ratio=round(statistics.median(ms['highest']) / statistics.median(ms['high']), 4))), flush=True)
        del engines


def run_trace_step(steps):
    import torch
    import dsgcn_amd as D
    kp, lb = batch()
    eng = D.TrainEngine(build('ds').cuda().train(), lr=0.1, use_graph=True, warmup_eager=2, matmul_precision='high')
    for _ in range(2 + steps):
        eng.step(kp, lb)
    torch.cuda.synchronize()
    if not eng.graphed(kp, lb):
        raise SystemExit(f'capture failed: {eng.capture_error}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--steps', action='store_true')
    ap.add_argument('--trace-step', action='store_true')
    ap.add_argument('--reps', type=int, default=20, help='launches per timed block')
    ap.add_argument('--nsteps', type=int, default=30, help='engine steps per timed block')
    ap.add_argument('--warmup', type=int, default=8)
    args = ap.parse_args()
    import torch
    from dsgcn_amd import native
    native.lib()
    if not torch.cuda.is_available():
        raise SystemExit('precision_bench.py needs the GPU')
    if args.kernels:
        run_kernels(args.reps)
    if args.steps:
        run_steps(args.nsteps, args.warmup)
    if args.trace_step:
        run_trace_step(5)


if __name__ == '__main__':
    main()
