"""What reading momentum / beta1 from device memory costs — the numbers of profiles/lr_schedules/README.md.

    python tools/lr_schedules_bench.py --kernels    each of the six update entry points and its *_hyper form on the flat
                                                    buffer of the headline DS-STGCN model: us per launch, spread
    python tools/lr_schedules_bench.py --steps      one TrainEngine step (hipGraph replay) with and without
                                                    scheduled_momentum, SGD and AdamW

The pattern of tools/precision_bench.py: device events around blocks of back-to-back launches on warm buffers, the two
forms ALTERNATING inside one process (block of the parent, block of the *_hyper form, ...), five timed blocks each;
the figure is the median, spread = max - min of the five.  The *_clip forms are timed as the pair they run as
(dsgcn_grad_norm_partials + the update)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BLOCKS = 5
FORMS = ('sgd', 'sgd_clip', 'sgd_group', 'sgd_group_clip', 'adam', 'adam_clip')


def launches(flat):
    """{form: (parent launch, *_hyper launch)} over the optimizer state of ``flat`` (a FlatParams of the model)."""
    import torch
    from dsgcn_amd import native
    from dsgcn_amd.paramwise import param_rules
    from dsgcn_amd.train import GroupTable
    lib = native.lib()
    st = torch.cuda.current_stream().cuda_stream
    n = flat.flat_p.numel()
    p, g = flat.flat_p, flat.flat_g
    g.copy_(torch.randn(n, generator=torch.Generator().manual_seed(1)).cuda() * 1e-3)
    buf, m, v = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    pw = dict(norm_decay_mult=0., bias_lr_mult=2., custom_keys={'alpha': dict(lr_mult=0.1)})
    rules = {id(r.param): r for r in param_rules(flat.module, 1e-4, 5e-4, pw)}
    table = GroupTable(flat, [rules[id(q)].lr for q in flat.params], [rules[id(q)].weight_decay for q in flat.params])
    lr_t = torch.full((1,), 1e-4, device='cuda')
    hyper = torch.full((1,), 0.9, dtype=torch.float64, device='cuda')
    step = torch.zeros(table.chunks, dtype=torch.int32, device='cuda')
    rows = lib.dsgcn_grad_norm_rows(n)
    partial = torch.zeros(rows, dtype=torch.float64, device='cuda')
    out = torch.zeros(1, device='cuda')
    keep = [buf, m, v, table, lr_t, hyper, step, partial, out]
    P, G, B, M, V, H = p.data_ptr(), g.data_ptr(), buf.data_ptr(), m.data_ptr(), v.data_ptr(), hyper.data_ptr()
    clip = (partial.data_ptr(), rows, 2, 1e9, out.data_ptr())                      # coefficient 1: the state stays bounded
    norm = lambda: lib.dsgcn_grad_norm_partials(G, n, 2, partial.data_ptr(), st)   # noqa: E731
    tab = table.pointers()
    calls = {
        'sgd': (lambda: lib.dsgcn_sgd_step(P, G, B, lr_t.data_ptr(), 0.9, 5e-4, 1, n, st),
                lambda: lib.dsgcn_sgd_step_hyper(P, G, B, lr_t.data_ptr(), H, 5e-4, 1, n, st)),
        'sgd_clip': (lambda: norm() or lib.dsgcn_sgd_step_clip(P, G, B, lr_t.data_ptr(), *clip, 0.9, 5e-4, 1, n, st),
                     lambda: norm() or lib.dsgcn_sgd_step_clip_hyper(P, G, B, lr_t.data_ptr(), *clip, H, 5e-4, 1, n, st)),
        'sgd_group': (lambda: lib.dsgcn_sgd_group_step(P, G, B, *tab, 0.9, 1, n, st),
                      lambda: lib.dsgcn_sgd_group_step_hyper(P, G, B, *tab, H, 1, n, st)),
        'sgd_group_clip': (lambda: norm() or lib.dsgcn_sgd_group_step_clip(P, G, B, *tab, *clip, 0.9, 1, n, st),
                           lambda: norm() or lib.dsgcn_sgd_group_step_clip_hyper(P, G, B, *tab, *clip, H, 1, n, st)),
        'adam': (lambda: lib.dsgcn_adam_step(P, G, M, V, step.data_ptr(), *tab, 0.9, 0.999, 1e-8, 1, n, st),
                 lambda: lib.dsgcn_adam_step_hyper(P, G, M, V, step.data_ptr(), *tab, H, 0.999, 1e-8, 1, n, st)),
        'adam_clip': (lambda: norm() or lib.dsgcn_adam_step_clip(P, G, M, V, step.data_ptr(), *tab, *clip, 0.9, 0.999, 1e-8, 1,
                                                                 n, st),
                      lambda: norm() or lib.dsgcn_adam_step_clip_hyper(P, G, M, V, step.data_ptr(), *tab, *clip, H, 0.999,
                                                                       1e-8, 1, n, st)),
    }
    return n, calls, keep


def time_pair(pair, reps):
    """us per launch of BLOCKS blocks per form, the two forms alternating -> ([parent], [hyper])"""
    import torch
    out = ([], [])
    for fn in pair:
        for _ in range(3):
            if fn() != 0:
                raise SystemExit('launch failed')
    torch.cuda.synchronize()
    for _ in range(BLOCKS):
        for k, fn in enumerate(pair):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) * 1e3 / reps)
    return out


def run_kernels(reps):
    import bench
    import dsgcn_amd as D
    flat = D.FlatParams(bench.build_model().cuda().train(), gather=True)
    n, calls, keep = launches(flat)
    for form in FORMS:
        a, b = time_pair(calls[form], reps)
        print(json.dumps(dict(form=form, n=n, us_parent=round(statistics.median(a), 2), us_hyper=round(statistics.median(b), 2),
                              spread_parent=round(max(a) - min(a), 2), spread_hyper=round(max(b) - min(b), 2),
                              ratio=round(statistics.median(b) / statistics.median(a), 4))), flush=True)


def run_steps(steps, warmup):
    import bench
    import torch
    import dsgcn_amd as D
    g = torch.Generator().manual_seed(1234)
    kp = torch.randn(bench.CLIPS_PER_GPU, 1, bench.M, bench.T, bench.V, bench.C, generator=g).cuda()
    lb = torch.randint(0, bench.CLASSES, (bench.CLIPS_PER_GPU, 1), generator=g).cuda()
    for name, opt in (('SGD', dict(type='SGD', lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True)),
                      ('AdamW', dict(type='AdamW', lr=1e-3, weight_decay=0.01))):
        engines = {flag: D.TrainEngine(bench.build_model().cuda().train(), optimizer=opt, use_graph=True, warmup_eager=3,
                                       scheduled_momentum=flag) for flag in (False, True)}
        for flag, eng in engines.items():
            for i in range(warmup):
                eng.step(kp, lb, lr=opt['lr'], momentum=0.9 - 0.01 * (i % 5) if flag else None)
            torch.cuda.synchronize()
            if not eng.graphed(kp, lb):
                raise SystemExit(f'{name}: capture failed: {eng.capture_error}')
        ms = {flag: [] for flag in engines}
        for _ in range(BLOCKS):
            for flag, eng in engines.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(steps):
                    eng.step(kp, lb, lr=opt['lr'], momentum=0.9 - 0.01 * (i % 5) if flag else None)
                e1.record()
                e1.synchronize()
                ms[flag].append(e0.elapsed_time(e1) / steps)
        med = {flag: statistics.median(v) for flag, v in ms.items()}
        print(json.dumps(dict(optimizer=name, ms_by_value=round(med[False], 4), ms_scheduled=round(med[True], 4),
                              spread_by_value=round(max(ms[False]) - min(ms[False]), 4),
                              spread_scheduled=round(max(ms[True]) - min(ms[True]), 4),
                              ratio=round(med[True] / med[False], 4))), flush=True)
        del engines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--steps', action='store_true')
    ap.add_argument('--reps', type=int, default=200, help='launches per timed block')
    ap.add_argument('--nsteps', type=int, default=30, help='engine steps per timed block')
    ap.add_argument('--warmup', type=int, default=8)
    args = ap.parse_args()
    import torch
    from dsgcn_amd import native
    native.lib()
    if not torch.cuda.is_available():
        raise SystemExit('lr_schedules_bench.py needs the GPU')
    if args.kernels:
        run_kernels(args.reps)
    if args.steps:
        run_steps(args.nsteps, args.warmup)


if __name__ == '__main__':
    main()
