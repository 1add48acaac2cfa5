"""Same-box A/B of dghgcn (typed K-B on all subsets, csrc/dynadj_typed.hip) against the shipped dgphgcn1 (K-B,
csrc/dynadj.hip):

  step    one 64-clip DS-STGCN training step (TrainEngine, hipGraph replay) with gcn_type='dgphgcn1' (bench.py's model) and
          with gcn_type='dghgcn' (the same flags, no decompose), ratio 0.125; blocks of `--steps` replays, the two models
          interleaved `--blocks` times, median per model
  kb      the adjacency alone, forward + backward, at n = 128, V = 25 on every width of the net: dgphgcn1.adjacency against
          dghgcn.adjacency (projections, select, edge linear and typed K-B), plus the typed K-B launches alone and their
          bandwidth against the Ahat bytes (written forward, read backward)

    python tools/dghgcn_ab.py [--steps 20] [--blocks 5] [--out FILE.json]
Prints one JSON document (and writes it to --out)."""
import copy
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
import dsgcn_amd as D
from dsgcn_amd import kernels as K
from dsgcn_amd import native


def dgh_cfg():
    cfg = bench.ds_cfg()
    cfg['backbone']['gcn_type'] = 'dghgcn'
    del cfg['backbone']['gcn_decompose']
    return cfg


def live_model(cfg, seed=0):
    np.random.seed(seed)
    torch.manual_seed(seed)
    m = D.build_model(copy.deepcopy(cfg))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith(('alpha', 'beta', 'add_coeff')):
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
    return m.cuda().train()


def time_block(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def step_ab(steps, blocks):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(64, 1, bench.M, bench.T, bench.V, bench.C, generator=g).cuda()
    y = torch.randint(0, bench.CLASSES, (64, 1), generator=g).cuda()
    engines = {}
    for name, cfg in (('dgphgcn1', bench.ds_cfg()), ('dghgcn', dgh_cfg())):
        eng = D.TrainEngine(live_model(cfg), lr=0.01, use_graph=True, warmup_eager=2)
        for _ in range(5):
            eng.step(x, y)
        torch.cuda.synchronize()
        assert eng.graphed(x, y), eng.capture_error
        engines[name] = eng
    ms = {name: [] for name in engines}
    for _ in range(blocks):
        for name, eng in engines.items():
            ms[name].append(time_block(lambda: eng.step(x, y), steps))
    med = {name: statistics.median(v) for name, v in ms.items()}
    return dict(blocks_ms=ms, median_ms=med, ratio=med['dghgcn'] / med['dgphgcn1'])


def kb_ab(reps, blocks):
    out = []
    gr = D.Graph(layout='nturgb+d', mode='spatial')
    torch.manual_seed(0)
    np.random.seed(0)
    A = torch.tensor(np.asarray(D.Graph(layout='nturgb+d', mode='random', num_filter=3, init_off=.04, init_std=.02).A),
                     dtype=torch.float32)
    n, V = 128, 25
    et, nt = torch.tensor(gr.edge_type), torch.tensor(gr.node_type)
    for ci, co in ((64, 64), (64, 128), (128, 128), (128, 256), (256, 256)):
        units = {
            'dgphgcn1': D.dgphgcn1(ci, co, A, et, nt, ratio=0.125, decompose=True, node_attention=True,
                                   edge_attention=True, subset_wise=True).cuda(),
            'dghgcn': D.dghgcn(ci, co, A, et, nt, ratio=0.125, node_attention=True, edge_attention=True,
                               subset_wise=True).cuda()}
        for u in units.values():
            with torch.no_grad():
                u.alpha.normal_(0, 0.5)
                u.beta.normal_(0, 0.5)
        xbar = torch.randn(n, ci, 32, device='cuda')
        xbar[..., V:] = 0
        mid = units['dghgcn'].mid_channels
        dah = torch.randn(n, 3 * mid, V, V, device='cuda')

        def run(u):
            for p in u.parameters():
                p.grad = None
            (u.adjacency(xbar) * dah).sum().backward()
        ms = {k: [] for k in units}
        for u in units.values():
            run(u)
        for _ in range(blocks):
            for k, u in units.items():
                ms[k].append(time_block(lambda: run(u), reps))
        # the typed K-B launches alone (forward, backward) on the unit's own operands
        u = units['dghgcn']
        with torch.no_grad():
            w = u.edge_linears.weight.flatten(1)
            x12 = torch.randn(n, 3 * mid, 2, 32, device='cuda')
            x12[..., V:] = 0
            pq = K.pwconv(x12, None, None, None, False, w, None, 1, False)[0]
        lib = native.lib()
        ahat = torch.empty(n, 3 * mid, V, V, device='cuda')
        E = u.edge_num
        st = torch.cuda.current_stream().cuda_stream
        ptr = lambda t: t.data_ptr()
        fwd = lambda: lib.dsgcn_dyntyped_fwd(ptr(x12), ptr(pq), ptr(u.edge_linears.bias), ptr(u.A), ptr(u.alpha),
                                             ptr(u.beta), ptr(u.edge_type_idx), ptr(ahat), n, mid, V, E, 1, st)
        pstride = lib.dsgcn_dyntyped_partial_stride(mid, V, E, 1)
        dd, dx12, dpq = torch.empty_like(ahat), torch.empty_like(x12), torch.empty_like(pq)
        ppar = torch.empty(n, pstride, device='cuda')
        bwd = lambda: lib.dsgcn_dyntyped_bwd(ptr(x12), ptr(pq), ptr(u.edge_linears.bias), ptr(u.alpha), ptr(u.beta),
                                             ptr(u.edge_type_idx), ptr(dah), ptr(dd), ptr(dx12), ptr(dpq), ptr(ppar),
                                             pstride, n, mid, V, E, 1, st)
        assert fwd() == 0 and bwd() == 0
        tf = statistics.median(time_block(fwd, reps) for _ in range(blocks))
        tb = statistics.median(time_block(bwd, reps) for _ in range(blocks))
        nbytes = ahat.numel() * 4
        med = {k: statistics.median(v) for k, v in ms.items()}
        out.append(dict(ci=ci, co=co, mid=mid, n=n, blocks_ms=ms, median_ms=med, ratio=med['dghgcn'] / med['dgphgcn1'],
                        typed_kb_fwd_us=tf * 1e3, typed_kb_bwd_us=tb * 1e3, ahat_MB=nbytes / 1e6,
                        fwd_GBps_ahat_write=nbytes / (tf * 1e-3) / 1e9, bwd_GBps_dahat_read=nbytes / (tb * 1e-3) / 1e9))
    return out


def main():
    args = sys.argv[1:]
    steps = int(args[args.index('--steps') + 1]) if '--steps' in args else 20
    blocks = int(args[args.index('--blocks') + 1]) if '--blocks' in args else 5
    out_path = args[args.index('--out') + 1] if '--out' in args else None
    res = dict(device=torch.cuda.get_device_name(0), step=step_ab(steps, blocks), kb=kb_ab(steps, blocks))
    text = json.dumps(res, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
