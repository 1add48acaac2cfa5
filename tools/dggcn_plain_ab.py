"""Same-box figures for the plain K-B (csrc/dynadj_plain.hip, dggcn at any number of subsets):

  pair    the adjacency path alone, forward + backward, at K = 3, n = 128, V = 25 on the six (Ci, Co) of the 10-stage
          model, ratio 0.125: dggcn.adjacency (two dsgcn_dynadj launches with the typed slots fed constants, and a
          concatenation) against one kernels.dynadj_plain call on the same weights
  kb8     the plain K-B launches alone at K = 8, ratio 0.125 (and the 256-channel layer at 0.25): time forward and
          backward, and the Ahat bytes (written forward, read backward) over that time against 8 TB/s
  step    one 64-clip DG-STGCN training step (TrainEngine, hipGraph replay) at K = 8 next to K = 3

    python tools/dggcn_plain_ab.py [--steps 20] [--blocks 5] [--out FILE.json]
Blocks of `--steps` calls, the arms interleaved `--blocks` times, median per arm.  Prints one JSON document (and writes
it to --out)."""
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

HBM_BPS = 8e12
WIDTHS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256))


def dg_cfg(num_filter):
    cfg = bench.other_cfg('dggcn')
    cfg['backbone']['graph_cfg'] = dict(cfg['backbone']['graph_cfg'], num_filter=num_filter)
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


def graph_A(num_filter):
    np.random.seed(0)
    g = D.Graph(layout='nturgb+d', mode='random', num_filter=num_filter, init_off=.04, init_std=.02)
    return torch.tensor(np.asarray(g.A), dtype=torch.float32)


def pair_ab(reps, blocks):
    out = []
    n, V = 128, 25
    for ci, co in WIDTHS:
        torch.manual_seed(0)
        u = D.dggcn(ci, co, graph_A(3), ratio=0.125, subset_wise=True).cuda()
        with torch.no_grad():
            u.alpha.normal_(0, 0.5)
            u.beta.normal_(0, 0.5)
        xbar = torch.randn(n, ci, 32, device='cuda')
        xbar[..., V:] = 0
        dah = torch.randn(n, 3 * u.mid_channels, V, V, device='cuda')

        def old():
            return u.adjacency(xbar)

        def new():
            return K.dynadj_plain(xbar, u.A, u.alpha, u.beta, u.conv1.weight.flatten(1), u.conv1.bias,
                                  u.conv2.weight.flatten(1), u.conv2.bias)

        def run(fn):
            for p in u.parameters():
                p.grad = None
            fn().backward(dah)
        arms = dict(two_launch=old, plain=new)
        ms = {k: [] for k in arms}
        for fn in arms.values():
            run(fn)
        for _ in range(blocks):
            for k, fn in arms.items():
                ms[k].append(time_block(lambda: run(fn), reps))
        med = {k: statistics.median(v) for k, v in ms.items()}
        out.append(dict(ci=ci, co=co, mid=u.mid_channels, n=n, blocks_ms=ms, median_ms=med,
                        ratio=med['plain'] / med['two_launch']))
    return out


def kb8(reps, blocks):
    out = []
    n, V, Kk = 128, 25, 8
    lib = native.lib()
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr()
    for co, ratio in ((64, 0.125), (128, 0.125), (256, 0.125), (256, 0.25)):
        mid = int(ratio * co)
        proj = torch.randn(n, 2 * Kk * mid, 32, device='cuda')
        proj[..., V:] = 0
        A = graph_A(Kk).cuda()
        alpha, beta = torch.randn(Kk, device='cuda') * 0.5, torch.randn(Kk, device='cuda') * 0.5
        ahat = torch.empty(n, Kk * mid, V, V, device='cuda')
        dah = torch.randn_like(ahat)
        dproj = torch.empty_like(proj)
        pstride = lib.dsgcn_dynplain_partial_stride(Kk, V)
        ppar = torch.empty(n, pstride, device='cuda')
        fwd = lambda: lib.dsgcn_dynplain_fwd(ptr(proj), ptr(A), ptr(alpha), ptr(beta), ptr(ahat), n, Kk, mid, V, 32, st)
        bwd = lambda: lib.dsgcn_dynplain_bwd(ptr(proj), ptr(alpha), ptr(beta), ptr(dah), ptr(dproj), ptr(ppar), pstride, n,
                                             Kk, mid, V, 32, st)
        assert fwd() == 0 and bwd() == 0
        torch.cuda.synchronize()
        tf = statistics.median(time_block(fwd, reps) for _ in range(blocks))
        tb = statistics.median(time_block(bwd, reps) for _ in range(blocks))
        nbytes = ahat.numel() * 4
        out.append(dict(co=co, ratio=ratio, mid=mid, n=n, K=Kk, ahat_MB=nbytes / 1e6, fwd_us=tf * 1e3, bwd_us=tb * 1e3,
                        fwd_GBps_ahat_write=nbytes / (tf * 1e-3) / 1e9, bwd_GBps_dahat_read=nbytes / (tb * 1e-3) / 1e9,
                        fwd_fraction_of_8TBps=nbytes / (tf * 1e-3) / HBM_BPS,
                        bwd_fraction_of_8TBps=nbytes / (tb * 1e-3) / HBM_BPS))
    return out


def step_ab(steps, blocks):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(64, 1, bench.M, bench.T, bench.V, bench.C, generator=g).cuda()
    y = torch.randint(0, bench.CLASSES, (64, 1), generator=g).cuda()
    engines = {}
    for name, nf in (('k3', 3), ('k8', 8)):
        eng = D.TrainEngine(live_model(dg_cfg(nf)), lr=0.01, use_graph=True, warmup_eager=2)
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
    return dict(blocks_ms=ms, median_ms=med, ratio=med['k8'] / med['k3'])


def main():
    args = sys.argv[1:]
    steps = int(args[args.index('--steps') + 1]) if '--steps' in args else 20
    blocks = int(args[args.index('--blocks') + 1]) if '--blocks' in args else 5
    out_path = args[args.index('--out') + 1] if '--out' in args else None
    with open(native.LIB_PATH + '.srchash') as f:
        srchash = f.read().strip()
    res = dict(device=torch.cuda.get_device_name(0), srchash=srchash, pair=pair_ab(steps, blocks), kb8=kb8(steps, blocks),
               step=step_ab(steps, blocks))
    text = json.dumps(res, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
