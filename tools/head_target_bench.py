"""Per-call time of the head's forward + backward: ``kernels.head_loss`` (csrc/head.hip) beside the three modes of
``kernels.head_target`` (csrc/head_target.hip) at one shape, replayed from a hipGraph (the way the training step runs
them: launch overhead on the device, none on the host).

    python tools/head_target_bench.py [--shape N M C K] [--iters 200] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dsgcn_amd import kernels as K  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, nargs=4, default=[64, 2, 256, 60])
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    N, M, C, Kc = a.shape
    g = torch.Generator().manual_seed(0)
    feat = torch.randn(N * M, C, generator=g).cuda().requires_grad_()
    w = (torch.randn(Kc, C, generator=g) * 0.2).cuda().requires_grad_()
    b = (torch.randn(Kc, generator=g) * 0.1).cuda().requires_grad_()
    hard = torch.randint(0, Kc, (N,), generator=g).cuda()
    soft = torch.softmax(torch.randn(N, Kc, generator=g), 1).cuda()
    multi = (torch.rand(N, Kc, generator=g) < 0.3).float().cuda()
    cw = (torch.rand(Kc, generator=g) + 0.5).cuda()
    seed = torch.ones((), device='cuda')
    variants = {
        'head_loss': lambda: K.head_loss(feat, w, b, hard, M, 1.0)[0],
        'head_target mode 0 (class weights)': lambda: K.head_target(feat, w, b, hard, M, 0, cw)[0],
        'head_target mode 1 (soft labels)': lambda: K.head_target(feat, w, b, soft, M, 1, None)[0],
        'head_target mode 1 (soft labels, class weights)': lambda: K.head_target(feat, w, b, soft, M, 1, cw)[0],
        'head_target mode 2 (BCE, class weights)': lambda: K.head_target(feat, w, b, multi, M, 2, cw)[0],
    }
    res = {}
    for name, fn in variants.items():
        def fwd_bwd():
            feat.grad = w.grad = b.grad = None
            fn().backward(seed)
        for _ in range(3):
            fwd_bwd()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fwd_bwd()
        for _ in range(10):
            graph.replay()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = []
        for _ in range(5):
            t0.record()
            for _ in range(a.iters):
                graph.replay()
            t1.record()
            torch.cuda.synchronize()
            best.append(t0.elapsed_time(t1) * 1e3 / a.iters)
        res[name] = dict(us_per_call_median=sorted(best)[2], us_per_call_min=min(best))
        print(f'{name:50s} {sorted(best)[2]:8.2f} us / forward + backward (min {min(best):.2f})', flush=True)
    out = dict(shape=a.shape, iters=a.iters, device=torch.cuda.get_device_name(0), results=res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
