"""Per-call time of feature / score-map extraction on a resident last-block activation: ``kernels.feat_ext``
(csrc/featext.hip, one launch) beside the framework composition the reference runs (recognizergcn.py:82-93: a chain of
``mean(keepdim=True)``, ``einsum('nmctv,oc->nmotv')`` + bias, the cast to float16), both replayed from a hipGraph and
timed in alternation; then a whole ``test_model`` extraction pass beside the scoring pass of the same model.

    python tools/feat_ext_bench.py [--iters 200] [--videos 16] [--out FILE.json]

Rows named '(plane means)' give ``feat_ext`` the (clips*M, C) plane means instead — what the recognizer does whenever
frames and joints are both pooled (``backbone(x, pool=True)``) — while the composition still reduces the activation.
Sizes: the two shipped test shapes — NTU-60 (1 video x 10 clips, M 2, C 256, T' 16, V 25, K 60) and K400 (V 17, K 400).
Also prints each form's largest difference from the composition run in fp64."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dsgcn_amd as D  # noqa: E402
from dsgcn_amd import kernels as K  # noqa: E402

SIZES = {'ntu60': dict(clips=10, M=2, C=256, T=16, V=25, K=60), 'k400': dict(clips=10, M=2, C=256, T=16, V=17, K=400)}
POOLS = ('none', 'nm', 'nmtv', 'v')          # ('v': lanes along the frames, the one form whose loads are strided)
AXES = dict(n=0, m=1, t=3, v=4)


def composition(x, pool, w, b):
    """x (clips, M, C, T, V) of one video, as the reference's branch has it"""
    if pool != 'none':
        for d in pool:
            x = x.mean(AXES[d], keepdim=True)
    if w is not None:
        x = torch.einsum('nmctv,oc->nmotv', x, w) + b[..., None, None]
    return x.to(torch.float16 if x.dtype == torch.float32 else x.dtype)


def graphed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(10):
        g.replay()
    return g


def time_pair(ga, gb, iters, rounds=5):
    """the two graphs in alternation -> (median us of a, median us of b)"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ta, tb = [], []
    for _ in range(rounds):
        for g, acc in ((ga, ta), (gb, tb)):
            t0.record()
            for _ in range(iters):
                g.replay()
            t1.record()
            torch.cuda.synchronize()
            acc.append(t0.elapsed_time(t1) * 1e3 / iters)
    return float(np.median(ta)), float(np.median(tb))


def kernel_rows(iters):
    rows = []
    for size, s in SIZES.items():
        g = torch.Generator().manual_seed(0)
        x = torch.randn(s['clips'], s['M'], s['C'], s['T'], s['V'], generator=g).cuda()
        w = (torch.randn(s['K'], s['C'], generator=g) * 0.2).cuda()
        b = (torch.randn(s['K'], generator=g) * 0.1).cuda()
        for mode in ('feat', 'score'):
            ww, bb = (w, b) if mode == 'score' else (None, None)
            for pool in POOLS:
                ours = lambda: K.feat_ext(x, 1, s['clips'], s['M'], pool, ww, bb)  # noqa: E731
                theirs = lambda: composition(x, pool, ww, bb)  # noqa: E731
                us_ours, us_theirs = time_pair(graphed(ours), graphed(theirs), iters)
                ref = composition(x.double(), pool, None if ww is None else ww.double(), None if bb is None else bb.double())
                got32 = K.feat_ext(x, 1, s['clips'], s['M'], pool, ww, bb, want_fp32=True)[1][0]
                top = ref.abs().max().item()
                e_ours = (got32.double() - ref).abs().max().item() / top
                x32 = x
                if pool != 'none':
                    for d in pool:
                        x32 = x32.mean(AXES[d], keepdim=True)
                if ww is not None:
                    x32 = torch.einsum('nmctv,oc->nmotv', x32, ww) + bb[..., None, None]
                e_theirs = (x32.double() - ref).abs().max().item() / top
                if pool == 'nmtv':
                    xm = x.mean((3, 4)).flatten(0, 1).contiguous()
                    pm = lambda: K.feat_ext(xm, 1, s['clips'], s['M'], pool, ww, bb)  # noqa: E731
                    us_pm, us_again = time_pair(graphed(pm), graphed(theirs), iters)
                    rows.append(dict(size=size, mode=mode, pool=pool + ' (plane means)', us_feat_ext=us_pm,
                                     us_composition=us_again, speedup=us_again / us_pm))
                    print(f'{size:6s} {mode:5s} {pool:5s} feat_ext {us_pm:8.2f} us   composition {us_again:8.2f} us   '
                          f'x{us_again / us_pm:5.2f}   (plane means in)', flush=True)
                rows.append(dict(size=size, mode=mode, pool=pool, us_feat_ext=us_ours, us_composition=us_theirs,
                                 speedup=us_theirs / us_ours, err_feat_ext=e_ours, err_composition=e_theirs))
                print(f'{size:6s} {mode:5s} {pool:5s} feat_ext {us_ours:8.2f} us   composition {us_theirs:8.2f} us   '
                      f'x{us_theirs / us_ours:5.2f}   fp32 error vs fp64: {e_ours:.2e} / {e_theirs:.2e}', flush=True)
    return rows


def pass_rows(videos):
    """test_model over `videos` synthetic NTU-60 test videos (10 clips x 2 persons x 64 frames), batch 4: the scoring pass
    and extraction passes of the same full-width DS-STGCN; wall time of the second pass of each kind (the first one
    captures the graphs)."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import ds_cfg
    torch.manual_seed(0)
    np.random.seed(0)
    m = D.build_model(ds_cfg(60)).cuda().eval()
    g = torch.Generator().manual_seed(1)
    data = [dict(keypoint=torch.randn(10, 2, 64, 25, 3, generator=g).numpy(), label=i % 60) for i in range(videos)]
    cfg = D.Config(dict(data=dict(test_dataloader=dict(videos_per_gpu=4))))
    rows = []
    for name, test_cfg in (('scoring', {}), ('feat_ext nmtv', dict(feat_ext=True, pool_opt='nmtv')),
                           ('feat_ext nm', dict(feat_ext=True, pool_opt='nm')),
                           ('score_ext nm', dict(score_ext=True, pool_opt='nm')),
                           ('score_ext none', dict(score_ext=True, pool_opt='none'))):
        for key in ('feat_ext', 'score_ext', 'pool_opt'):
            m.test_cfg.pop(key, None)
        m.test_cfg.update(test_cfg)
        times = []
        for _ in range(3):
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = D.test_model(m, data, cfg)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t) * 1e3)
        rows.append(dict(pass_=name, ms_first=times[0], ms_best_later=min(times[1:]), videos=videos,
                         result_shape=list(res['results'][0].shape)))
        print(f'test_model {name:16s} first pass {times[0]:8.1f} ms, later {min(times[1:]):8.1f} ms  '
              f'({videos} videos, result {tuple(res["results"][0].shape)})', flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--videos', type=int, default=16)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('feat_ext_bench measures on the GPU: none found')
    out = dict(device=torch.cuda.get_device_name(0), iters=a.iters, kernel=kernel_rows(a.iters), passes=pass_rows(a.videos))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
