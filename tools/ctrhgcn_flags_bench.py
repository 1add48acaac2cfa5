"""The position-typed 1x1 conv (csrc/typedconv.hip) next to the composition it replaces, and the shipped CTR-GCN step with
the three ``unit_ctrhgcn`` switches on next to the plain shipped step:

  node    per layer shape of the shipped CTR-GCN (n = 128): ``kernels.typed_conv`` over the three stacked subsets
          (x (n, Ci, T, 25), W (5, 3 Co, Ci)) against ``pwconv`` to 5 * 3 Co channels + the per-joint gather + ``pwconv``
          conv3 + the add — the reference's ``target_specific`` arm built from ops of this tree
  edge    the same for the edge-typed conv of subset 0 (d (n, R, 25, 25), W (15, Co, R)) against ``pwconv`` to 15 Co
          channels + the edge select (``_EdgeSelect``) — the reference's ``full_channels`` arm
          each: forward alone and forward + both gradients, the two sides alternating in one process, median of `--blocks`
          blocks of `--reps` calls with the spread (min .. max), and the bytes each side moves (algorithmic: every operand
          and result once, the composition's wide intermediate written and read back)
  step    one 64-clip training step (TrainEngine, hipGraph replay) of the shipped config and of the same config with
          target_specific + full_channels + add_type, interleaved

    python tools/ctrhgcn_flags_bench.py [--reps 10] [--blocks 5] [--out FILE.json] [--skip-step]
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

N, V, P, E, KS = 128, 25, 5, 15, 3
# (Ci, Co, T at the spatial unit, how many of the ten blocks)
LAYERS = [(3, 64, 64, 1), (64, 64, 64, 3), (64, 128, 64, 1), (128, 128, 32, 2), (128, 256, 32, 1), (256, 256, 16, 2)]


def time_block(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def ab(sides, reps, blocks):
    """sides: name -> callable; alternating blocks -> name -> dict(median_ms, min_ms, max_ms)"""
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(blocks):
        for k, fn in sides.items():
            ms[k].append(time_block(fn, reps))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in ms.items()}


def leaf(*shape, scale=1.0):
    return (torch.randn(*shape, device='cuda') * scale).requires_grad_()


def fwd_bwd(make, dy, leaves):
    def run():
        for t in leaves:
            t.grad = None
        make().backward(dy)
    return run


def fwd_only(make):
    def run():
        with torch.no_grad():
            make()
    return run


def node_case(ci, co, T, reps, blocks):
    g = D.Graph(layout='nturgb+d', mode='spatial')
    table = torch.as_tensor(np.asarray(g.node_type).astype(np.int32)).cuda()
    plan = K.typed_plan(table, P)
    plan = plan.on(plan.tensor.cuda())
    KC = KS * co
    x, w3, b3 = leaf(N, ci, T, V), leaf(KC, ci, scale=ci ** -.5), leaf(KC, scale=.1)
    wn, bn = leaf(P * KC, ci, scale=ci ** -.5), leaf(P * KC, scale=.1)          # row p*KC + o
    dy = torch.randn(N, KC, T, V, device='cuda')
    idx = (table.long().view(1, 1, 1, 1, V)).expand(N, 1, KC, T, V)

    def typed():
        return K.typed_conv(x, w3.unsqueeze(0) + wn.view(P, KC, ci), b3.unsqueeze(0) + bn.view(P, KC), table, P, plan)

    def composed():
        wide = K.pwconv(x, None, None, None, False, wn, bn, 1, False)[0].view(N, P, KC, T, V)
        return K.pwconv(x, None, None, None, False, w3, b3, 1, False)[0] + torch.gather(wide, 1, idx)[:, 0]

    leaves = [x, w3, b3, wn, bn]
    res = dict(kind='node', ci=ci, co=co, T=T, rows=KC)
    res['fwd'] = ab(dict(typed=fwd_only(typed), composed=fwd_only(composed)), reps, blocks)
    res['fwd_bwd'] = ab(dict(typed=fwd_bwd(typed, dy, leaves), composed=fwd_bwd(composed, dy, leaves)), reps, blocks)
    xb, yb, wide = N * ci * T * V * 4, N * KC * T * V * 4, N * P * KC * T * V * 4
    wb = (P + 1) * KC * (ci + 1) * 4
    # typed: fwd x + W -> y; bwd dy + x + W -> dx, dW.  composed: + the wide tensor written and read (fwd), its gradient
    # written and read (bwd), conv3's output written and read by the add
    res['bytes_MB'] = dict(typed_fwd=(xb + wb + yb) / 1e6, typed_fwd_bwd=(xb + wb + yb + 2 * yb + 2 * xb + 2 * wb) / 1e6,
                           composed_fwd=(2 * xb + wb + 2 * wide + 3 * yb) / 1e6,
                           composed_fwd_bwd=(2 * xb + wb + 2 * wide + 3 * yb + 2 * wide + 2 * wide + 4 * xb + 2 * wb +
                                             3 * yb) / 1e6)
    return res


def edge_case(ci, co, reps, blocks):
    R = 8 if ci <= 16 else ci // 8
    g = D.Graph(layout='nturgb+d', mode='spatial')
    table = torch.as_tensor(np.asarray(g.edge_type).reshape(-1).astype(np.int32)).cuda()
    plan = K.typed_plan(table, E)
    plan = plan.on(plan.tensor.cuda())
    d, we, be = leaf(N, R, V, V), leaf(E * co, R, scale=R ** -.5), leaf(E * co, scale=.1)     # row e*co + o
    dy = torch.randn(N, co, V, V, device='cuda')

    def typed():
        return K.typed_conv(d, we.view(E, co, R), be.view(E, co), table, E, plan)

    def composed():
        return K._EdgeSelect.apply(K.pwconv(d, None, None, None, False, we, be, 1, False)[0], table, co)

    leaves = [d, we, be]
    res = dict(kind='edge', ci=ci, co=co, R=R, rows=co)
    res['fwd'] = ab(dict(typed=fwd_only(typed), composed=fwd_only(composed)), reps, blocks)
    res['fwd_bwd'] = ab(dict(typed=fwd_bwd(typed, dy, leaves), composed=fwd_bwd(composed, dy, leaves)), reps, blocks)
    xb, yb, wide, wb = N * R * V * V * 4, N * co * V * V * 4, N * E * co * V * V * 4, E * co * (R + 1) * 4
    res['bytes_MB'] = dict(typed_fwd=(xb + wb + yb) / 1e6, typed_fwd_bwd=(xb + wb + yb + 2 * yb + 2 * xb + 2 * wb) / 1e6,
                           composed_fwd=(xb + wb + 2 * wide + yb) / 1e6,
                           composed_fwd_bwd=(xb + wb + 2 * wide + yb + yb + 2 * wide + 2 * xb + 2 * wb) / 1e6)
    return res


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


def step_ab(steps, blocks):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(64, 1, bench.M, bench.T, bench.V, bench.C, generator=g).cuda()
    y = torch.randint(0, bench.CLASSES, (64, 1), generator=g).cuda()
    cfgs = dict(shipped=bench.other_cfg('ctrgcn_shipped'),
                switches_on=bench.other_cfg('ctrgcn_shipped', gcn_target_specific=True, gcn_full_channels=True,
                                            gcn_add_type=True))
    engines = {}
    for name, cfg in cfgs.items():
        eng = D.TrainEngine(live_model(cfg), lr=0.01, use_graph=True, warmup_eager=2)
        for _ in range(5):
            eng.step(x, y)
        torch.cuda.synchronize()
        assert eng.graphed(x, y), eng.capture_error
        engines[name] = eng
    res = ab({name: (lambda e=eng: e.step(x, y)) for name, eng in engines.items()}, steps, blocks)
    res['ratio'] = res['switches_on']['median_ms'] / res['shipped']['median_ms']
    res['parameters'] = {name: sum(p.numel() for p in eng.model.parameters()) for name, eng in engines.items()}
    return res


def main():
    args = sys.argv[1:]
    reps = int(args[args.index('--reps') + 1]) if '--reps' in args else 10
    blocks = int(args[args.index('--blocks') + 1]) if '--blocks' in args else 5
    out_path = args[args.index('--out') + 1] if '--out' in args else None
    res = dict(device=torch.cuda.get_device_name(0), n=N, reps=reps, blocks=blocks, layers=[])
    for ci, co, T, count in LAYERS:
        for case in (node_case(ci, co, T, reps, blocks), edge_case(ci, co, reps, blocks)):
            case['blocks_of_ten'] = count
            res['layers'].append(case)
            r = case['fwd_bwd']
            print(f"# {case['kind']} {ci}->{co}: typed {r['typed']['median_ms']:.3f} ms, composed "
                  f"{r['composed']['median_ms']:.3f} ms (forward + gradients)", file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    if '--skip-step' not in args:
        res['step'] = step_ab(reps, blocks)
    text = json.dumps(res, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
