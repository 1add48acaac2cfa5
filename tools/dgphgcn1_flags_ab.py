"""Same-box cost of the dgphgcn1 ablation arms (flag-specialised K-B, csrc/dynadj_flags.hip) next to the shipped flag set
(K-B, csrc/dynadj.hip):

  step    one 64-clip DS-STGCN training step (TrainEngine, hipGraph replay) per arm: shipped, node attention off, edge
          attention off, gcn_stage=[1,3,5,7,9], decompose off, ada_attention on, and — lab switch of this tool only — the
          edge-attention-off arm routed through today's K-B with an identity edge linear over one class (the dggcn trick);
          blocks of `--steps` replays, the arms interleaved `--blocks` times, median per arm
  kb      the adjacency alone (projections + K-B), forward + backward, n = 128, V = 25, per width of the net: shipped
          K-B, the new K-B with edge attention off, and the identity-weights route

    python tools/dgphgcn1_flags_ab.py [--steps 20] [--blocks 5] [--out FILE.json] [--only step|kb]
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
from dghgcn_ab import live_model, time_block

ARMS = {
    'shipped': {},
    'node_off': dict(gcn_node_attention=False),
    'edge_off': dict(gcn_edge_attention=False),
    'stage_odd': dict(gcn_stage=[1, 3, 5, 7, 9]),
    'decompose_off': dict(gcn_decompose=False),
    'ada': dict(gcn_ada_attention=True),
}


def identity_route(unit):
    """Lab switch: the edge-attention-off unit on today's K-B, its subset-1 edge linear fed the identity over one class."""
    mid = unit.mid_channels
    V = unit.A.shape[-1]
    eye = torch.eye(mid, device=unit.A.device)
    zb = torch.zeros(mid, device=unit.A.device)
    et0 = torch.zeros(V, V, dtype=torch.int32, device=unit.A.device)

    def adjacency(xbar, host=None):
        c1, c2, cs = unit.conv1, unit.conv2, unit.conv1_se
        return K.dynadj(xbar, unit.A, unit.alpha, unit.beta, c1.weight.flatten(1), c1.bias, c2.weight.flatten(1), c2.bias,
                        cs.weight.flatten(1), cs.bias, eye, zb, unit.node_type_idx, et0)
    unit.adjacency = adjacency


def arm_cfg(bk):
    cfg = bench.ds_cfg()
    cfg['backbone'].update(bk)
    return cfg


def step_ab(steps, blocks):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(64, 1, bench.M, bench.T, bench.V, bench.C, generator=g).cuda()
    y = torch.randint(0, bench.CLASSES, (64, 1), generator=g).cuda()
    engines = {}
    for name in list(ARMS) + ['edge_off_identity']:
        m = live_model(arm_cfg(ARMS.get(name, ARMS['edge_off'])))
        if name == 'edge_off_identity':
            for b in m.backbone.gcn:
                identity_route(b.gcn)
        eng = D.TrainEngine(m, lr=0.01, use_graph=True, warmup_eager=2)
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
    return dict(blocks_ms=ms, median_ms=med, vs_shipped={k: v / med['shipped'] for k, v in med.items()})


def kb_ab(reps, blocks):
    out = []
    gr = D.Graph(layout='nturgb+d', mode='spatial')
    torch.manual_seed(0)
    np.random.seed(0)
    A = torch.tensor(np.asarray(D.Graph(layout='nturgb+d', mode='random', num_filter=3, init_off=.04, init_std=.02).A),
                     dtype=torch.float32)
    n, V = 128, 25
    et, nt = torch.tensor(gr.edge_type), torch.tensor(gr.node_type)
    on = dict(ratio=0.125, decompose=True, node_attention=True, subset_wise=True)
    for ci, co in ((64, 64), (64, 128), (128, 128), (128, 256), (256, 256)):
        units = {'shipped': D.dgphgcn1(ci, co, A, et, nt, edge_attention=True, **on).cuda(),
                 'edge_off': D.dgphgcn1(ci, co, A, et, nt, edge_attention=False, **on).cuda(),
                 'edge_off_identity': D.dgphgcn1(ci, co, A, et, nt, edge_attention=False, **on).cuda()}
        identity_route(units['edge_off_identity'])
        for u in units.values():
            with torch.no_grad():
                u.alpha.normal_(0, 0.5)
                u.beta.normal_(0, 0.5)
        xbar = torch.randn(n, ci, 32, device='cuda')
        xbar[..., V:] = 0
        dah = torch.randn(n, 3 * units['shipped'].mid_channels, V, V, device='cuda')

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
        med = {k: statistics.median(v) * 1e3 for k, v in ms.items()}
        out.append(dict(ci=ci, co=co, mid=units['shipped'].mid_channels, n=n, median_us=med,
                        new_vs_identity=med['edge_off'] / med['edge_off_identity']))
    return out


def main():
    args = sys.argv[1:]
    steps = int(args[args.index('--steps') + 1]) if '--steps' in args else 20
    blocks = int(args[args.index('--blocks') + 1]) if '--blocks' in args else 5
    out_path = args[args.index('--out') + 1] if '--out' in args else None
    only = args[args.index('--only') + 1] if '--only' in args else None
    res = dict(device=torch.cuda.get_device_name(0))
    if only in (None, 'step'):
        res['step'] = step_ab(steps, blocks)
    if only in (None, 'kb'):
        res['kb'] = kb_ab(steps, blocks)
    text = json.dumps(res, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
