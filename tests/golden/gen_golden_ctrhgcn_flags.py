"""Golden fixtures for ``unit_ctrhgcn``'s ``target_specific`` / ``full_channels`` / ``add_type`` switches, generated from
the IMPORTED reference (build container only: needs the reference checkout, see ref_shim):

    python tests/golden/gen_golden_ctrhgcn_flags.py

  unit_ctrhgcn_flags.npz                   eight units, n = 2, T = 8, live alpha / beta / bn.weight (CASES below).  Per unit:
                                           the seed, keys / shapes and digest of the constructor's state_dict (the tests
                                           rebuild the weights from the seed), the live values, the seed and digest of the
                                           input and output probe R, the fp64 output, input gradient and every parameter
                                           gradient, and the reference's own fp32 gradients (``g32_``): whole up to 512
                                           elements, as 32 fixed random projections above (tests/dghgcn_fp64.py: probe)
  model_reduced_ctrgcn_flags(.npz, _cfg.json)  the kwargs of the shipped configs/ctrgcn/CTRGCN_model.py with the three
                                           switches on and semantic_stage=[1, 2, 4], at reduced width (G.reduced_model:
                                           logits, loss, all gradients in fp32 and fp64), + fp64 eval-mode logits

Data only.  The archives are written with fixed member times, so a second run gives byte-identical files."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (ref_shim, liven, reduced_model)
from gen_golden_dghgcn import graph, reduced, savez_det, sd_digest  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
from dghgcn_fp64 import probe, unit_inputs  # noqa: E402  (the compact fixture form the tests read)

FULL_MAX = 512        # arrays up to this size are kept whole (fixture_rel reads either form): keeps the archive under 1 MiB

R = G.R

# (name, layout, Ci, Co, semantic_index, edge_attention, target_specific, full_channels, add_type, ada)
CASES = [
    ('ts', 'nturgb+d', 64, 64, True, False, True, False, False, False),
    ('full', 'nturgb+d', 64, 64, True, True, False, True, False, False),
    ('add', 'nturgb+d', 64, 64, True, True, False, False, True, False),
    ('full_add', 'nturgb+d', 64, 64, True, True, False, True, True, False),
    ('all', 'nturgb+d', 64, 128, True, True, True, True, True, True),
    ('first', 'nturgb+d', 3, 64, True, True, True, True, True, False),
    ('coco', 'coco', 64, 64, True, True, True, True, True, False),
    ('inert', 'nturgb+d', 64, 64, False, True, True, True, True, False),
]


def liven_unit(m, seed):
    """alpha, beta (G.liven) and bn.weight (the constructor leaves 1: any error in front of the BatchNorm would hide)"""
    G.liven(m, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        m.bn.weight.copy_(0.5 + torch.rand(m.bn.weight.shape, generator=g, dtype=torch.float64).to(m.bn.weight.dtype))


def units():
    out = {'cases': np.array([c[0] for c in CASES])}
    for i, (name, layout, ci, co, sem, ea, ts, full, add, ada) in enumerate(CASES):
        gr = graph(layout)
        A = torch.tensor(gr.A, dtype=torch.float32)
        V = A.shape[-1]
        node_type = torch.tensor(gr.node_type)
        edge_type = torch.tensor(gr.edge_type, dtype=torch.float32)
        seed = 700 + i
        torch.manual_seed(seed)
        m = R.gutils.unit_ctrhgcn(ci, co, A, edge_type, node_type, semantic_index=sem, edge_attention=ea,
                                  target_specific=ts, full_channels=full, add_type=add, ada=ada)
        tag = name + '_'
        out[tag + 'init_digest'] = np.array(sd_digest(m))
        out[tag + 'sd_manifest'] = np.array(json.dumps([[k, list(v.shape)] for k, v in m.state_dict().items()]))
        liven_unit(m, 51 + i)
        out[tag + 'alpha'] = m.alpha.detach().numpy().copy()
        out[tag + 'bn_weight'] = m.bn.weight.detach().numpy().copy()
        if ada:
            out[tag + 'beta'] = np.array([float(c.beta.detach()) for c in m.convs], dtype=np.float32)
        out[tag + 'cfg'] = np.array([ci, co, int(sem), int(ea), int(ts), int(full), int(add), int(ada), seed])
        out[tag + 'input_seed'] = np.array(80 + i)
        x32, r32 = unit_inputs(ci, co, V, 80 + i)
        out[tag + 'input_digest'] = np.array(hashlib.sha256(x32.numpy().tobytes() + r32.numpy().tobytes()).hexdigest())
        out[tag + 'node_type'] = node_type.numpy().astype(np.int64)
        out[tag + 'edge_type'] = edge_type.numpy().astype(np.int64)

        def put(key, a):
            a = np.asarray(a, dtype=np.float64)
            if a.size <= FULL_MAX:
                out[key] = a
            else:
                out[key + '_probe'] = probe(a, key)

        # the reference's own fp32 run
        x = x32.clone().requires_grad_()
        (m(x) * r32).sum().backward()
        put(tag + 'g32_dx', x.grad.numpy())
        for k, p in m.named_parameters():
            put(tag + 'g32_' + k, (p.grad if p.grad is not None else torch.zeros_like(p)).numpy())
        # fp64 truth
        m.zero_grad(set_to_none=True)
        m64 = m.double()
        x = x32.double().requires_grad_()
        y = m64(x)
        (y * r32.double()).sum().backward()
        put(tag + 'y', y.detach().numpy())
        put(tag + 'dx', x.grad.numpy())
        for k, p in m64.named_parameters():
            put(tag + 'grad_' + k, (p.grad if p.grad is not None else torch.zeros_like(p)).numpy())
    savez_det(os.path.join(HERE, 'unit_ctrhgcn_flags.npz'), **out)


def reduced_model():
    backbone = dict(type='CTRGCN', gcn_type='unit_ctrhgcn', gcn_node_attention=True, gcn_edge_attention=True,
                    gcn_target_specific=True, gcn_full_channels=True, gcn_add_type=True, gcn_ada=True, gcn_num_types=5,
                    gcn_rel_reduction=8, gcn_edge_num=15, tcn_type='msmlp', tcn_add_tcn=True, tcn_merge_after=True,
                    semantic_stage=[1, 2, 4],
                    graph_cfg=dict(layout='nturgb+d', mode='random', num_filter=3, init_off=.04, init_std=.02),
                    base_channels=16, num_stages=4, inflate_stages=[3], down_stages=[3])
    cfg = dict(type='RecognizerGCN', backbone=backbone, cls_head=dict(type='GCNHead', num_classes=12, in_channels=32))
    reduced(cfg, 'model_reduced_ctrgcn_flags', seed=10)


if __name__ == '__main__':
    units()
    reduced_model()
    print('wrote unit_ctrhgcn_flags.npz, model_reduced_ctrgcn_flags(.npz, _cfg.json)')
