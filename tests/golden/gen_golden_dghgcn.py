"""Golden fixtures for ``dghgcn``, DGSTGCN's default spatial unit (node-typed projections and edge-typed attention on every
subset), generated from the IMPORTED reference (build container only: needs the reference checkout, see ref_shim):

    python tests/golden/gen_golden_dghgcn.py

  unit_dghgcn.npz                      seven units, n = 2, T = 8: every (node_attention, edge_attention) combination,
                                       subset_wise on and off, add_type with edge attention, 64 -> 64 and 64 -> 128, one
                                       coco unit (V = 17) and one 128 -> 256 unit at ratio 0.25 (mid = 64).  Per unit: the
                                       seed, keys / shapes and digest of the constructor's state_dict (the tests rebuild the
                                       weights from the seed), the live alpha / beta, the seed and digest of the input and
                                       output probe R, and the fp64 output, input gradient and every parameter gradient:
                                       whole up to 4096 elements, as 32 fixed random projections above (tests/dghgcn_fp64.py:
                                       probe), which keeps the archive small
  model_reduced_dghgcn(.npz, _cfg.json)          the shipped DS-STGCN flags with gcn_type='dghgcn' (no decompose),
                                                 dgmstcn, at reduced width (G.reduced_model), + fp64 eval-mode logits
  model_reduced_dghgcn_default(.npz, _cfg.json)  DGSTGCN at its defaults (dghgcn + unit_tcn), reduced width, the same

Data only.  The archives are written with fixed member times, so a second run gives byte-identical files."""
import copy
import hashlib
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (ref_shim, liven, reduced_model)

sys.path.insert(0, os.path.dirname(HERE))
from dghgcn_fp64 import FULL_MAX, probe, unit_inputs  # noqa: E402  (the compact fixture form the tests read)

R = G.R

# (name, layout, Ci, Co, ratio, node_attention, edge_attention, add_type, subset_wise)
UNIT_CASES = [
    ('plain', 'nturgb+d', 64, 64, 0.25, False, False, False, False),
    ('node', 'nturgb+d', 64, 64, 0.25, True, False, False, True),
    ('edge', 'nturgb+d', 64, 128, 0.25, False, True, False, False),
    ('node_edge', 'nturgb+d', 64, 128, 0.25, True, True, False, True),
    ('add_type', 'nturgb+d', 64, 64, 0.25, True, True, True, False),
    ('coco', 'coco', 64, 64, 0.25, True, True, False, True),
    ('wide', 'nturgb+d', 128, 256, 0.25, True, False, False, True),
]


def sd_digest(module):
    """sha256 over the state_dict's keys and fp32 bytes (the constructor's weights; the tests rebuild them from the seed)"""
    h = hashlib.sha256()
    for k, v in module.state_dict().items():
        h.update(k.encode())
        h.update(v.detach().cpu().numpy().tobytes())
    return h.hexdigest()


def savez_det(path, **arrays):
    """np.savez_compressed with fixed member times (zipfile stamps the current time otherwise)."""
    with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_DEFLATED) as zf:
        for k in arrays:
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def graph(layout):
    np.random.seed(21)
    return R.graph.Graph(layout=layout, mode='random', num_filter=3, init_off=.04, init_std=.02)


def unit_dghgcn():
    out = {'cases': np.array([c[0] for c in UNIT_CASES])}
    for i, (name, layout, ci, co, ratio, na, ea, at, sw) in enumerate(UNIT_CASES):
        gr = graph(layout)
        A = torch.tensor(gr.A, dtype=torch.float32)
        V = A.shape[-1]
        node_type = torch.tensor(gr.node_type)
        edge_type = torch.tensor(gr.edge_type, dtype=torch.float32)
        seed = 500 + i
        torch.manual_seed(seed)
        m = R.gutils.dghgcn(ci, co, A, edge_type, node_type, ratio=ratio, node_attention=na, edge_attention=ea,
                            add_type=at, subset_wise=sw)
        tag = name + '_'
        out[tag + 'init_digest'] = np.array(sd_digest(m))
        out[tag + 'sd_manifest'] = np.array(json.dumps([[k, list(v.shape)] for k, v in m.state_dict().items()]))
        G.liven(m, 41 + i)
        out[tag + 'alpha'] = m.alpha.detach().numpy().copy()
        out[tag + 'beta'] = m.beta.detach().numpy().copy()
        m64 = m.double()
        x32, r32 = unit_inputs(ci, co, V, 60 + i)
        x = x32.double().requires_grad_()
        Rm = r32.double()
        y = m64(x)
        (y * Rm).sum().backward()
        out[tag + 'cfg'] = np.array([ci, co, int(na), int(ea), int(at), int(sw), seed])
        out[tag + 'input_seed'] = np.array(60 + i)
        out[tag + 'input_digest'] = np.array(hashlib.sha256(x32.numpy().tobytes() + r32.numpy().tobytes()).hexdigest())
        out[tag + 'ratio'] = np.array(ratio)
        out[tag + 'node_type'] = node_type.numpy().astype(np.int64)
        out[tag + 'edge_type'] = edge_type.numpy().astype(np.int64)

        def put(key, a):
            a = np.asarray(a, dtype=np.float64)
            if a.size <= FULL_MAX:
                out[key] = a
            else:
                out[key + '_probe'] = probe(a, key)
        put(tag + 'y', y.detach().numpy())
        put(tag + 'dx', x.grad.numpy())
        for k, p in m64.named_parameters():
            put(tag + 'grad_' + k, (p.grad if p.grad is not None else torch.zeros_like(p)).numpy())
    savez_det(os.path.join(HERE, 'unit_dghgcn.npz'), **out)


def reduced(cfg, name, seed):
    """G.reduced_model (fp32 reference run + fp64 truth, train mode) plus the fp64 eval-mode logits of the same weights."""
    save0 = np.savez_compressed
    np.savez_compressed = savez_det            # G.reduced_model writes through numpy: make its archive reproducible
    try:
        G.reduced_model(copy.deepcopy(cfg), name, seed=seed)
    finally:
        np.savez_compressed = save0
    path = os.path.join(HERE, name + '.npz')
    with np.load(path) as f:
        z = {k: f[k] for k in f.files}
    m64 = R.builder.build_model(copy.deepcopy(cfg)).double()
    m64.load_state_dict({k[3:]: torch.from_numpy(v).double() if v.dtype.kind == 'f' else torch.from_numpy(v)
                         for k, v in z.items() if k.startswith('sd_')})
    m64.eval()
    with torch.no_grad():
        logits = m64.cls_head(G.extract_feat_f64(m64, torch.from_numpy(z['x'])[:, 0].double()))
    z['logits_eval_f64'] = logits.numpy()
    savez_det(path, **z)


def reduced_models():
    small = dict(base_channels=16, num_stages=4, inflate_stages=[3], down_stages=[3])
    cfg = G.ds_cfg(num_classes=12, gcn_type='dghgcn', **small)
    del cfg['backbone']['gcn_decompose']       # dghgcn has no decompose flag
    cfg['cls_head']['in_channels'] = 32
    reduced(cfg, 'model_reduced_dghgcn', seed=8)
    cfg = dict(type='RecognizerGCN',
               backbone=dict(type='DGSTGCN',
                             graph_cfg=dict(layout='nturgb+d', mode='random', num_filter=3, init_off=.04, init_std=.02),
                             **small),
               cls_head=dict(type='GCNHead', num_classes=12, in_channels=32))
    reduced(cfg, 'model_reduced_dghgcn_default', seed=9)


if __name__ == '__main__':
    unit_dghgcn()
    reduced_models()
    print('wrote unit_dghgcn.npz, model_reduced_dghgcn(.npz, _cfg.json), model_reduced_dghgcn_default(.npz, _cfg.json)')
