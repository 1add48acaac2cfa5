"""Golden fixtures for the ``dgphgcn1`` switches (the DS-GCN ablation arms) and ``DGSTGCN(gcn_stage=[...])``, generated
from the IMPORTED reference (build container only: needs the reference checkout, see ref_shim):

    python tests/golden/gen_golden_ablation.py [--out DIR]

  unit_dgphgcn1_flags.npz      the units of UNIT_CASES, n = 2, T = 8: the eight (decompose, node_attention, edge_attention)
                               combinations, subset_wise / sub_att / stage off, add_type on, ada_attention with decompose on
                               and off, a 64 -> 128 unit with `down`, a coco unit (V = 17) and a 128 -> 256 unit.  Per unit,
                               in the compact form of tests/dghgcn_fp64.py: the seed, keys / shapes and digest of the
                               constructor's state_dict (the tests rebuild the weights from the seed), the live alpha /
                               beta, the seed and digest of the input and the output probe R, and the fp64 output, input
                               gradient and every parameter gradient (whole up to 512 elements, 32 fixed random
                               projections above)
  model_reduced_ds_<arm>(.npz, _cfg.json)   reduced-width DS-STGCN models, one per arm of MODEL_ARMS: weights, input,
                               labels, and the fp64 train-mode logits / loss / gradients and eval-mode logits

Data only.  The archives are written with fixed member times, so a second run gives byte-identical files."""
import copy
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (ref_shim, liven, ds_cfg)
from gen_golden_dghgcn import graph, savez_det, sd_digest  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
from dghgcn_fp64 import probe, unit_inputs  # noqa: E402  (the compact fixture form the tests read)

FULL_MAX = 512      # arrays up to this many elements are kept whole (seventeen units: a lower bar than unit_dghgcn.npz's)

R = G.R

SHIPPED = dict(decompose=True, node_attention=True, edge_attention=True, subset_wise=True)


def _dne(d, n, e):
    return dict(decompose=d, node_attention=n, edge_attention=e, subset_wise=True)


# (name, layout, Ci, Co, ratio, constructor flags)
UNIT_CASES = [(f'd{int(d)}n{int(n)}e{int(e)}', 'nturgb+d', 64, 64, 0.125, _dne(d, n, e))
              for d in (False, True) for n in (False, True) for e in (False, True)]
UNIT_CASES += [
    ('subset_off', 'nturgb+d', 64, 64, 0.125, dict(SHIPPED, subset_wise=False)),
    ('sub_att_off', 'nturgb+d', 64, 64, 0.125, dict(SHIPPED, sub_att=False)),
    ('stage_off', 'nturgb+d', 64, 64, 0.125, dict(SHIPPED, stage=False)),
    ('add_type', 'nturgb+d', 64, 64, 0.125, dict(SHIPPED, add_type=True)),
    ('ada', 'nturgb+d', 64, 64, 0.125, dict(SHIPPED, ada_attention=True)),
    ('ada_plain', 'nturgb+d', 64, 64, 0.125, dict(decompose=False, ada_attention=True, subset_wise=True)),
    ('down', 'nturgb+d', 64, 128, 0.125, dict(SHIPPED, edge_attention=False)),
    ('coco', 'coco', 64, 64, 0.125, dict(SHIPPED, node_attention=False, ada_attention=True)),
    ('wide', 'nturgb+d', 128, 256, 0.125, dict(SHIPPED, subset_wise=False, edge_attention=False)),
]

# arm -> (backbone overrides, number of stages of the reduced model)
MODEL_ARMS = {
    'stage_odd': (dict(gcn_stage=[1, 3, 5, 7, 9]), 4),
    'stage_head': (dict(gcn_stage=[0, 1, 2, 3]), 5),
    'node_off': (dict(gcn_node_attention=False), 4),
    'edge_off': (dict(gcn_edge_attention=False), 4),
    'ada': (dict(gcn_ada_attention=True), 4),
}


def unit_flags():
    out = {'cases': np.array([c[0] for c in UNIT_CASES])}
    for i, (name, layout, ci, co, ratio, flags) in enumerate(UNIT_CASES):
        gr = graph(layout)
        A = torch.tensor(gr.A, dtype=torch.float32)
        V = A.shape[-1]
        node_type = torch.tensor(gr.node_type)
        edge_type = torch.tensor(gr.edge_type, dtype=torch.float32)
        seed = 700 + i
        torch.manual_seed(seed)
        m = R.gutils.dgphgcn1(ci, co, A, edge_type, node_type, ratio=ratio, **flags)
        tag = name + '_'
        out[tag + 'init_digest'] = np.array(sd_digest(m))
        out[tag + 'sd_manifest'] = np.array(json.dumps([[k, list(v.shape)] for k, v in m.state_dict().items()]))
        G.liven(m, 71 + i)
        out[tag + 'alpha'] = m.alpha.detach().numpy().copy()
        out[tag + 'beta'] = m.beta.detach().numpy().copy()
        m64 = m.double()
        x32, r32 = unit_inputs(ci, co, V, 90 + i)
        x = x32.double().requires_grad_()
        y = m64(x)
        (y * r32.double()).sum().backward()
        out[tag + 'cfg'] = np.array(json.dumps(dict(layout=layout, ci=ci, co=co, ratio=ratio, seed=seed, flags=flags),
                                               sort_keys=True))
        out[tag + 'input_seed'] = np.array(90 + i)
        out[tag + 'input_digest'] = np.array(hashlib.sha256(x32.numpy().tobytes() + r32.numpy().tobytes()).hexdigest())
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
    savez_det(os.path.join(HERE, 'unit_dgphgcn1_flags.npz'), **out)


def reduced(cfg, name, seed):
    """weights, input, labels + the fp64 truth: train-mode logits / loss / gradients, eval-mode logits"""
    np.random.seed(seed)
    torch.manual_seed(seed)
    m = R.builder.build_model(copy.deepcopy(cfg))
    G.liven(m, 33)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 1, 2, 16, 25, 3, generator=g)
    y = torch.randint(0, 12, (4, 1), generator=g)
    out = {'sd_' + k: v for k, v in G.sd_np(m).items()}
    out['x'] = x.numpy()
    out['label'] = y.numpy()
    m64 = R.builder.build_model(copy.deepcopy(cfg)).double()
    m64.load_state_dict({k: v.double() if v.dtype.is_floating_point else v for k, v in m.state_dict().items()})
    logits = m64.cls_head(G.extract_feat_f64(m64, x[:, 0].double()))
    loss = torch.nn.functional.cross_entropy(logits, y.squeeze(-1))
    loss.backward()
    out['logits_f64'] = logits.detach().numpy()
    out['loss_f64'] = np.array(loss.item())
    for k, p in m64.named_parameters():
        if p.grad is not None:
            out['g64_' + k] = p.grad.numpy().astype(np.float32)
    m64.load_state_dict({k: v.double() if v.dtype.is_floating_point else v for k, v in m.state_dict().items()})
    m64.eval()
    with torch.no_grad():
        out['logits_eval_f64'] = m64.cls_head(G.extract_feat_f64(m64, x[:, 0].double())).numpy()
    savez_det(os.path.join(HERE, name + '.npz'), **out)
    with open(os.path.join(HERE, name + '_cfg.json'), 'w') as f:
        json.dump(cfg, f, indent=1)
        f.write('\n')


def reduced_models():
    for i, (arm, (bk, stages)) in enumerate(MODEL_ARMS.items()):
        cfg = G.ds_cfg(num_classes=12, base_channels=16, num_stages=stages, inflate_stages=[3], down_stages=[3], **bk)
        cfg['cls_head']['in_channels'] = 32
        reduced(cfg, 'model_reduced_ds_' + arm, seed=20 + i)


if __name__ == '__main__':
    torch.set_num_threads(1)            # one summation order whatever the machine: the files are compared byte for byte
    if '--out' in sys.argv:             # write somewhere else (the regeneration test)
        HERE = sys.argv[sys.argv.index('--out') + 1]
    unit_flags()
    reduced_models()
    print('wrote unit_dgphgcn1_flags.npz and model_reduced_ds_{' + ', '.join(MODEL_ARMS) + '}(.npz, _cfg.json)')
