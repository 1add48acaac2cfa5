"""Golden fixtures for ``dggcn`` (the original DG-STGCN spatial unit) at numbers of subsets other than three, generated
from the IMPORTED reference (build container only: needs the reference checkout, see ref_shim):

    python tests/golden/gen_golden_dggcn_k.py

  unit_dggcn_k.npz                    seven units, n = 2, T = 8: K = 8 at ratio 0.125 (64 -> 64 scalar alpha / beta,
                                      64 -> 128 subset-wise), K = 2 at 0.25, K = 1 and K = 5 (60 -> 60: mid = 12) at
                                      ratio=None, K = 8 on the coco graph (V = 17) and K = 8 128 -> 256 at 0.25 (mid = 64).
                                      Per unit what unit_dghgcn.npz holds (gen_golden_dghgcn.py): the seed, keys / shapes
                                      and digest of the constructor's state_dict, the live alpha / beta, the seed and
                                      digest of the input and output probe R, and the fp64 output, input gradient and every
                                      parameter gradient — whole up to 4096 elements, 32 fixed random projections above
  model_reduced_dggcn_k8(.npz, _cfg.json)   model_reduced_dggcn's config with num_filter = 8, gcn_ratio = 0.125 at reduced
                                      width (G.reduced_model), + fp64 eval-mode logits, + keys / shapes / digest of the
                                      seeded constructor's state_dict

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
import gen_golden as G  # noqa: E402  (ref_shim, liven, reduced_model)
from gen_golden_dghgcn import reduced, savez_det, sd_digest  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
from dghgcn_fp64 import FULL_MAX, probe, unit_inputs  # noqa: E402  (the compact fixture form the tests read)

R = G.R

# (name, layout, K, Ci, Co, ratio, subset_wise)
UNIT_CASES = [
    ('k8', 'nturgb+d', 8, 64, 64, 0.125, False),
    ('k8_sw', 'nturgb+d', 8, 64, 128, 0.125, True),
    ('k2', 'nturgb+d', 2, 64, 64, 0.25, False),
    ('k1', 'nturgb+d', 1, 64, 64, None, True),
    ('k5', 'nturgb+d', 5, 60, 60, None, True),
    ('k8_coco', 'coco', 8, 64, 64, 0.125, True),
    ('k8_wide', 'nturgb+d', 8, 128, 256, 0.25, False),
]
# The reduced model's seed: the first of these at which the REFERENCE's own fp32 gradient lies within REF_FP32_MAX of its
# fp64 gradient (whole-gradient relative L2).  Four clips through train-mode BatchNorm, ReLU and max-pool branches: at some
# seeds one pre-activation sits at rounding distance from a kink and an fp32 and an fp64 run take different sides of it,
# which moves the block-0 gradients by ~5e-4 in the reference's fp32 run too (seed 10: 4.6e-4).  Such a draw measures the
# kink, not an implementation, so the fixture is taken where the reference agrees with itself — a tenth of the tests'
# 2e-4 bar.  The criterion reads nothing but the reference's two runs.
MODEL_SEEDS = range(10, 30)
REF_FP32_MAX = 2e-5


def graph(layout, K):
    np.random.seed(21)
    return R.graph.Graph(layout=layout, mode='random', num_filter=K, init_off=.04, init_std=.02)


def unit_dggcn_k():
    out = {'cases': np.array([c[0] for c in UNIT_CASES])}
    for i, (name, layout, K, ci, co, ratio, sw) in enumerate(UNIT_CASES):
        A = torch.tensor(graph(layout, K).A, dtype=torch.float32)
        V = A.shape[-1]
        seed = 700 + i
        torch.manual_seed(seed)
        m = R.gutils.dggcn(ci, co, A, ratio=ratio, subset_wise=sw)
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
        out[tag + 'cfg'] = np.array([ci, co, K, V, int(sw), seed])
        out[tag + 'layout'] = np.array(layout)
        out[tag + 'ratio'] = np.array(np.nan if ratio is None else ratio)
        out[tag + 'input_seed'] = np.array(90 + i)
        out[tag + 'input_digest'] = np.array(hashlib.sha256(x32.numpy().tobytes() + r32.numpy().tobytes()).hexdigest())

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
    savez_det(os.path.join(HERE, 'unit_dggcn_k.npz'), **out)


def reduced_dggcn_k8():
    with open(os.path.join(HERE, 'model_reduced_dggcn_cfg.json')) as f:
        cfg = json.load(f)
    cfg['backbone']['graph_cfg']['num_filter'] = 8
    cfg['backbone']['gcn_ratio'] = 0.125
    cfg['backbone']['tcn_ms_cfg'] = [tuple(c) if isinstance(c, list) else c for c in cfg['backbone']['tcn_ms_cfg']]
    name = 'model_reduced_dggcn_k8'
    path = os.path.join(HERE, name + '.npz')
    for seed in MODEL_SEEDS:
        reduced(cfg, name, seed=seed)
        with np.load(path) as f:
            z = {k: f[k] for k in f.files}
        keys = [k[4:] for k in z if k.startswith('g64_')]
        num = sum(float(((z['g32_' + k].astype(np.float64) - z['g64_' + k]) ** 2).sum()) for k in keys)
        den = sum(float((z['g64_' + k].astype(np.float64) ** 2).sum()) for k in keys)
        print(f'seed {seed}: the reference in fp32 vs fp64, whole gradient: {(num / den) ** .5:.2e}')
        if (num / den) ** .5 < REF_FP32_MAX:
            break
    else:
        raise SystemExit('no seed at which the reference agrees with itself')
    np.random.seed(seed)
    torch.manual_seed(seed)
    m = R.builder.build_model(copy.deepcopy(cfg))              # the constructor's values (the archive's are livened)
    z['init_seed'] = np.array(seed)
    z['ref_fp32_gradient_error'] = np.array((num / den) ** .5)
    z['init_digest'] = np.array(sd_digest(m))
    z['init_manifest'] = np.array(json.dumps([[k, list(v.shape)] for k, v in m.state_dict().items()]))
    savez_det(path, **z)


if __name__ == '__main__':
    unit_dggcn_k()
    reduced_dggcn_k8()
    print('wrote unit_dggcn_k.npz, model_reduced_dggcn_k8(.npz, _cfg.json)')
