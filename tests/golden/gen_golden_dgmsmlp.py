"""Golden fixtures for ``dgmsmlp`` and for ``tcn_type='mstcn'`` / ``'dgmsmlp'`` inside DGSTGCN, generated from the
IMPORTED reference (build container only: needs the reference checkout, see ref_shim):

    python tests/golden/gen_golden_dgmsmlp.py

  unit_dgmsmlp.npz                         eight units (tests/dgmsmlp_fp64.py: CASES), n = 2, live add_coeff / alpha / BatchNorm
                                           affines (liven_unit).  Per unit: the seed, keys / shapes and digest of the
                                           constructor's state_dict (the tests rebuild the weights from the seed), the digest
                                           of the live state, the seed and digest of the input and output probe R, the fp64
                                           output, input gradient and every parameter gradient, and the reference's own fp32
                                           gradients (``g32_``): whole up to 512 elements, as 32 fixed random projections above
                                           (tests/dghgcn_fp64.py: probe)
  model_reduced_dg_mstcn(.npz, _cfg.json)  the kwargs of the shipped configs/dsstgcn/DSSTGCN_model.py at reduced width with
  model_reduced_dg_msmlp(.npz, _cfg.json)  tcn_type='mstcn', and with tcn_type='dgmsmlp', tcn_add_tcn, tcn_merge_after
                                           (G.reduced_model: logits, loss, all gradients in fp32 and fp64), + fp64 eval logits

Data only.  The archives are written with fixed member times, so a second run gives byte-identical files."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (ref_shim, ds_cfg, reduced_model)
from gen_golden_dghgcn import reduced, savez_det, sd_digest  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import dgmsmlp_fp64 as F  # noqa: E402  (CASES, inputs, liven_unit, the compact fixture form)

R = G.R


def units():
    out = {'cases': np.array([c[0] for c in F.CASES])}
    for i, row in enumerate(F.CASES):
        c = F.case(row[0])
        seed = 900 + i
        torch.manual_seed(seed)
        m = R.gutils.dgmsmlp(c['C'], c['C'], **F.unit_kwargs(c))
        tag = c['tag'] + '_'
        out[tag + 'seed'] = np.array(seed)
        out[tag + 'init_digest'] = np.array(sd_digest(m))
        out[tag + 'sd_manifest'] = np.array(json.dumps([[k, list(v.shape)] for k, v in m.state_dict().items()]))
        out[tag + 'live_seed'] = np.array(61 + i)
        F.liven_unit(m, 61 + i)
        out[tag + 'live_digest'] = np.array(sd_digest(m))
        out[tag + 'input_seed'] = np.array(90 + i)
        x32, r32 = F.unit_inputs(c, 90 + i)
        out[tag + 'input_digest'] = np.array(hashlib.sha256(x32.numpy().tobytes() + r32.numpy().tobytes()).hexdigest())

        def put(key, a):
            a = np.asarray(a, dtype=np.float64)
            if a.size <= F.FULL_MAX:
                out[key] = a
            else:
                out[key + '_probe'] = F.probe(a, key)

        m.train()
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
    savez_det(os.path.join(HERE, 'unit_dgmsmlp.npz'), **out)


def reduced_models():
    small = dict(base_channels=16, num_stages=4, inflate_stages=[3], down_stages=[3])
    cfg = G.ds_cfg(num_classes=12, tcn_type='mstcn', **small)
    cfg['cls_head']['in_channels'] = 32
    reduced(cfg, 'model_reduced_dg_mstcn', seed=11)
    cfg = G.ds_cfg(num_classes=12, tcn_type='dgmsmlp', tcn_add_tcn=True, tcn_merge_after=True, **small)
    cfg['cls_head']['in_channels'] = 32
    reduced(cfg, 'model_reduced_dg_msmlp', seed=12)


if __name__ == '__main__':
    units()
    reduced_models()
    print('wrote unit_dgmsmlp.npz, model_reduced_dg_mstcn(.npz, _cfg.json), model_reduced_dg_msmlp(.npz, _cfg.json)')
