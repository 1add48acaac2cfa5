"""fp64 fixtures of the oracle-vs-reference unit checks, generated from the IMPORTED reference (needs the reference tree,
see ref_shim.py):

    python tests/golden/gen_golden_fp64.py

  reference_fp64.npz   the cases of tests/test_oracle_golden.py's *_vs_reference_live tests — closed_form.REF64_GROUPS
                       (unit_aagcn, dgphgcn1 and dggcn on the coco graph, dgmstcn / mstcn) and the closed_form.UNIT_CASES
                       units — each with the reference module's fp64 train-mode output, kept as
                         {name}_y_at     its values at the fixed positions {name}_idx (closed_form.ref64_sample)
                         {name}_y_sums   its sums over samples and joints, per (channel, frame): every element counts
                         {name}_shape    its shape
                       Weights and inputs are rebuilt by the tests from the shared seeded recipes (closed_form.make_unit,
                       make_ref64_group); their digests ({name}_sd_digest, {name}_x_digest) pin them.
Data only (digests and the reference's outputs); no reference source."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shim  # noqa: E402
from closed_form import REF64_GROUPS, array_digest, make_ref64_group, make_unit, ref64_sample, sd_digest  # noqa: E402

R = ref_shim.load()

UNIT_TAGS = ('gcn', 'gcn_res', 'tcn9', 'tcn1s2', 'ctrgcn', 'MSTCN', 'gcn_offset_post', 'gcn_importance', 'gcn_fixed_post',
             'ctrhgcn', 'ctrhgcn_same', 'msmlp', 'msmlp_s2', 'unitmlp9', 'unitmlp9_s2')


def put_output(out, name, y):
    y = y.detach().numpy()
    idx = ref64_sample(y.size)
    out[f'{name}_shape'] = np.array(y.shape)
    out[f'{name}_idx'] = idx
    out[f'{name}_y_at'] = y.reshape(-1)[idx]
    out[f'{name}_y_sums'] = y.sum((0, 3))


def groups(out):
    for group in REF64_GROUPS:
        for name, m, x in make_ref64_group(R.gutils, R.graph.Graph, group):
            out[f'{name}_sd_digest'] = np.array(sd_digest(m))
            out[f'{name}_x_digest'] = np.array(array_digest(x))
            if group == 'dggcn':
                out[f'{name}_subset_wise'] = np.array(bool(m.subset_wise))
            with torch.no_grad():
                put_output(out, name, m(x))


def units(out):
    Gs = R.graph.Graph(layout='nturgb+d', mode='spatial')
    A = torch.tensor(Gs.A, dtype=torch.float32)
    for tag in UNIT_TAGS:
        m, x, _ = make_unit(R.gutils, tag, A, Gs.edge_type, Gs.node_type)
        out[f'unit_{tag}_sd_digest'] = np.array(sd_digest(m))
        out[f'unit_{tag}_x_digest'] = np.array(array_digest(x))
        with torch.no_grad():
            put_output(out, f'unit_{tag}', m.double().train()(x.double()))


if __name__ == '__main__':
    out = {}
    groups(out)
    units(out)
    path = os.path.join(HERE, 'reference_fp64.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
