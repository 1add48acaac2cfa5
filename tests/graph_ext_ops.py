"""Test infrastructure of ``test_cfg['graph_ext']`` (the per-video learned adjacency of every layer):

* ``cpu_ops()`` — the CPU seam (``kernels.use_ops``): the tests/torch_ops.py namespace plus the torch statement of the
  ``graph_pool`` op, and of the three adjacency ops torch_ops leaves to the units' own fp64 files (``dynadj_plain``,
  ``dynadj_typed``, ``dynadj_flags``) so that every unit type runs on the CPU;
* ``pool64`` / ``unit_graph64`` — the fp64 statements the GPU tests compare against;
* the fixture readers of tests/golden/graph_ext.npz (tests/golden/gen_golden_graph_ext.py)."""
import json
import os
import types

import numpy as np
import torch

import dggcn_plain_fp64 as P64
import dghgcn_fp64 as H64
import dgphgcn1_flags_fp64 as F64

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'graph_ext.npz')
MODEL_BAR = 2e-6          # the project's K-B forward bar (relative L2, check_dynadj)


def graph_pool(ahat, group, K, out, layer):
    """``kernels.graph_pool`` in torch: out[:, layer] = mean over the group's person-samples and the channels."""
    n, KM, V, _ = ahat.shape
    out[:, layer] = ahat.reshape(n // group, group, K, KM // K, V, V).mean((1, 3)).to(out.dtype)
    return out


def pool64(ahat, group, K):
    """(videos*group, K*mid, V, V) -> fp64 (videos, K, V, V)"""
    n, KM, V, _ = ahat.shape
    return ahat.double().reshape(n // group, group, K, KM // K, V, V).mean((1, 3))


def dynadj_typed(xbar, A, alpha, beta, w1, b1, w2, b2, we, be, node_type, edge_type, P, add_type, single_use=True):
    """``kernels.dynadj_typed`` in torch (alpha / beta hold 3 values: the unit expands a scalar itself)."""
    return H64.adjacency(xbar[..., :A.shape[-1]], A, alpha, beta, w1, b1, w2, b2, we, be, node_type, edge_type, P, add_type,
                         True)


def dynadj_flags(xbar, A, alpha, beta, w1, b1, w2, b2, wse, bse, wel, bel, wal, bal, node_type, edge_type, P, edge_num,
                 subset_wise):
    """``kernels.dynadj_flags`` in torch."""
    p = {'A': A, 'alpha': alpha, 'beta': beta, 'conv1.weight': w1, 'conv1.bias': b1, 'conv2.weight': w2, 'conv2.bias': b2,
         'conv1_se.weight': wse, 'conv1_se.bias': bse, 'edge_linears.weight': wel, 'edge_linears.bias': bel,
         'ada_linears.weight': wal, 'ada_linears.bias': bal}
    fl = dict(decompose=wse is not None, node_attention=wse is not None, edge_attention=wel is not None,
              subset_wise=bool(subset_wise), ada_attention=wal is not None, num_types=P, edge_num=edge_num)
    return F64.adjacency(xbar[..., :A.shape[-1]], p, node_type, edge_type, fl)


def cpu_ops(calls=None):
    """The CPU namespace.  calls (a list): the name of every adjacency / graph_pool op called is appended."""
    import torch_ops
    ns = types.SimpleNamespace(**{k: v for k, v in vars(torch_ops).items() if not k.startswith('__')})

    def rec(name, fn):
        def wrapped(*a, **kw):
            if calls is not None:
                calls.append(name)
            return fn(*a, **kw)
        return wrapped
    ns.dynadj = rec('dynadj', torch_ops.dynadj)
    ns.dynadj_plain = rec('dynadj_plain', P64.dynadj_plain)
    ns.dynadj_typed = rec('dynadj_typed', dynadj_typed)
    ns.dynadj_flags = rec('dynadj_flags', dynadj_flags)
    ns.graph_pool = rec('graph_pool', graph_pool)
    return ns


def unit_graph64(unit, xbar, mode):
    """fp64 Ahat (n, K*mid, V, V) of a unit from its parameters and xbar (n, Ci, V): 'ahat' as the layer builds it, 'ctr'
    with beta set to 0."""
    from dsgcn_amd.gcn_units import dggcn, dghgcn, dgphgcn1
    p = {k: v.detach().double().cpu() for k, v in unit.state_dict().items()}
    p = {k: (v.flatten(1) if k.endswith('.weight') and v.dim() == 4 else v) for k, v in p.items()}
    if mode == 'ctr':
        p['beta'] = torch.zeros_like(p['beta'])
    xbar = xbar.detach().double().cpu()[..., :unit.A.shape[-1]]
    if isinstance(unit, dggcn):
        return P64.adjacency(xbar, p['A'], p['alpha'], p['beta'], p['conv1.weight'], p['conv1.bias'], p['conv2.weight'],
                             p['conv2.bias'], bool(unit.subset_wise))
    nt, et = unit.node_type_idx.cpu(), unit.edge_type_idx.cpu()
    if isinstance(unit, dghgcn):
        edge = unit.edge_attention
        return H64.adjacency(xbar, p['A'], p['alpha'], p['beta'], p['conv1.weight'], p['conv1.bias'], p['conv2.weight'],
                             p['conv2.bias'], p['edge_linears.weight'] if edge else None,
                             p['edge_linears.bias'] if edge else None, nt, et,
                             unit.num_types if unit.node_attention else 1, unit.add_type, bool(unit.subset_wise))
    assert isinstance(unit, dgphgcn1)
    fl = F64.effective_flags(decompose=unit.decompose, node_attention=unit.node_attention,
                             edge_attention=unit.edge_attention, ada_attention=unit.ada_attention,
                             subset_wise=unit.subset_wise, num_types=unit.num_types, edge_num=unit.edge_num)
    return F64.adjacency(xbar, p, nt, et, fl)


def rel_l2(got, want):
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    return float((got - want).norm() / want.norm())


# ---- the fixture -------------------------------------------------------------------------------------------------------
_fixture = None


def fixture():
    """dict(cfg, sd, x, g64, g32, ref32_rel) of tests/golden/graph_ext.npz, loaded once (read-only by convention)."""
    global _fixture
    if _fixture is None:
        with np.load(GOLDEN) as z:
            cfg = json.loads(str(z['cfg']))
            cfg['backbone']['tcn_ms_cfg'] = [tuple(c) if isinstance(c, list) else c for c in cfg['backbone']['tcn_ms_cfg']]
            sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd_')}
            g = torch.Generator().manual_seed(int(z['input_seed']))
            x = torch.randn(tuple(int(v) for v in z['input_shape']), generator=g)
            _fixture = dict(cfg=cfg, sd=sd, x=x, g64=torch.from_numpy(z['g64']), g32=torch.from_numpy(z['g32']),
                            ref32_rel=z['ref32_rel'].copy())
    return _fixture


def fixture_model(graph_ext='ctr', **test_cfg):
    """The fixture's reduced DS-STGCN with its weights, eval mode, ``test_cfg['graph_ext']`` = graph_ext (None: absent)."""
    import copy

    import dsgcn_amd
    fx = fixture()
    cfg = copy.deepcopy(fx['cfg'])
    cfg['test_cfg'] = dict(test_cfg)
    if graph_ext is not None:
        cfg['test_cfg']['graph_ext'] = graph_ext
    m = dsgcn_amd.build_model(cfg)
    m.load_state_dict(fx['sd'])
    return m.eval()


def layer_rel(got, want):
    """per-layer relative L2 of (videos, L, K, V, V) graphs"""
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    return [rel_l2(got[:, i], want[:, i]) for i in range(want.shape[1])]


# ---- units -------------------------------------------------------------------------------------------------------------
UNIT_KINDS = ('dgphgcn1', 'dgphgcn1_edge_off', 'dghgcn', 'dggcn_k8')      # shipped flags, one flag arm, typed, plain K = 8
LAYOUTS = {25: 'nturgb+d', 17: 'coco'}


def make_unit(kind, V, ci=32, co=32, seed=5):
    """An eval-mode unit of ``kind`` on the V-joint layout with live alpha / beta / conv biases."""
    import dsgcn_amd as D
    layout = LAYOUTS[V]
    K = 8 if kind == 'dggcn_k8' else 3
    np.random.seed(seed)
    torch.manual_seed(seed)
    A = torch.tensor(np.asarray(D.Graph(layout=layout, mode='random', num_filter=K, init_off=.04, init_std=.02).A),
                     dtype=torch.float32)
    g = D.Graph(layout=layout, mode='spatial')
    nt, et = torch.tensor(g.node_type), torch.tensor(g.edge_type)
    types = dict(num_types=int(nt.max()) + 1, edge_num=int(et.max()) + 1)
    if kind == 'dgphgcn1':
        m = D.dgphgcn1(ci, co, A, et, nt, ratio=0.125, decompose=True, node_attention=True, edge_attention=True,
                       subset_wise=True, **types)
        assert m._shipped
    elif kind == 'dgphgcn1_edge_off':
        m = D.dgphgcn1(ci, co, A, et, nt, ratio=0.125, decompose=True, node_attention=True, edge_attention=False,
                       subset_wise=False, **types)
        assert not m._shipped
    elif kind == 'dghgcn':
        m = D.dghgcn(ci, co, A, et, nt, ratio=0.125, node_attention=True, edge_attention=True, subset_wise=True, **types)
    else:
        m = D.dggcn(ci, co, A, ratio=0.125, subset_wise=True)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        m.alpha.copy_(torch.randn(m.alpha.shape, generator=gen) * 0.5)
        m.beta.copy_(torch.randn(m.beta.shape, generator=gen) * 0.5)
        for name, p in m.named_parameters():
            if name.endswith('.bias') and name.split('.')[0] in ('conv1', 'conv2', 'conv1_se', 'edge_linears'):
                p.copy_(torch.randn(p.shape, generator=gen) * 0.1)
    return m.eval()
