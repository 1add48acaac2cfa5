"""fp64 restatement of the ``dgphgcn1`` unit under its switches, in plain torch ops (written from the unit's equations,
not from the reference's code): the truth the GPU tests compare the flag-specialised K-B path against element by element.
tests/test_dgphgcn1_flags_host.py pins it to the imported reference at 1e-12 and to the reference's fp64 fixture
(tests/golden/unit_dgphgcn1_flags.npz).

K = 3 subsets of mid channels.  decompose: subsets 0, 1 from conv1 / conv2, subset 2 from the conv1_se rows on BOTH sides
(node-typed: joint v keeps row c*P + type(v)); the edge linear (E classes) sits on subset 1.  ada_attention: the three
Grams are mixed per edge class before the softmax.  flags = dict(decompose, node_attention, edge_attention, subset_wise,
ada_attention, num_types, edge_num), already the EFFECTIVE ones (``effective_flags`` applies stage=False)."""
import torch

from dghgcn_fp64 import (FULL_MAX, PROBES, _bn_train, _conv, fixture_is_zero, fixture_rel, probe,  # noqa: F401
                         typed_select, unit_inputs)


def effective_flags(decompose=False, node_attention=False, edge_attention=False, ada_attention=False, sub_att=True,
                    stage=True, add_type=False, subset_wise=True, num_types=5, edge_num=15, **_):
    if stage is False:
        decompose = node_attention = edge_attention = subset_wise = False
    return dict(decompose=bool(decompose), node_attention=bool(decompose and node_attention),
                edge_attention=bool(decompose and edge_attention), subset_wise=bool(subset_wise),
                ada_attention=bool(ada_attention), num_types=num_types, edge_num=edge_num)


def adjacency(xbar, p, node_type, edge_type, fl):
    """xbar (n, Ci, V), p: parameters by state_dict key -> Ahat (n, 3*mid, V, V)"""
    n, _, V = xbar.shape
    dev = xbar.device
    x1 = _conv(xbar, p['conv1.weight'], p['conv1.bias'])
    x2 = _conv(xbar, p['conv2.weight'], p['conv2.bias'])
    if fl['decompose']:
        xs = typed_select(_conv(xbar, p['conv1_se.weight'], p['conv1_se.bias']), node_type,
                          fl['num_types'] if fl['node_attention'] else 1)
        x1, x2 = torch.cat([x1, xs], 1), torch.cat([x2, xs], 1)
    m = x1.shape[1] // 3
    x1, x2 = x1.view(n, 3, m, V), x2.view(n, 3, m, V)
    D = x1[..., :, None] - x2[..., None, :]                                  # (n, 3, m, V, V)
    et = torch.as_tensor(edge_type).long().reshape(V, V).to(dev)
    j = torch.arange(V, device=dev)
    if fl['edge_attention']:
        we, be = p['edge_linears.weight'], p['edge_linears.bias']
        E = fl['edge_num']
        # edge_linears(x1_1[u] - x2_1[w]) = We x1_1[u] + be - We x2_1[w]; the class of (u, w) picks the row block
        pe = _conv(x1[:, 1], we, be).view(n, E, m, V).permute(1, 3, 0, 2)   # (E, V, n, m)
        qe = _conv(x2[:, 1], we, torch.zeros_like(be)).view(n, E, m, V).permute(1, 3, 0, 2)
        att = (pe[et, j[:, None]] - qe[et, j[None, :]]).permute(2, 3, 0, 1)  # (n, m, V, V)
        D = torch.stack([D[:, 0], att, D[:, 2]], 1)
    gram = torch.einsum('nkcu,nkcw->nkuw', x1, x2)
    if fl['ada_attention']:
        E = fl['edge_num']
        wa = p['ada_linears.weight'].reshape(3, E, 3)                        # row k*E + e
        ba = p['ada_linears.bias'].reshape(3, E)
        gram = torch.einsum('uwkq,nquw->nkuw', wa[:, et].permute(1, 2, 0, 3), gram) + ba[:, et][None]
    soft = torch.softmax(gram, dim=-2)
    a = p['alpha'] if fl['subset_wise'] else p['alpha'][0].expand(3)
    b = p['beta'] if fl['subset_wise'] else p['beta'][0].expand(3)
    ahat = p['A'][None, :, None] + a.view(1, 3, 1, 1, 1) * torch.tanh(D) + b.view(1, 3, 1, 1, 1) * soft[:, :, None]
    return ahat.reshape(n, 3 * m, V, V)


def unit_forward(p, x, node_type, edge_type, fl):
    """train-mode BatchNorm (batch statistics) -> relu(bn(post(pre(x) x Ahat)) + res)"""
    ahat = adjacency(x.mean(2), p, node_type, edge_type, fl)
    pre = torch.relu(_bn_train(_conv(x, p['pre.0.weight'], p['pre.0.bias']), p['pre.1.weight'], p['pre.1.bias']))
    y = torch.einsum('nctv,ncvw->nctw', pre, ahat)
    out = _bn_train(_conv(y, p['post.weight'], p['post.bias']), p['bn.weight'], p['bn.bias'])
    if 'down.0.weight' in p:
        res = _bn_train(_conv(x, p['down.0.weight'], p['down.0.bias']), p['down.1.weight'], p['down.1.bias'])
    else:
        res = x
    return torch.relu(out + res)
