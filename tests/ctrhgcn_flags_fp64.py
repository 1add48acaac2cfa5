"""Restatement of ``unit_ctrhgcn`` with the ``target_specific`` / ``full_channels`` / ``add_type`` switches in plain torch
ops (written from the unit's equations, any dtype: the GPU tests run it in fp64 as truth), the position-typed 1x1 conv it
rests on, and an op namespace (``OPS``) that extends ``torch_ops`` by the two calls the switches add, so that the module's
wiring runs on the CPU under ``kernels.use_ops``.  tests/test_ctrhgcn_flags_host.py pins the restatement to the reference's
fp64 outputs (tests/golden/unit_ctrhgcn_flags.npz).

Notation: K = 3 subsets, R reduced channels, P node types, E edge classes; positions of a (T, V) plane are t*V + v."""
import types

import torch

import torch_ops
from dghgcn_fp64 import FULL_MAX, fixture_is_zero, fixture_rel, probe, unit_inputs  # noqa: F401  (the compact fixture form)


def typed_conv(x, W, b, table, P, plan=None):
    """y[n, o, pos] = sum_c W[type(pos)][o][c] x[n, c, pos] + b[type(pos)][o], type(pos) = table[pos % L].
    x (n, Ci, T, V), W (P, Co, Ci), b (P, Co).  Type by type, so a type no position carries gets an exact-zero gradient."""
    n, Ci, T, V = x.shape
    table = torch.as_tensor(table).reshape(-1).long().to(x.device)
    t = table[torch.arange(T * V, device=x.device) % table.numel()]
    xf = x.reshape(n, Ci, T * V)
    parts, order = [], []
    for p in range(P):
        idx = (t == p).nonzero().reshape(-1)
        parts.append(torch.einsum('oc,ncl->nol', W[p], xf[:, :, idx]) + b[p][None, :, None])
        order.append(idx)
    inv = torch.argsort(torch.cat(order))
    return torch.cat(parts, -1)[:, :, inv].reshape(n, W.shape[1], T, V)


def _conv(z, w, b):
    w = w.reshape(w.shape[0], -1)
    out = torch.einsum('oc,nc...->no...', w, z)
    return out + b.reshape((1, -1) + (1,) * (z.dim() - 2))


def _bn(z, w, b, mean=None, var=None, eps=1e-5):
    if mean is None:
        mean, var = z.mean(dim=(0, 2, 3)), z.var(dim=(0, 2, 3), unbiased=False)
    c = lambda t: t.view(1, -1, 1, 1)        # noqa: E731
    return (z - c(mean)) / torch.sqrt(c(var) + eps) * c(w) + c(b)


def unit_forward(p, x, node_type, edge_type, full_channels, add_type, num_types=5, edge_num=15, running=None):
    """p: the unit's parameters by state_dict key -> relu(bn(sum_k aggregate_k) + down(x)).  Edge attention and
    target_specific are read from the keys (``edge_att_conv``, ``nodeconv``: present only where the switch acts);
    full_channels / add_type are passed and act on the subsets that own an ``edge_att_conv``.  running: a dict of running
    statistics by state_dict key for eval mode, None = batch statistics."""
    n, Ci, T, V = x.shape
    xbar = x.mean(2)
    K = p['A'].shape[0]
    y = 0
    for k in range(K):
        g = lambda name: p[f'convs.{k}.{name}']      # noqa: E731
        x1, x2 = _conv(xbar, g('conv1.weight'), g('conv1.bias')), _conv(xbar, g('conv2.weight'), g('conv2.bias'))
        R = x1.shape[1]
        d = torch.tanh(x1[..., :, None] - x2[..., None, :])                      # (n, R, V, V)
        w4, b4 = g('conv4.weight'), g('conv4.bias')
        Co = w4.shape[0]
        if f'convs.{k}.edge_att_conv.weight' in p:
            we, be = g('edge_att_conv.weight'), g('edge_att_conv.bias')
            Cx = Co if full_channels else R                                       # row e*Cx + c
            att = typed_conv(d, we.reshape(edge_num, Cx, R), be.reshape(edge_num, Cx), edge_type, edge_num)
            if not full_channels:
                att = _conv(att, w4, b4)
            if add_type:
                att = att + _conv(d, w4, b4)
        else:
            att = _conv(d, w4, b4)
        ahat = att * p['alpha'][k] + p['A'][k][None, None]
        if f'convs.{k}.beta' in p:
            ahat = ahat + g('beta') * torch.einsum('ncu,ncw->nuw', x1, x2)[:, None]
        x3 = _conv(x, g('conv3.weight'), g('conv3.bias'))
        if f'convs.{k}.nodeconv.weight' in p:
            wn, bn_ = g('nodeconv.weight'), g('nodeconv.bias')                    # row p*Co + o
            x3 = x3 + typed_conv(x, wn.reshape(num_types, Co, Ci), bn_.reshape(num_types, Co), node_type, num_types)
        y = y + torch.einsum('ncuv,nctu->nctv', ahat, x3)
    r = (lambda key: None) if running is None else running.get
    out = _bn(y, p['bn.weight'], p['bn.bias'], r('bn.running_mean'), r('bn.running_var'))
    if 'down.0.weight' in p:
        res = _bn(_conv(x, p['down.0.weight'], p['down.0.bias']), p['down.1.weight'], p['down.1.bias'],
                  r('down.1.running_mean'), r('down.1.running_var'))
    else:
        res = x
    return torch.relu(out + res)


def ctr_topology(xbar, w1, b1, w2, b2, w4, b4, alpha, A, beta=None, edge=None, subset_major=False, edge_mode=None):
    """``kernels.ctr_topology`` with the edge modes (full_channels, add_type, E, plan) in plain torch ops."""
    if not edge_mode:
        return torch_ops.ctr_topology(xbar, w1, b1, w2, b2, w4, b4, alpha, A, beta, edge, subset_major)
    n, Ci, V = xbar.shape
    K = A.shape[0]
    R = w1.shape[0] // K
    x1 = (torch.einsum('oc,ncv->nov', w1, xbar) + b1[None, :, None]).view(n, K, R, V)
    x2 = (torch.einsum('oc,ncv->nov', w2, xbar) + b2[None, :, None]).view(n, K, R, V)
    d = torch.tanh(x1[..., :, None] - x2[..., None, :])
    out = []
    for k in range(K):
        dk = d[:, k]
        conv4 = lambda z: torch.einsum('or,nruv->nouv', w4[k], z) + b4[k][None, :, None, None]      # noqa: E731
        if edge and k in edge:
            we, be, et = edge[k]
            full, add, E, _ = edge_mode.get(k, (False, False, we.shape[0] // R, None))
            Cx = we.shape[0] // E
            s = typed_conv(dk, we.view(E, Cx, R), be.view(E, Cx), et, E)
            if not full:
                s = conv4(s)
            if add:
                s = s + conv4(dk)
        else:
            s = conv4(dk)
        a = s * alpha[k] + A[k][None, None]
        if beta is not None:
            a = a + beta[k] * torch.einsum('nru,nrv->nuv', x1[:, k], x2[:, k])[:, None]
        out.append(a)
    return torch.cat(out, 1)


# torch_ops + the two calls the switches add: the namespace for ``kernels.use_ops`` in the CPU tests
OPS = types.SimpleNamespace(**{k: v for k, v in vars(torch_ops).items() if not k.startswith('__')})
OPS.NAME = 'torch_ops + typed_conv (test reference)'
OPS.typed_conv = typed_conv
OPS.ctr_topology = ctr_topology
