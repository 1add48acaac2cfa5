"""fp64 restatement of the ``dggcn`` unit for any number of subsets K in plain torch ops (written from the unit's
equations, not from the reference's code): the truth the full-size GPU tests compare the plain K-B path against.
tests/test_dggcn_plain_host.py pins it to the reference's fp64 outputs (tests/golden/unit_dggcn_k.npz).  Also the torch
statement of the ``dynadj_plain`` op for the CPU seam (``kernels.use_ops``): tests/torch_ops.py plus that one function."""
import types

import torch

from dghgcn_fp64 import FULL_MAX, _bn_train, _conv, fixture_is_zero, fixture_rel, probe, unit_inputs  # noqa: F401


def adjacency(xbar, A, alpha, beta, w1, b1, w2, b2, subset_wise=True):
    """xbar (n, Ci, V) -> Ahat (n, K*mid, V, V); alpha / beta (K), of which only entry 0 counts without subset_wise."""
    n, _, V = xbar.shape
    K = A.shape[0]
    x1 = _conv(xbar, w1, b1)
    x2 = _conv(xbar, w2, b2)
    m = x1.shape[1] // K
    x1, x2 = x1.view(n, K, m, V), x2.view(n, K, m, V)
    a = alpha if subset_wise else alpha[0].expand(K)
    b = beta if subset_wise else beta[0].expand(K)
    soft = torch.softmax(torch.einsum('nkcu,nkcw->nkuw', x1, x2), dim=-2)
    ahat = (A[None, :, None] + a.view(1, K, 1, 1, 1) * torch.tanh(x1[..., :, None] - x2[..., None, :])
            + b.view(1, K, 1, 1, 1) * soft[:, :, None])
    return ahat.reshape(n, K * m, V, V)


def unit_forward(p, x, subset_wise):
    """p: the unit's parameters by state_dict key (train-mode BatchNorm, batch statistics) -> relu(bn(post) + res)"""
    ahat = adjacency(x.mean(2), p['A'], p['alpha'], p['beta'], p['conv1.weight'], p['conv1.bias'], p['conv2.weight'],
                     p['conv2.bias'], subset_wise)
    pre = torch.relu(_bn_train(_conv(x, p['pre.0.weight'], p['pre.0.bias']), p['pre.1.weight'], p['pre.1.bias']))
    y = torch.einsum('nctv,ncvw->nctw', pre, ahat)
    out = _bn_train(_conv(y, p['post.weight'], p['post.bias']), p['bn.weight'], p['bn.bias'])
    if 'down.0.weight' in p:
        res = _bn_train(_conv(x, p['down.0.weight'], p['down.0.bias']), p['down.1.weight'], p['down.1.bias'])
    else:
        res = x
    return torch.relu(out + res)


def dynadj_plain(xbar, A, alpha, beta, w1, b1, w2, b2, single_use=True):
    """The ``kernels.dynadj_plain`` op in torch: alpha / beta hold K values (the unit expands a scalar itself)."""
    return adjacency(xbar[..., :A.shape[-1]], A, alpha, beta, w1, b1, w2, b2, True)


def cpu_ops(calls=None):
    """tests/torch_ops.py plus ``dynadj_plain``; with `calls` (a list) the names of the adjacency ops called are appended."""
    import torch_ops
    ns = types.SimpleNamespace(**{k: v for k, v in vars(torch_ops).items() if not k.startswith('__')})

    def rec(name, fn):
        def wrapped(*a, **kw):
            if calls is not None:
                calls.append(name)
            return fn(*a, **kw)
        return wrapped
    ns.dynadj = rec('dynadj', torch_ops.dynadj)
    ns.dynadj_plain = rec('dynadj_plain', dynadj_plain)
    return ns
