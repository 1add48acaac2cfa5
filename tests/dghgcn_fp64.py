"""fp64 restatement of the ``dghgcn`` unit in plain torch ops (written from the unit's equations, not from the reference's
code): the truth the full-size GPU tests compare the typed K-B path against.  tests/test_dghgcn_host.py pins it to the
reference's fp64 outputs (tests/golden/unit_dghgcn.npz).

Notation: K = 3 subsets, mid channels each (KM = 3*mid), P node types (1 = untyped), E edge classes."""
import torch


def _conv(z, w, b):
    """1x1 conv of (n, C, ...) with weight (O, C[, 1, 1])"""
    w = w.reshape(w.shape[0], -1)
    out = torch.einsum('oc,nc...->no...', w, z)
    return out + b.reshape((1, -1) + (1,) * (z.dim() - 2))


def typed_select(proj, node_type, P):
    """proj (n, KM*P, V), row r*P + p -> (n, KM, V): joint v keeps row r*P + node_type[v]"""
    n, R, V = proj.shape
    KM = R // P
    dev = proj.device
    rows = torch.arange(KM, device=dev)[:, None] * P + (torch.as_tensor(node_type).long().to(dev)[None, :] if P > 1 else 0)
    return torch.gather(proj, 1, rows.expand(KM, V).unsqueeze(0).expand(n, KM, V))


def adjacency(xbar, A, alpha, beta, w1, b1, w2, b2, we, be, node_type, edge_type, P, add_type, subset_wise):
    """xbar (n, Ci, V) -> Ahat (n, KM, V, V); we / be None: no edge attention."""
    n, _, V = xbar.shape
    x1 = typed_select(_conv(xbar, w1, b1), node_type, P)
    x2 = typed_select(_conv(xbar, w2, b2), node_type, P)
    KM = x1.shape[1]
    m = KM // 3
    diff = x1[..., :, None] - x2[..., None, :]                                # (n, KM, V, V)
    if we is None:
        D = diff
    else:
        E = we.shape[0] // KM
        # edge_linears(diff) = We x1[u] + be - We x2[w]: the class eps(u, w) of each pair picks its row block
        pe = _conv(x1, we, be).view(n, 3, E, m, V).permute(2, 4, 0, 1, 3)    # (E, V, n, 3, m)
        qe = (_conv(x2, we, torch.zeros_like(be))).view(n, 3, E, m, V).permute(2, 4, 0, 1, 3)
        et = torch.as_tensor(edge_type).long().reshape(V, V).to(xbar.device)
        j = torch.arange(V, device=xbar.device)
        att = pe[et, j[:, None]] - qe[et, j[None, :]]                        # (V, V, n, 3, m)
        att = att.permute(2, 3, 4, 0, 1).reshape(n, KM, V, V)
        D = diff + att if add_type else att
    a = alpha if subset_wise else alpha[0].expand(3)
    b = beta if subset_wise else beta[0].expand(3)
    gram = torch.einsum('nkcu,nkcw->nkuw', x1.view(n, 3, m, V), x2.view(n, 3, m, V))
    soft = torch.softmax(gram, dim=-2)
    ahat = (A[None, :, None] + a.view(1, 3, 1, 1, 1) * torch.tanh(D.view(n, 3, m, V, V))
            + b.view(1, 3, 1, 1, 1) * soft[:, :, None])
    return ahat.reshape(n, KM, V, V)


def _bn_train(z, w, b, eps=1e-5):
    mean = z.mean(dim=(0, 2, 3), keepdim=True)
    var = z.var(dim=(0, 2, 3), unbiased=False, keepdim=True)
    return (z - mean) / torch.sqrt(var + eps) * w.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)


def unit_forward(p, x, node_type, edge_type, P, add_type, subset_wise):
    """p: the unit's parameters by state_dict key (train-mode BatchNorm, batch statistics) -> relu(bn(post) + res)"""
    edge = 'edge_linears.weight' in p
    ahat = adjacency(x.mean(2), p['A'], p['alpha'], p['beta'], p['conv1.weight'], p['conv1.bias'], p['conv2.weight'],
                     p['conv2.bias'], p['edge_linears.weight'] if edge else None, p['edge_linears.bias'] if edge else None,
                     node_type, edge_type, P, add_type, subset_wise)
    pre = torch.relu(_bn_train(_conv(x, p['pre.0.weight'], p['pre.0.bias']), p['pre.1.weight'], p['pre.1.bias']))
    y = torch.einsum('nctv,ncvw->nctw', pre, ahat)
    out = _bn_train(_conv(y, p['post.weight'], p['post.bias']), p['bn.weight'], p['bn.bias'])
    if 'down.0.weight' in p:
        res = _bn_train(_conv(x, p['down.0.weight'], p['down.0.bias']), p['down.1.weight'], p['down.1.bias'])
    else:
        res = x
    return torch.relu(out + res)


# ---- compact fixture form ----------------------------------------------------------------------------------------------
# tests/golden/unit_dghgcn.npz keeps arrays of up to FULL_MAX elements whole (fp64) and every larger one as `probe(a, key)`:
# its fp64 products with PROBES fixed Gaussian directions (seeded by the array's key).  A difference e between two arrays
# shows in the probes with |Q e| ~ sqrt(PROBES) |e|, so |probe(a) - probe(b)| / |probe(b)| estimates the relative L2 error
# |a - b| / |b|; the full arrays of the unit (n = 2, T = 8) would make a fixture of tens of MB.
FULL_MAX = 4096
PROBES = 32


def probe(a, key):
    import zlib
    import numpy as np
    v = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).reshape(-1)
    g = torch.Generator().manual_seed(zlib.crc32(key.encode()))
    q = torch.randn(PROBES, v.numel(), generator=g, dtype=torch.float64)
    return (q @ v).numpy()


def unit_inputs(ci, co, V, seed):
    """The unit fixture's input x (2, ci, 8, V) and output probe R (2, co, 8, V), fp32, regenerated from their seed."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, ci, 8, V, generator=g), torch.randn(2, co, 8, V, generator=g)


def fixture_rel(z, key, a):
    """Relative L2 difference of array `a` from fixture entry `key` (whole, or through its probes)."""
    import numpy as np
    a = np.asarray(a, dtype=np.float64)
    if key in z:
        want = np.asarray(z[key], dtype=np.float64)
        return float(np.linalg.norm(a - want) / (np.linalg.norm(want) + 1e-300))
    want = z[key + '_probe']
    return float(np.linalg.norm(probe(a, key) - want) / (np.linalg.norm(want) + 1e-300))


def fixture_is_zero(z, key):
    import numpy as np
    return not np.any(z[key] if key in z else z[key + '_probe'])
