"""Restatement of ``dgmsmlp`` (DGSTGCN's "mlp" temporal unit) and of its window stage in plain torch ops, written from
the unit's equations, any dtype: the GPU tests run it in fp64 as truth.  ``temporal_dgmlp`` is the one call the unit adds
to the op namespace, in torch (tests/test_dgmsmlp_host.py puts it beside ``torch_ops`` so that the module's wiring runs on
the CPU under ``kernels.use_ops``) and pins the restatement to the reference's fp64 outputs
(tests/golden/unit_dgmsmlp.npz).

  h  = relu(bn(z | zaug)) on channels < n_act, raw on the '1x1' window          (V + 1 columns)
  dw[c,t',v] = b[c] + sum_k w[c,k] h[c, t'*stride - (KM-1-k)*d, v]              (zero for frames < 0; KM = (k+1)/2)
  tc = alpha * dilated (k,1) conv of h                                          (add_tcn)
  u  = W1.dw + b1 + tc  (merge_after) | W1.(dw + tc) + b1 | W1.dw + b1  (no add_tcn);  max-pool / strided copy elsewhere
  f  = u[..., :V] + u[..., V] * add_coeff[:V]"""
import torch
import torch.nn.functional as F

from dghgcn_fp64 import fixture_is_zero, fixture_rel, probe  # noqa: F401  (the compact fixture form)

FULL_MAX = 512        # fixture arrays up to this size are kept whole, larger ones as 32 projections

DEFAULT_CFG = [(3, 1), (3, 2), (3, 3), (3, 4), ('max', 3), '1x1']

# (tag, C, stride, T, V, constructor switches): the smallest shapes at which the window kernel can go wrong
CASES = [
    ('d64', 64, 1, 9, 25, {}),                                           # widths 14/10: K no multiple of 4; T odd
    ('d128s2', 128, 2, 9, 25, {}),                                       # widths 23/21; T' = 5; stride in the taps
    ('tcn_after', 64, 1, 9, 25, dict(add_tcn=True, merge_after=True)),   # addend after the mix
    ('tcn_before_s2', 128, 2, 8, 25, dict(add_tcn=True, adaptive=False)),    # addend before the mix; buffer alpha
    ('short', 64, 1, 3, 25, {}),                                         # T < the reach of dilations 3, 4: mostly zero padding
    ('coco', 64, 2, 9, 17, dict(add_tcn=True, merge_after=True)),        # V1 = 18
    ('k5', 64, 1, 9, 25, dict(ms_cfg=[(5, 1), (5, 2), ('max', 3), '1x1'])),  # KM = 3, widths 16/16
    ('wide', 256, 1, 5, 25, {}),                                         # widths 46/42: three 16-row tiles, two padded rows
]


def case(tag):
    for c in CASES:
        if c[0] == tag:
            return dict(tag=tag, C=c[1], stride=c[2], T=c[3], V=c[4], kw=dict(c[5]))
    raise KeyError(tag)


def unit_kwargs(c):
    """constructor kwargs of fixture case c (num_joints follows the layout)"""
    return dict(num_joints=c['V'], stride=c['stride'], **c['kw'])


def unit_inputs(c, seed, n=2):
    """The unit fixture's input x (n, C, T, V) and output probe R (n, C, T', V), fp32, regenerated from their seed."""
    g = torch.Generator().manual_seed(seed)
    Tout = (c['T'] + c['stride'] - 1) // c['stride']
    return torch.randn(n, c['C'], c['T'], c['V'], generator=g), torch.randn(n, c['C'], Tout, c['V'], generator=g)


def liven_unit(m, seed):
    """add_coeff and every learnable alpha get N(0, 0.25) values (the constructor leaves zeros: the global joint and the
    dilated conv would not show), every BatchNorm weight 0.5 + U(0, 1) (the constructor leaves 1: an error in front of a
    BatchNorm would hide) and every BatchNorm bias N(0, 0.09): with a zero bias the max-pool branch relu(g * xhat) is
    homogeneous in its BatchNorm weight g, transform.0 normalises the same channel, and the gradient of g is zero up to eps
    — nothing a relative bar could be applied to.  Walks the module in definition order, so the reference class and ours
    draw the same values."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith(('alpha', 'add_coeff')):
                p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64).to(p.dtype) * 0.5)
        for _, mod in m.named_modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.copy_(0.5 + torch.rand(mod.weight.shape, generator=g, dtype=torch.float64).to(mod.weight.dtype))
                mod.bias.copy_(0.3 * torch.randn(mod.bias.shape, generator=g, dtype=torch.float64).to(mod.bias.dtype))


def _conv(z, w, b):
    out = torch.einsum('oc,nc...->no...', w.reshape(w.shape[0], -1), z)
    return out + b.reshape((1, -1) + (1,) * (z.dim() - 2))


def _bn(z, w, b, mean=None, var=None, eps=1e-5):
    if mean is None:
        mean, var = z.mean(dim=(0, 2, 3)), z.var(dim=(0, 2, 3), unbiased=False)
    c = lambda t: t.view(1, -1, 1, 1)        # noqa: E731
    return (z - c(mean)) / torch.sqrt(c(var) + eps) * c(w) + c(b)


def causal_taps(h, w, b, d, stride):
    """h (n, bc, T, X), w (bc, KM), b (bc) -> (n, bc, T', X): left zero pad by (KM-1)*d frames, taps d apart, every
    stride-th frame."""
    KM = w.shape[1]
    T = h.shape[2]
    Tout = (T + stride - 1) // stride
    xp = F.pad(h, (0, 0, (KM - 1) * d, 0))
    out = b.view(1, -1, 1, 1)
    for j in range(KM):
        out = out + w[:, j].view(1, -1, 1, 1) * xp[:, :, j * d:j * d + (Tout - 1) * stride + 1:stride]
    return out


def dilated_conv(h, w, b, d, stride):
    k = w.shape[2]
    pad = (k + (k - 1) * (d - 1) - 1) // 2
    return F.conv2d(h, w, b, stride=(stride, 1), padding=(pad, 0), dilation=(d, 1))


def windows(h, branch_cfg, widths, conv_w, conv_b, dw_w, dw_b, w1s, b1s, merge_after, stride):
    """The window stage: h (n, C, T, X) activated -> u (n, C, T', X).  conv_w / conv_b: the dilated convs already scaled by
    alpha (None or empty: no add_tcn); dw_w (C, KM), dw_b (C) by channel; w1s / b1s per mlp window."""
    outs = []
    c0 = mi = 0
    for cfg, bc in zip(branch_cfg, widths):
        hb = h[:, c0:c0 + bc]
        if cfg == '1x1':
            outs.append(hb[:, :, ::stride])
        elif cfg[0] == 'max':
            outs.append(F.max_pool2d(hb, (cfg[1], 1), (stride, 1), (1, 0)))
        else:
            d = int(cfg[1])
            dw = causal_taps(hb, dw_w[c0:c0 + bc], dw_b[c0:c0 + bc], d, stride)
            mix = lambda t, i=mi: _conv(t, w1s[i], b1s[i])        # noqa: E731
            if conv_w:
                tc = dilated_conv(hb, conv_w[mi], conv_b[mi], d, stride)
                outs.append(mix(dw) + tc if merge_after else mix(dw + tc))
            else:
                outs.append(mix(dw))
            mi += 1
        c0 += bc
    return torch.cat(outs, 1)


def temporal_dgmlp(z, zaug, scale, shift, n_act, branch_cfg, widths, conv_w, conv_b, dw_w, dw_b, dw_dil, w1s, b1s,
                   add_coeff, merge_after, stride, gamma=None, beta=None, eps=1e-5, want_bn=False):
    """``kernels.temporal_dgmlp`` in plain torch ops."""
    n, C, T, V = z.shape
    bc_ = lambda p: p.view(1, -1, 1, 1)        # noqa: E731
    h = torch.cat([z, zaug[..., None]], -1) * bc_(scale) + bc_(shift)
    h = torch.cat([F.relu(h[:, :n_act]), h[:, n_act:]], 1)
    u = windows(h, branch_cfg, widths, conv_w, conv_b, dw_w, dw_b, w1s, b1s, merge_after, int(stride))
    f = u[..., :V] + u[..., V, None] * add_coeff[:V]
    if not want_bn:
        return f, None, None, None, None
    mean = f.mean((0, 2, 3))
    var = f.var((0, 2, 3), unbiased=False)
    g = gamma if gamma is not None else f.new_ones(C)
    b = beta if beta is not None else f.new_zeros(C)
    sc = g * torch.rsqrt(var + eps)
    return f, sc, b - mean * sc, mean.detach(), var.detach()


def unit_forward(p, x, ms_cfg=None, stride=1, merge_after=False, running=None):
    """p: the unit's state by state_dict key (parameters; ``alpha`` may be a buffer or absent) -> bn(transform(f)).
    add_tcn is read from the keys (``conv2``).  running: running statistics by key for eval mode, None = batch statistics."""
    ms_cfg = DEFAULT_CFG if ms_cfg is None else ms_cfg
    N, C, T, V = x.shape
    xa = torch.cat([x, x.mean(-1, keepdim=True)], -1)
    r = (lambda key: None) if running is None else running.get
    outs = []
    for i, cfg in enumerate(ms_cfg):
        pre = f'branches.{i}.'
        if cfg == '1x1':
            outs.append(_conv(xa[:, :, ::stride], p[pre + 'weight'], p[pre + 'bias']))
            continue
        hb = torch.relu(_bn(_conv(xa, p[pre + '0.weight'], p[pre + '0.bias']), p[pre + '1.weight'], p[pre + '1.bias'],
                            r(pre + '1.running_mean'), r(pre + '1.running_var')))
        if cfg[0] == 'max':
            outs.append(F.max_pool2d(hb, (cfg[1], 1), (stride, 1), (1, 0)))
            continue
        d = int(cfg[1])
        dw = causal_taps(hb, p[pre + '3.conv.weight'].flatten(1), p[pre + '3.conv.bias'], d, stride)
        mix = lambda t, q=pre: _conv(t, p[q + '3.conv1.weight'], p[q + '3.conv1.bias'])        # noqa: E731
        if pre + '3.conv2.weight' in p:
            alpha = p[pre + '3.alpha'] if pre + '3.alpha' in p else 1.0
            tc = alpha * dilated_conv(hb, p[pre + '3.conv2.weight'], p[pre + '3.conv2.bias'], d, stride)
            outs.append(mix(dw) + tc if merge_after else mix(dw + tc))
        else:
            outs.append(mix(dw))
    o = torch.cat(outs, 1)
    f = o[..., :V] + o[..., V, None] * p['add_coeff'][:V]
    t = _bn(f, p['transform.0.weight'], p['transform.0.bias'], r('transform.0.running_mean'), r('transform.0.running_var'))
    t = _conv(torch.relu(t), p['transform.2.weight'], p['transform.2.bias'])
    return _bn(t, p['bn.weight'], p['bn.bias'], r('bn.running_mean'), r('bn.running_var'))
