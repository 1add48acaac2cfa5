"""RNG-free weights and inputs of the full-size fixtures (tests/golden/full_size.npz): shared by the generator
(reference side) and the tests (this repo's side), so only outputs need to be stored."""
import torch


def closed_form_fill(module):
    """Deterministic, RNG-free weights for the full-size fixtures: every floating tensor gets
    scale * sin(0.37*i + phase(name)); BatchNorm scales ~1, running_var > 0; alpha/beta/add_coeff alive."""
    import zlib
    with torch.no_grad():
        for k, v in module.state_dict().items():
            if not v.dtype.is_floating_point:
                continue
            i = torch.arange(v.numel(), dtype=torch.float64)
            phase = (zlib.crc32(k.encode()) % 1000) / 1000.0 * 6.283185307179586
            wave = torch.sin(0.37 * i + phase).reshape(v.shape)
            if k.endswith('running_var'):
                t = 1.0 + 0.25 * wave
            elif k.endswith('running_mean'):
                t = 0.05 * wave
            elif k.endswith('weight') and v.dim() == 1:            # BatchNorm gamma
                t = 1.0 + 0.1 * wave
            elif k.endswith('bias'):
                t = 0.02 * wave
            elif k.endswith(('alpha', 'beta', 'add_coeff')):
                t = 0.5 * wave
            elif k.endswith('.A') or k == 'backbone.A':
                t = 0.04 + 0.02 * wave
            else:
                fan_in = max(1, v[0].numel()) if v.dim() > 1 else 1
                t = wave * (1.5 / fan_in) ** 0.5
            v.copy_(t.to(v.dtype))


def counter_input(N, T, V, classes):
    i = torch.arange(N * 2 * T * V * 3, dtype=torch.float64)
    x = (torch.sin(0.0137 * i) + 0.3 * torch.cos(0.00071 * i * i % 6.283185307179586)).reshape(N, 1, 2, T, V, 3).float()
    y = (torch.arange(N) * 7 % classes).reshape(N, 1)
    return x, y


def liven32(module, seed, scale=0.5):
    """alpha / beta / add_coeff ~ N(0, scale^2) (default 0.5) from a seeded generator (zero-init would switch the dynamic-adjacency
    and global-joint paths off): the bench's and the round-2 fixtures' way of making a default-initialised model live."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in module.named_parameters():
            if k.endswith(('alpha', 'beta', 'add_coeff')):
                p.copy_(torch.randn(p.shape, generator=g) * scale)


def fill_running(module):
    """RNG-free BatchNorm running statistics (eval-mode fixtures): mean 0.05*sin, var 1 + 0.25*sin, phase by key."""
    import zlib
    with torch.no_grad():
        for k, v in module.state_dict().items():
            if not k.endswith(('running_mean', 'running_var')):
                continue
            i = torch.arange(v.numel(), dtype=torch.float64)
            phase = (zlib.crc32(k.encode()) % 1000) / 1000.0 * 6.283185307179586
            wave = torch.sin(0.37 * i + phase).reshape(v.shape)
            v.copy_((1.0 + 0.25 * wave if k.endswith('running_var') else 0.05 * wave).to(v.dtype))


def calibrate_running(model, x, extract):
    """Running statistics of a plausible trained state (eval-mode fixtures): one train-mode pass over `x` with momentum 1
    (running = batch statistics), then the closed-form wobble of fill_running scaled to them — closed-form statistics
    alone leave activations mis-scaled, which the quadratic Gram terms of the CTR variants amplify to overflow."""
    import zlib
    bns = [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    saved = [m.momentum for m in bns]
    for m in bns:
        m.momentum = 1.0
    model.train()
    with torch.no_grad():
        extract(model, x)
    for m, mom in zip(bns, saved):
        m.momentum = mom
    with torch.no_grad():
        sd = model.state_dict()
        for k, v in sd.items():
            if not k.endswith(('running_mean', 'running_var')):
                continue
            i = torch.arange(v.numel(), dtype=torch.float64)
            phase = (zlib.crc32(k.encode()) % 1000) / 1000.0 * 6.283185307179586
            wave = torch.sin(0.37 * i + phase).reshape(v.shape).to(v.dtype)
            if k.endswith('running_var'):
                v.mul_(1.0 + 0.1 * wave)
            else:
                v.add_(0.05 * wave * sd[k[:-len('running_mean')] + 'running_var'].sqrt())
    return model.eval()


def counter_clips(N, clips, T, V):
    """(N, clips, 2, T, V, 3) test-time input (several views per sample), closed form."""
    i = torch.arange(N * clips * 2 * T * V * 3, dtype=torch.float64)
    x = torch.sin(0.0211 * i) + 0.3 * torch.cos(0.00053 * i * i % 6.283185307179586)
    return x.reshape(N, clips, 2, T, V, 3).float()


def eval_clips(name, T, V):
    """(2, 10, 2, T, V, 3) test-time input of the eval fixture `name`."""
    return counter_clips(2, 10, T, V)


# alpha / beta scale of the eval fixtures.  The shipped CTR-GCN variant carries an unbounded quadratic Gram term (beta *
# x1^T x2, no softmax): in eval mode (no batch renormalisation) a random-init network with beta != 0 overflows fp32
# within a few blocks on any clip other than the one its running statistics came from (measured on the reference:
# 7e2 -> 2e5 -> 1e13 -> inf over blocks 5-8).  Its eval fixture therefore keeps the reference's own initial state
# alpha = beta = 0; the dynamic terms are pinned by the train-mode fixtures (full_grads_*, unit_others).
EVAL_LIVEN = {'ctrgcn_shipped_ntu60': 0.0}


def pick_tensors(named_numels, count=12, max_numel=70000):
    """A fixed, name-ordered selection of `count` gradient tensors (each <= max_numel elements) spread over the
    parameter list — the tensors whose full fp64 gradients the full-size fixtures store."""
    names = [k for k, n in named_numels if n <= max_numel]
    if len(names) <= count:
        return names
    idx = sorted({round(j * (len(names) - 1) / (count - 1)) for j in range(count)})
    return [names[i] for i in idx]


UNIT_CASES = {       # tag -> (class name, ctor args after the graph, input shape): the same call builds the reference's
    'gcn': ('unit_gcn', dict(in_channels=64, out_channels=128, adaptive='init'), (2, 64, 8, 25)),           # unit and ours
    'gcn_res': ('unit_gcn', dict(in_channels=64, out_channels=128, adaptive='init', with_res=True), (2, 64, 8, 25)),
    'tcn9': ('unit_tcn', dict(in_channels=64, out_channels=64, kernel_size=9, stride=1), (2, 64, 8, 25)),
    'tcn1s2': ('unit_tcn', dict(in_channels=64, out_channels=128, kernel_size=1, stride=2), (2, 64, 8, 25)),
    'ctrgcn': ('unit_ctrgcn', dict(in_channels=64, out_channels=128), (2, 64, 8, 25)),
    'MSTCN': ('MSTCN', dict(in_channels=64, out_channels=64, kernel_size=5, stride=1, dilations=[1, 2], residual=False),
              (2, 64, 8, 25)),
    'MSTCNs2': ('MSTCN', dict(in_channels=64, out_channels=128, kernel_size=5, stride=2, dilations=[1, 2], residual=True),
                (2, 64, 8, 25)),
    'gcn_offset_post': ('unit_gcn', dict(in_channels=64, out_channels=128, adaptive='offset', conv_pos='post'), (2, 64, 8, 25)),
    'gcn_importance': ('unit_gcn', dict(in_channels=64, out_channels=64, adaptive='importance', with_res=True), (2, 64, 8, 25)),
    'gcn_fixed_post': ('unit_gcn', dict(in_channels=3, out_channels=64, adaptive=None, conv_pos='post'), (2, 3, 8, 25)),
    # the heterogeneous CTR unit with the shipped config's flags (configs/ctrgcn/CTRGCN_model.py)
    'ctrhgcn': ('unit_ctrhgcn', dict(in_channels=64, out_channels=128, semantic_index=True, node_attention=True,
                                     edge_attention=True, add_type=False, ada=True, num_types=5, rel_reduction=8,
                                     edge_num=15), (2, 64, 8, 25)),
    'msmlp': ('msmlp', dict(in_channels=64, out_channels=64, stride=1, add_tcn=True, merge_after=True), (2, 64, 8, 25)),
    'msmlp_s2': ('msmlp', dict(in_channels=128, out_channels=128, stride=2, add_tcn=True, merge_after=False), (2, 128, 8, 25)),
    'ctrhgcn_same': ('unit_ctrhgcn', dict(in_channels=64, out_channels=64, semantic_index=True, node_attention=True,
                                          edge_attention=True, ada=True), (2, 64, 8, 25)),
    # unitmlp as the whole temporal unit of the shipped ST-GCN config (configs/stgcn/STGCN_model.py: kernel 9 -> 5 causal taps)
    'unitmlp9': ('unitmlp', dict(in_channels=64, out_channels=64, kernel_size=9, stride=1, add_tcn=True, merge_after=True),
                 (2, 64, 12, 25)),
    'unitmlp9_s2': ('unitmlp', dict(in_channels=128, out_channels=128, kernel_size=9, stride=2, add_tcn=True,
                                    merge_after=False), (2, 128, 12, 25)),
}


def make_unit(ns, tag, A, edge_type=None, node_type=None):
    """Build unit `tag` from namespace `ns` (the reference's gcns.utils or this package) with seeded default init,
    live alpha/beta and BatchNorm affines away from (1, 0); -> (module fp32, input fp32, cotangent R fp32).
    edge_type (V,V) / node_type (V): the graph's type tables, needed by the heterogeneous units."""
    idx = list(UNIT_CASES).index(tag)
    cls, kw, shape = UNIT_CASES[tag]
    kw = dict(kw)
    if cls in ('unit_gcn', 'unit_ctrgcn', 'unit_ctrhgcn'):
        kw['A'] = A.clone()
    if cls == 'unit_ctrhgcn':
        kw['edge_type'] = torch.as_tensor(edge_type, dtype=torch.float32)
        kw['node_type'] = torch.as_tensor(node_type)
    torch.manual_seed(300 + idx)
    m = getattr(ns, cls)(**kw)
    liven32(m, 40 + idx)
    g = torch.Generator().manual_seed(50 + idx)
    with torch.no_grad():
        if hasattr(m, 'PA'):                                   # offset / importance: move PA off its init value
            m.PA.add_(torch.randn(m.PA.shape, generator=g) * 0.05)
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.2)
    x = torch.randn(*shape, generator=g)
    stride = kw.get('stride', 1)
    yshape = (shape[0], kw['out_channels'], (shape[2] + stride - 1) // stride, shape[3])
    Rm = torch.randn(*yshape, generator=g)
    return m.train(), x, Rm


def sd_digest(module):
    import hashlib
    h = hashlib.sha256()
    for k, v in module.state_dict().items():
        h.update(k.encode())
        h.update(v.detach().cpu().numpy().tobytes())
    return h.hexdigest()


# The two headline units of DS-STGCN at every width the model uses (round 3): tag -> (class, layout, ctor kwargs, input shape)
DS_KW = dict(ratio=0.125, decompose=True, node_attention=True, edge_attention=True, subset_wise=True, ctr='T', ada='T')
DS_UNIT_CASES = {
    'g3_64': ('dgphgcn1', 'nturgb+d', dict(in_channels=3, out_channels=64), (2, 3, 8, 25)),
    'g64_64': ('dgphgcn1', 'nturgb+d', dict(in_channels=64, out_channels=64), (2, 64, 8, 25)),
    'g64_128': ('dgphgcn1', 'nturgb+d', dict(in_channels=64, out_channels=128), (2, 64, 8, 25)),
    'g128_128': ('dgphgcn1', 'nturgb+d', dict(in_channels=128, out_channels=128), (2, 128, 8, 25)),
    'g128_256': ('dgphgcn1', 'nturgb+d', dict(in_channels=128, out_channels=256), (3, 128, 4, 25)),
    'g256_256': ('dgphgcn1', 'nturgb+d', dict(in_channels=256, out_channels=256), (3, 256, 4, 25)),
    'g64_64_coco': ('dgphgcn1', 'coco', dict(in_channels=64, out_channels=64), (2, 64, 10, 17)),
    't64': ('dgmstcn', 'nturgb+d', dict(in_channels=64, out_channels=64, stride=1), (2, 64, 8, 25)),
    't128_s2': ('dgmstcn', 'nturgb+d', dict(in_channels=128, out_channels=128, stride=2), (2, 128, 8, 25)),
    't256': ('dgmstcn', 'nturgb+d', dict(in_channels=256, out_channels=256, stride=1), (3, 256, 4, 25)),
    't64_s2_coco': ('dgmstcn', 'coco', dict(in_channels=64, out_channels=64, stride=2, num_joints=17), (2, 64, 10, 17)),
}


def make_ds_unit(ns, graph_cls, tag):
    """Build the DS-STGCN unit `tag` from namespace `ns` (the reference's gcns.utils or this package) with the graph class
    of the same side: seeded default init (the random graph draws from numpy's RNG), live alpha / beta / add_coeff,
    BatchNorm affines away from (1, 0); -> (module fp32, input fp32, cotangent R fp32)."""
    import numpy as np
    idx = list(DS_UNIT_CASES).index(tag)
    cls, layout, kw, shape = DS_UNIT_CASES[tag]
    kw = dict(kw)
    np.random.seed(600 + idx)
    torch.manual_seed(600 + idx)
    if cls == 'dgphgcn1':
        G = graph_cls(layout=layout, mode='random', num_filter=3, init_off=.04, init_std=.02)
        m = getattr(ns, cls)(kw['in_channels'], kw['out_channels'], torch.tensor(G.A, dtype=torch.float32),
                             torch.tensor(G.edge_type, dtype=torch.float32), torch.tensor(G.node_type), **DS_KW)
    else:
        m = getattr(ns, cls)(**kw)
    liven32(m, 700 + idx)
    g = torch.Generator().manual_seed(800 + idx)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.2)
    x = torch.randn(*shape, generator=g)
    stride = kw.get('stride', 1)
    Rm = torch.randn(shape[0], kw['out_channels'], (shape[2] + stride - 1) // stride, shape[3], generator=g)
    return m.train(), x, Rm


def step_input(step, N, T, V, classes):
    """Closed-form batch `step` of the training-trajectory fixture: (N,1,2,T,V,3) clips and (N,1) labels."""
    i = torch.arange(N * 2 * T * V * 3, dtype=torch.float64) + 1000003.0 * step
    x = (torch.sin(0.0137 * i) + 0.3 * torch.cos(0.00071 * i * i % 6.283185307179586)).reshape(N, 1, 2, T, V, 3).float()
    y = ((torch.arange(N) * 7 + 3 * step) % classes).reshape(N, 1)
    return x, y


# The fp64 oracle-vs-reference cases (gen_golden_fp64.py, the *_vs_reference_live tests): group -> the cases it builds
REF64_GROUPS = ('aagcn', 'dgphgcn1', 'dggcn', 'temporal')


def make_ref64_group(ns, graph_cls, group):
    """Build the cases of `group` from namespace `ns` (the reference's gcns.utils or this package) with the graph class of
    the same side: seeded default init, live alpha / beta / add_coeff, then an fp64 input drawn from the same global RNG
    stream; -> [(name, module fp64 in train mode, input fp64)].  Weights and inputs are rebuilt, never stored: the
    fixture keeps their digests (sd_digest, array_digest)."""
    import numpy as np
    out = []
    if group == 'aagcn':
        torch.manual_seed(4)
        A = torch.tensor(graph_cls(layout='coco', mode='spatial').A, dtype=torch.float32)
        for i, (ci, co) in enumerate(((48, 48), (32, 64))):
            m = ns.unit_aagcn(ci, co, A.clone())
            m.init_weights()
            with torch.no_grad():
                m.alpha.normal_(0, .5)
                m.conv_ta.weight.normal_(0, .1)
                m.fc2c.weight.normal_(0, .05)
                m.bn.weight.fill_(1.0)
            m = m.double()
            out.append((f'aagcn{i}', m, torch.randn(2, ci, 10, 17, dtype=torch.float64)))
    elif group == 'dgphgcn1':
        torch.manual_seed(1)
        np.random.seed(1)
        G = graph_cls(layout='coco', mode='random', num_filter=3, init_off=.04, init_std=.02)
        m = ns.dgphgcn1(64, 64, torch.tensor(G.A, dtype=torch.float32), torch.tensor(G.edge_type, dtype=torch.float32),
                        torch.tensor(G.node_type), ratio=0.125, decompose=True, node_attention=True, edge_attention=True,
                        subset_wise=True, ctr='T', ada='T').double()
        with torch.no_grad():
            m.alpha.normal_(0, .5)
            m.beta.normal_(0, .5)
        out.append(('dgphgcn1', m, torch.randn(2, 64, 10, 17, dtype=torch.float64)))
    elif group == 'dggcn':
        torch.manual_seed(2)
        np.random.seed(2)
        G = graph_cls(layout='coco', mode='random', num_filter=3, init_off=.04, init_std=.02)
        A = torch.tensor(G.A, dtype=torch.float32)
        for i, (ci, co, sw) in enumerate(((48, 48, False), (32, 64, True))):
            m = ns.dggcn(ci, co, A, ratio=0.25, subset_wise=sw).double()
            with torch.no_grad():
                m.alpha.normal_(0, .5)
                m.beta.normal_(0, .5)
            out.append((f'dggcn{i}', m, torch.randn(2, ci, 10, 17, dtype=torch.float64)))
    elif group == 'temporal':
        for cls, stride in (('dgmstcn', 1), ('dgmstcn', 2), ('mstcn', 1), ('mstcn', 2)):
            torch.manual_seed(5)
            m = getattr(ns, cls)(64, 64, stride=stride).double()
            with torch.no_grad():
                if hasattr(m, 'add_coeff'):
                    m.add_coeff.normal_(0, .5)
            out.append((f'temporal_{cls}_s{stride}', m, torch.randn(2, 64, 10, 25, dtype=torch.float64)))
    else:
        raise KeyError(group)
    return [(name, m.train(), x) for name, m, x in out]


def array_digest(t):
    import hashlib
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


def ref64_sample(n, count=512):
    """Fixed, spread-out flat positions (multiplicative hashing, no RNG) at which the fp64 fixture keeps an output's
    values; every element is also covered by the fixture's per-(channel, frame) sums."""
    import numpy as np
    return np.unique((np.arange(count, dtype=np.int64) * 2654435761) % n)
