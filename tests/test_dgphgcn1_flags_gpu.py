"""-m gpu: the ``dgphgcn1`` switches on the HIP path — the flag-specialised K-B (csrc/dynadj_flags.hip) behind
``kernels.dynadj_flags`` — against the reference's fixtures (tests/golden/unit_dgphgcn1_flags.npz, model_reduced_ds_*),
against the fp64 restatement (tests/dgphgcn1_flags_fp64.py) at full batch for every compile-time instantiation, through a
captured TrainEngine step of a ``gcn_stage`` model, and a guard that the shipped flag set still calls today's K-B.
The bars are the ones tests/test_dghgcn_gpu.py uses for the same comparisons."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import dsgcn_amd as D
import dgphgcn1_flags_fp64 as F
from test_dgphgcn1_flags_host import CASES, MODELS, Z, ZERO_GRAD_BIASES, ds_cfg, make_unit, unit_inputs
from test_oracle_golden import GOLD, load, rel, sd_of

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('tag', CASES)
def test_unit_vs_reference_fixture(tag):
    """Output 1e-5, input gradient 5e-5, every parameter gradient 1e-4, against the reference's fp64 fixture (whole arrays
    or their probes) and element by element against the fp64 restatement of the same weights."""
    m, fl = make_unit(tag)
    with torch.no_grad():
        m.alpha.copy_(torch.from_numpy(Z[tag + '_alpha']))
        m.beta.copy_(torch.from_numpy(Z[tag + '_beta']))
    p64 = {k: v.detach().double().cuda().requires_grad_() for k, v in m.named_parameters()}
    m = m.cuda().train()
    x32, r32 = unit_inputs(tag)
    x = x32.cuda().requires_grad_()
    y = m(x)
    (y * r32.cuda()).sum().backward()
    x64 = x32.double().cuda().requires_grad_()
    y64 = F.unit_forward(p64, x64, Z[tag + '_node_type'], Z[tag + '_edge_type'], fl)
    (y64 * r32.double().cuda()).sum().backward()
    for got, want, key, bar in ((y, y64, '_y', 1e-5), (x.grad, x64.grad, '_dx', 5e-5)):
        e_fix = F.fixture_rel(Z, tag + key, got.detach().cpu().numpy())
        e_ful = rel(got.detach().cpu(), want.detach().cpu())
        print(tag, key, e_fix, e_ful)
        assert e_fix < bar and e_ful < bar, (key, e_fix, e_ful)
    for k, p in m.named_parameters():
        key = tag + '_grad_' + k
        if k in ZERO_GRAD_BIASES:
            continue
        if F.fixture_is_zero(Z, key):              # conv2_se (quirk Q1); alpha[1:], beta[1:] without subset_wise
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
        else:
            e_fix = F.fixture_rel(Z, key, p.grad.cpu().numpy())
            e_ful = rel(p.grad.cpu(), p64[k].grad.cpu())
            print(tag, k, e_fix, e_ful)
            assert e_fix < 1e-4 and e_ful < 1e-4, (k, e_fix, e_ful)


def test_subset_wise_off_gives_zero_not_none():
    m, _ = make_unit('subset_off')
    m = m.cuda().train()
    x32, r32 = unit_inputs('subset_off')
    (m(x32.cuda()) * r32.cuda()).sum().backward()
    for p in (m.alpha, m.beta):
        assert p.grad is not None and p.grad.shape == (3,) and float(p.grad[1:].abs().max()) == 0.0


def _reduced(arm):
    name = 'model_reduced_ds_' + arm
    z = load(name + '.npz')
    with open(os.path.join(GOLD, name + '_cfg.json')) as f:
        cfg = json.load(f)
    cfg['backbone']['tcn_ms_cfg'] = [tuple(c) if isinstance(c, list) else c for c in cfg['backbone']['tcn_ms_cfg']]
    m = D.build_model(copy.deepcopy(cfg))
    m.load_state_dict(sd_of(z, 'sd_', torch.float32))
    return z, cfg, m


@pytest.mark.parametrize('arm', MODELS)
def test_reduced_model_vs_golden(arm):
    """Logits and loss 1e-4, whole-gradient relative L2 2e-4, against the reference's fp64 run."""
    z, _, m = _reduced(arm)
    assert any(not b.gcn._shipped for b in m.backbone.gcn)
    m = m.cuda().train()
    x, y = torch.from_numpy(z['x']).cuda(), torch.from_numpy(z['label']).cuda()
    logits = m.cls_head(m.extract_feat(x[:, 0]))
    loss = m.cls_head.loss(logits, y.squeeze(-1))['loss_cls']
    loss.backward()
    e_log = rel(logits.detach().cpu(), z['logits_f64'])
    e_loss = abs(loss.item() - float(z['loss_f64'])) / abs(float(z['loss_f64']))
    num = den = 0.0
    for k, p in m.named_parameters():
        if 'g64_' + k in z:
            g64 = z['g64_' + k].astype(np.float64)
            got = p.grad.double().cpu().numpy() if p.grad is not None else np.zeros_like(g64)
            num += float(((got - g64) ** 2).sum())
            den += float((g64 ** 2).sum())
    err = (num / den) ** .5
    print(arm, e_log, e_loss, err)
    assert e_log < 1e-4 and e_loss < 1e-4, (e_log, e_loss)
    assert err < 2e-4, err                                    # whole-gradient relative L2 vs fp64 truth


@pytest.mark.parametrize('arm', MODELS)
def test_eval_logits_and_fuse_conv_bn(arm):
    z, _, m = _reduced(arm)
    m = m.cuda().eval()
    x = torch.from_numpy(z['x']).cuda()
    with torch.no_grad():
        logits = m.cls_head(m.extract_feat(x[:, 0]))
        assert rel(logits.cpu(), z['logits_eval_f64']) < 1e-4, rel(logits.cpu(), z['logits_eval_f64'])
        D.fuse_conv_bn(m)
        fused = m.cls_head(m.extract_feat(x[:, 0]))
    assert rel(fused.cpu(), logits.cpu()) <= 1e-5, rel(fused.cpu(), logits.cpu())


# flag word of csrc/dynadj_flags.hip -> constructor flags: every compile-time instantiation (SEM x EDGE x ADA x SW)
def _word_flags(w):
    sem = w & 3
    return dict(decompose=sem > 0, node_attention=sem == 2, edge_attention=bool(w & 4), ada_attention=bool(w & 8),
                subset_wise=bool(w & 16))


WORDS = [0, 1, 2, 5, 6, 8, 9, 10, 13, 14]
WORDS += [w | 16 for w in WORDS]
WORDS.remove(6 | 16)                      # the shipped flag set: today's K-B, not an instantiation of the new kernel
# every (Ci, Co) of the 10-stage DS-STGCN at ratio 0.125 on two instantiations, the others on a narrow and the widest layer
FULL = [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256)]
FULL_CASES = [(c, w) for c in FULL for w in (17, 6)] + [(c, w) for c in ((64, 64), (256, 256)) for w in WORDS
                                                        if w not in (17, 6)]


@pytest.mark.parametrize('case,word', FULL_CASES)
def test_flag_kb_full_size_vs_fp64(case, word):
    """n = 128, V = 25: Ahat (1e-5), the input gradient (of the time mean) and every parameter gradient (1e-4) of the
    adjacency path (K-C projections [+ K-C edge linear] + the flag K-B) against the fp64 restatement."""
    ci, co = case
    kw = _word_flags(word)
    g = D.Graph(layout='nturgb+d', mode='spatial')
    torch.manual_seed(7)
    np.random.seed(7)
    A = torch.tensor(np.asarray(D.Graph(layout='nturgb+d', mode='random', num_filter=3, init_off=.04, init_std=.02).A),
                     dtype=torch.float32)
    m = D.dgphgcn1(ci, co, A, torch.tensor(g.edge_type), torch.tensor(g.node_type), ratio=0.125, **kw)
    assert not m._shipped
    with torch.no_grad():
        m.alpha.normal_(0, 0.5)
        m.beta.normal_(0, 0.5)
    m = m.cuda()
    n, V = 128, 25
    gen = torch.Generator().manual_seed(11)
    xbar = torch.randn(n, ci, V, generator=gen).cuda().requires_grad_()
    dah = torch.randn(n, 3 * m.mid_channels, V, V, generator=gen).cuda()
    calls = _count_native()
    ahat = m.adjacency(xbar)
    (ahat * dah).sum().backward()
    _count_native(restore=calls)
    assert calls['dsgcn_dynflag_fwd'] == calls['dsgcn_dynflag_bwd'] == 1 and not calls['dsgcn_dynadj_fwd_jobs']
    names = [k for k, _ in m.named_parameters() if k.split('.')[0] in ('A', 'alpha', 'beta', 'conv1', 'conv2', 'conv1_se',
                                                                      'edge_linears', 'ada_linears')]
    params = dict(m.named_parameters())
    p64 = {k: params[k].detach().double().requires_grad_() for k in names}
    x64 = xbar.detach().double().requires_grad_()
    want = F.adjacency(x64, p64, m.node_type_idx, m.edge_type_idx, F.effective_flags(**kw))
    (want * dah.double()).sum().backward()
    e = rel(ahat.detach().cpu(), want.detach().cpu())
    assert e < 1e-5, e
    e = rel(xbar.grad.cpu(), x64.grad.cpu())
    assert e < 1e-4, e
    for k in names:
        if not kw['subset_wise'] and k in ('alpha', 'beta'):
            assert float(params[k].grad[1:].abs().max()) == 0.0
        e = rel(params[k].grad.cpu(), p64[k].grad.cpu())
        assert e < 1e-4, (k, e)


# (n, Ci, mid, V, P, E, columns of xbar): V = 17 / 32 / 11 take the generic-V instantiations (32: the full pair grid and the
# LDS maxima), mid = 5 / 3 / 9 leave a partial last round of the class bins (8 channels, 4 under ADA); 40 columns: ld > 32
SMALL = [(2, 8, 5, 17, 3, 4, 17), (2, 8, 3, 32, 16, 16, 32), (3, 8, 9, 11, 2, 3, 11), (2, 8, 5, 17, 3, 4, 40)]


@pytest.mark.parametrize('word', [6, 14, 17])
@pytest.mark.parametrize('shape', SMALL)
def test_flag_kb_small_shapes_vs_fp64(shape, word):
    """``kernels.dynadj_flags`` with hand-made weights on a graph that is not NTU's: Ahat (1e-5), the input gradient and
    every parameter gradient (1e-4) against the fp64 restatement, the bounds of the full-size test.  Words without SEM 2
    run untyped (P = 1)."""
    n, ci, mid, V, P, E, cols = shape
    kw = _word_flags(word)
    P = P if kw['node_attention'] else 1
    gen = torch.Generator().manual_seed(5)
    A = torch.randn(3, V, V, generator=gen) * 0.1
    nt = (torch.arange(V) % P).to(torch.int32)
    et = torch.randint(E, (V, V), generator=gen).to(torch.int32)
    r = lambda *sh, scale=1.0: (torch.randn(*sh, generator=gen) * scale).cuda().requires_grad_()
    p = {'A': A.cuda().requires_grad_(), 'alpha': r(3, scale=.5), 'beta': r(3, scale=.5),
         'conv1.weight': r(2 * mid, ci, scale=ci ** -.5), 'conv1.bias': r(2 * mid, scale=.1),
         'conv2.weight': r(2 * mid, ci, scale=ci ** -.5), 'conv2.bias': r(2 * mid, scale=.1),
         'conv1_se.weight': r(mid * P, ci, scale=ci ** -.5), 'conv1_se.bias': r(mid * P, scale=.1)}
    if kw['edge_attention']:
        p.update({'edge_linears.weight': r(E * mid, mid, scale=mid ** -.5), 'edge_linears.bias': r(E * mid, scale=.1)})
    if kw['ada_attention']:
        p.update({'ada_linears.weight': r(3 * E, 3, scale=3 ** -.5), 'ada_linears.bias': r(3 * E, scale=.1)})
    xbar = r(n, ci, V)
    dah = torch.randn(n, 3 * mid, V, V, generator=gen).cuda()
    ahat = D.kernels.dynadj_flags(
        torch.nn.functional.pad(xbar, (0, cols - V)), p['A'], p['alpha'], p['beta'], p['conv1.weight'], p['conv1.bias'],
        p['conv2.weight'], p['conv2.bias'], p['conv1_se.weight'], p['conv1_se.bias'], p.get('edge_linears.weight'),
        p.get('edge_linears.bias'), p.get('ada_linears.weight'), p.get('ada_linears.bias'), nt.cuda(), et.reshape(-1).cuda(),
        P, E, kw['subset_wise'])
    (ahat * dah).sum().backward()
    p64 = {k: v.detach().double().requires_grad_() for k, v in p.items()}
    x64 = xbar.detach().double().requires_grad_()
    want = F.adjacency(x64, p64, nt, et, F.effective_flags(num_types=P, edge_num=E, **kw))
    (want * dah.double()).sum().backward()
    errs = dict(ahat=rel(ahat.detach().cpu(), want.detach().cpu()), xbar=rel(xbar.grad.cpu(), x64.grad.cpu()))
    for k in p:
        if not kw['subset_wise'] and k in ('alpha', 'beta'):
            assert float(p[k].grad[1:].abs().max()) == 0.0
        errs[k] = rel(p[k].grad.cpu(), p64[k].grad.cpu())
    assert errs['ahat'] < 1e-5, errs['ahat']
    del errs['ahat']
    assert all(e < 1e-4 for e in errs.values()), errs


WATCHED = ('dsgcn_dynadj_fwd_jobs', 'dsgcn_dynadj_bwd_jobs', 'dsgcn_dynadj_fwd', 'dsgcn_dynadj_bwd', 'dsgcn_dynflag_fwd',
           'dsgcn_dynflag_bwd', 'dsgcn_dyntyped_fwd', 'dsgcn_dyntyped_bwd')


def _count_native(restore=None):
    """Wrap the K-B entry points of the loaded library with call counters (-> the counter dict); restore=: unwrap."""
    lib = D.native.lib()
    if restore is not None:
        for name, fn in restore.pop('_saved').items():
            setattr(lib, name, fn)
        return None
    counts = {name: 0 for name in WATCHED}
    counts['_saved'] = {name: getattr(lib, name) for name in WATCHED}

    def wrap(name, fn):
        def call(*a):
            counts[name] += 1
            return fn(*a)
        return call
    for name, fn in counts['_saved'].items():
        setattr(lib, name, wrap(name, fn))
    return counts


@pytest.mark.parametrize('extra', [{}, dict(sub_att=False), dict(add_type=True)])
def test_shipped_flag_set_still_calls_todays_kb(extra):
    """The guard for "changes nothing": the shipped flags (and the two switches that do not enter the arithmetic at K = 3)
    dispatch to dsgcn_dynadj_*; the flag K-B is not called."""
    g = D.Graph(layout='nturgb+d', mode='spatial')
    np.random.seed(7)
    A = torch.tensor(np.asarray(D.Graph(layout='nturgb+d', mode='random', num_filter=3, init_off=.04, init_std=.02).A),
                     dtype=torch.float32)
    torch.manual_seed(3)
    m = D.dgphgcn1(64, 64, A, torch.tensor(g.edge_type), torch.tensor(g.node_type), ratio=0.125, decompose=True,
                   node_attention=True, edge_attention=True, subset_wise=True, **extra).cuda().train()
    x = torch.randn(2, 64, 8, 25, device='cuda', requires_grad=True)
    calls = _count_native()
    try:
        m(x).sum().backward()
        torch.cuda.synchronize()
    finally:
        _count_native(restore=calls)
    assert calls['dsgcn_dynadj_fwd_jobs'] + calls['dsgcn_dynadj_fwd'] == 1
    assert calls['dsgcn_dynadj_bwd_jobs'] + calls['dsgcn_dynadj_bwd'] == 1
    assert calls['dsgcn_dynflag_fwd'] == calls['dsgcn_dynflag_bwd'] == 0
    assert calls['dsgcn_dyntyped_fwd'] == calls['dsgcn_dyntyped_bwd'] == 0


def test_gcn_stage_train_engine_step_graphed_bit_identical():
    """A 64-clip TrainEngine step of DGSTGCN(gcn_stage=[1,3,5,7,9]): the step replayed from a hipGraph gives the bits of
    the eager step, and two runs from the same weights are bit-identical (no float atomics on the new path)."""
    cfg = ds_cfg(gcn_stage=[1, 3, 5, 7, 9])
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(64, 1, 2, 64, 25, 3, generator=gen).cuda()
    y = torch.randint(0, 60, (64, 1), generator=gen).cuda()
    torch.manual_seed(0)
    np.random.seed(0)
    sd = D.build_model(copy.deepcopy(cfg)).state_dict()
    runs = {}
    for mode in ('graph', 'graph2', 'eager'):
        m = D.build_model(copy.deepcopy(cfg))
        m.load_state_dict(sd)
        m = m.cuda().train()
        eng = D.TrainEngine(m, lr=0.05, use_graph=mode != 'eager', warmup_eager=2)
        for _ in range(3):
            logs = eng.step(x, y)
        torch.cuda.synchronize()
        if mode != 'eager':
            assert eng.graphed(x, y), eng.capture_error
        assert torch.isfinite(logs['loss']).item()
        runs[mode] = (eng.flat.flat_g.detach().clone(), eng.flat.flat_p.detach().clone())
    assert torch.isfinite(runs['graph'][0]).all()
    for other in ('graph2', 'eager'):
        assert torch.equal(runs['graph'][0], runs[other][0]), other
        assert torch.equal(runs['graph'][1], runs[other][1]), other
