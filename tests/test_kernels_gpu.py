"""-m gpu: every HIP op through the C ABI vs the plain-PyTorch statement of the same op
(tests/torch_ops.py) evaluated in fp64 on the same inputs.  Tolerances are written per test."""
import numpy as np
import pytest
import torch

import dsgcn_amd
from dsgcn_amd import kernels as K
K_ = K
import torch_ops as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def rel(a, b):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def maxabs(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


def ref_dev(n):
    """Where the fp64 statement of an op is evaluated: the small cases on the host, the FULL-SIZE ones (n = 128 person-samples
    = BASELINE's 64 clips: VERDICT r4 6 — a tile-shape bug can be invisible below the size where tiles straddle samples and
    the grid wraps) with torch in fp64 on the GPU itself, where a 13 M-element conv takes milliseconds."""
    return DEV if n >= 64 else 'cpu'


def off_knife_edge(x1, a1, x2, a2, relu, tol=1e-4):
    """Nudge x1 (in place) wherever the pre-activation v = x1*s1+h1 (+ x2*s2+h2) lies within `tol` of zero.  An fp32 and an
    fp64 evaluation of relu'(v) disagree where |v| is at rounding level; at full size (13-52 M elements) one or two such
    elements exist and each is wrong by a whole gradient value — 1e-4 of dx's L2 norm, and of the per-channel sums d scale /
    d shift it enters (tools/tcg_diag.py found exactly one, the same in dx1 and dx2).  That is a property of comparing two
    precisions at a discontinuity, not of the kernel: the inputs are moved off the edge instead."""
    if not relu:
        return
    s1 = a1[0].double().view(1, -1, 1, 1) if a1 is not None else 1.0
    v = x1.double() * s1
    if a1 is not None:
        v = v + a1[1].double().view(1, -1, 1, 1)
    if x2 is not None:
        v = v + x2.double() * (a2[0].double().view(1, -1, 1, 1) if a2 is not None else 1.0)
        if a2 is not None:
            v = v + a2[1].double().view(1, -1, 1, 1)
    near = v.abs() < tol
    if near.any():
        step = torch.where(v >= 0, 1.0, -1.0) * (2 * tol) / s1
        x1 += (step * near).float()
        v = v + step * near * s1
    assert float(v.abs().min()) >= 0.9 * tol


@pytest.mark.parametrize('n,KC,T,V,relu,affine', [
    (3, 24, 64, 25, True, True), (2, 48, 32, 25, True, True), (2, 96, 16, 25, True, True),
    (2, 24, 100, 17, True, True), (2, 10, 25, 17, True, True), (2, 6, 64, 25, False, False),
    (1, 5, 7, 25, True, True), (2, 4, 130, 18, True, True),
    (2, 6, 100, 25, True, True),        # 25 joints x 100 frames: the four-wave workgroup's LDS slices pass 64 KB
    (1, 3, 128, 25, False, True),
    # full size: the four K-A layer shapes of the bench step
    (128, 24, 64, 25, True, True), (128, 48, 64, 25, True, True), (128, 48, 32, 25, True, True), (128, 96, 32, 25, True, True),
    (128, 96, 16, 25, True, True)])
def test_aggregate(n, KC, T, V, relu, affine):
    check_aggregate(n, KC, T, V, relu, affine)


def check_aggregate(n, KC, T, V, relu, affine):
    g = torch.Generator().manual_seed(n * 1000 + KC + T)
    zp = torch.randn(n, KC, T, V, generator=g)
    ahat = torch.randn(n, KC, V, V, generator=g) * 0.3
    sc = torch.randn(KC, generator=g) if affine else None
    sh = torch.randn(KC, generator=g) * 0.5 if affine else None
    dy = torch.randn(n, KC, T, V, generator=g)

    def run(mod, dt, dev):
        t = [x.to(dev, dt).requires_grad_() if x is not None else None for x in (zp, ahat, sc, sh)]
        y = mod.aggregate(t[0], (t[2], t[3]) if affine else None, relu, t[1])
        y.backward(dy.to(dev, dt))
        return [y] + [x.grad if x is not None else None for x in t]

    got = run(K, torch.float32, DEV)
    ref = run(R, torch.float64, ref_dev(n))
    names = ['y', 'dzp', 'dahat', 'dscale', 'dshift']
    for nm, a, b in zip(names, got, ref):
        if b is None:
            continue
        # fp32 accumulation over <= V (fwd) / T (dahat) / n*T*V (dscale) terms: 2e-6 relative L2
        assert rel(a.cpu(), b) < 2e-6, (nm, rel(a.cpu(), b))


def _dyn_inputs(n, Ci, mid, V, layout, seed=0):
    g = torch.Generator().manual_seed(seed)
    gr = dsgcn_amd.Graph(layout=layout, mode='spatial')
    P, E = 5, 15
    nt = torch.tensor(gr.node_type, dtype=torch.int32)
    et = torch.tensor(gr.edge_type, dtype=torch.int32)
    t = dict(
        xbar=torch.randn(n, Ci, V, generator=g),
        A=torch.randn(3, V, V, generator=g) * 0.02 + 0.04,
        alpha=torch.randn(3, generator=g) * 0.5, beta=torch.randn(3, generator=g) * 0.5,
        w1=torch.randn(2 * mid, Ci, generator=g) / Ci ** 0.5, b1=torch.randn(2 * mid, generator=g) * 0.1,
        w2=torch.randn(2 * mid, Ci, generator=g) / Ci ** 0.5, b2=torch.randn(2 * mid, generator=g) * 0.1,
        wse=torch.randn(mid * P, Ci, generator=g) / Ci ** 0.5, bse=torch.randn(mid * P, generator=g) * 0.1,
        we=torch.randn(E * mid, mid, generator=g) / mid ** 0.5, be=torch.randn(E * mid, generator=g) * 0.1)
    return t, nt, et


@pytest.mark.parametrize('n,Ci,mid,V,layout', [
    (3, 3, 8, 25, 'nturgb+d'), (2, 64, 8, 25, 'nturgb+d'), (2, 64, 16, 25, 'nturgb+d'),
    (2, 128, 32, 25, 'nturgb+d'), (2, 256, 32, 25, 'nturgb+d'), (2, 64, 8, 17, 'coco'),
    # full size: the six (Ci, mid) pairs of the DS-STGCN step at 128 person-samples, and K400's widest
    (128, 3, 8, 25, 'nturgb+d'), (128, 64, 8, 25, 'nturgb+d'), (128, 64, 16, 25, 'nturgb+d'), (128, 128, 16, 25, 'nturgb+d'),
    (128, 128, 32, 25, 'nturgb+d'), (128, 256, 32, 25, 'nturgb+d'), (64, 256, 32, 17, 'coco')])
def test_dynadj(n, Ci, mid, V, layout):
    check_dynadj(n, Ci, mid, V, layout)


def _dyn_host_chunks(t, nt, et, dah, order, single_use, chunk=16):
    """The fp64 statement on the HOST, a few samples at a time: parameter gradients add over the chunks, the per-sample one
    (xbar) concatenates.  Only a failing full-size comparison pays for it."""
    n = dah.shape[0]
    grads = {}
    for s in range(0, n, chunk):
        tt = {k: v.detach().clone().double() for k, v in t.items()}
        tt['xbar'] = tt['xbar'][s:s + chunk].clone()
        for v in tt.values():
            v.requires_grad_()
        out = R.dynadj(*[tt[k] for k in order], nt, et, single_use=single_use)
        out.backward(dah[s:s + chunk].double())
        for k, v in tt.items():
            if k == 'xbar':
                grads.setdefault(k, []).append(v.grad)
            else:
                grads[k] = v.grad if k not in grads else grads[k] + v.grad
    grads['xbar'] = torch.cat(grads['xbar'])
    return grads


def _dyn_diagnosis(k, got, gpu_ref, n, host):
    """What goes into the message of a failing gradient comparison at full size (n >= 64: the fp64 statement ran on the
    GPU): the same gradient against a host evaluation of the statement, so that the failure says which side moved."""
    if n < 64:
        return ()
    h = host()[k]
    return ('rel(kernel, host) %.3e' % rel(got, h), 'rel(gpu_ref, host) %.3e' % rel(gpu_ref, h),
            'rel(kernel, gpu_ref) %.3e' % rel(got, gpu_ref))


def check_dynadj(n, Ci, mid, V, layout, single_use=True, inputs=None):
    """single_use=False: what dggcn passes (its A feeds two calls; the parameter sums are never deferred).
    inputs: (t, node_type, edge_type) of ``dynadj_cases.dyn_inputs`` in place of a layout's graph (any V, P, E)."""
    t, nt, et = _dyn_inputs(n, Ci, mid, V, layout, seed=Ci + mid) if inputs is None else inputs
    g = torch.Generator().manual_seed(7)
    dah = torch.randn(n, 3 * mid, V, V, generator=g)
    order = list(t)

    def run(mod, dt, dev):
        tt = {k: v.to(dev, dt).requires_grad_() for k, v in t.items()}
        out = mod.dynadj(*[tt[k] for k in order], nt.to(dev), et.to(dev), single_use=single_use)
        out.backward(dah.to(dev, dt))
        return out, {k: v.grad for k, v in tt.items()}

    out, grads = run(K, torch.float32, DEV)
    ro, rg = run(R, torch.float64, ref_dev(n))
    # forward: tanh/exp in fp32 (ocml, ~1-2 ulp) + <=256-term dot products
    assert rel(out.cpu(), ro) < 2e-6, rel(out.cpu(), ro)
    for k in order:
        assert rel(grads[k].cpu(), rg[k]) < 2e-5, (k, rel(grads[k].cpu(), rg[k])) + _dyn_diagnosis(      # fp32 chain rule
            k, grads[k], rg[k], n, lambda: _dyn_host_chunks(t, nt, et, dah, order, single_use))
    # no float atomics anywhere in K-B (per-sample partials + ordered column sums): bit-reproducible run to run
    out2, grads2 = run(K, torch.float32, DEV)
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in order)


def _rand(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def test_bn_jobs_batched_and_hosted_are_bit_identical():
    """Round 6 (csrc/bn_jobs.h): BatchNorm finalize / coefficient launches as jobs.  (i) dsgcn_bn_finalize_multi and
    dsgcn_bn_coef_rows_multi with jobs of different widths and row counts (and an accumulating second consumer) against the
    single launches; (ii) the same jobs hosted as extra workgroups of K-B's launches (dsgcn_dynadj_fwd_jobs / _bwd_jobs) —
    outputs AND K-B's own results bit-identical to the plain calls."""
    from dsgcn_amd import native
    lib = native.lib()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(21)
    P = lambda t: None if t is None else t.data_ptr()
    specs = [(400, 24, 24, True), (1600, 256, 200, True), (37, 70, 70, False), (800, 96, 96, True)]    # rows, C, c_affine, gamma?
    fin = []
    for rows, C, ca, hasg in specs:
        part = (_rand(g, rows, C, 2).abs() + 0.1).to(DEV)
        part[..., 1] += part[..., 0] ** 2 + 1.0
        gamma = (torch.rand(C, generator=g) + 0.5).to(DEV) if hasg else None
        beta = _rand(g, C, scale=0.2).to(DEV) if hasg else None
        fin.append(dict(part=part, gamma=gamma, beta=beta, rows=rows, C=C, ca=ca, count=float(rows * 97)))

    def fin_single(f):
        out = torch.empty(4, f['C'], device=DEV)
        native.check(lib.dsgcn_bn_finalize(P(f['part']), f['rows'], f['C'], f['count'], P(f['gamma']), P(f['beta']), 1e-5,
                                           P(out[0]), P(out[1]), P(out[2]), P(out[3]), f['ca'], st), 'fin')
        return out

    def fin_jobs(outs):
        return (native.BnFinJob * len(fin))(*[native.BnFinJob(P(f['part']), P(f['gamma']), P(f['beta']), P(o[0]), P(o[1]), P(o[2]),
                                                              P(o[3]), f['count'], 1e-5, f['rows'], f['C'], f['ca'])
                                              for f, o in zip(fin, outs)])
    want = [fin_single(f) for f in fin]
    got = [torch.full((4, f['C']), float('nan'), device=DEV) for f in fin]
    native.check(lib.dsgcn_bn_finalize_multi(fin_jobs(got), len(fin), st), 'fin_multi')
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert lib.dsgcn_bn_finalize_multi(fin_jobs(got), 5, st) == -1 and lib.dsgcn_bn_finalize_multi(None, 1, st) == -1

    # coefficient jobs: k = 2 / 3 / 4 columns, the last one accumulating into coefficients that already hold a consumer's share
    cspecs = [(400, 24, 2, 0, 1, 0), (1200, 256, 3, 2, 1, 0), (55, 70, 4, 0, 3, 0), (800, 96, 3, 0, 1, 1)]
    coef = []
    for (R_, C, k, ids, idh, acc), w in zip(cspecs, want):
        coef.append(dict(part=_rand(g, R_, C, k).to(DEV), R=R_, C=C, k=k, ids=ids, idh=idh, acc=acc, mean=w[0].clone(),
                         var=w[1].clone(), gamma=(torch.rand(C, generator=g) + 0.5).to(DEV), init=_rand(g, 4, C).to(DEV)))

    def coef_single(c):
        out = c['init'].clone()
        native.check(lib.dsgcn_bn_coef_rows(P(c['part']), c['R'], c['C'], c['k'], c['ids'], c['idh'], P(c['mean']), P(c['var']),
                                            P(c['gamma']), 1e-5, float(c['R'] * 31), c['C'], P(out), c['acc'], st), 'coef')
        return out

    def coef_jobs(outs):
        return (native.BnCoefJob * len(coef))(*[native.BnCoefJob(P(c['part']), P(c['mean']), P(c['var']), P(c['gamma']), P(o),
                                                                 float(c['R'] * 31), 1e-5, c['R'], c['C'], c['k'], c['ids'],
                                                                 c['idh'], c['C'], c['acc']) for c, o in zip(coef, outs)])
    cwant = [coef_single(c) for c in coef]
    cgot = [c['init'].clone() for c in coef]
    native.check(lib.dsgcn_bn_coef_rows_multi(coef_jobs(cgot), len(coef), st), 'coef_multi')
    for a, b in zip(cgot, cwant):
        assert torch.equal(a, b)

    # hosted in K-B's launches
    n, Ci, mid, V = 6, 64, 16, 25
    t, nt, et = _dyn_inputs(n, Ci, mid, V, 'nturgb+d', seed=5)
    E, Pn = 15, 5
    proj = _rand(g, n, (4 + Pn) * mid, 32).to(DEV)
    A, alpha, beta = t['A'].to(DEV), t['alpha'].to(DEV), t['beta'].to(DEV)
    we, be = t['we'].to(DEV).contiguous(), t['be'].to(DEV).contiguous()
    nt, et = nt.to(DEV), et.to(DEV)
    ah0 = torch.empty(n, 3 * mid, V, V, device=DEV)
    native.check(lib.dsgcn_dynadj_fwd(P(proj), P(A), P(alpha), P(beta), P(we), P(be), P(nt), P(et), P(ah0), n, mid, V, 32, Pn, E,
                                      st), 'dyn')
    ah1 = torch.empty_like(ah0)
    got = [torch.full((4, f['C']), float('nan'), device=DEV) for f in fin]
    native.check(lib.dsgcn_dynadj_fwd_jobs(P(proj), P(A), P(alpha), P(beta), P(we), P(be), P(nt), P(et), P(ah1), n, mid, V, 32,
                                           Pn, E, fin_jobs(got), len(fin), st), 'dyn_jobs')
    assert torch.equal(ah0, ah1)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    dah = _rand(g, n, 3 * mid, V, V).to(DEV)
    ps = lib.dsgcn_dynadj_partial_stride(mid, V, E)

    def bwd(jobs, nj):
        dd, dproj, ppar = torch.empty_like(dah), torch.empty_like(proj), torch.empty(n, ps, device=DEV)
        native.check(lib.dsgcn_dynadj_bwd_jobs(P(proj), P(alpha), P(beta), P(we), P(be), P(nt), P(et), P(dah), P(dd), P(dproj),
                                               P(ppar), ps, n, mid, V, 32, Pn, E, jobs, nj, st), 'dyn_bwd_jobs')
        return dproj, ppar
    d0 = bwd(None, 0)
    cgot = [c['init'].clone() for c in coef]
    d1 = bwd(coef_jobs(cgot), len(coef))
    assert torch.equal(d0[0], d1[0]) and torch.equal(d0[1], d1[1])
    for a, b in zip(cgot, cwant):
        assert torch.equal(a, b)


@pytest.mark.parametrize('kind', ['ds', 'ds_k400'])
def test_bn_batching_leaves_the_step_bit_identical(kind, monkeypatch):
    """The model with DSGCN_BN_BATCH on (jobs batched / hosted, `pre` conv ahead of K-B, the block's residual conv ahead of
    the temporal unit) against the single launches: logits, loss and EVERY gradient bit for bit — the jobs run the same
    blocks in the same summation order, and no kernel's inputs change."""
    from bench import ds_cfg
    import numpy as np
    cfg = ds_cfg(60) if kind == 'ds' else ds_cfg(400, 'coco')
    T, V = (32, 25) if kind == 'ds' else (20, 17)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(3, 1, 2, T, V, 3, generator=g).to(DEV)
    y = torch.randint(0, 60, (3, 1), generator=g).to(DEV)
    res = []
    for flag in (False, True):
        monkeypatch.setattr(K, 'BN_BATCH', flag)
        np.random.seed(0)
        torch.manual_seed(0)
        m = dsgcn_amd.build_model(cfg).to(DEV).train()
        with torch.no_grad():
            for k_, p_ in m.named_parameters():
                if k_.endswith(('alpha', 'beta', 'add_coeff')):
                    p_.normal_(0, 0.5)
        out = m.train_step(dict(keypoint=x, label=y), None, sync_log_vars=False)
        out['loss'].backward()
        res.append((out['loss'].detach().clone(), {k_: p_.grad.clone() for k_, p_ in m.named_parameters() if p_.grad is not None},
                    {k_: b_.clone() for k_, b_ in m.named_buffers()}))
    assert torch.equal(res[0][0], res[1][0])
    assert res[0][1].keys() == res[1][1].keys()
    for k_ in res[0][1]:
        assert torch.equal(res[0][1][k_], res[1][1][k_]), k_
    for k_ in res[0][2]:
        assert torch.equal(res[0][2][k_], res[1][2][k_]), k_


@pytest.mark.parametrize('n,Ci,Co,T,V,stride,aug,mode', [
    (3, 3, 24, 64, 25, 1, False, 'plain'),        # block-0 pre conv
    (2, 64, 64, 64, 25, 1, True, 'res_plain'),    # tcn branch conv: relu(bn(zo)+x), global joint
    (2, 64, 128, 32, 25, 1, True, 'res_affine'),  # gcn with down: relu(bn(zo)+bn(zd))
    (2, 96, 256, 16, 25, 1, False, 'plain'),      # post conv, 8 M-tiles
    (2, 256, 256, 16, 25, 1, False, 'affine_relu'),   # transform conv: relu(bn1(f))
    (2, 64, 128, 64, 25, 2, False, 'plain'),      # strided residual conv
    (2, 128, 96, 50, 17, 1, True, 'res_plain'),   # coco, T not a multiple of the row tile, unaligned planes
    (1, 5, 7, 9, 18, 2, True, 'affine_relu'),     # ragged everything
    (2, 256, 96, 16, 25, 1, False, 'plain'),      # pre conv of the last stage: 3 M-tiles
    (2, 24, 64, 64, 25, 1, False, 'affine_relu'), # post conv: K = 24 (one padded k-group)
    (5, 64, 64, 64, 25, 1, False, 'res_affine'),  # 65 wave tiles: the last workgroup is partly empty
    (3, 48, 128, 32, 25, 1, False, 'affine_relu'),
    (2, 64, 64, 25, 17, 1, False, 'res_affine'),  # coco last stage: odd plane length (425): dword-aligned 16-B loads in wgrad
    (2, 128, 256, 25, 17, 1, False, 'plain'),
    # one-pass backward (csrc/bwd64.hip): narrow outputs, one / two input tiles, every input mode
    (3, 128, 48, 32, 25, 1, False, 'plain'),      # pre conv of the middle stage: two 64-channel input tiles
    (2, 96, 40, 20, 17, 1, False, 'affine_relu'), # second input tile half empty (narrow wave roles), coco planes
    (2, 64, 24, 64, 25, 1, False, 'res_affine'),  # two input streams, 24 output rows
    (3, 64, 64, 64, 25, 1, False, 'affine_relu'),
    # GEMM form with three-term bf16 products (csrc/pw4.hip k_pwg; weight gradient csrc/wgrad.hip B3): wide on both sides
    (3, 128, 160, 12, 25, 1, False, 'res_affine'),   # 900 positions: tiles straddle samples, last tile partly empty, 2 row blocks
    (5, 96, 256, 8, 17, 1, False, 'affine_relu'),    # K = 96: odd chunk count (ping-pong tail), 136-position planes
    (2, 64, 128, 8, 16, 1, False, 'plain'),          # smallest eligible plane (128), K = 64
    (2, 256, 132, 16, 25, 1, True, 'res_plain'),     # 132 rows: second row block nearly empty; global-joint column beside it
    # ragged planes on the wide-load kernels (runs of 4 with a partly empty last run per plane, dword-aligned 16-byte loads)
    (2, 16, 24, 7, 25, 1, False, 'plain'),           # 175 positions, narrow
    (2, 16, 16, 7, 25, 1, True, 'res_affine'),       # two streams + global joint
    (1, 3, 24, 7, 25, 1, False, 'plain'),            # one sample, 3 input channels
    (3, 32, 48, 3, 25, 1, False, 'affine_relu'),     # 75 positions: a 128-position tile spans two planes
    (2, 256, 256, 25, 17, 1, False, 'res_affine'),   # K400 last stage on the GEMM form (425 positions)
    (2, 8, 64, 25, 25, 1, False, 'plain'),           # CTR-GCN conv4 on (V x V) planes of R channels (625 positions)
    # FULL SIZE (128 person-samples): every 1x1 conv shape / input mode of the DS-STGCN step, stage by stage
    (128, 3, 24, 64, 25, 1, False, 'plain'),         # block 0: pre
    (128, 3, 64, 64, 25, 1, False, 'plain'),         # block 0: down
    (128, 64, 24, 64, 25, 1, False, 'plain'),        # stage 1: pre (one-pass backward)
    (128, 24, 64, 64, 25, 1, False, 'plain'),        # post
    (128, 64, 64, 64, 25, 1, True, 'res_plain'),     # branch convs + global joint, identity residual
    (128, 64, 64, 64, 25, 1, True, 'res_affine'),    # ... after a block with a down conv
    (128, 64, 64, 64, 25, 1, False, 'affine_relu'),  # transform
    (128, 64, 48, 64, 25, 1, False, 'plain'),        # block 4: pre at 64 frames
    (128, 48, 128, 64, 25, 1, False, 'plain'),       # post
    (128, 64, 128, 64, 25, 1, False, 'plain'),       # down
    (128, 128, 128, 64, 25, 1, True, 'res_affine'),  # branch convs at 64 frames (the largest K-C launch of the step)
    (128, 128, 128, 32, 25, 1, False, 'affine_relu'),  # transform after the stride
    (128, 64, 128, 32, 25, 1, False, 'plain'),       # block residual conv on the pre-strided frames
    (128, 128, 48, 32, 25, 1, False, 'plain'),       # stage 2
    (128, 48, 128, 32, 25, 1, False, 'plain'),
    (128, 128, 128, 32, 25, 1, True, 'res_plain'),
    (128, 128, 96, 32, 25, 1, False, 'plain'),       # block 7
    (128, 96, 256, 32, 25, 1, False, 'plain'),
    (128, 128, 256, 32, 25, 1, False, 'plain'),
    (128, 256, 256, 32, 25, 1, True, 'res_affine'),
    (128, 256, 256, 16, 25, 1, False, 'affine_relu'),
    (128, 128, 256, 16, 25, 1, False, 'plain'),
    (128, 256, 96, 16, 25, 1, False, 'plain'),       # stage 3
    (128, 96, 256, 16, 25, 1, False, 'plain'),
    (128, 256, 256, 16, 25, 1, True, 'res_plain'),
    (64, 256, 256, 25, 17, 1, True, 'res_plain'),    # K400 (config 5 per GPU: 32 clips): ragged 425-position planes
    (128, 8, 64, 25, 25, 1, False, 'plain'),         # CTR-GCN conv4 (config 4)
])
def test_pwconv(n, Ci, Co, T, V, stride, aug, mode):
    check_pwconv(n, Ci, Co, T, V, stride, aug, mode)


def check_pwconv(n, Ci, Co, T, V, stride, aug, mode, want_bn=True, bias=True, grad=True):
    """want_bn / bias False: the convs without a BatchNorm behind them (K-B's and the CTR-GCN refinement's projections).
    grad False: the eval-mode call (torch.no_grad(), inputs without history, want_bn False) and its outputs alone."""
    assert grad or not want_bn
    g = torch.Generator().manual_seed(Ci * 7 + Co + T)
    x1 = _rand(g, n, Ci, T, V)
    a1 = a2 = x2 = None
    relu = False
    if mode in ('res_plain', 'res_affine', 'affine_relu'):
        a1 = (torch.rand(Ci, generator=g) + 0.5, _rand(g, Ci, scale=0.3))
        relu = True
    if mode in ('res_plain', 'res_affine'):
        x2 = _rand(g, n, Ci, T, V)
    if mode == 'res_affine':
        a2 = (torch.rand(Ci, generator=g) + 0.5, _rand(g, Ci, scale=0.3))
    off_knife_edge(x1, a1, x2, a2, relu)
    w = _rand(g, Co, Ci, 1, 1, scale=Ci ** -0.5)
    b = _rand(g, Co, scale=0.1)
    n_aff = Co - Co // 6 if aug else Co
    gamma = torch.rand(n_aff, generator=g) + 0.5
    beta = _rand(g, n_aff, scale=0.2)
    Tout = (T + stride - 1) // stride
    gz = _rand(g, n, Co, Tout, V)
    gza = _rand(g, n, Co, Tout)
    gsc = _rand(g, Co)
    gsh = _rand(g, Co)

    def run(mod, dt, dev):
        def mk(t):
            return None if t is None else t.to(dev, dt).requires_grad_(grad)
        tx1, tx2, tw, tb, tg, tbeta = mk(x1), mk(x2), mk(w), mk(b if bias else None), mk(gamma), mk(beta)
        ta1 = None if a1 is None else (mk(a1[0]), mk(a1[1]))
        ta2 = None if a2 is None else (mk(a2[0]), mk(a2[1]))
        if not grad:
            with torch.no_grad():
                z, zaug = mod.pwconv(tx1, ta1, tx2, ta2, relu, tw, tb, stride, aug)[:2]
            return dict(z=z, zaug=zaug) if aug else dict(z=z)
        if want_bn:
            z, zaug, sc, sh, mean, var = mod.pwconv(tx1, ta1, tx2, ta2, relu, tw, tb, stride, aug, tg, tbeta, 1e-5, n_aff,
                                                    True)
            loss = (z * gz.to(dev, dt)).sum() + (sc * gsc.to(dev, dt)).sum() + (sh * gsh.to(dev, dt)).sum()
        else:
            z, zaug = mod.pwconv(tx1, ta1, tx2, ta2, relu, tw, tb, stride, aug)[:2]
            loss = (z * gz.to(dev, dt)).sum()
        if aug:
            loss = loss + (zaug * gza.to(dev, dt)).sum()
        loss.backward()
        outs = dict(z=z, dx1=tx1.grad, dw=tw.grad)
        if want_bn:
            outs.update(sc=sc, sh=sh, mean=mean, var=var, dgamma=tg.grad, dbeta=tbeta.grad)
        if bias:
            outs['db'] = tb.grad
        if aug:
            outs['zaug'] = zaug
        if tx2 is not None:
            outs['dx2'] = tx2.grad
        if ta1 is not None:
            outs['ds1'], outs['dh1'] = ta1[0].grad, ta1[1].grad
        if ta2 is not None:
            outs['ds2'], outs['dh2'] = ta2[0].grad, ta2[1].grad
        return outs

    got = run(K, torch.float32, DEV)
    ref = run(R, torch.float64, ref_dev(n))
    for k, v in ref.items():
        # fp32 MFMA dot products over <=256 channels, sums over <= n*T*V positions: 1e-5 relative L2
        tol = 2e-5 if k not in ('db',) else 2e-4      # db of a conv feeding BN is ~0 analytically (cancellation)
        err = rel(got[k].detach().cpu(), v.detach())
        if k == 'db':
            err = maxabs(got[k].detach().cpu(), v.detach()) / (ref['dw'].abs().max().item() + 1e-30)
        if n >= 64 and k in ('ds1', 'dh1', 'ds2', 'dh2', 'dgamma', 'dbeta', 'dw'):
            tol = 5e-5           # sums over 2e5 positions in fp32 (sqrt(N) * 2^-24 = 2.7e-5)
        assert err < tol, (k, err)


def check_pwconv_group(Kk, n, Ci, Co, T, V, affine):
    """pwconv_group (CTR-GCN's conv4 of the Kk subsets in one launch each way: csrc/pw4.hip grouped over blockIdx.y) against
    Kk single pwconv calls of the same operands — the same kernel, so the outputs and the data gradients bit for bit; the
    weight and input-scale gradients too where the single call's backward takes the same dgrad / wgrad kernels (the
    one-pass backward of narrow convs, csrc/bwd64.hip, sums in another order: 2e-6 there) — and against fp64 with
    test_pwconv's bars."""
    lib = dsgcn_amd.native.lib()
    assert lib.dsgcn_pwconv_group_ok(n, Ci, Co, T, V) == 1
    g = torch.Generator().manual_seed(Kk * 100 + Ci + Co)
    xs = [_rand(g, n, Ci, T, V) for _ in range(Kk)]
    affs = [(torch.rand(Ci, generator=g) + 0.5, _rand(g, Ci, scale=0.3)) if affine else None for _ in range(Kk)]
    ws = [_rand(g, Co, Ci, scale=Ci ** -0.5) for _ in range(Kk)]
    gzs = [_rand(g, n, Co, T, V) for _ in range(Kk)]

    def run(how, dt, dev):
        tx = [x.to(dev, dt).requires_grad_() for x in xs]
        ta = [None if a is None else (a[0].to(dev, dt).requires_grad_(), a[1].to(dev, dt).requires_grad_()) for a in affs]
        tw = [w.to(dev, dt).requires_grad_() for w in ws]
        if how == 'group':
            buf = torch.empty((Kk, n, Co, T, V), device=dev, dtype=dt)
            zs = K.pwconv_group(tx, ta, tw, [K.OutSlot(buf[k]) for k in range(Kk)])
        else:
            mod = K if how == 'single' else R
            zs = [mod.pwconv(x, a, None, None, False, w, None, 1, False)[0] for x, a, w in zip(tx, ta, tw)]
        sum((z * gz.to(dev, dt)).sum() for z, gz in zip(zs, gzs)).backward()
        res = {}
        for k in range(Kk):
            res[f'z{k}'], res[f'dx{k}'], res[f'dw{k}'] = zs[k], tx[k].grad, tw[k].grad
            if affine:
                res[f'ds{k}'], res[f'dh{k}'] = ta[k][0].grad, ta[k][1].grad
        return res

    got = run('group', torch.float32, DEV)
    single = run('single', torch.float32, DEV)
    same_bwd = lib.dsgcn_pwconv_bwd_rows(n, Ci, Co, T, V, 1) <= 0
    for k, v in single.items():
        if k[0] == 'z' or k[:2] == 'dx' or same_bwd:
            assert torch.equal(got[k], v), (k, rel(got[k], v))
        else:
            assert rel(got[k], v) < 2e-6, (k, rel(got[k], v))
    ref = run('ref', torch.float64, ref_dev(n))
    for k, v in ref.items():
        tol = 5e-5 if (n >= 64 and k[:2] in ('dw', 'ds', 'dh')) else 2e-5
        assert rel(got[k], v) < tol, (k, rel(got[k], v))


@pytest.mark.parametrize('n,Ci,Co,T,V,KT,mode,stride', [(a_ + (1,)) for a_ in [
    (2, 64, 64, 16, 25, 9, 'res_affine'),     # ST-GCN unit_tcn after unit_gcn with a conv residual
    (3, 64, 64, 64, 25, 9, 'res_plain'),      # first stage: 13 tiles per sample, the last one partial
    (2, 128, 128, 32, 25, 9, 'affine_relu'),
    (2, 256, 256, 16, 25, 9, 'res_plain'),    # two row tiles per position tile, 8 channel chunks
    (2, 48, 80, 12, 17, 9, 'plain'),          # ragged widths, coco joints (7 frames per tile)
    (1, 32, 40, 20, 18, 5, 'affine_relu'),    # 5 taps
    (2, 16, 24, 8, 25, 3, 'res_affine'),      # 3 taps, fewer frames than a tile holds... (R = 5 < T = 8)
    (2, 24, 16, 4, 25, 9, 'plain'),           # T < R: one tile per sample, halo larger than the sample
]] + [
    (2, 64, 128, 32, 25, 9, 'res_affine', 2),  # ST-GCN's stage transitions: stride 2
    (2, 128, 256, 16, 25, 9, 'res_plain', 2),
    (3, 32, 48, 15, 17, 5, 'affine_relu', 2),  # odd frame count (8 output frames: 136 positions)
    (2, 16, 16, 12, 18, 3, 'plain', 2),
    # full size: ST-GCN's five temporal convs (BASELINE config 1) at 128 person-samples
    (128, 64, 64, 64, 25, 9, 'res_plain', 1), (128, 64, 128, 64, 25, 9, 'res_affine', 2), (128, 128, 128, 32, 25, 9, 'res_plain', 1),
    (128, 128, 256, 32, 25, 9, 'res_affine', 2), (128, 256, 256, 16, 25, 9, 'res_plain', 1),
])
def test_tconv_gemm(n, Ci, Co, T, V, KT, mode, stride):
    check_tconv_gemm(n, Ci, Co, T, V, KT, mode, stride)


def check_tconv_gemm(n, Ci, Co, T, V, KT, mode, stride):
    """csrc/tcg.hip: the dense (KT,1) temporal conv as a GEMM on bf16 terms — forward with BatchNorm statistics, data
    gradient with the mask / affine epilogue, weight gradient — against the fp64 evaluation of the same op."""
    g = torch.Generator().manual_seed(Ci * 3 + Co + T + KT)
    x1 = _rand(g, n, Ci, T, V)
    a1 = a2 = x2 = None
    relu = False
    if mode in ('res_plain', 'res_affine', 'affine_relu'):
        a1 = (torch.rand(Ci, generator=g) + 0.5, _rand(g, Ci, scale=0.3))
        relu = True
    if mode in ('res_plain', 'res_affine'):
        x2 = _rand(g, n, Ci, T, V)
    if mode == 'res_affine':
        a2 = (torch.rand(Ci, generator=g) + 0.5, _rand(g, Ci, scale=0.3))
    off_knife_edge(x1, a1, x2, a2, relu)
    w = _rand(g, Co, Ci, KT, 1, scale=(Ci * KT) ** -0.5)
    b = _rand(g, Co, scale=0.1)
    gamma = torch.rand(Co, generator=g) + 0.5
    beta = _rand(g, Co, scale=0.2)
    gz = _rand(g, n, Co, (T + stride - 1) // stride, V)
    gsc, gsh = _rand(g, Co), _rand(g, Co)
    assert K.tconv_gemm_ok(n, Ci, Co, T, V, KT, stride)

    def run(mod, dt, dev):
        def mk(t):
            return None if t is None else t.to(dev, dt).requires_grad_()
        tx1, tx2, tw, tb, tg, tbeta = mk(x1), mk(x2), mk(w), mk(b), mk(gamma), mk(beta)
        ta1 = None if a1 is None else (mk(a1[0]), mk(a1[1]))
        ta2 = None if a2 is None else (mk(a2[0]), mk(a2[1]))
        z, sc, sh, mean, var = mod.tconv_bn(tx1, ta1, tx2, ta2, relu, tw, tb, tg, tbeta, 1e-5, True, stride)
        loss = (z * gz.to(dev, dt)).sum() + (sc * gsc.to(dev, dt)).sum() + (sh * gsh.to(dev, dt)).sum()
        loss.backward()
        outs = dict(z=z, sc=sc, sh=sh, mean=mean, var=var, dx1=tx1.grad, dw=tw.grad, db=tb.grad, dgamma=tg.grad,
                    dbeta=tbeta.grad)
        if tx2 is not None:
            outs['dx2'] = tx2.grad
        if ta1 is not None:
            outs['ds1'], outs['dh1'] = ta1[0].grad, ta1[1].grad
        if ta2 is not None:
            outs['ds2'], outs['dh2'] = ta2[0].grad, ta2[1].grad
        return outs

    got = run(K, torch.float32, DEV)
    ref = run(R, torch.float64, ref_dev(n))
    for k, v in ref.items():
        err = rel(got[k].detach().cpu(), v.detach())
        if k == 'db':           # db of a conv feeding BN is ~0 analytically (cancellation): absolute, against dW's scale
            err = maxabs(got[k].detach().cpu(), v.detach()) / (ref['dw'].abs().max().item() + 1e-30)
        # full size: the per-channel sums run over 2e5 positions in fp32 (sqrt(N) * 2^-24 = 2.7e-5): 5e-5 for them, the
        # small cases and every elementwise output keep 2e-5
        bar = 5e-5 if (n >= 64 and k in ('ds1', 'dh1', 'ds2', 'dh2', 'dgamma', 'dbeta', 'dw')) else 2e-5
        assert err < (2e-4 if k == 'db' else bar), (k, err)
    got2 = run(K, torch.float32, DEV)          # ordered partial sums: bit-reproducible
    assert all(torch.equal(got[k], got2[k]) for k in got)


@pytest.mark.parametrize('Ci,Co,T', [(256, 256, 16), (128, 128, 32), (96, 256, 16)])
def test_pwconv_bf16_terms_are_fp32_class(Ci, Co, T):
    """The wide 1x1 convs carry every fp32 product as six bf16 MFMA terms of the exact three-way bf16 split of both
    operands (csrc/common.h b3_split).  Claim pinned here: the error against an fp64 evaluation is that of an fp32 dot
    product — measured 3.0e-7 (z), 2.4e-7 (dx), 2.2e-8 (dW) relative L2 at 256 -> 256, against 2.6e-7 / 2.9e-7 / 1.8e-8 for
    the fp32 MFMA form (tools/kc_check.py) — an order of magnitude tighter than this file's generic 2e-5 bar, and three
    orders below what a plain bf16 product would give (4e-3)."""
    n, V = 6, 25
    g = torch.Generator().manual_seed(Ci + Co)
    x = _rand(g, n, Ci, T, V)
    s1, h1 = torch.rand(Ci, generator=g) + 0.5, _rand(g, Ci, scale=0.1)
    w = _rand(g, Co, Ci, 1, 1, scale=Ci ** -0.5)
    b = _rand(g, Co, scale=0.1)
    gz = _rand(g, n, Co, T, V)

    def run(mod, dt, dev):
        tx, tw, tb = (t.to(dev, dt).requires_grad_() for t in (x, w, b))
        z = mod.pwconv(tx, (s1.to(dev, dt), h1.to(dev, dt)), None, None, True, tw, tb, 1, False)[0]
        (z * gz.to(dev, dt)).sum().backward()
        return z.detach().cpu(), tx.grad.cpu(), tw.grad.cpu()

    got = run(K, torch.float32, DEV)
    ref = run(R, torch.float64, 'cpu')
    for name, a, r_, bar in zip(('z', 'dx', 'dW'), got, ref, (6e-7, 6e-7, 3e-7)):      # (dW at n = 6: 1.0-1.2e-7)
        assert rel(a, r_) < bar, (name, rel(a, r_))


@pytest.mark.parametrize('case', ['big_x_small_w', 'small_x_big_w', 'mixed_binades', 'near_subnormal', 'non_finite'])
def test_pwconv_bf16_split_edge_cases(case):
    """The three-term bf16 split away from O(1) operands.  bf16 has fp32's exponent range, so the split is
    scale-free while every term stays normal: operands around 1e+-30 and rows spread over 80 binades must give the same
    fp32-class error as O(1) data.  Below ~1e-33 the third term (2^-16 of the value) leaves the normal range; and a
    non-finite input poisons only its own output positions (NaN where an fp32 FMA chain would keep the infinity)."""
    n, Ci, Co, T, V = 4, 256, 256, 16, 25
    g = torch.Generator().manual_seed(11)
    x = _rand(g, n, Ci, T, V)
    w = _rand(g, Co, Ci, 1, 1, scale=Ci ** -0.5)
    gz = _rand(g, n, Co, T, V)
    if case == 'big_x_small_w':
        x, w, gz = x * 1e30, w * 1e-30, gz
    elif case == 'small_x_big_w':
        x, w, gz = x * 1e-30, w * 1e30, gz
    elif case == 'mixed_binades':
        k = torch.arange(Ci) % 81 - 40                       # channel c scaled by 2^k, its weight column by 2^-k
        sc = torch.pow(torch.tensor(2.0), k.float())
        x = x * sc.view(1, Ci, 1, 1)
        w = w / sc.view(1, Ci, 1, 1)
    elif case == 'near_subnormal':
        x = x * 1e-36                                        # third bf16 term ~1e-41: subnormal
    elif case == 'non_finite':
        x = x.clone()
        x[1, 7, 3, 5] = float('inf')
        x[2, 100, 9, 0] = float('nan')

    def run(mod, dt, dev):
        tx, tw = (t.to(dev, dt).requires_grad_() for t in (x, w))
        z = mod.pwconv(tx, None, None, None, False, tw, None, 1, False)[0]
        (z * gz.to(dev, dt)).sum().backward()
        return z.detach().cpu(), tx.grad.cpu(), tw.grad.cpu()

    got = run(K, torch.float32, DEV)
    if case == 'non_finite':
        z = got[0]
        bad = torch.zeros(n, T, V, dtype=torch.bool)
        bad[1, 3, 5] = bad[2, 9, 0] = True
        fin = torch.isfinite(z).all(1)                      # (n, T, V): positions whose every output channel is finite
        assert torch.equal(~fin, bad), 'a non-finite input must poison exactly its own output positions'
        xc = torch.where(torch.isfinite(x), x, torch.zeros_like(x))
        zr = R.pwconv(xc.double(), None, None, None, False, w.double(), None, 1, False)[0]
        assert rel(z.permute(0, 2, 3, 1)[fin], zr.permute(0, 2, 3, 1)[fin]) < 6e-7
        return
    ref = run(R, torch.float64, 'cpu')
    errs = {nm: rel(a, r_) for nm, a, r_ in zip(('z', 'dx', 'dW'), got, ref)}
    print(case, errs)
    # measured on gfx950: every case 2-4e-7 except near_subnormal (the residue terms flush): still below the north_star's
    # 1e-4 by two orders, but NOT fp32-class — documented in csrc/common.h and DESIGN §4
    bars = dict(z=6e-7, dx=6e-7, dW=3e-7) if case != 'near_subnormal' else dict(z=2e-5, dx=2e-5, dW=2e-5)
    for nm, e in errs.items():
        assert e < bars[nm], (case, nm, e)


@pytest.mark.parametrize('n,C,T,V,mode,tmean,flags', [
    (3, 64, 64, 25, 'res_plain', True, 1), (2, 128, 32, 25, 'res_affine', True, 1), (2, 64, 64, 25, 'affine', True, 1),
    (2, 256, 16, 25, 'res_plain', False, 1), (2, 12, 25, 17, 'res_affine', True, 1), (1, 5, 7, 18, 'plain', True, 1),
    (2, 64, 32, 25, 'res_plain', True, 3), (2, 32, 16, 25, 'res_affine', False, 3), (2, 16, 8, 17, 'affine', False, 2),
    (2, 16, 8, 25, 'res_affine', False, 0)])
def test_fuse_out(n, C, T, V, mode, tmean, flags):
    check_fuse_out(n, C, T, V, mode, tmean, flags)


def check_fuse_out(n, C, T, V, mode, tmean, flags, tee=False):
    """tmean: False / True / an int ld > V (the time mean with its joint row zero-padded to ld, the layout dynadj reads);
    tee: the output as three aliases (1), the third one the even frames as a tensor of their own (2)."""
    g = torch.Generator().manual_seed(C + T)
    x1 = _rand(g, n, C, T, V)
    a1 = None if mode in ('plain', 'res_x1') else (torch.rand(C, generator=g) + 0.5, _rand(g, C, scale=0.3))
    x2 = _rand(g, n, C, T, V) if mode.startswith('res') else None
    a2 = (torch.rand(C, generator=g) + 0.5, _rand(g, C, scale=0.3)) if mode == 'res_affine' else None
    # the ReLU's input off the knife edge (off_knife_edge): the inner one on the first term (flags bit 1), else the outer
    if int(flags) & 2:
        off_knife_edge(x1, a1, None, None, True)
    elif int(flags) & 1:
        off_knife_edge(x1, a1, x2, a2, True)
    go = _rand(g, n, C, T, V)
    gb = _rand(g, n, C, V if tmean is True or not tmean else int(tmean))

    def run(mod, dt, dev):
        def mk(t):
            return None if t is None else t.to(dev, dt).requires_grad_()
        tx1, tx2 = mk(x1), mk(x2)
        ta1 = None if a1 is None else (mk(a1[0]), mk(a1[1]))
        ta2 = None if a2 is None else (mk(a2[0]), mk(a2[1]))
        out, xbar = mod.fuse_out(tx1, ta1, tx2, ta2, flags, tmean, tee)
        even = None
        if tee:
            out, _, third = out
            even = third.x if tee == 2 and mod is K else (out[:, :, ::2] if tee == 2 else None)
        loss = (out * go.to(dev, dt)).sum()
        if even is not None:
            loss = loss + (even * go[:, :, ::2].to(dev, dt)).sum()
        if tmean:
            loss = loss + (xbar * gb.to(dev, dt)).sum()
        loss.backward()
        res = dict(out=out, dx1=tx1.grad)
        if even is not None:
            res['even'] = even
        if tmean:
            res['xbar'] = xbar
        if tx2 is not None:
            res['dx2'] = tx2.grad
        if ta1 is not None:
            res['ds1'], res['dh1'] = ta1[0].grad, ta1[1].grad
        if ta2 is not None:
            res['ds2'], res['dh2'] = ta2[0].grad, ta2[1].grad
        return res

    got = run(K, torch.float32, DEV)
    ref = run(R, torch.float64, ref_dev(n))
    for k, v in ref.items():
        # elementwise fp32 + sums over <= n*T*V terms: 1e-5 relative L2
        assert rel(got[k].detach().cpu(), v.detach()) < 1e-5, (k, rel(got[k].detach().cpu(), v.detach()))


def _drop_record_of_last_call(p):
    """the record the LAST fuse_out(dropout=p) call used (kernels._drop_state: its call number, this device's step counter)"""
    from dsgcn_amd import native
    st = K._drop_state
    step = next(iter(st['step'].values()))
    return native.Dropout(step.data_ptr(), int(torch.initial_seed()) & 0xffffffffffffffff, st['call'], float(p))


@pytest.mark.parametrize('n,C,T,V,mode,flags,form', [
    (2, 64, 16, 25, 'res_plain', 1, 'plain'),       # ST-GCN's block: relu(drop(bn(conv)) + x), 16-byte planes
    (3, 12, 9, 25, 'res_affine', 1, 'tmean'),       # odd planes (scalar kernels), residual through its own BatchNorm
    (2, 32, 16, 25, 'res_plain', 3, 'tee2'),        # CTR-GCN's MSTCN: its own ReLU first, even-frame second output
    (2, 48, 8, 17, 'affine', 1, 'pool'),            # the last block under the pooling head, no residual
    (2, 16, 7, 18, 'res_plain', 3, 'pool')])
@pytest.mark.parametrize('p', [0.5, 0.1])
def test_fuse_out_dropout(n, C, T, V, mode, flags, form, p):
    check_fuse_out_dropout(n, C, T, V, mode, flags, form, p)


def check_fuse_out_dropout(n, C, T, V, mode, flags, form, p):
    """Dropout inside fuse_out (csrc/dropout.h; reference: nn.Dropout behind the temporal unit's BatchNorm, tcn.py:30,33):
    no mask tensor exists in the product — the test asks dsgcn_dropout_mask for the multipliers the call used and checks
    (i) the multipliers: {0, 1/(1-p)}, keep rate within 5 sigma; (ii) forward AND backward (regenerated masks) against fp64
    torch given the same multipliers: relu(m * relu2?(x1*s1+h1) + residual); (iii) another call draws another mask."""
    torch.manual_seed(1234)
    g = torch.Generator().manual_seed(C + T + flags)
    x1 = _rand(g, n, C, T, V)
    a1 = (torch.rand(C, generator=g) + 0.5, _rand(g, C, scale=0.3))
    x2 = _rand(g, n, C, T, V) if mode.startswith('res') else None
    a2 = (torch.rand(C, generator=g) + 0.5, _rand(g, C, scale=0.3)) if mode == 'res_affine' else None
    T2 = (T + 1) // 2
    go, ge, gb, gp = _rand(g, n, C, T, V), _rand(g, n, C, T2, V), _rand(g, n, C, V), _rand(g, n, C)

    def mk(t, dev, dt):
        return None if t is None else t.to(dev, dt).requires_grad_()
    tx1, tx2 = mk(x1, DEV, torch.float32), mk(x2, DEV, torch.float32)
    ta1 = (mk(a1[0], DEV, torch.float32), mk(a1[1], DEV, torch.float32))
    ta2 = None if a2 is None else (mk(a2[0], DEV, torch.float32), mk(a2[1], DEV, torch.float32))
    if form == 'pool':
        pm = K.fuse_out_pool(tx1, ta1, tx2, ta2, flags, dropout=p)
        loss = (pm * gp.to(DEV)).sum()
        outs = dict(pm=pm)
    else:
        out, xbar = K.fuse_out(tx1, ta1, tx2, ta2, flags, form == 'tmean', 2 if form == 'tee2' else False, dropout=p)
        if form == 'tee2':
            oa, ob, oc = out
            loss = (oa * go.to(DEV)).sum() + (oc.x * ge.to(DEV)).sum()
            outs = dict(out=oa, even=oc.x)
        else:
            loss = (out * go.to(DEV)).sum()
            outs = dict(out=out)
            if form == 'tmean':
                loss = loss + (xbar * gb.to(DEV)).sum()
                outs['xbar'] = xbar
    rec = _drop_record_of_last_call(p)
    loss.backward()                                               # regenerates the masks from the same record
    m = K.dropout_mask(x1.numel(), rec).view(n, C, T, V)
    keep = (m > 0)
    assert torch.all((m == 0) | ((m - 1 / (1 - p)).abs() < 1e-6))
    N = m.numel()
    assert abs(keep.float().mean().item() - (1 - p)) < 5 * (p * (1 - p) / N) ** 0.5
    # fp64 reference with the same multipliers
    rdev = ref_dev(n)
    md = m.double().to(rdev)
    rx1, rx2 = mk(x1, rdev, torch.float64), mk(x2, rdev, torch.float64)
    ra1 = (mk(a1[0], rdev, torch.float64), mk(a1[1], rdev, torch.float64))
    ra2 = None if a2 is None else (mk(a2[0], rdev, torch.float64), mk(a2[1], rdev, torch.float64))
    v = rx1 * ra1[0].view(1, -1, 1, 1) + ra1[1].view(1, -1, 1, 1)
    if flags & 2:
        v = v.relu()
    v = v * md
    if rx2 is not None:
        v = v + (rx2 * ra2[0].view(1, -1, 1, 1) + ra2[1].view(1, -1, 1, 1) if ra2 is not None else rx2)
    ro = v.relu() if flags & 1 else v
    if form == 'pool':
        rloss = (ro.mean((2, 3)) * gp.double().to(rdev)).sum()
        refs = dict(pm=ro.mean((2, 3)))
    elif form == 'tee2':
        rloss = (ro * go.double().to(rdev)).sum() + (ro[:, :, ::2] * ge.double().to(rdev)).sum()
        refs = dict(out=ro, even=ro[:, :, ::2])
    else:
        rloss = (ro * go.double().to(rdev)).sum()
        refs = dict(out=ro)
        if form == 'tmean':
            rloss = rloss + (ro.mean(2) * gb.double().to(rdev)).sum()
            refs['xbar'] = ro.mean(2)
    rloss.backward()
    for k, want in refs.items():
        assert rel(outs[k].detach().cpu(), want.detach()) < 1e-6, (k, rel(outs[k].detach().cpu(), want.detach()))
    pairs = [('dx1', tx1, rx1), ('ds1', ta1[0], ra1[0]), ('dh1', ta1[1], ra1[1])]
    if tx2 is not None:
        pairs.append(('dx2', tx2, rx2))
    if ta2 is not None:
        pairs += [('ds2', ta2[0], ra2[0]), ('dh2', ta2[1], ra2[1])]
    for k, a, b in pairs:
        assert rel(a.grad.cpu(), b.grad) < 1e-5, (k, rel(a.grad.cpu(), b.grad))
    # the next call (another layer / another eager forward) draws another mask; so does the next training step
    K.fuse_out(tx1.detach(), None, None, None, 0, False, False, dropout=p)
    m2 = K.dropout_mask(x1.numel(), _drop_record_of_last_call(p)).view_as(m)
    agree = ((m2 > 0) == keep).float().mean().item()
    assert abs(agree - ((1 - p) ** 2 + p ** 2)) < 6 * (0.25 / N) ** 0.5, agree
    K.dropout_step_advance()
    m3 = K.dropout_mask(x1.numel(), rec).view_as(m)
    agree = ((m3 > 0) == keep).float().mean().item()
    assert abs(agree - ((1 - p) ** 2 + p ** 2)) < 6 * (0.25 / N) ** 0.5, agree
    # p = 0 through the dropout entry points is exactly the plain call
    o0 = K.fuse_out(tx1.detach(), (ta1[0].detach(), ta1[1].detach()), None, None, 1, False, False)[0]
    lib = __import__('dsgcn_amd').native.lib()
    o1 = torch.empty_like(o0)
    st = torch.cuda.current_stream().cuda_stream
    x1d, s1d, h1d = tx1.detach(), ta1[0].detach(), ta1[1].detach()
    z = __import__('dsgcn_amd').native.Dropout(0, 5, 7, 0.0)
    import ctypes
    assert lib.dsgcn_fuse_out_fwd_drop(x1d.data_ptr(), s1d.data_ptr(), h1d.data_ptr(), None, None, None, 1, o1.data_ptr(), None,
                                       None, None, n, C, T, V, V, ctypes.byref(z), st) == 0
    assert torch.equal(o0, o1)


@pytest.mark.parametrize('n,C,T,V', [(2, 16, 16, 25), (3, 8, 9, 25), (2, 12, 7, 17), (1, 64, 64, 25)])
@pytest.mark.parametrize('streams', [3, 2, 1])
def test_fuse_out_even_frame_output(n, C, T, V, streams):
    """fuse_out(tee=2): the third output is out[:, :, ::2] as a tensor of its own (what a stride-2 block's 1x1 residual conv
    reads, dgstgcn.py:35-40) and its gradient comes back in that shape — against the three-alias form with the strided
    slice taken by torch (odd frame counts, planes that are not multiples of four floats, missing alias gradients)."""
    g = torch.Generator().manual_seed(C + T + streams)
    x1, x2 = _rand(g, n, C, T, V), _rand(g, n, C, T, V)
    a1 = (torch.rand(C, generator=g) + 0.5, _rand(g, C, scale=0.3))
    T2 = (T + 1) // 2
    ga, gb, gc, gx = _rand(g, n, C, T, V), _rand(g, n, C, T, V), _rand(g, n, C, T2, V), _rand(g, n, C, V)

    def run(even):
        tx1, tx2 = x1.to(DEV).requires_grad_(), x2.to(DEV).requires_grad_()
        ta1 = (a1[0].to(DEV).requires_grad_(), a1[1].to(DEV).requires_grad_())
        (oa, ob, oc), xbar = K.fuse_out(tx1, ta1, tx2, None, True, True, 2 if even else True)
        if even:
            assert isinstance(oc, K.Prestrided) and (oc.stride, oc.frames) == (2, T) and oc.x.shape == (n, C, T2, V)
            oc_s = oc.x
        else:
            oc_s = oc[:, :, ::2]
        loss = (oc_s * gc.to(DEV)).sum() + (xbar * gx.to(DEV)).sum()
        if streams >= 2:
            loss = loss + (oa * ga.to(DEV)).sum()
        if streams >= 3:
            loss = loss + (ob * gb.to(DEV)).sum()
        loss.backward()
        return dict(out=oa, oc=oc_s, xbar=xbar, dx1=tx1.grad, dx2=tx2.grad, ds1=ta1[0].grad, dh1=ta1[1].grad)

    got, ref = run(True), run(False)
    for k, v in ref.items():
        if k in ('out', 'oc', 'xbar'):
            assert torch.equal(got[k], v), k
        else:
            # the alias form adds the zero-interleaved slice gradient through autograd (a different order of the adds)
            assert rel(got[k].cpu(), v.cpu().double()) < 1e-6, (k, rel(got[k].cpu(), v.cpu().double()))


@pytest.mark.parametrize('n,C,T,V,stride', [(2, 64, 32, 25, 1), (2, 128, 32, 25, 2), (2, 48, 20, 17, 1), (1, 12, 9, 18, 2),
                                            # the fused stage (csrc/tms.hip): full tiles, a ragged last tile, two tiles per
                                            # sample at stride 2, three m-tiles, K400 planes
                                            (3, 64, 64, 25, 1), (2, 64, 24, 25, 1), (2, 128, 64, 25, 2), (2, 256, 8, 25, 1),
                                            (2, 64, 100, 17, 2), (5, 128, 32, 25, 1),
                                            # wide-load kernels at 2 MFMA row tiles / 64-channel weight-gradient tiles, both strides
                                            (2, 256, 16, 25, 1), (2, 256, 16, 25, 2),
                                            # frame counts the weight gradient's 4-frame units do not divide (mixed paths)
                                            (2, 64, 10, 25, 1), (2, 64, 12, 25, 2), (3, 64, 6, 17, 1),
                                            # split layout (csrc/tmsplit.hip): a single 4-frame unit (every halo outside the plane), the
                                            # smallest joint count (128 frames of haug per block), K400's stride-1 planes
                                            (1, 64, 4, 25, 1), (2, 36, 8, 5, 1), (2, 64, 100, 17, 1)])
@pytest.mark.parametrize('fused', ['1', '0', 'split'])
def test_temporal_ms(n, C, T, V, stride, fused, monkeypatch):
    check_temporal_ms(n, C, T, V, stride, fused, monkeypatch)


def check_temporal_ms(n, C, T, V, stride, fused, monkeypatch, want_bn=True):
    """fused '1': the one-launch-per-direction stage (csrc/tms.hip) wherever the shape is eligible; '0': the staged chain
    (branch_act -> tapconv -> combine); 'split': the split layout (csrc/tmsplit.hip: no (V+1)-column tensors) wherever
    the shape is eligible (V odd, T % 4 == 0; stride 2: T % 8 == 0) — ineligible shapes are skipped, not silently run on
    the staged chain.  All against the fp64 statement of the op.  want_bn False: the eval-mode call — no statistics,
    under torch.no_grad() on inputs without history — and its output alone."""
    monkeypatch.setattr(K, 'FUSED_TEMPORAL', '0' if fused == 'split' else fused)
    monkeypatch.setattr(K, 'SPLIT_TEMPORAL', '2' if fused == 'split' else '0')
    g = torch.Generator().manual_seed(C + T + stride)
    cfg = [(3, 1), (3, 2), (3, 3), (3, 4), ('max', 3), '1x1']
    mid = C // 6
    widths = [C - 5 * mid] + [mid] * 5
    if fused == 'split':
        # the split layout takes V odd, T % 4 == 0 (stride 2: T % 8 == 0, T <= 128), windows <= 64 channels; every other
        # shape would silently run the staged chain ('0' already covers it): the library's answer must be this rule, and
        # only the shapes it takes count as split cases
        takes = dsgcn_amd.native.lib().dsgcn_tms_split_rows(
            -1, n, C, T, V, stride, 3, 6, K._int_array([0, 0, 0, 0, 1, 2]), K._int_array([sum(widths[:i]) for i in range(6)]),
            K._int_array(widths), K._int_array([1, 2, 3, 4, 1, 1]))
        rule = V % 2 == 1 and max(widths) <= 64 and (T % 4 == 0 if stride == 1 else (T % 8 == 0 and T <= 128))
        assert (takes == 1) == rule, (takes, rule)
        if not rule:
            pytest.skip('not a split-layout shape (covered by the staged chain, fused = 0)')
    n_act = C - mid
    z = _rand(g, n, C, T, V)
    zaug = _rand(g, n, C, T)
    scale = torch.cat([torch.rand(n_act, generator=g) + 0.5, torch.ones(mid)])
    shift = torch.cat([_rand(g, n_act, scale=0.3), torch.zeros(mid)])
    cw = [_rand(g, w, w, 3, 1, scale=(3 * w) ** -0.5) for w in widths[:4]]
    cb = [_rand(g, w, scale=0.1) for w in widths[:4]]
    coeff = _rand(g, 25, scale=0.5)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = _rand(g, C, scale=0.2)
    Tout = (T + stride - 1) // stride
    gf = _rand(g, n, C, Tout, V)
    gsc, gsh = _rand(g, C), _rand(g, C)

    def run(mod, dt, dev):
        def mk(t):
            return t.to(dev, dt).requires_grad_(want_bn)
        tz, tza, tsc, tsh, tco, tga, tbe = mk(z), mk(zaug), mk(scale), mk(shift), mk(coeff), mk(gamma), mk(beta)
        tw, tb = [mk(w) for w in cw], [mk(b) for b in cb]
        if not want_bn:
            with torch.no_grad():
                return dict(f=mod.temporal_ms(tz, tza, tsc, tsh, n_act, cfg, widths, tw, tb, tco, stride)[0])
        f, sc, sh, mean, var = mod.temporal_ms(tz, tza, tsc, tsh, n_act, cfg, widths, tw, tb, tco, stride, tga, tbe,
                                               1e-5, True)
        ((f * gf.to(dev, dt)).sum() + (sc * gsc.to(dev, dt)).sum() + (sh * gsh.to(dev, dt)).sum()).backward()
        res = dict(f=f, sc=sc, sh=sh, mean=mean, var=var, dz=tz.grad, dzaug=tza.grad, dscale=tsc.grad, dshift=tsh.grad,
                   dcoeff=tco.grad[:V], dgamma=tga.grad, dbeta=tbe.grad)
        for i in range(4):
            res[f'dw{i}'] = tw[i].grad
            res[f'db{i}'] = tb[i].grad
        return res

    got = run(K, torch.float32, DEV)
    ref = run(R, torch.float64, ref_dev(n))
    for k, v in ref.items():
        # three HIP stages (branch_act, the fp32-MFMA tap kernels, combine + statistics): 5e-5 relative L2 against fp64
        assert rel(got[k].detach().cpu(), v.detach()) < 5e-5, (k, rel(got[k].detach().cpu(), v.detach()))


@pytest.mark.parametrize('C,T,stride', [(64, 64, 1), (128, 32, 1), (256, 16, 1), (128, 64, 2), (256, 32, 2)])
def test_temporal_ms_split_at_full_size(C, T, stride, monkeypatch):
    """The split layout at BASELINE's size (128 person-samples, the five unit shapes of DS-STGCN): thousands of position
    tiles, tiles that cross samples, the window pairs of the 64-channel weight gradient — against the staged chain (which
    the cases above pin to the fp64 statement of the op) on every output and gradient."""
    n, V = 128, 25
    g = torch.Generator().manual_seed(C + T)
    cfg = [(3, 1), (3, 2), (3, 3), (3, 4), ('max', 3), '1x1']
    mid = C // 6
    widths = [C - 5 * mid] + [mid] * 5
    n_act = C - mid
    z, zaug = _rand(g, n, C, T, V).to(DEV), _rand(g, n, C, T).to(DEV)
    scale = torch.cat([torch.rand(n_act, generator=g) + 0.5, torch.ones(mid)]).to(DEV)
    shift = torch.cat([_rand(g, n_act, scale=0.3), torch.zeros(mid)]).to(DEV)
    cw = [_rand(g, w, w, 3, 1, scale=(3 * w) ** -0.5).to(DEV) for w in widths[:4]]
    cb = [_rand(g, w, scale=0.1).to(DEV) for w in widths[:4]]
    coeff, gamma, beta = _rand(g, 25, scale=0.5).to(DEV), (torch.rand(C, generator=g) + 0.5).to(DEV), _rand(g, C, scale=0.2).to(DEV)
    gf, gsc, gsh = _rand(g, n, C, T // stride, V).to(DEV), _rand(g, C).to(DEV), _rand(g, C).to(DEV)

    def run(split):
        monkeypatch.setattr(K, 'FUSED_TEMPORAL', '0')
        monkeypatch.setattr(K, 'SPLIT_TEMPORAL', '2' if split else '0')
        lv = [t.clone().requires_grad_() for t in (z, zaug, scale, shift, coeff, gamma, beta)]
        tw, tb = [w.clone().requires_grad_() for w in cw], [b.clone().requires_grad_() for b in cb]
        f, sc, sh, mean, var = K.temporal_ms(lv[0], lv[1], lv[2], lv[3], n_act, cfg, widths, tw, tb, lv[4], stride, lv[5], lv[6],
                                             1e-5, True)
        ((f * gf).sum() + (sc * gsc).sum() + (sh * gsh).sum()).backward()
        return [f, sc, sh, mean, var] + [t.grad for t in lv] + [w.grad for w in tw] + [b.grad for b in tb]

    assert dsgcn_amd.native.lib().dsgcn_tms_split_rows(-1, n, C, T, V, stride, 3, 6, K._int_array([0, 0, 0, 0, 1, 2]),
                                             K._int_array([sum(widths[:i]) for i in range(6)]), K._int_array(widths),
                                             K._int_array([1, 2, 3, 4, 1, 1])) == 1
    got, ref = run(True), run(False)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert rel(a.detach().cpu(), b.detach().cpu().double()) < 2e-6, (i, rel(a.detach().cpu(), b.detach().cpu().double()))


@pytest.mark.parametrize('n,K,Co,T,V,shared,bn', [
    (2, 3, 16, 64, 25, True, True), (2, 3, 64, 16, 25, True, True), (3, 3, 8, 100, 17, True, False),
    (2, 3, 16, 64, 25, False, True), (2, 3, 32, 32, 25, False, True), (2, 3, 8, 130, 17, False, True),
    (1, 2, 5, 7, 18, False, False),
    # full size: CTR-GCN's three stage shapes (per-sample, per-channel adjacency) and ST-GCN's (shared) at 128 person-samples
    (128, 3, 64, 64, 25, False, True), (128, 3, 128, 32, 25, False, True), (128, 3, 256, 16, 25, False, True),
    (128, 3, 64, 64, 25, True, True), (128, 3, 256, 16, 25, True, True)])
def test_aggregate_sum(n, K, Co, T, V, shared, bn):
    check_aggregate_sum(n, K, Co, T, V, shared, bn)


def check_aggregate_sum(n, K, Co, T, V, shared, bn, grad=True):
    """grad False: the eval-mode call (torch.no_grad(), inputs without history, bn False) and its output alone."""
    assert grad or not bn
    g = torch.Generator().manual_seed(Co + T + V)
    p = _rand(g, n, K * Co, T, V)
    adj = _rand(g, K, V, V, scale=0.3) if shared else _rand(g, n, K * Co, V, V, scale=0.3)
    gamma = torch.rand(Co, generator=g) + 0.5
    beta = _rand(g, Co, scale=0.2)
    gy, gsc, gsh = _rand(g, n, Co, T, V), _rand(g, Co), _rand(g, Co)

    def run(mod, dt, dev):
        def mk(t):
            return t.to(dev, dt).requires_grad_(grad)
        tp, ta, tg, tb = mk(p), mk(adj), mk(gamma), mk(beta)
        if not grad:
            with torch.no_grad():
                return dict(y=mod.aggregate_sum(tp, ta, K)[0])
        y, sc, sh, mean, var = mod.aggregate_sum(tp, ta, K, tg if bn else None, tb if bn else None, 1e-5, bn)
        loss = (y * gy.to(dev, dt)).sum()
        if bn:
            loss = loss + (sc * gsc.to(dev, dt)).sum() + (sh * gsh.to(dev, dt)).sum()
        loss.backward()
        res = dict(y=y, dp=tp.grad, dadj=ta.grad)
        if bn:
            res.update(sc=sc, sh=sh, mean=mean, var=var, dgamma=tg.grad, dbeta=tb.grad)
        return res

    got = run(K_, torch.float32, DEV)
    ref = run(R, torch.float64, ref_dev(n))
    for k, v in ref.items():
        # fp32 accumulation over K*V (fwd) / T (dadj, x n*Co for the shared form) terms: 1e-5 relative L2
        assert rel(got[k].detach().cpu(), v.detach()) < 1e-5, (k, rel(got[k].detach().cpu(), v.detach()))


@pytest.mark.parametrize('n,K,Co,T,V', [(2, 3, 16, 64, 25), (3, 3, 32, 32, 25), (2, 3, 8, 130, 17), (128, 3, 64, 64, 25),
                                        (128, 3, 256, 16, 25)])
def test_aggregate_sum_subset_major_adjacency(n, K, Co, T, V):
    check_aggregate_sum_subset_major_adjacency(n, K, Co, T, V)


def check_aggregate_sum_subset_major_adjacency(n, K, Co, T, V):
    """The per-sample, per-channel adjacency handed over as (K, n, Co, V, V) (what ctr_topology's one-conv form writes): the
    same launches with other strides — bit-identical to the (n, K*Co, V, V) call on the permuted tensor, gradient included."""
    g = torch.Generator().manual_seed(Co + T)
    p = _rand(g, n, K * Co, T, V).to(DEV)
    adj = _rand(g, n, K * Co, V, V, scale=0.3).to(DEV)
    gamma, beta = (torch.rand(Co, generator=g) + 0.5).to(DEV), _rand(g, Co, scale=0.2).to(DEV)
    gy = _rand(g, n, Co, T, V).to(DEV)

    def run(major):
        tp = p.clone().requires_grad_()
        ta = (adj.view(n, K, Co, V, V).permute(1, 0, 2, 3, 4).contiguous() if major else adj.clone()).requires_grad_()
        y, sc, sh, mean, var = K_.aggregate_sum(tp, ta, K, gamma, beta, 1e-5, True)
        ((y * gy).sum() + sc.sum() + (sh * sh).sum()).backward()
        da = ta.grad.permute(1, 0, 2, 3, 4).reshape(n, K * Co, V, V) if major else ta.grad
        return dict(y=y, sc=sc, sh=sh, dp=tp.grad, dadj=da)

    a, b = run(False), run(True)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('n,Ci,Co,V', [(2, 3, 64, 25), (2, 64, 64, 25), (3, 128, 256, 25), (2, 256, 256, 17),
                                       # full size: CTR-GCN's first and last stage at 128 person-samples
                                       (128, 64, 64, 25), (128, 256, 256, 25)])
@pytest.mark.parametrize('subset_major', [False, True])
def test_ctr_topology(n, Ci, Co, V, subset_major):
    check_ctr_topology(n, Ci, Co, V, subset_major)


def check_ctr_topology(n, Ci, Co, V, subset_major, alpha_per_subset=False, beta=False, edge=(), E=15):
    """subset_major: Ahat as (K, n, Co, V, V) through the one-conv form of the classic refinement (conv4 + alpha + A as one
    1x1 conv over [d | A[k] | 1]); the plain call keeps the (n, K*Co, V, V) contract and the separate affine pass.
    alpha_per_subset / beta / edge: unit_ctrhgcn's form on the per-subset path — one alpha per subset (_CtrAffine), the
    Gram term beta_k x1_k^T x2_k (kernels.gram on one-frame planes), and on the subsets in ``edge`` the edge-typed attention
    conv over E classes + select (_EdgeSelect) before conv4."""
    g = torch.Generator().manual_seed(Ci + Co)
    K = 3
    Rr = 8 if Ci <= 16 else Ci // 8
    t = dict(xbar=_rand(g, n, Ci, V), w1=_rand(g, K * Rr, Ci, scale=Ci ** -0.5), b1=_rand(g, K * Rr, scale=0.1),
             w2=_rand(g, K * Rr, Ci, scale=Ci ** -0.5), b2=_rand(g, K * Rr, scale=0.1), alpha=_rand(g, 1, scale=0.7),
             A=_rand(g, K, V, V, scale=0.2))
    w4 = [_rand(g, Co, Rr, scale=Rr ** -0.5) for _ in range(K)]
    b4 = [_rand(g, Co, scale=0.1) for _ in range(K)]
    gah = _rand(g, n, K * Co, V, V)
    classic = not (alpha_per_subset or beta or edge)
    if alpha_per_subset:
        t['alpha'] = _rand(g, K, scale=0.7)
    if beta:
        t['beta'] = _rand(g, K, scale=0.5)
    et = torch.tensor(dsgcn_amd.Graph(layout={25: 'nturgb+d', 17: 'coco'}[V], mode='spatial').edge_type,
                      dtype=torch.int32).reshape(-1) if edge else None
    assert et is None or int(et.max()) < E
    we = {k: _rand(g, E * Rr, Rr, scale=Rr ** -0.5) for k in edge}
    be = {k: _rand(g, E * Rr, scale=0.1) for k in edge}

    def run(mod, dt, dev):
        tt = {k: v.to(dev, dt).requires_grad_() for k, v in t.items()}
        tw4 = [w.to(dev, dt).requires_grad_() for w in w4]
        tb4 = [b.to(dev, dt).requires_grad_() for b in b4]
        twe = {k: w.to(dev, dt).requires_grad_() for k, w in we.items()}
        tbe = {k: b.to(dev, dt).requires_grad_() for k, b in be.items()}
        ted = {k: (twe[k], tbe[k], et.to(dev)) for k in edge}
        ah = mod.ctr_topology(tt['xbar'], tt['w1'], tt['b1'], tt['w2'], tt['b2'], tw4, tb4, tt['alpha'], tt['A'],
                              tt.get('beta'), ted, subset_major=subset_major)
        if ah.dim() == 5:
            assert mod is K_ and ah.shape == (K, n, Co, V, V)
            ah = ah.permute(1, 0, 2, 3, 4).reshape(n, K * Co, V, V)
        else:
            assert not (mod is K_ and subset_major and classic)
        ah.backward(gah.to(dev, dt))
        res = {'ahat': ah}
        res.update({'d' + k: v.grad for k, v in tt.items()})
        for k in range(K):
            res[f'dw4_{k}'], res[f'db4_{k}'] = tw4[k].grad, tb4[k].grad
        for k in edge:
            res[f'dwe_{k}'], res[f'dbe_{k}'] = twe[k].grad, tbe[k].grad
        return res

    got = run(K_, torch.float32, DEV)
    ref = run(R, torch.float64, ref_dev(n))
    for k, v in ref.items():
        # tanhf + fp32 MFMA accumulation over <= 32 (fwd) / n*V*V*Co (grads) terms: 2e-5 relative L2
        assert rel(got[k].detach().cpu(), v.detach()) < 2e-5, (k, rel(got[k].detach().cpu(), v.detach()))


@pytest.mark.parametrize('shared', [False, True])
def test_ctr_one_conv_deferred_sums_with_shared_leaves(shared):
    """inside a deferred_param_sums() region the one-conv refinement defers the conv's partial-row sums
    and _CtrWPrep's finishing launch to the flush — both sides must take the SAME decision.  With conv4 / alpha shared by
    two units (leaves registered by two deferring calls) both fall back to immediate sums; either way the gradients equal
    the ones computed without the region."""
    g = torch.Generator().manual_seed(11)
    K, n, Ci, Co, V = 3, 4, 64, 64, 25
    Rr = Ci // 8
    mk = lambda *sh, scale=1.0: _rand(g, *sh, scale=scale).to(DEV)
    xb = [mk(n, Ci, V), mk(n, Ci, V)]
    base = dict(w1=mk(K * Rr, Ci, scale=Ci ** -0.5), b1=mk(K * Rr, scale=0.1), w2=mk(K * Rr, Ci, scale=Ci ** -0.5),
                b2=mk(K * Rr, scale=0.1), alpha=mk(1, scale=0.7), A=mk(K, V, V, scale=0.2))
    w4 = [mk(Co, Rr, scale=Rr ** -0.5) for _ in range(K)]
    b4 = [mk(Co, scale=0.1) for _ in range(K)]
    gah = [mk(K, n, Co, V, V), mk(K, n, Co, V, V)]

    def run(deferred):
        K_.reset_leaf_uses()
        sets = []
        for u in range(2):
            if u == 0 or not shared:
                tt = {k: v.clone().requires_grad_() for k, v in base.items()}
                tw4 = [w.clone().requires_grad_() for w in w4]
                tb4 = [b.clone().requires_grad_() for b in b4]
            sets.append((tt, tw4, tb4))
        outs = [K_.ctr_topology(x, tt['w1'], tt['b1'], tt['w2'], tt['b2'], tw4, tb4, tt['alpha'], tt['A'],
                                subset_major=True) for x, (tt, tw4, tb4) in zip(xb, sets)]
        loss = sum((o * gg).sum() for o, gg in zip(outs, gah))
        if deferred:
            with K_.deferred_param_sums():
                loss.backward()
        else:
            loss.backward()
        K_.end_step()
        res = {}
        for u, (tt, tw4, tb4) in enumerate(sets[:1] if shared else sets):
            res.update({f'{u}.d{k}': v.grad.clone() for k, v in tt.items()})
            for k in range(K):
                res[f'{u}.dw4_{k}'], res[f'{u}.db4_{k}'] = tw4[k].grad.clone(), tb4[k].grad.clone()
        return res

    want = run(False)
    got = run(True)
    for k, v in want.items():
        assert torch.isfinite(got[k]).all(), k
        # not shared: the same ordered sums either way, bit for bit; shared: autograd adds the two calls' gradients in the
        # same order in both runs as well
        assert torch.equal(got[k], v), (k, rel(got[k].cpu(), v.cpu()))


def test_ctr_operands_one_launch_per_step_is_bit_identical(monkeypatch):
    """The augmented conv4 operands of all CTR-GCN units come from ONE launch per step (rebuilt from the weights at the first
    unit's call) and their finishing launches ride in one launch behind the deferred sums: three units, three steps with the
    parameters rewritten between steps the way dsgcn_sgd_step does (through .data — no version counter moves), against the
    same steps with every unit building its own operands.  Outputs and gradients must match bit for bit, and the
    second and third steps must really have taken the batched path."""
    from dsgcn_amd import native
    g = torch.Generator().manual_seed(23)
    K, n, Ci, V = 3, 4, 64, 25
    Rr = Ci // 8
    mk = lambda *sh, scale=1.0: _rand(g, *sh, scale=scale).to(DEV)
    units = []
    for Co in (64, 64, 128):
        base = dict(w1=mk(K * Rr, Ci, scale=Ci ** -0.5), b1=mk(K * Rr, scale=0.1), w2=mk(K * Rr, Ci, scale=Ci ** -0.5),
                    b2=mk(K * Rr, scale=0.1), alpha=mk(1, scale=0.7), A=mk(K, V, V, scale=0.2))
        units.append((base, [mk(Co, Rr, scale=Rr ** -0.5) for _ in range(K)], [mk(Co, scale=0.1) for _ in range(K)],
                      mk(n, Ci, V), mk(K, n, Co, V, V)))

    def steps(batch):
        monkeypatch.setattr(K_, 'CTR_PREP_BATCH', batch)
        K_._ctr_prep_cache.clear()
        leaves = [({k: v.clone().requires_grad_() for k, v in base.items()}, [w.clone().requires_grad_() for w in w4],
                   [b.clone().requires_grad_() for b in b4]) for base, w4, b4, _, _ in units]
        out, took = [], []
        for step in range(3):
            K_.reset_leaf_uses()
            ahat = [K_.ctr_topology(x, tt['w1'], tt['b1'], tt['w2'], tt['b2'], tw4, tb4, tt['alpha'], tt['A'],
                                    subset_major=True) for (tt, tw4, tb4), (_, _, _, x, _) in zip(leaves, units)]
            took.append(K_._ctr_prep_cache.batched == K_._wsplit_state['epoch'])
            loss = sum((o * u[4]).sum() for o, u in zip(ahat, units))
            with K_.deferred_param_sums():
                loss.backward()
            K_.end_step()
            res = {f'{i}.ahat': o.detach().clone() for i, o in enumerate(ahat)}
            for i, (tt, tw4, tb4) in enumerate(leaves):
                res.update({f'{i}.d{k}': v.grad.clone() for k, v in tt.items()})
                for k in range(K):
                    res[f'{i}.dw4_{k}'], res[f'{i}.db4_{k}'] = tw4[k].grad.clone(), tb4[k].grad.clone()
                for p in [*tt.values(), *tw4, *tb4]:
                    p.data.mul_(0.9).add_(0.01)              # the optimizer's raw write
                    p.grad = None
            out.append(res)
        return out, took

    want, took0 = steps(False)
    got, took1 = steps(True)
    assert took0 == [False] * 3 and took1 == [False, True, True], (took0, took1)
    for a, b in zip(want, got):
        for k, v in a.items():
            assert torch.equal(b[k], v), k
    assert not torch.equal(want[0]['0.ahat'], want[1]['0.ahat'])       # (the rewritten weights were seen)
    # more records than one launch holds (DSGCN_CTR_JOBS_MAX = 16): the entry points chunk
    nj, Co = 19, 32
    w = [[mk(Co, Rr) for _ in range(K)] for _ in range(nj)]
    b = [[mk(Co) for _ in range(K)] for _ in range(nj)]
    al = [mk(1) for _ in range(nj)]
    wout = torch.zeros(nj, K, Co, Rr + 2, device=DEV)
    sh = torch.zeros(nj, K, 2, Rr + 2, device=DEV)
    tab = (native.CtrPrepJob * nj)()
    for i, rec in enumerate(tab):
        for k in range(K):
            rec.w[k], rec.b[k] = w[i][k].data_ptr(), (b[i][k].data_ptr() if (i + k) % 3 else None)
        rec.alpha, rec.wout, rec.sh, rec.K, rec.Co, rec.R = al[i].data_ptr(), wout[i].data_ptr(), sh[i].data_ptr(), K, Co, Rr
    native.check(native.lib().dsgcn_ctr_wprep_multi(tab, nj, K_._stream()), 'dsgcn_ctr_wprep_multi')
    for i in range(nj):
        for k in range(K):
            bias = b[i][k] if (i + k) % 3 else torch.zeros(Co, device=DEV)
            assert torch.equal(wout[i, k], torch.cat([w[i][k], torch.ones(Co, 1, device=DEV), bias[:, None]], 1)), (i, k)
            assert torch.equal(sh[i, k, 0], torch.cat([al[i].expand(Rr), torch.ones(1, device=DEV), al[i]])), (i, k)
            assert not sh[i, k, 1].any()
    dwp = [[mk(Co, Rr + 2) for _ in range(K)] for _ in range(nj)]
    ds = [[mk(Rr + 2, 3) for _ in range(K)] for _ in range(nj)]
    out = torch.zeros(nj, K, Co * Rr + Co, device=DEV)
    dal = torch.zeros(nj, device=DEV)
    ftab = (native.CtrFinJob * nj)()
    for i, rec in enumerate(ftab):
        for k in range(K):
            rec.dwp[k], rec.ds[k], rec.out[k] = dwp[i][k].data_ptr(), ds[i][k].data_ptr(), out[i, k].data_ptr()
        rec.dalpha, rec.K, rec.Co, rec.R, rec.ds_stride = dal[i:].data_ptr(), K, Co, Rr, 3
    native.check(native.lib().dsgcn_ctr_wfin_multi(ftab, nj, K_._stream()), 'dsgcn_ctr_wfin_multi')
    for i in range(nj):
        a = 0.0
        for k in range(K):
            assert torch.equal(out[i, k, :Co * Rr].view(Co, Rr), dwp[i][k][:, :Rr]) and \
                torch.equal(out[i, k, Co * Rr:], dwp[i][k][:, Rr + 1]), (i, k)
            a += float(ds[i][k][:Rr, 0].double().sum() + ds[i][k][Rr + 1, 0].double())
        assert abs(float(dal[i]) - a) <= 1e-5 * max(1.0, abs(a)), (i, float(dal[i]), a)


@pytest.mark.parametrize('n,C,T,V,stride,ks', [(2, 64, 32, 25, 1, 5), (2, 128, 32, 25, 2, 5), (2, 256, 16, 25, 1, 5),
                                               (2, 32, 21, 17, 2, 5), (1, 16, 9, 18, 1, 3)])
@pytest.mark.parametrize('fused', ['1', '0'])
def test_temporal_branches_bn(n, C, T, V, stride, ks, fused, monkeypatch):
    check_temporal_branches_bn(n, C, T, V, stride, ks, fused, monkeypatch)


def _ms_widths(C, cfg):
    """dgmstcn / mstcn / msmlp's branch widths: C // branches each, the remainder on the first branch"""
    mid = C // len(cfg)
    return [C - mid * (len(cfg) - 1)] + [mid] * (len(cfg) - 1)


def check_temporal_branches_bn(n, C, T, V, stride, ks, fused, monkeypatch, cfg=None):
    """MSTCN's stage: BN+ReLU, two dilated (k,1) convs, max-pool, strided copy, closing BatchNorm statistics.
    cfg: another branch table (mstcn's six branches, widths as the unit makes them) instead of MSTCN's four of kernel ks."""
    monkeypatch.setattr(K, 'FUSED_TEMPORAL', fused)
    g = torch.Generator().manual_seed(C + T + stride)
    if cfg is None:
        cfg = [(ks, 1), (ks, 2), ('max', 3), '1x1']
        bc = C // 4
        widths = [bc, bc, bc, C - 3 * bc]
    else:
        cfg = [tuple(c) if isinstance(c, (tuple, list)) else c for c in cfg]
        widths = _ms_widths(C, cfg)
    n_act = sum(w for w, c in zip(widths, cfg) if c != '1x1')
    convs = [(w, c[0]) for w, c in zip(widths, cfg) if c != '1x1' and c[0] != 'max']
    z = _rand(g, n, C, T, V)
    scale = torch.cat([torch.rand(n_act, generator=g) + 0.5, torch.ones(C - n_act)])
    shift = torch.cat([_rand(g, n_act, scale=0.3), torch.zeros(C - n_act)])
    cw = [_rand(g, w, w, k, 1, scale=(k * w) ** -0.5) for w, k in convs]
    cb = [_rand(g, w, scale=0.1) for w, _ in convs]
    gamma = torch.rand(C, generator=g) + 0.5
    beta = _rand(g, C, scale=0.2)
    Tout = (T + stride - 1) // stride
    go, gsc, gsh = _rand(g, n, C, Tout, V), _rand(g, C), _rand(g, C)

    def run(mod, dt, dev):
        def mk(t):
            return t.to(dev, dt).requires_grad_()
        tz, tsc, tsh, tga, tbe = mk(z), mk(scale), mk(shift), mk(gamma), mk(beta)
        tw, tb = [mk(w) for w in cw], [mk(b) for b in cb]
        o, sc, sh, mean, var = mod.temporal_branches_bn(tz, tsc, tsh, n_act, cfg, widths, tw, tb, stride, tga, tbe,
                                                        1e-5, True)
        ((o * go.to(dev, dt)).sum() + (sc * gsc.to(dev, dt)).sum() + (sh * gsh.to(dev, dt)).sum()).backward()
        res = dict(o=o, sc=sc, sh=sh, mean=mean, var=var, dz=tz.grad, dscale=tsc.grad, dshift=tsh.grad,
                   dgamma=tga.grad, dbeta=tbe.grad)
        for i in range(len(convs)):
            res[f'dw{i}'], res[f'db{i}'] = tw[i].grad, tb[i].grad
        return res

    got = run(K_, torch.float32, DEV)
    ref = run(R, torch.float64, ref_dev(n))
    for k, v in ref.items():
        # fp32 MFMA accumulation over <= 5*64 (fwd) / n*T*V (wgrad, statistics) terms: 2e-5 relative L2
        assert rel(got[k].detach().cpu(), v.detach()) < 2e-5, (k, rel(got[k].detach().cpu(), v.detach()))


CFG6 = ((3, 1), (3, 2), (3, 3), (3, 4), ('max', 3), '1x1')       # msmlp / mstcn / dgmstcn's default branches


# the edges of k_dwcausal_*: T odd with stride 2, (KM-1)*dil >= T (every tap but the last reads the zero padding), channels
# with dil = 0 (msmlp's max-pool / pass-through windows; set by zero_dil for unitmlp) next to active ones, V = 17 / 18, n = 1
@pytest.mark.parametrize('n,C,T,V,stride,cfg,merge_after', [
    (2, 24, 9, 25, 2, CFG6, True), (2, 24, 9, 25, 2, CFG6, False), (1, 12, 4, 17, 1, CFG6, True),
    (2, 18, 7, 18, 2, CFG6, False), (2, 16, 12, 25, 1, ((5, 1), (5, 2), ('max', 3), '1x1'), True)])
def test_temporal_mlp_bn(n, C, T, V, stride, cfg, merge_after):
    check_temporal_mlp_bn(n, C, T, V, stride, cfg, merge_after)


def check_temporal_mlp_bn(n, C, T, V, stride, cfg, merge_after, want_bn=True):
    """msmlp's stage (kernels.temporal_mlp_bn) as the unit builds its operands: BN+ReLU, the alpha-scaled dilated convs /
    max-pool / strided copy, the depthwise causal taps (zero outside the mlp windows), the windows' 1x1 convs as one
    block-diagonal mix (zero blocks for the other windows with merge_after, identity blocks without), the closing
    BatchNorm statistics — outputs, statistics and every input / parameter gradient.  want_bn False: the eval-mode call
    (no statistics, torch.no_grad(), inputs without history) and its output alone."""
    cfg = [tuple(c) if isinstance(c, (tuple, list)) else c for c in cfg]
    g = torch.Generator().manual_seed(C * 5 + T + stride)
    widths = _ms_widths(C, cfg)
    n_act = sum(w for w, c in zip(widths, cfg) if c != '1x1')
    mlp = [(w, c) for w, c in zip(widths, cfg) if c != '1x1' and c[0] != 'max']
    assert [c for _, c in mlp] == cfg[:len(mlp)]                  # the mlp windows come first (block-diagonal mix)
    kms = {(c[0] + 1) // 2 for _, c in mlp}
    assert len(kms) == 1
    KM = kms.pop()
    nm = sum(w for w, _ in mlp)
    dil = torch.tensor(sum(([c[1]] * w for w, c in mlp), []) + [0] * (C - nm), dtype=torch.int32)
    z = _rand(g, n, C, T, V)
    scale = torch.cat([torch.rand(n_act, generator=g) + 0.5, torch.ones(C - n_act)])
    shift = torch.cat([_rand(g, n_act, scale=0.3), torch.zeros(C - n_act)])
    cw = [_rand(g, w, w, c[0], 1, scale=(c[0] * w) ** -0.5) for w, c in mlp]
    cb = [_rand(g, w, scale=0.1) for w, _ in mlp]
    dw_w = torch.cat([_rand(g, nm, KM, scale=0.5), torch.zeros(C - nm, KM)])
    dw_b = torch.cat([_rand(g, nm, scale=0.1), torch.zeros(C - nm)])
    rest = torch.zeros(C - nm, C - nm) if merge_after else torch.eye(C - nm)
    pw_w = torch.block_diag(*[_rand(g, w, w, scale=w ** -0.5) for w, _ in mlp], rest)
    pw_b = torch.cat([_rand(g, nm, scale=0.1), torch.zeros(C - nm)])
    gamma = torch.rand(C, generator=g) + 0.5
    beta = _rand(g, C, scale=0.2)
    Tout = (T + stride - 1) // stride
    go, gsc, gsh = _rand(g, n, C, Tout, V), _rand(g, C), _rand(g, C)

    def run(mod, dt, dev):
        def mk(t):
            return t.to(dev, dt).requires_grad_(want_bn)
        tz, tsc, tsh, tga, tbe = mk(z), mk(scale), mk(shift), mk(gamma), mk(beta)
        tw, tb = [mk(w) for w in cw], [mk(b) for b in cb]
        tdw, tdb, tpw, tpb = mk(dw_w), mk(dw_b), mk(pw_w), mk(pw_b)
        if not want_bn:
            with torch.no_grad():
                return dict(o=mod.temporal_mlp_bn(tz, tsc, tsh, n_act, cfg, widths, tw, tb, tdw, tdb, dil.to(dev), tpw,
                                                  tpb, merge_after, stride)[0])
        o, sc, sh, mean, var = mod.temporal_mlp_bn(tz, tsc, tsh, n_act, cfg, widths, tw, tb, tdw, tdb, dil.to(dev), tpw,
                                                   tpb, merge_after, stride, tga, tbe, 1e-5, True)
        ((o * go.to(dev, dt)).sum() + (sc * gsc.to(dev, dt)).sum() + (sh * gsh.to(dev, dt)).sum()).backward()
        res = dict(o=o, sc=sc, sh=sh, mean=mean, var=var, dz=tz.grad, dscale=tsc.grad, dshift=tsh.grad,
                   ddw_w=tdw.grad, ddw_b=tdb.grad, dpw_w=tpw.grad, dpw_b=tpb.grad, dgamma=tga.grad, dbeta=tbe.grad)
        for i in range(len(mlp)):
            res[f'dw{i}'], res[f'db{i}'] = tw[i].grad, tb[i].grad
        return res

    got = run(K_, torch.float32, DEV)
    ref = run(R, torch.float64, ref_dev(n))
    for k, v in ref.items():
        # fp32 accumulation over <= 3*C (fwd) / n*T*V (weight gradients, statistics) terms: 2e-5 relative L2
        assert rel(got[k].detach().cpu(), v.detach()) < 2e-5, (k, rel(got[k].detach().cpu(), v.detach()))


@pytest.mark.parametrize('n,C,T,V,stride,ks,dil,add_tcn,merge_after,zero_dil', [
    (2, 16, 9, 25, 2, 9, 1, True, True, False), (2, 16, 9, 25, 2, 9, 1, True, False, True),
    (1, 8, 6, 17, 1, 9, 2, False, False, False), (2, 12, 7, 18, 2, 5, 4, False, True, True),
    (1, 24, 13, 18, 1, 5, 2, True, True, True), (2, 20, 11, 17, 1, 3, 2, True, False, False)])
def test_temporal_unitmlp_bn(n, C, T, V, stride, ks, dil, add_tcn, merge_after, zero_dil):
    check_temporal_unitmlp_bn(n, C, T, V, stride, ks, dil, add_tcn, merge_after, zero_dil)


def check_temporal_unitmlp_bn(n, C, T, V, stride, ks, dil, add_tcn, merge_after, zero_dil=False, want_bn=True):
    """unitmlp as a whole temporal unit (kernels.temporal_unitmlp_bn): the (ks+1)/2 depthwise causal taps at dilation dil,
    the alpha-scaled dense (ks,1) conv (add_tcn), the 1x1 conv after (merge_after) or before the add, the BatchNorm
    statistics.  zero_dil: every third channel gets dil = 0 (no taps: zero output, zero gradients).  want_bn False: the
    eval-mode call (no statistics, torch.no_grad(), inputs without history) and its output alone."""
    g = torch.Generator().manual_seed(C * 3 + T + ks + stride)
    KM = (ks + 1) // 2
    h = _rand(g, n, C, T, V)
    dw_w, dw_b = _rand(g, C, KM, scale=0.5), _rand(g, C, scale=0.1)
    dils = torch.tensor([0 if zero_dil and c % 3 == 1 else dil for c in range(C)], dtype=torch.int32)
    tw = _rand(g, C, C, ks, 1, scale=(ks * C) ** -0.5) if add_tcn else None
    tb = _rand(g, C, scale=0.1) if add_tcn else None
    pw_w, pw_b = _rand(g, C, C, scale=C ** -0.5), _rand(g, C, scale=0.1)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = _rand(g, C, scale=0.2)
    Tout = (T + stride - 1) // stride
    go, gsc, gsh = _rand(g, n, C, Tout, V), _rand(g, C), _rand(g, C)

    def run(mod, dt, dev):
        def mk(t):
            return None if t is None else t.to(dev, dt).requires_grad_(want_bn)
        th, tdw, tdb, ttw, ttb, tpw, tpb, tga, tbe = [mk(t) for t in (h, dw_w, dw_b, tw, tb, pw_w, pw_b, gamma, beta)]
        if not want_bn:
            with torch.no_grad():
                return dict(o=mod.temporal_unitmlp_bn(th, tdw, tdb, dils.to(dev), ttw, ttb, dil, tpw, tpb, merge_after,
                                                      stride)[0])
        o, sc, sh, mean, var = mod.temporal_unitmlp_bn(th, tdw, tdb, dils.to(dev), ttw, ttb, dil, tpw, tpb, merge_after,
                                                       stride, tga, tbe, 1e-5, True)
        ((o * go.to(dev, dt)).sum() + (sc * gsc.to(dev, dt)).sum() + (sh * gsh.to(dev, dt)).sum()).backward()
        res = dict(o=o, sc=sc, sh=sh, mean=mean, var=var, dh=th.grad, ddw_w=tdw.grad, ddw_b=tdb.grad, dpw_w=tpw.grad,
                   dpw_b=tpb.grad, dgamma=tga.grad, dbeta=tbe.grad)
        if add_tcn:
            res.update(dtw=ttw.grad, dtb=ttb.grad)
        return res

    got = run(K_, torch.float32, DEV)
    ref = run(R, torch.float64, ref_dev(n))
    for k, v in ref.items():
        # fp32 accumulation over <= ks*C (fwd) / n*T*V (weight gradients, statistics) terms: 2e-5 relative L2
        assert rel(got[k].detach().cpu(), v.detach()) < 2e-5, (k, rel(got[k].detach().cpu(), v.detach()))
    if zero_dil and want_bn:
        off = (dils == 0).nonzero().view(-1)
        assert not got['ddw_w'][off].any() and not got['ddw_b'][off].any()


def check_typed_kb(case, flags):
    """n = 128, V = 25: Ahat, the input gradient (of the time mean) and every parameter gradient of dghgcn's adjacency path
    (K-C projections + typed select + K-C edge linear + typed K-B, kernels.dynadj_typed) against the fp64 restatement
    (tests/dghgcn_fp64.py).  case = (Ci, Co, ratio): mid = ratio * Co channels per subset."""
    import dghgcn_fp64 as F64
    ci, co, ratio = case
    na, ea, at = {'node_edge': (True, True, False), 'plain': (False, False, False), 'node': (True, False, False),
                  'edge': (False, True, False), 'add_type': (True, True, True)}[flags]
    g = dsgcn_amd.Graph(layout='nturgb+d', mode='spatial')
    torch.manual_seed(7)
    np.random.seed(7)
    A = torch.tensor(np.asarray(dsgcn_amd.Graph(layout='nturgb+d', mode='random', num_filter=3, init_off=.04,
                                                init_std=.02).A), dtype=torch.float32)
    m = dsgcn_amd.dghgcn(ci, co, A, torch.tensor(g.edge_type), torch.tensor(g.node_type), ratio=ratio, node_attention=na,
                         edge_attention=ea, add_type=at, subset_wise=True)
    with torch.no_grad():
        m.alpha.normal_(0, 0.5)
        m.beta.normal_(0, 0.5)
    m = m.cuda()
    n, V = 128, 25
    gen = torch.Generator().manual_seed(11)
    xbar = torch.randn(n, ci, V, generator=gen).cuda().requires_grad_()
    dah = torch.randn(n, 3 * m.mid_channels, V, V, generator=gen).cuda()
    ahat = m.adjacency(xbar)
    (ahat * dah).sum().backward()
    names = ['A', 'alpha', 'beta', 'conv1.weight', 'conv1.bias', 'conv2.weight', 'conv2.bias'] + (
        ['edge_linears.weight', 'edge_linears.bias'] if ea else [])
    params = dict(m.named_parameters())
    p64 = {k: params[k].detach().double().requires_grad_() for k in names}
    x64 = xbar.detach().double().requires_grad_()
    want = F64.adjacency(x64, p64['A'], p64['alpha'], p64['beta'], p64['conv1.weight'], p64['conv1.bias'],
                         p64['conv2.weight'], p64['conv2.bias'], p64.get('edge_linears.weight'),
                         p64.get('edge_linears.bias'), m.node_type_idx, m.edge_type_idx, m.num_types if na else 1, at, True)
    (want * dah.double()).sum().backward()
    assert rel(ahat.detach().cpu(), want.detach().cpu()) < 1e-5, rel(ahat.detach().cpu(), want.detach().cpu())
    assert rel(xbar.grad.cpu(), x64.grad.cpu()) < 1e-4, rel(xbar.grad.cpu(), x64.grad.cpu())
    for k in names:
        e = rel(params[k].grad.cpu(), p64[k].grad.cpu())
        assert e < 1e-4, (k, e)


@pytest.mark.parametrize('n,Ci,Co,T,V,stride,ks,dil,bn', [
    (2, 64, 64, 32, 25, 1, 9, 1, True), (2, 64, 64, 32, 25, 2, 9, 1, True), (2, 128, 128, 16, 25, 1, 9, 1, True),
    (1, 256, 256, 8, 25, 1, 9, 1, True), (2, 40, 72, 21, 17, 2, 9, 1, False), (2, 16, 16, 12, 18, 1, 3, 2, True),
    (2, 70, 130, 10, 25, 1, 5, 2, True)])
def test_tconv_dense(n, Ci, Co, T, V, stride, ks, dil, bn):
    check_tconv_dense(n, Ci, Co, T, V, stride, ks, dil, bn)


def check_tconv_dense(n, Ci, Co, T, V, stride, ks, dil, bn, grad=True):
    """unit_tcn's dense (k,1) temporal conv (ST-GCN: k=9) + the statistics of the BatchNorm that follows.  grad False:
    the eval-mode call (torch.no_grad(), inputs without history, bn False) and its output alone."""
    assert grad or not bn
    g = torch.Generator().manual_seed(Ci + Co + T)
    h = _rand(g, n, Ci, T, V)
    w = _rand(g, Co, Ci, ks, 1, scale=(ks * Ci) ** -0.5)
    b = _rand(g, Co, scale=0.1)
    gamma = torch.rand(Co, generator=g) + 0.5
    beta = _rand(g, Co, scale=0.2)
    Tout = (T + stride - 1) // stride
    gz, gsc, gsh = _rand(g, n, Co, Tout, V), _rand(g, Co), _rand(g, Co)

    def run(mod, dt, dev):
        def mk(t):
            return t.to(dev, dt).requires_grad_(grad)
        th, tw, tb, tga, tbe = mk(h), mk(w), mk(b), mk(gamma), mk(beta)
        if not grad:
            with torch.no_grad():
                return dict(z=mod.tconv(th, tw, tb, stride, dil)[0])
        zz, sc, sh, mean, var = mod.tconv(th, tw, tb, stride, dil, tga if bn else None, tbe if bn else None, 1e-5, bn)
        loss = (zz * gz.to(dev, dt)).sum()
        if bn:
            loss = loss + (sc * gsc.to(dev, dt)).sum() + (sh * gsh.to(dev, dt)).sum()
        loss.backward()
        res = dict(z=zz, dh=th.grad, dw=tw.grad, db=tb.grad)
        if bn:
            res.update(sc=sc, sh=sh, mean=mean, var=var, dgamma=tga.grad, dbeta=tbe.grad)
        return res

    got = run(K_, torch.float32, DEV)
    ref = run(R, torch.float64, ref_dev(n))
    for k, v in ref.items():
        # fp32 MFMA accumulation over <= 9*256 (fwd) / n*T*V (wgrad) terms: 2e-5 relative L2
        assert rel(got[k].detach().cpu(), v.detach()) < 2e-5, (k, rel(got[k].detach().cpu(), v.detach()))


def test_tmean():
    check_tmean(4, 3, 20, 25, True)


def check_tmean(n, C, T, V, ld):
    """ld: True (rows of V joints) or an int >= V (rows zero-padded to ld, the layout dynadj reads)."""
    x = torch.randn(n, C, T, V, generator=torch.Generator().manual_seed(n + T))
    got = K_.tmean(x.cuda(), ld)
    want = x.to(ref_dev(n), torch.float64).mean(2)
    if ld is not True:
        assert got.shape == (n, C, ld) and not got[..., V:].any()
        got = got[..., :V]
    assert rel(got.cpu(), want) < 1e-6


@pytest.mark.parametrize('R,C', [(32768, 25), (1664, 192), (128, 48), (7, 3), (4096, 70000 // 64)])
def test_colsum(R, C):
    """Column sums incl. the folded two-stage path for tall, narrow inputs (fp64 accumulation: 1e-6 relative)."""
    t = torch.randn(R, C)
    assert rel(K_.colsum(t.cuda()).cpu(), t.double().sum(0)) < 1e-6


@pytest.mark.parametrize('Ra,Ca,Rb,Cb', [(128, 4160, 100, 64), (512, 4160, 1600, 64), (1600, 300, 64, 4160), (4096, 96, 2048, 64),
                                         (7, 3, 5, 2)])
def test_colsum_pair(Ra, Ca, Rb, Cb):
    """Two column sums sharing their launches: both short, only one tall (its first stage rides with the other's whole
    reduction), both tall; the second one with its (C, 3) columns split into three contiguous vectors."""
    ta, tb = torch.randn(Ra, Ca), torch.randn(Rb, Cb, 3)
    a, b = K_.colsum_pair(ta.cuda(), tb.cuda(), split_last_b=True)
    assert rel(a.cpu(), ta.double().sum(0)) < 1e-6
    assert rel(b.cpu(), tb.double().sum(0).t()) < 1e-6
    a2, b2 = K_.colsum_pair(ta.cuda(), tb.cuda())
    assert rel(b2.cpu(), tb.double().sum(0)) < 1e-6 and rel(a2.cpu(), ta.double().sum(0)) < 1e-6


@pytest.mark.parametrize('tag,layout,ci,co', [('v25', 'nturgb+d', 64, 64), ('v17', 'coco', 64, 128)])
def test_dgphgcn1_kernels_vs_reference_intermediates(tag, layout, ci, co):
    """K-B and K-A against the intermediates the REFERENCE computed inside dgphgcn1.forward (captured from its own
    einsum / conv calls, tests/golden/unit_intermediates.npz): the time mean, the dynamic adjacency Ahat, the aggregate
    Y = P x Ahat, and the unit output."""
    import dsgcn_amd as D
    from test_oracle_golden import load, sd_of
    z = load('unit_intermediates.npz')
    A = torch.from_numpy(z[f'{tag}_sd_A'])
    m = D.dgphgcn1(ci, co, A, torch.from_numpy(z[f'{tag}_edge_type']).float(), torch.from_numpy(z[f'{tag}_node_type']),
                   ratio=0.125, decompose=True, node_attention=True, edge_attention=True, subset_wise=True, ctr='T',
                   ada='T')
    m.load_state_dict(sd_of({k[len(tag) + 1:]: v for k, v in z.items() if k.startswith(tag + '_')}, 'sd_', torch.float32))
    m = m.cuda().train()
    x = torch.from_numpy(z[f'{tag}_x']).cuda()
    xbar = K.tmean(x)
    assert rel(xbar.cpu(), z[f'{tag}_xbar']) < 1e-6
    with torch.no_grad():
        ahat = m.adjacency(xbar)                                  # (n, K*mid, V, V)
    want = torch.from_numpy(z[f'{tag}_Ahat'])
    assert rel(ahat.cpu().reshape(want.shape), want) < 3e-6       # tanh / exp in fp32
    P = torch.from_numpy(z[f'{tag}_P']).cuda()                    # (n, K, mid, T, V): after pre's BN + ReLU
    n, Kk, mid, T, V = P.shape
    y = K.aggregate(P.reshape(n, Kk * mid, T, V), None, False, want.cuda().reshape(n, Kk * mid, V, V))
    assert rel(y.cpu().reshape(z[f'{tag}_Y'].shape), z[f'{tag}_Y']) < 2e-6
    with torch.no_grad():
        out = m(x)
    assert rel(out.cpu(), z[f'{tag}_out']) < 1e-5


def test_dggcn_wide_vs_oracle():
    """dggcn at its class-default ratio on the last stage (128 -> 256: mid = 64, above the fixtures' 16 / 32) against the
    oracle's fp64 evaluation of the same state_dict."""
    import dsgcn_amd as D
    from oracle import dsgcn_oracle as O
    torch.manual_seed(7)
    A = torch.randn(3, 25, 25) * 0.02 + 0.04
    m = D.dggcn(128, 256, A, ratio=0.25)
    with torch.no_grad():
        m.alpha.normal_(0, .5)
        m.beta.normal_(0, .5)
    sd = {k: v.detach().double() for k, v in m.state_dict().items()}
    x = torch.randn(3, 128, 8, 25)
    g = torch.randn(3, 256, 8, 25)
    xo = x.double().requires_grad_()
    yo = O.dggcn_forward(xo, sd)
    (yo * g.double()).sum().backward()
    m = m.cuda().train()
    xg = x.cuda().requires_grad_()
    y = m(xg)
    (y * g.cuda()).sum().backward()
    assert rel(y.detach().cpu(), yo.detach()) < 1e-5
    assert rel(xg.grad.cpu(), xo.grad) < 5e-5


@pytest.mark.parametrize('i', [0, 1])
def test_unit_aagcn_vs_reference_fixture(i):
    """The 2s-AGCN / AAGCN unit (gcn.py:349-460) with the HIP channel mixes (embedding convs and conv_d as one K-C launch
    each, BN + down + ReLU fused) against the REFERENCE's fp64 output, input gradient and parameter gradients
    (tests/golden/unit_aagcn.npz); the module takes the reference's state_dict as is."""
    import dsgcn_amd as D
    from test_oracle_golden import load, sd_of, AAGCN_GRADS
    z = load('unit_aagcn.npz')
    tag = f'u{i}_'
    sd = sd_of(z, tag + 'sd_', torch.float32)
    Co, Ci = sd['conv_d.0.weight'].shape[:2]
    m = D.unit_aagcn(Ci, Co, sd['A'].clone())
    m.load_state_dict(sd)
    m = m.cuda().train()
    x = torch.from_numpy(z[tag + 'x']).cuda().requires_grad_()
    y = m(x)
    (y * torch.from_numpy(z[tag + 'R']).cuda()).sum().backward()
    assert rel(y.detach().cpu(), z[tag + 'y']) < 1e-5
    assert rel(x.grad.cpu(), z[tag + 'dx']) < 5e-5
    params = dict(m.named_parameters())
    for k in AAGCN_GRADS:
        assert rel(params[k].grad.cpu(), z[tag + 'grad_' + k]) < 1e-4, (k, rel(params[k].grad.cpu(), z[tag + 'grad_' + k]))


@pytest.mark.parametrize('i', [0, 1])
def test_dggcn_unit_vs_reference_fixture(i):
    """The original DG-STGCN unit `dggcn` (gcn.py:1445-1584) on the HIP path — two K-B launches with the typed slots made
    plain, K-A, K-C — against the REFERENCE's fp64 output, input gradient and parameter gradients
    (tests/golden/unit_dggcn.npz); the module takes the reference's state_dict as is."""
    import dsgcn_amd as D
    from test_oracle_golden import load, sd_of
    z = load('unit_dggcn.npz')
    tag = f'u{i}_'
    sd = sd_of(z, tag + 'sd_', torch.float32)
    Co, Ci = sd['post.weight'].shape[0], sd['pre.0.weight'].shape[1]
    m = D.dggcn(Ci, Co, sd['A'].clone(), ratio=0.25, subset_wise=bool(z[tag + 'subset_wise']))
    m.load_state_dict(sd)                       # strict: same keys and shapes as the reference module
    m = m.cuda().train()
    x = torch.from_numpy(z[tag + 'x']).cuda().requires_grad_()
    y = m(x)
    (y * torch.from_numpy(z[tag + 'R']).cuda()).sum().backward()
    assert rel(y.detach().cpu(), z[tag + 'y']) < 1e-5
    assert rel(x.grad.cpu(), z[tag + 'dx']) < 5e-5
    params = dict(m.named_parameters())
    for k in ('A', 'alpha', 'beta', 'conv1.weight', 'conv2.bias', 'pre.1.weight', 'post.weight'):
        want = z[tag + 'grad_' + k]
        if np.abs(want).max() < 1e-12:           # alpha[1:], beta[1:] are unused without subset_wise
            assert params[k].grad is None or float(params[k].grad.abs().max()) < 1e-6, k
        else:
            assert rel(params[k].grad.cpu(), want) < 1e-4, (k, rel(params[k].grad.cpu(), want))


@pytest.mark.parametrize('tag', ['gcn', 'gcn_res', 'tcn9', 'tcn1s2', 'ctrgcn', 'MSTCN', 'MSTCNs2', 'gcn_offset_post',
                                 'gcn_importance', 'gcn_fixed_post', 'ctrhgcn', 'ctrhgcn_same', 'msmlp', 'msmlp_s2',
                                 'unitmlp9', 'unitmlp9_s2'])
def test_units_vs_reference_fixture(tag):
    """unit_gcn, unit_tcn (k=9 dense; k=1 stride 2), unit_ctrgcn / CTRGC and MSTCN at real widths on the HIP path
    against the REFERENCE's output, input gradient, parameter gradients and running statistics (fp64 run;
    tests/golden/unit_others.npz).  The seeded weights are rebuilt here and their digest compared with the fixture's."""
    import sys
    import dsgcn_amd as D
    from test_oracle_golden import GOLD, load
    from oracle import dsgcn_oracle as O
    sys.path.insert(0, GOLD)
    from closed_form import make_unit, sd_digest
    z = load('unit_others.npz')
    A = torch.tensor(O.graph_A('nturgb+d', 'spatial'), dtype=torch.float32)
    gc = O.graph_constants('nturgb+d')
    m, x, Rm = make_unit(D, tag, A, np.asarray(gc['edge_type']), np.asarray(gc['node_type']))
    assert sd_digest(m) == str(z[f'{tag}_digest'])
    m = m.cuda().train()
    x = x.cuda().requires_grad_()
    y = m(x)
    (y * Rm.cuda()).sum().backward()
    assert rel(y.detach().cpu(), z[f'{tag}_y']) < 1e-5
    assert rel(x.grad.cpu(), z[f'{tag}_dx']) < 5e-5
    gmax = max(float(np.abs(z[k]).max()) for k in z if k.startswith(f'{tag}_grad_'))
    for k, p in m.named_parameters():
        if f'{tag}_grad_{k}' in z:
            want = z[f'{tag}_grad_{k}']
            if np.abs(want).max() < 1e-9:      # analytically zero (a conv bias feeding BatchNorm): fp32 cancellation noise
                assert p.grad is None or float(p.grad.abs().max()) < 2e-4 * gmax, k
            else:
                assert rel(p.grad.cpu(), want) < 1e-4, (k, rel(p.grad.cpu(), want))
        elif f'{tag}_gnorm_{k}' in z:
            assert abs(float(p.grad.double().norm()) - float(z[f'{tag}_gnorm_{k}'])) < 1e-4 * float(z[f'{tag}_gnorm_{k}']), k
    for k, v in m.state_dict().items():
        if 'running' in k:
            assert rel(v.cpu(), z[f'{tag}_{k}']) < 1e-5, k


def _check_param_grads(m, z, tag, bar=1e-4):
    """Every parameter gradient the fixture stores (full tensors, or norms for the large ones) against the module's."""
    gmax = max([float(np.abs(z[k]).max()) for k in z if k.startswith(f'{tag}grad_')] + [1e-30])
    seen = 0
    for k, p in m.named_parameters():
        if f'{tag}grad_{k}' in z:
            want = z[f'{tag}grad_{k}']
            seen += 1
            if np.abs(want).max() < 1e-9 * max(gmax, 1.0):     # analytically zero (a conv bias feeding BatchNorm): fp32 noise
                assert p.grad is None or float(p.grad.abs().max()) < 2e-4 * gmax, k
            else:
                assert p.grad is not None, k
                assert rel(p.grad.cpu(), want) < bar, (k, rel(p.grad.cpu(), want))
        elif f'{tag}gnorm_{k}' in z:
            seen += 1
            want = float(z[f'{tag}gnorm_{k}'])
            assert abs(float(p.grad.double().norm()) - want) < bar * want, k
    return seen


@pytest.mark.parametrize('i', [0, 1, 2])
def test_dgphgcn1_unit_vs_reference_fixture(i):
    """The DS-GCN spatial unit (gcn.py:2074-2372) on the HIP path — K-B, K-A, K-C — against the REFERENCE's fp64 output,
    input gradient and stored parameter gradients (tests/golden/unit_dgphgcn1.npz: 3->64 with `down`, 64->64, 64->128);
    the module takes the reference's state_dict as is."""
    import dsgcn_amd as D
    from oracle import dsgcn_oracle as O
    from test_oracle_golden import load, sd_of
    z = load('unit_dgphgcn1.npz')
    tag = f'u{i}_'
    sd = sd_of(z, tag + 'sd_', torch.float32)
    Co, Ci = sd['post.weight'].shape[0], sd['pre.0.weight'].shape[1]
    gc = O.graph_constants('nturgb+d')
    m = D.dgphgcn1(Ci, Co, sd['A'].clone(), torch.as_tensor(gc['edge_type']).float(), torch.as_tensor(gc['node_type']),
                   ratio=0.125, decompose=True, node_attention=True, edge_attention=True, subset_wise=True, ctr='T', ada='T')
    m.load_state_dict(sd)                       # strict: same keys and shapes as the reference module
    m = m.cuda().train()
    x = torch.from_numpy(z[tag + 'x']).cuda().requires_grad_()
    y = m(x)
    (y * torch.from_numpy(z[tag + 'R']).cuda()).sum().backward()
    assert rel(y.detach().cpu(), z[tag + 'y']) < 1e-5
    assert rel(x.grad.cpu(), z[tag + 'dx']) < 5e-5
    assert _check_param_grads(m, z, tag) == 6


@pytest.mark.parametrize('i,stride', [(0, 1), (1, 2)])
def test_dgmstcn_unit_vs_reference_fixture(i, stride):
    """The DS-GCN temporal unit (tcn.py:344-431) on the HIP path — K-C with the global-joint column, K-D, K-C — against the
    REFERENCE's fp64 output, input gradient and add_coeff gradient (tests/golden/unit_dgmstcn.npz: 64 / stride 1, 96 /
    stride 2)."""
    import dsgcn_amd as D
    from test_oracle_golden import load, sd_of
    z = load('unit_dgmstcn.npz')
    tag = f't{i}_'
    sd = sd_of(z, tag + 'sd_', torch.float32)
    C = sd['transform.2.weight'].shape[0]
    m = D.dgmstcn(C, C, stride=stride)
    m.load_state_dict(sd)
    m = m.cuda().train()
    x = torch.from_numpy(z[tag + 'x']).cuda().requires_grad_()
    y = m(x)
    (y * torch.from_numpy(z[tag + 'R']).cuda()).sum().backward()
    assert rel(y.detach().cpu(), z[tag + 'y']) < 1e-5
    assert rel(x.grad.cpu(), z[tag + 'dx']) < 5e-5
    assert rel(m.add_coeff.grad.cpu(), z[tag + 'grad_add_coeff']) < 1e-4


def _ds_unit_cases():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    from closed_form import DS_UNIT_CASES
    return list(DS_UNIT_CASES)


@pytest.mark.parametrize('tag', _ds_unit_cases())
def test_ds_units_all_widths_vs_reference_fixture(tag):
    """dgphgcn1 and dgmstcn at EVERY width DS-STGCN uses (3->64 ... 256->256, stride 1 / 2, NTU and coco graphs) on the HIP
    path against the REFERENCE's fp64 run (tests/golden/unit_ds_r3.npz): output 1e-5, input gradient 5e-5, EVERY
    parameter gradient 1e-4 (norms for tensors > 16384 elements), BatchNorm running statistics 1e-5.  The seeded weights
    are rebuilt here and their digest compared with the fixture's."""
    import dsgcn_amd as D
    from closed_form import make_ds_unit, sd_digest
    from test_oracle_golden import load
    z = load('unit_ds_r3.npz')
    m, x, Rm = make_ds_unit(D, D.Graph, tag)
    assert sd_digest(m) == str(z[f'{tag}_digest'])
    m = m.cuda().train()
    x = x.cuda().requires_grad_()
    y = m(x)
    (y * Rm.cuda()).sum().backward()
    assert rel(y.detach().cpu(), z[f'{tag}_y']) < 1e-5
    assert rel(x.grad.cpu(), z[f'{tag}_dx']) < 5e-5
    assert _check_param_grads(m, z, f'{tag}_') >= 17
    for k, v in m.state_dict().items():
        if 'running' in k:
            assert rel(v.cpu(), z[f'{tag}_{k}']) < 1e-5, k


@pytest.mark.parametrize('n,C,T,V', [(3, 16, 64, 25), (2, 64, 16, 25), (2, 8, 100, 17), (1, 5, 7, 18)])
def test_aagcn_gram_gates_and_per_sample_aggregate(n, C, T, V):
    """The AAGCN pieces on the HIP path (gcn.py:431-437, 447-459): the embedding Gram (K-A''s backward product + ordered
    channel sum), K-A' with one topology per sample shared by the channels, and the three gate passes with the next gate's
    mean in the same launch — values and gradients against the fp64 statement of each op."""
    check_gram(n, C, T, V)
    check_aggregate_sum_per_sample(n, 3, max(C // 2, 1), T, V)
    for mode in range(3):
        for rmode in ((1, 2, 0)[mode], 0):
            check_gate(n, C, T, V, mode, rmode)


def check_gram(n, C, T, V):
    """G = sum_{c,t} a[., c, t, u] b[., c, t, w] and its two gradients (AAGCN's embeddings; CTRHGC's one-frame planes)."""
    g = torch.Generator().manual_seed(n + C + T)
    a, b = _rand(g, n, C, T, V), _rand(g, n, C, T, V)
    dG = _rand(g, n, V, V)

    def run(mod, dt, dev):
        ta, tb = a.to(dev, dt).requires_grad_(), b.to(dev, dt).requires_grad_()
        G = mod.gram(ta, tb)
        (G * dG.to(dev, dt)).sum().backward()
        return dict(G=G, da=ta.grad, db=tb.grad)

    got = run(K, torch.float32, DEV)
    ref = run(R, torch.float64, ref_dev(n))
    for k, v in ref.items():
        # fp32 sums over <= C*T (Gram) / V (its gradients) terms: 2e-5 relative L2
        assert rel(got[k].detach().cpu(), v.detach()) < 2e-5, (k, rel(got[k].detach().cpu(), v.detach()))


def check_aggregate_sum_per_sample(n, S, Co, T, V):
    """K-A' with one (S, V, V) topology per sample shared by the channels (AAGCN), with the BatchNorm statistics."""
    g = torch.Generator().manual_seed(n + S * Co + T)
    p = _rand(g, n, S * Co, T, V)
    adj = _rand(g, n, S, V, V, scale=0.3)
    gam, bet = torch.rand(Co, generator=g) + 0.5, _rand(g, Co, scale=0.2)
    gy, gsc, gsh = _rand(g, n, Co, T, V), _rand(g, Co), _rand(g, Co)

    def run(mod, dt, dev):
        mk = lambda t: t.to(dev, dt).requires_grad_()            # noqa: E731
        tp, tadj, tg, tbt = mk(p), mk(adj), mk(gam), mk(bet)
        yy, sc, sh, mean, var = mod.aggregate_sum(tp, tadj, S, tg, tbt, 1e-5, True, per_sample=True)
        ((yy * gy.to(dev, dt)).sum() + (sc * gsc.to(dev, dt)).sum() + (sh * gsh.to(dev, dt)).sum()).backward()
        return dict(y=yy, sc=sc, sh=sh, mean=mean, var=var, dp=tp.grad, dadj=tadj.grad, dgamma=tg.grad, dbeta=tbt.grad)

    got = run(K, torch.float32, DEV)
    ref = run(R, torch.float64, ref_dev(n))
    for k, v in ref.items():
        # fp32 sums over S*V (fwd) / Co*T (dadj) / n*T*V (statistics) terms: 2e-5 relative L2
        assert rel(got[k].detach().cpu(), v.detach()) < 2e-5, (k, rel(got[k].detach().cpu(), v.detach()))


def check_gate(n, C, T, V, mode, rmode):
    """out = y * (1 + g) with g per joint / frame / channel (mode 0 / 1 / 2) and the next gate's mean (rmode 1: over
    joints, 2: over the plane) from the same pass, with both gradients."""
    g = torch.Generator().manual_seed(n + C + T + 10 * mode + rmode)
    y = _rand(g, n, C, T, V)
    gt = torch.rand(n, (V, T, C)[mode], generator=g)
    gout = _rand(g, n, C, T, V)
    dr = _rand(g, *((n, C, T) if rmode == 1 else (n, C))) if rmode else None

    def run(mod, dt, dev):
        ty, tg = y.to(dev, dt).requires_grad_(), gt.to(dev, dt).requires_grad_()
        out, r = mod.gate(ty, tg, mode, rmode)
        loss = (out * gout.to(dev, dt)).sum()
        if rmode:
            loss = loss + (r * dr.to(dev, dt)).sum()
        loss.backward()
        res = dict(out=out, dy=ty.grad, dg=tg.grad)
        if rmode:
            res['r'] = r
        return res

    got = run(K, torch.float32, DEV)
    ref = run(R, torch.float64, ref_dev(n))
    for k, v in ref.items():
        e = rel(got[k].detach().cpu(), v.detach())
        # out, dy: a product per element (plus, for dy, the mean's gradient spread over its terms): a few fp32 roundings.
        # r, dg: fp32 sums over <= T*V / C*T*V terms: 2e-5 relative L2
        assert e < (1e-6 if k in ('out', 'dy') else 2e-5), (k, e)


def test_wsplit_images_batched_per_step_and_never_stale():
    """The bf16-term weight images of the wide convs are rebuilt by ONE launch at the first wide conv of a step
    (kernels._wsplit_image); an image is trusted only for the step and weight version it was built at.  Two convs, weights
    changed in place between forwards, with and without a step boundary: every output must match the current weights."""
    g = torch.Generator().manual_seed(3)
    x = _rand(g, 2, 128, 16, 25).to(DEV)
    ws = [(_rand(g, 256, 128, 1, 1, scale=128 ** -0.5).to(DEV).requires_grad_()), (_rand(g, 160, 128, 1, 1, scale=128 ** -0.5).to(DEV).requires_grad_())]
    K._wsplit_state['jobs'].clear()

    def check(tag):
        for w in ws:
            z = K.pwconv(x, None, None, None, False, w, None, 1, False)[0]
            want = torch.einsum('oc,nctv->notv', w.detach().double().view(w.shape[0], -1), x.double())
            assert rel(z, want) < 2e-6, (tag, rel(z, want))

    K.reset_leaf_uses()
    check('first visit: split on the spot')
    assert len(K._wsplit_state['jobs']) == 2
    with torch.no_grad():
        ws[0].mul_(1.5)
    check('same step, weight version moved: re-split on the spot')
    K.reset_leaf_uses()
    with torch.no_grad():
        ws[1].add_(0.25)
    check('new step: one batched launch')
    assert K._wsplit_state['batched'] == K._wsplit_state['epoch']
    stamps = [j['stamp'] for j in K._wsplit_state['jobs'].values()]
    assert all(s[0] == K._wsplit_state['epoch'] for s in stamps)
    with torch.no_grad():
        ws[0].add_(-0.5)
    check('after the batched launch, a later in-place change')
    # a write that moves NO version counter (what dsgcn_sgd_step does to the flat buffer): inside a step the image is
    # trusted (nothing writes weights there), after end_step() it never is
    K.end_step()
    for w in ws:
        w.data.mul_(0.75)
    assert all(j['stamp'][1] == j['w']._version for j in K._wsplit_state['jobs'].values())
    check('outside a step: raw-pointer weight update, split on the spot')
    K.reset_leaf_uses()
    check('next step after a raw-pointer update')
    # a backward through the saved image
    K.reset_leaf_uses()
    z = K.pwconv(x, None, None, None, False, ws[0], None, 1, False)[0]
    xg = x.clone().requires_grad_()
    z = K.pwconv(xg, None, None, None, False, ws[0], None, 1, False)[0]
    z.sum().backward()
    want = ws[0].detach().double().view(256, -1).sum(0).view(1, -1, 1, 1).expand_as(x)
    assert rel(xg.grad, want) < 2e-6


@pytest.mark.parametrize('N,M,C,K,lw,bias', [(64, 2, 256, 60, 1.0, True), (64, 2, 256, 120, 1.0, True),
                                             (32, 2, 256, 400, 0.5, True), (5, 1, 96, 3, 1.0, False),
                                             (7, 3, 70, 11, 2.0, True), (1, 2, 256, 60, 1.0, True)])
def test_head_loss(N, M, C, K, lw, bias):
    check_head_loss(N, M, C, K, lw, bias)


def check_head_loss(N, M, C, K, lw, bias):
    """Person mean + Linear + cross entropy + accuracies (csrc/head.hip) against torch in fp64: loss and gradients to 2e-6
    of their norm, the accuracies EXACT (a rank is an integer; ties are planted to pin the stable-argsort rule)."""
    g = torch.Generator().manual_seed(N * 31 + K)
    feat = torch.randn(N * M, C, generator=g)
    w = torch.randn(K, C, generator=g) * 0.2
    b = torch.randn(K, generator=g) * 0.1 if bias else None
    label = torch.randint(0, K, (N,), generator=g)
    gl = torch.tensor(0.7)

    def run(mod, dt, dev):
        f, ww = feat.to(dev, dt).requires_grad_(), w.to(dev, dt).requires_grad_()
        bb = b.to(dev, dt).requires_grad_() if bias else None
        loss, acc, score = mod.head_loss(f, ww, bb, label.to(dev), M, lw)
        loss.backward(gl.to(dev, dt))
        return dict(loss=loss, acc=acc, score=score, dfeat=f.grad, dw=ww.grad, **({'db': bb.grad} if bias else {}))

    got, ref = run(K_, torch.float32, DEV), run(R, torch.float64, 'cpu')
    assert got['loss'].dtype == torch.float32 and got['acc'].dtype == torch.float64 and got['loss'].dim() == 0
    for k in ref:
        if k == 'acc':
            assert torch.equal(got[k].cpu(), ref[k]), (got[k], ref[k])
        else:
            assert rel(got[k], ref[k]) < 2e-6, (k, rel(got[k], ref[k]))
    # twice the same launch: bit-identical (fixed-order sums)
    again = run(K_, torch.float32, DEV)
    assert all(torch.equal(got[k], again[k]) for k in got)


def test_head_loss_ties_and_bad_label():
    """Equal scores: the label counts as a hit when a stable ascending argsort leaves it among the last k — classes with
    an equal score and a GREATER index outrank it.  A label outside [0, K) gives a NaN loss (torch asserts on the device)."""
    K = 8
    w = torch.zeros(K, 4, device=DEV)
    b = torch.tensor([1., 1., 1., 1., 1., 1., 0., 0.], device=DEV)           # six classes tie at the top
    feat = torch.zeros(6, 4, device=DEV)
    label = torch.tensor([0, 1, 4, 5, 6, 7], device=DEV)
    _, acc, _ = K_.head_loss(feat, w, b, label, 1)
    # ranks: label 0 -> 5 (five equal scores with a greater index), 1 -> 4, 4 -> 1, 5 -> 0, 6 -> 7 (6 greater + index 7), 7 -> 6
    assert acc.tolist() == [1 / 6, 3 / 6]
    _, acc_ref, _ = R.head_loss(feat.cpu().double(), w.cpu().double(), b.cpu().double(), label.cpu(), 1)
    assert acc_ref.tolist() == acc.tolist()
    loss, acc, _ = K_.head_loss(feat, w, b, torch.tensor([0, 1, 4, 5, 6, 99], device=DEV), 1)
    assert torch.isnan(loss) and acc.tolist() == [1 / 6, 3 / 6]


def test_bn_running_update_matches_batch_norm():
    """One launch for the buffers of many BatchNorm layers == what F.batch_norm(training=True) does to each of them."""
    import torch.nn as nn
    g = torch.Generator().manual_seed(5)
    widths = [64] * 30 + [128] * 30 + [256] * 20 + [24, 7, 300]
    items, refs = [], []
    for i, C in enumerate(widths):
        bn = nn.BatchNorm2d(C, momentum=0.1 if i % 3 else 0.25).to(DEV)
        ref = nn.BatchNorm2d(C, momentum=bn.momentum).to(DEV)
        with torch.no_grad():
            bn.running_mean.copy_(torch.randn(C, generator=g)); bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
        ref.load_state_dict(bn.state_dict())
        x = torch.randn(4, C, 3, 5, generator=g).to(DEV)
        ref.train()(x)
        items.append((bn, x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False), float(4 * 3 * 5)))
        refs.append(ref)
    K_.bn_running_update(items)
    for (bn, _, _, _), ref in zip(items, refs):
        assert int(bn.num_batches_tracked) == 1 == int(ref.num_batches_tracked)
        assert maxabs(bn.running_mean, ref.running_mean) < 1e-6 and maxabs(bn.running_var, ref.running_var) < 2e-6


@pytest.mark.parametrize('n,C,T,V,mode,flags', [
    (3, 64, 64, 25, 'res_plain', 1), (2, 128, 32, 25, 'res_affine', 1), (2, 64, 64, 25, 'affine', 1),
    (2, 12, 25, 17, 'res_affine', 1), (1, 5, 7, 18, 'plain', 1), (2, 64, 32, 25, 'res_plain', 3),
    (2, 16, 9, 17, 'res_affine', 3), (2, 16, 8, 25, 'res_affine', 0),
    (128, 256, 25, 25, 'res_plain', 1)])                     # the bench step's last block
def test_fuse_out_pool(n, C, T, V, mode, flags):
    check_fuse_out_pool(n, C, T, V, mode, flags)


def check_fuse_out_pool(n, C, T, V, mode, flags):
    """The last block's output as plane means only (no activation written) against mean(fuse_out) in fp64, and — same
    launches, same order of operations — bit-identical to the mean the full kernel's output gives when summed the same way
    is NOT claimed: torch's mean runs in another order, so 2e-6 of the norm."""
    g = torch.Generator().manual_seed(C + T + flags)
    x1 = _rand(g, n, C, T, V)
    a1 = None if mode in ('plain', 'res_x1') else (torch.rand(C, generator=g) + 0.5, _rand(g, C, scale=0.3))
    x2 = _rand(g, n, C, T, V) if mode.startswith('res') else None
    a2 = (torch.rand(C, generator=g) + 0.5, _rand(g, C, scale=0.3)) if mode == 'res_affine' else None
    gp = _rand(g, n, C)
    if flags == 1:
        off_knife_edge(x1, a1, x2, a2, True)

    def run(mod, dt, dev):
        def mk(t):
            return None if t is None else t.to(dev, dt).requires_grad_()
        tx1, tx2 = mk(x1), mk(x2)
        ta1 = None if a1 is None else (mk(a1[0]), mk(a1[1]))
        ta2 = None if a2 is None else (mk(a2[0]), mk(a2[1]))
        pm = mod.fuse_out_pool(tx1, ta1, tx2, ta2, flags)
        (pm * gp.to(dev, dt)).sum().backward()
        res = dict(pm=pm, dx1=tx1.grad)
        if tx2 is not None:
            res['dx2'] = tx2.grad
        if ta1 is not None:
            res['ds1'], res['dh1'] = ta1[0].grad, ta1[1].grad
        if ta2 is not None:
            res['ds2'], res['dh2'] = ta2[0].grad, ta2[1].grad
        return res

    got = run(K, torch.float32, DEV)
    ref = run(R, torch.float64, ref_dev(n))
    assert got['pm'].shape == (n, C)
    for k, v in ref.items():
        assert rel(got[k], v) < (1e-5 if k[0] == 'd' and k[1] in 'sh' else 2e-6), (k, rel(got[k], v))
    # against the materialising kernel: the same gradients to rounding (the only difference is where the pooled
    # gradient is divided by T*V)
    tx1 = x1.to(DEV).requires_grad_()
    tx2 = None if x2 is None else x2.to(DEV).requires_grad_()
    ta1 = None if a1 is None else (a1[0].to(DEV), a1[1].to(DEV))
    ta2 = None if a2 is None else (a2[0].to(DEV), a2[1].to(DEV))
    out, _ = K.fuse_out(tx1, ta1, tx2, ta2, flags)
    (out.mean((2, 3)) * gp.to(DEV)).sum().backward()
    assert rel(got['dx1'], tx1.grad) < 1e-6


@pytest.mark.parametrize('n', [1, 3, 4, 1027, 1378101])
@pytest.mark.parametrize('mom,wd,nesterov', [(0.9, 5e-4, True), (0.9, 0.0, False), (0.0, 1e-3, False)])
def test_sgd_step_matches_torch(n, mom, wd, nesterov):
    """csrc/head.hip k_sgd == torch.optim.SGD, three steps with a changing rate (the reference's optimizer:
    configs/_init_/lr_schedual.py:11-15); elementwise fp32: 1e-6 absolute on O(1) values."""
    g = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) for _ in range(3)]
    ref = torch.nn.Parameter(p0.clone().to(DEV))
    topt = torch.optim.SGD([ref], lr=0.1, momentum=mom, weight_decay=wd, nesterov=nesterov)
    p = p0.clone().to(DEV)
    buf = torch.zeros_like(p) if mom else None
    lr_t = torch.zeros(1, device=DEV)
    from dsgcn_amd import native
    for it, gr in enumerate(grads):
        lr = 0.1 / (it + 1)
        topt.param_groups[0]['lr'] = lr
        ref.grad = gr.to(DEV)
        topt.step()
        lr_t.fill_(lr)
        gd = gr.to(DEV)
        rc = native.lib().dsgcn_sgd_step(p.data_ptr(), gd.data_ptr(), None if buf is None else buf.data_ptr(), lr_t.data_ptr(),
                                         mom, wd, int(nesterov), n, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    assert maxabs(p, ref) < 1e-6
    if mom:
        assert maxabs(buf, topt.state[ref]['momentum_buffer']) < 1e-6


@pytest.mark.parametrize('N,M,T,V,C,bn_type', [(4, 2, 64, 25, 3, 'VC'), (3, 2, 100, 17, 3, 'MVC'), (64, 2, 64, 25, 3, 'VC'),
                                               (5, 1, 7, 18, 2, 'MVC'), (2, 3, 30, 25, 9, 'VC')])
@pytest.mark.parametrize('affine', [True, False])
def test_data_bn(N, M, T, V, C, bn_type, affine):
    check_data_bn(N, M, T, V, C, bn_type, affine)


def check_data_bn(N, M, T, V, C, bn_type, affine):
    """The backbones' input BatchNorm1d (dgstgcn.py:158-164) in two launches, no permute copies: output, parameter
    gradients and the buffer updates against nn.BatchNorm1d in fp64 on the permuted clip; then eval mode on the buffers."""
    import torch.nn as nn
    g = torch.Generator().manual_seed(N * T + V)
    x = torch.randn(N, M, T, V, C, generator=g) * 2 + 0.5
    Ch = (M if bn_type == 'MVC' else 1) * V * C
    gy = torch.randn(N * M, C, T, V, generator=g)

    def make(dt, dev):
        bn = nn.BatchNorm1d(Ch, affine=affine).to(dev, dt)
        with torch.no_grad():
            bn.running_mean.copy_(torch.linspace(-1, 1, Ch)); bn.running_var.copy_(torch.linspace(0.5, 2, Ch))
            if affine:
                bn.weight.copy_(torch.linspace(0.5, 1.5, Ch)); bn.bias.copy_(torch.linspace(-0.3, 0.3, Ch))
        return bn

    def run(mod, dt, dev):
        bn = make(dt, dev).train()
        xx = x.to(dev, dt)
        assert mod.data_bn_eligible(xx, bn)
        y = mod.data_bn(xx, bn, bn_type)
        res = dict(y=y)
        if affine:
            (y * gy.to(dev, dt)).sum().backward()
            res.update(dgamma=bn.weight.grad, dbeta=bn.bias.grad)
        res.update(rm=bn.running_mean.clone(), rv=bn.running_var.clone(), nbt=bn.num_batches_tracked.clone())
        with torch.no_grad():
            res['y_eval'] = mod.data_bn(xx, bn.eval(), bn_type)
        return res

    got, ref = run(K_, torch.float32, DEV), run(R, torch.float64, 'cpu')
    assert got['y'].shape == (N * M, C, T, V) and int(got['nbt']) == 1 == int(ref['nbt'])
    for k in ('y', 'y_eval', 'rm', 'rv', 'dgamma', 'dbeta'):
        if k in ref:
            assert rel(got[k], ref[k]) < 3e-6, (k, rel(got[k], ref[k]))
    again = run(K_, torch.float32, DEV)
    assert all(torch.equal(got[k], again[k]) for k in got)
