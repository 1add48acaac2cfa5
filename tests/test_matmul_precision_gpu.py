"""-m gpu: matmul precision 'high' — every kernel that carries an fp32 product on bf16 terms against the fp64 EMULATION of
the three-product form (tests/matmul_precision_emul.py), the elementwise bound of csrc/common.h, and the level's semantics
(really reduced, reproducible, no leak into 'highest'); then the engines on DS-STGCN and ST-GCN against the fp64 oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dsgcn_amd as D
from dsgcn_amd import kernels as K
from dsgcn_amd import native
import torch_ops as R
from matmul_precision_emul import HIGH_BOUND, fma32, term_product
from test_kernels_gpu import _rand, off_knife_edge, rel

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bc(p):
    return p.view(1, -1, 1, 1)


class ConvCase:
    """One conv (1x1: KT = 0; dense temporal: KT taps) with its operands, the device runs at both levels and the fp64
    statements: exact, emulated per direction with the number of bf16 products the library reports, and of magnitudes."""

    def __init__(self, n, Ci, Co, T, V, KT, stride, mode, bn, seed):
        self.n, self.Ci, self.Co, self.T, self.V, self.KT, self.stride, self.bn = n, Ci, Co, T, V, KT, stride, bn
        g = torch.Generator().manual_seed(seed)
        self.x1 = _rand(g, n, Ci, T, V)
        self.a1 = self.a2 = self.x2 = None
        self.relu = False
        if mode in ('res_plain', 'res_affine', 'affine_relu'):
            self.a1 = (torch.rand(Ci, generator=g) + 0.5, _rand(g, Ci, scale=0.3))
            self.relu = True
        if mode in ('res_plain', 'res_affine'):
            self.x2 = _rand(g, n, Ci, T, V)
        if mode == 'res_affine':
            self.a2 = (torch.rand(Ci, generator=g) + 0.5, _rand(g, Ci, scale=0.3))
        off_knife_edge(self.x1, self.a1, self.x2, self.a2, self.relu)
        taps = max(KT, 1)
        self.w = _rand(g, Co, Ci, taps, 1, scale=(Ci * taps) ** -0.5)
        self.b = _rand(g, Co, scale=0.1)
        self.gamma = torch.rand(Co, generator=g) + 0.5
        self.beta = _rand(g, Co, scale=0.2)
        self.To = (T + stride - 1) // stride
        self.gz = _rand(g, n, Co, self.To, V)
        self.gsc, self.gsh = _rand(g, Co), _rand(g, Co)
        self.eps = 1e-5

    # ---- the op, as a bilinear map of (weight, virtual input) without bias
    def lin(self, w, v):
        pad = (w.shape[2] - 1) // 2
        return F.conv2d(v, w, None, stride=(self.stride, 1), padding=(pad, 0))

    def lin_t(self, w, d):                          # data gradient: bilinear in (weight, dz)
        v = torch.zeros(self.n, self.Ci, self.T, self.V, dtype=d.dtype, device=d.device, requires_grad=True)
        return torch.autograd.grad(self.lin(w, v), v, d)[0]

    def lin_w(self, d, v):                          # weight gradient: bilinear in (dz, virtual input)
        w = torch.zeros(self.Co, self.Ci, max(self.KT, 1), 1, dtype=d.dtype, device=d.device, requires_grad=True)
        return torch.autograd.grad(self.lin(w, v), w, d)[0]

    def terms(self, d):
        lib = native.lib()
        if self.KT:
            return lib.dsgcn_tconv_terms(d, self.n, self.Ci, self.Co, self.T, self.V, self.KT, self.stride)
        return lib.dsgcn_pwconv_terms(d, self.n, self.Ci, self.Co, self.T, self.V, self.stride)

    # ---- the device
    def run_device(self):
        def mk(t):
            return None if t is None else t.to(DEV).requires_grad_()
        tx1, tx2, tw, tb, tg, tbeta = mk(self.x1), mk(self.x2), mk(self.w), mk(self.b), mk(self.gamma), mk(self.beta)
        ta1 = None if self.a1 is None else (mk(self.a1[0]), mk(self.a1[1]))
        ta2 = None if self.a2 is None else (mk(self.a2[0]), mk(self.a2[1]))
        if self.KT:
            z, sc, sh, mean, var = K.tconv_bn(tx1, ta1, tx2, ta2, self.relu, tw, tb, tg, tbeta, self.eps, True, self.stride)
        elif self.bn:
            z, _, sc, sh, mean, var = K.pwconv(tx1, ta1, tx2, ta2, self.relu, tw, tb, 1, False, tg, tbeta, self.eps, self.Co,
                                               True)
        else:
            z = K.pwconv(tx1, ta1, tx2, ta2, self.relu, tw, tb, 1, False)[0]
        loss = (z * self.gz.to(DEV)).sum()
        if self.bn:
            loss = loss + (sc * self.gsc.to(DEV)).sum() + (sh * self.gsh.to(DEV)).sum()
        loss.backward()
        out = dict(z=z.detach(), dx1=tx1.grad, dw=tw.grad)
        if self.bn:
            out.update(sc=sc.detach(), sh=sh.detach(), mean=mean, var=var)
        if tx2 is not None:
            out['dx2'] = tx2.grad
        return {k: v.clone() for k, v in out.items()}

    # ---- fp64 statements (on the device: an fp64 conv of these sizes takes milliseconds there)
    def virt32(self):
        """The virtual input in fp32 as the kernels form it: fmaf(x1, s1, h1) [+ fmaf(x2, s2, h2)], max(., 0)."""
        x1, x2 = self.x1.to(DEV), None if self.x2 is None else self.x2.to(DEV)
        v = x1
        if self.a1 is not None:
            v = fma32(x1, bc(self.a1[0].to(DEV)), bc(self.a1[1].to(DEV)))
        if x2 is not None:
            v = v + (fma32(x2, bc(self.a2[0].to(DEV)), bc(self.a2[1].to(DEV))) if self.a2 is not None else x2)
        return torch.relu(v) if self.relu else v

    def bn_of(self, z):
        mean, var = z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False)
        sc = self.gamma.to(z) * torch.rsqrt(var + self.eps)
        return sc, self.beta.to(z) - mean * sc, mean, var

    def dz_coef(self, z):
        """dL/dz = gz + A0 + B0*z for L = sum(z*gz) + sum(sc*gsc) + sum(sh*gsh) (None, None without the BatchNorm)."""
        if not self.bn:
            return None, None
        sc, _, mean, var = self.bn_of(z)
        N = z.numel() // z.shape[1]
        B0 = -(self.gsc.to(z) - self.gsh.to(z) * mean) * sc / ((var + self.eps) * N)
        A0 = -self.gsh.to(z) * sc / N - B0 * mean
        return A0, B0

    def emulate(self, z_dev):
        """What the kernels of the CURRENT level compute, in fp64 from the fp32 operands as they form them: the forward from
        the virtual input, the gradients from dz_eff built on the device's own z (which is what the kernels read)."""
        w32, gz = self.w.to(DEV), self.gz.to(DEV)
        v32 = self.virt32()
        out = dict(z=term_product(self.lin, w32, v32, self.terms(0)) + bc(self.b.to(DEV).double()))
        if self.bn:
            out['sc'], out['sh'], out['mean'], out['var'] = self.bn_of(out['z'])
        A0, B0 = self.dz_coef(z_dev.double())
        if A0 is None:
            dz_d = dz_w = gz
        else:
            A32, B32 = A0.float(), B0.float()
            # data gradient: fmaf(gz, 1, A0) + fmaf(z, B0, 0); weight gradient: gz + fmaf(B0, z, A0)
            dz_d = (gz + bc(A32)) + z_dev * bc(B32)
            dz_w = gz + fma32(z_dev, bc(B32), bc(A32))
        dv = term_product(self.lin_t, w32, dz_d, self.terms(1))
        if self.relu:
            dv = dv * (v32 > 0)
        out['dx1'] = dv * (bc(self.a1[0].to(DEV).double()) if self.a1 is not None else 1.0)
        if self.x2 is not None:
            out['dx2'] = dv * (bc(self.a2[0].to(DEV).double()) if self.a2 is not None else 1.0)
        out['dw'] = term_product(self.lin_w, dz_w, v32, self.terms(2))
        return out

    def exact(self):
        """fp64 on the exact operands, and the magnitudes sum|a||b| of every product (R on absolute values)."""
        def d(t):
            return None if t is None else t.to(DEV).double()
        a1 = None if self.a1 is None else (d(self.a1[0]), d(self.a1[1]))
        a2 = None if self.a2 is None else (d(self.a2[0]), d(self.a2[1]))
        v = R.virt(d(self.x1), a1, d(self.x2), a2, self.relu)
        w = d(self.w)
        z = self.lin(w, v) + bc(d(self.b))
        A0, B0 = self.dz_coef(z)
        dz = d(self.gz) if A0 is None else d(self.gz) + bc(A0) + bc(B0) * z
        mask = (v > 0).double() if self.relu else 1.0
        s1 = bc(a1[0]) if a1 is not None else 1.0
        ex = dict(z=z, dx1=self.lin_t(w, dz) * mask * s1, dw=self.lin_w(dz, v))
        mag = dict(z=self.lin(w.abs(), v.abs()) + bc(d(self.b)).abs(), dx1=self.lin_t(w.abs(), dz.abs()) * mask * s1,
                   dw=self.lin_w(dz.abs(), v.abs()))
        taps = max(self.KT, 1)
        kacc = dict(z=self.Ci * taps, dx1=self.Co * taps, dw=self.n * self.To * self.V)
        return ex, mag, kacc


def check_case(c, bars):
    """The five assertions of a case.  bars: relative L2 against the emulation per output."""
    assert D.get_matmul_precision() == 'highest'
    before = c.run_device()
    with D.matmul_precision('high'):
        terms = [c.terms(d) for d in range(3)]
        got = c.run_device()
        again = c.run_device()
        emu = c.emulate(got['z'])
    after = c.run_device()
    # 1. the arithmetic: the fp64 emulation of the form each direction reports, to the bars the six-term kernels meet
    for k, bar in bars.items():
        if k in got:
            err = rel(got[k], emu[k])
            print(f'{k}: vs emulation {err:.3e} (bar {bar:.1e})')
            assert err < bar, (k, err, terms)
    # 2. the bound, elementwise against fp64 on the exact operands
    ex, mag, kacc = c.exact()
    for k, d in (('z', 0), ('dx1', 1), ('dw', 2)):
        if terms[d] == 3:
            bound = (HIGH_BOUND + (kacc[k] + 4) * 2.0 ** -24) * mag[k]
            diff = (got[k].double() - ex[k]).abs()
            worst = (diff / mag[k].clamp_min(1e-300)).max().item()
            print(f'{k}: max |err| / sum|a||b| = {worst:.3e} (bound {HIGH_BOUND + (kacc[k] + 4) * 2.0 ** -24:.3e})')
            assert bool((diff <= bound).all()), (k, worst)
    # 3. really reduced where the library says three products; the same bits as 'highest' where it says it is not
    # (a gradient behind a BatchNorm reads the forward's z through dz_eff: only the forward is comparable then)
    for k, d in (('z', 0), ('dx1', 1), ('dw', 2)):
        if terms[d] == 3:
            assert not torch.equal(got[k], before[k]), f"{k}: 'high' gave the bits of 'highest'"
        elif d == 0 or not (c.bn and terms[0] == 3):
            assert torch.equal(got[k], before[k]), f'{k}: {terms[d]} products reported, but the result moved'
    # 4. reproducible, 5. no leak
    for k in got:
        assert torch.equal(got[k], again[k]), f"{k}: two 'high' runs differ"
        assert torch.equal(before[k], after[k]), f"{k}: 'highest' after the context differs from before"
    return terms


PW_SHAPES = [(64, 128, 8, 25),       # MT = 1, two chunks
             (128, 256, 8, 25),      # MT = 2; k_wg3
             (96, 160, 8, 25),       # padded K, half-filled second row tile
             (256, 96, 8, 25),       # a wave past M only loads
             (128, 128, 8, 25),      # k_wg2<..B3>
             (256, 256, 8, 25), (256, 128, 8, 25),      # k_wg3
             (128, 128, 9, 17)]      # ragged plane
PW_MODES = ['plain', 'affine_relu', 'res_affine', 'affine_relu+bn', 'res_affine+bn']      # +bn: gamma / beta, dz_eff carries A0 / B0


@pytest.mark.parametrize('mode', PW_MODES)
@pytest.mark.parametrize('Ci,Co,T,V', PW_SHAPES)
def test_pwconv_high(Ci, Co, T, V, mode):
    """K-C through kernels.pwconv, forward + backward, n = 2: k_pwg3h (forward, data gradient), k_wg2h / k_wg3h (weight
    gradient).  Bars against the emulation: the ones of test_pwconv_bf16_terms_are_fp32_class (6e-7 / 6e-7 / 3e-7 for
    z / dx / dW: what is left is the fp32 accumulation), test_pwconv's 2e-5 for the BatchNorm statistics."""
    base, _, bn = mode.partition('+')
    c = ConvCase(2, Ci, Co, T, V, 0, 1, base, bool(bn), seed=Ci * 7 + Co + T)
    terms = check_case(c, dict(z=6e-7, dx1=6e-7, dx2=6e-7, dw=3e-7, sc=2e-5, sh=2e-5, mean=2e-5, var=2e-5))
    assert terms[0] == 3, 'every shape of this list runs its forward on the weight image'


TC_CASES = [(2, 128, 128, 32, 25, 9, 'affine_relu', 1), (2, 256, 256, 16, 25, 9, 'res_plain', 1), (2, 48, 80, 12, 17, 9, 'plain', 1),
            (1, 32, 40, 20, 18, 5, 'affine_relu', 1), (2, 16, 24, 8, 25, 3, 'res_affine', 1),
            (2, 64, 128, 32, 25, 9, 'res_affine', 2), (3, 32, 48, 15, 17, 5, 'affine_relu', 2)]


@pytest.mark.parametrize('n,Ci,Co,T,V,KT,mode,stride', TC_CASES)
def test_tconv_high(n, Ci, Co, T, V, KT, mode, stride):
    """The dense temporal conv through kernels.tconv_bn (what check_tconv_gemm uses), its small cases: k_tcgh forward / data
    gradient, k_tcwh weight gradient.  check_tconv_gemm's bar (2e-5 relative L2), here against the emulation."""
    assert K.tconv_gemm_ok(n, Ci, Co, T, V, KT, stride)
    c = ConvCase(n, Ci, Co, T, V, KT, stride, mode, True, seed=Ci * 3 + Co + T + KT)
    terms = check_case(c, {k: 2e-5 for k in ('z', 'dx1', 'dx2', 'dw', 'sc', 'sh', 'mean', 'var')})
    assert terms == [3, 3, 3]


@pytest.mark.parametrize('case', ['big_x_small_w', 'small_x_big_w', 'mixed_binades', 'non_finite'])
def test_pwconv_high_edge_cases(case):
    """The two-term form away from O(1) operands, as test_pwconv_bf16_split_edge_cases: bf16 has fp32's exponent range, so
    the emulation bars and the bound hold unchanged at 1e+-30 and over 80 binades; a non-finite input poisons exactly its own
    output positions."""
    n, Ci, Co, T, V = 4, 256, 256, 16, 25
    c = ConvCase(n, Ci, Co, T, V, 0, 1, 'plain', False, seed=11)
    c.b = torch.zeros(Co)
    if case == 'big_x_small_w':
        c.x1, c.w = c.x1 * 1e30, c.w * 1e-30
    elif case == 'small_x_big_w':
        c.x1, c.w = c.x1 * 1e-30, c.w * 1e30
    elif case == 'mixed_binades':
        sc = torch.pow(torch.tensor(2.0), (torch.arange(Ci) % 81 - 40).float())
        c.x1, c.w = c.x1 * sc.view(1, Ci, 1, 1), c.w / sc.view(1, Ci, 1, 1)
    else:
        c.x1[1, 7, 3, 5] = float('inf')
        c.x1[2, 100, 9, 0] = float('nan')
        with D.matmul_precision('high'):
            z = c.run_device()['z'].cpu()
        bad = torch.zeros(n, T, V, dtype=torch.bool)
        bad[1, 3, 5] = bad[2, 9, 0] = True
        fin = torch.isfinite(z).all(1)
        assert torch.equal(~fin, bad), 'a non-finite input must poison exactly its own output positions'
        c.x1 = torch.where(torch.isfinite(c.x1), c.x1, torch.zeros_like(c.x1))
        with D.matmul_precision('high'):
            emu = c.emulate(z.to(DEV))['z'].cpu()
        assert rel(z.permute(0, 2, 3, 1)[fin], emu.permute(0, 2, 3, 1)[fin]) < 6e-7
        return
    assert check_case(c, dict(z=6e-7, dx1=6e-7, dw=3e-7)) == [3, 3, 3]


# ---- the engines ---------------------------------------------------------------------------------------------------------
def _model(kind):
    from bench import ds_cfg, other_cfg
    torch.manual_seed(0)
    np.random.seed(0)
    m = D.build_model(ds_cfg(60, 'nturgb+d') if kind == 'ds' else other_cfg('stgcn', tcn_dropout=0.0))
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith(('alpha', 'beta', 'add_coeff')):
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
    x = torch.randn(2, 1, 2, 32, 25, 3, generator=g)
    y = torch.randint(0, 60, (2, 1), generator=g)
    return m, x, y


_ORACLE = {}


def _oracle(kind):
    """fp64 oracle of the first training step: logits, loss and every parameter gradient (computed once per model)."""
    if kind not in _ORACLE:
        from oracle import dsgcn_oracle as O
        m, x, y = _model(kind)
        sd = {k: (v.detach().double().requires_grad_(v.is_floating_point() and k in dict(m.named_parameters())))
              for k, v in m.state_dict().items()}
        if kind == 'ds':
            gc = O.graph_constants('nturgb+d')
            logits, loss = O.recognizer_forward_train(x.double(), y, sd, gc['node_type'], gc['edge_type'], O.dgstgcn_plan())
        else:
            logits, loss = O.recognizer_forward_train_backbone('stgcn', x.double(), y, sd, O.dgstgcn_plan())
        names = [k for k, v in sd.items() if v.requires_grad]
        grads = torch.autograd.grad(loss, [sd[k] for k in names], allow_unused=True)
        _ORACLE[kind] = (logits.detach(), loss.detach(), {k: g for k, g in zip(names, grads) if g is not None})
    return _ORACLE[kind]


def _grad_error(m, ref):
    num = sum(float((p.grad.detach().cpu().double() - ref[k]).pow(2).sum()) for k, p in m.named_parameters() if k in ref)
    den = sum(float(ref[k].pow(2).sum()) for k, p in m.named_parameters() if k in ref)
    return (num / den) ** 0.5


def _steps(kind, level, graph, steps=3):
    m, x, y = _model(kind)
    m = m.cuda().train()
    eng = D.TrainEngine(m, lr=0.05, use_graph=graph, warmup_eager=1, matmul_precision=level)
    losses = [eng.step(x.cuda(), y.cuda())['loss'].clone() for _ in range(steps)]
    return eng, torch.stack(losses).cpu(), eng.flat.flat_p.detach().clone().cpu()


_FRESH = '''
import sys, torch
sys.path.insert(0, {tests!r})
import test_matmul_precision_gpu as T
eng, losses, params = T._steps({kind!r}, None, True)
assert eng.matmul_precision == 'highest' and eng.capture_error is None
torch.save(dict(losses=losses, params=params), {out!r})
'''


@pytest.mark.parametrize('kind', ['ds', 'stgcn'])
def test_train_engine_high(kind, tmp_path):
    """DS-STGCN (dgphgcn1 / dgmstcn, shipped flags) and ST-GCN (unit_gcn / unit_tcn, dropout off), 2 clips, T = 32, V = 25,
    through TrainEngine(matmul_precision='high', warmup_eager=1)."""
    ref_logits, ref_loss, ref_grads = _oracle(kind)
    # step 1 against the fp64 oracle: the north star's 1e-4 on logits and loss; every gradient finite
    errs = {}
    for level in ('highest', 'high'):
        m, x, y = _model(kind)
        m = m.cuda().train()
        with D.matmul_precision(level):
            out = m.train_step(dict(keypoint=x.cuda(), label=y.cuda()), None)
            logits = m.cls_head(m.extract_feat(x.cuda()[:, 0]))
            out['loss'].backward()
        el = rel(logits.detach().cpu(), ref_logits)
        es = abs(float(out['log_vars']['loss']) - ref_loss.item()) / abs(ref_loss.item())
        errs[level] = _grad_error(m, ref_grads)
        print(f'{kind} {level}: logits rel {el:.3e}, loss rel {es:.3e}, whole-gradient rel L2 {errs[level]:.3e} (recorded, not gated)')
        assert el < 1e-4 and es < 1e-4, (level, el, es)
        assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    # captured: replayed steps 2-3 are the bits of an all-eager 'high' run
    eng, losses, params = _steps(kind, 'high', True)
    assert eng.capture_error is None and eng.graphed(*[t.cuda() for t in _model(kind)[1:]])
    assert abs(float(losses[0]) - ref_loss.item()) / abs(ref_loss.item()) < 1e-4
    _, losses_e, params_e = _steps(kind, 'high', False)
    assert torch.equal(losses, losses_e) and torch.equal(params, params_e)
    assert D.get_matmul_precision() == 'highest', "the engine's level must not leak into the process"
    # a 'high' engine does not depend on a later set_matmul_precision: its replay under process level 'highest' (above) and
    # an engine built at 'highest' afterwards is bit-identical to a fresh process that never touched 'high'
    _, losses_h, params_h = _steps(kind, None, True)
    assert not torch.equal(params_h, params), "'high' trained to the bits of 'highest'"
    out = str(tmp_path / 'fresh.pt')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    env.pop('DSGCN_MATMUL_PRECISION', None)
    r = subprocess.run([sys.executable, '-c', _FRESH.format(tests=os.path.join(ROOT, 'tests'), kind=kind, out=out)], env=env,
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    fresh = torch.load(out)
    assert torch.equal(fresh['losses'], losses_h) and torch.equal(fresh['params'], params_h)


def test_train_engine_high_survives_a_process_level_change():
    """Two engines at different levels in one process, stepped alternately, with the process level flipped in between: each
    reproduces its own single-engine trajectory."""
    _, want_h, _ = _steps('ds', 'high', True, steps=4)
    _, want_0, _ = _steps('ds', 'highest', True, steps=4)
    ma, x, y = _model('ds')
    mb = _model('ds')[0]
    ea = D.TrainEngine(ma.cuda().train(), lr=0.05, warmup_eager=1, matmul_precision='high')
    eb = D.TrainEngine(mb.cuda().train(), lr=0.05, warmup_eager=1, matmul_precision='highest')
    la, lb = [], []
    for i in range(4):
        D.set_matmul_precision('highest' if i % 2 else 'high')
        la.append(ea.step(x.cuda(), y.cuda())['loss'].clone())
        lb.append(eb.step(x.cuda(), y.cuda())['loss'].clone())
    D.set_matmul_precision('highest')
    assert torch.equal(torch.stack(la).cpu(), want_h) and torch.equal(torch.stack(lb).cpu(), want_0)


def test_infer_engine_high():
    """Same shape through InferEngine(matmul_precision='high'): scores within 1e-4 of the fp64 oracle in eval mode, and the
    replay equals the eager call."""
    from oracle import dsgcn_oracle as O
    m, x, y = _model('ds')
    m = m.cuda().eval()
    m.test_cfg['average_clips'] = None
    eager = D.InferEngine(m, use_graph=False, matmul_precision='high')(x.cuda())
    eng = D.InferEngine(m, warmup_eager=1, matmul_precision='high')
    first, second = eng(x.cuda()), eng(x.cuda())
    assert eng.capture_error is None and eng.graphed(x.cuda()) and eng.replays == 1
    assert torch.equal(first, eager) and torch.equal(second, eager)
    assert D.get_matmul_precision() == 'highest'
    base = D.InferEngine(m, use_graph=False)(x.cuda())
    assert not torch.equal(base, eager), "'high' scored to the bits of 'highest'"
    with torch.no_grad():
        sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
        gc = O.graph_constants('nturgb+d')
        ref = O.recognizer_forward_train(x.double(), y, sd, gc['node_type'], gc['edge_type'], O.dgstgcn_plan(),
                                         training=False)[0]
    for name, got in (('high', eager), ('highest', base)):
        err = rel(got.reshape(ref.shape).cpu(), ref)
        print(f'InferEngine {name}: scores rel {err:.3e}')
        assert err < 1e-4, (name, err)
