"""-m gpu: the shipped K-B (csrc/dynadj.hip) off its six instantiated (V, mid) pairs — the run-time form L(0, 0) that any
other skeleton or gcn_ratio runs — against the fp64 statement (tests/torch_ops.py) at check_dynadj's bars, the C ABI called
directly at three row strides into poisoned, fenced buffers (one writer per element, zero pad columns, nothing outside),
the return codes that come back before a launch, and the forward past 128 samples at a width that needs two windows.

Measured (relative L2 against fp64; bars 2e-6 forward, 2e-5 every gradient).  "statement": tests/torch_ops.py itself in fp32
on the host (test_dynadj_limits_host.py holds it to a fifth of each bar); "kernel": the MI355X.  forward / worst gradient:

    (n, Ci, mid, V, P, E)      statement            kernel
    (3, 8, 8, 18, 5, 15)       9.2e-8 / 4.3e-7      8.4e-8 / 4.7e-7
    (2, 16, 12, 25, 5, 15)     1.2e-7 / 3.1e-7      1.2e-7 / 3.1e-7
    (2, 8, 6, 25, 5, 15)       9.6e-8 / 3.4e-7      9.1e-8 / 4.4e-7
    (2, 7, 5, 11, 3, 7)        7.3e-8 / 2.8e-7      6.6e-8 / 2.9e-7
    (2, 8, 4, 32, 5, 15)       1.7e-7 / 5.5e-7      1.4e-7 / 9.2e-7
    (2, 8, 16, 8, 2, 4)        8.4e-8 / 7.6e-7      8.0e-8 / 9.5e-7
    (2, 16, 32, 11, 3, 5)      9.8e-8 / 7.0e-7      1.0e-7 / 4.4e-7
    (2, 8, 17, 11, 3, 7)       9.5e-8 / 2.5e-7      9.2e-8 / 2.9e-7
    (130, 8, 17, 11, 3, 7)     1.2e-7 / 5.2e-7      1.2e-7 / 4.1e-7
    (2, 16, 20, 17, 5, 15)     1.0e-7 / 3.5e-7      9.7e-8 / 4.9e-7
    (2, 64, 36, 25, 5, 15)     2.2e-7 / 1.9e-6      2.3e-7 / 1.9e-6      (beta)
    (2, 16, 37, 25, 5, 15)     2.0e-7 / 2.7e-6      2.0e-7 / 1.2e-6      (beta / bse)
    (2, 8, 27, 32, 5, 15)      1.2e-7 / 5.2e-7      1.3e-7 / 7.4e-7
    (2, 8, 8, 25, 5, 17)       8.2e-8 / 3.8e-7      7.6e-8 / 2.3e-7
    (2, 8, 9, 25, 7, 33)       7.4e-8 / 3.4e-7      7.3e-8 / 4.1e-7      (4.0e-2 on w2 before the K-split fix)
    (2, 8, 8, 25, 1, 1)        8.5e-8 / 2.0e-6      7.9e-8 / 2.2e-6      (bse)
    (2, 8, 3, 3, 2, 2)         6.7e-8 / 6.5e-7      7.0e-8 / 9.7e-7
    (1, 8, 1, 2, 1, 1)         1.6e-7 / 2.8e-7      5.3e-8 / 2.6e-7      (1.1 on b2 before the K-split fix)

The fix: where the long tiles of the subset-1 backward split K = E * mid in two, the first half was the FLOOR of K / 2
rounded up to a k-step, so at K = 8j + 1 the two halves ended one row short and the last row of We never reached d a1 /
d b1.  Every instantiated shape has an even K."""
import pytest
import torch

import dynadj_cases as C
import torch_ops as R
from dsgcn_amd import kernels as K
from dsgcn_amd import native
from test_kernels_gpu import check_dynadj, ref_dev, rel

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EINVAL, EUNSUPPORTED = -1, -2
SENTINEL = 0x7FA5C3E1                   # the fence words around every buffer (a NaN with a payload, as int32)
NAN_BITS = 0x7FC00000


@pytest.mark.parametrize('case', C.RUNTIME_CASES, ids=C.case_id)
def test_runtime_form_against_fp64(case):
    n, Ci, mid, V, P, E = case
    check_dynadj(n, Ci, mid, V, None, inputs=C.dyn_inputs(*case, seed=C.case_seed(case)))


# ---- the C ABI, directly ------------------------------------------------------------------------------------------------

class Fenced:
    """A buffer that is a view into a larger tensor, 64 fence words on each side."""

    def __init__(self, shape, src=None, fill=None, dtype=torch.float32):
        numel = 1
        for s in shape:
            numel *= s
        self.big = torch.full((numel + 128,), SENTINEL, dtype=torch.int32, device=DEV)
        self.bits = self.big[64:64 + numel].view(shape)                  # the body as int32
        self.t = self.bits if dtype == torch.int32 else self.bits.view(torch.float32)
        if src is not None:
            self.t.copy_(src.to(DEV).reshape(shape))
        else:
            self.t.fill_(fill)

    def ptr(self):
        return self.t.data_ptr()

    def fences_intact(self):
        return bool((self.big[:64] == SENTINEL).all()) and bool((self.big[-64:] == SENTINEL).all())


def _abi_operands(case):
    n, Ci, mid, V, P, E = case
    t, nt, et = C.dyn_inputs(*case, seed=C.case_seed(case))
    d = {k: v.to(DEV) for k, v in t.items()}
    proj = K._kb_projections(d['xbar'], V, [d['w1'], d['w2'], d['wse']], [d['b1'], d['b2'], d['bse']])
    assert proj.shape == (n, (4 + P) * mid, 32)
    ops = {k: Fenced(d[k].shape, src=d[k]) for k in ('A', 'alpha', 'beta', 'we', 'be')}
    ops['nt'] = Fenced(nt.shape, src=nt, dtype=torch.int32)
    ops['et'] = Fenced(et.shape, src=et, dtype=torch.int32)
    ops['dah'] = Fenced((n, 3 * mid, V, V), src=C.dyn_cotangent(n, mid, V))
    return proj, ops


def _abi_run(case, proj, ops, ld, fill, pad=3):
    """forward + backward through dsgcn_dynadj_fwd / _bwd into prefilled, fenced buffers -> dict of Fenced"""
    n, Ci, mid, V, P, E = case
    lib = native.lib()
    st = torch.cuda.current_stream().cuda_stream
    stride = lib.dsgcn_dynadj_partial_stride(mid, V, E)
    o = dict(proj=Fenced(proj.shape, src=proj),
             ahat=Fenced((n, 3 * mid, V, V), fill=fill), dd=Fenced((n, 3 * mid, V, V), fill=fill),
             dproj=Fenced(proj.shape, fill=fill), ppar=Fenced((n, stride + pad), fill=fill))
    before = o['ppar'].bits.clone()
    p = lambda k: (o[k] if k in o else ops[k]).ptr()
    native.check(lib.dsgcn_dynadj_fwd(p('proj'), p('A'), p('alpha'), p('beta'), p('we'), p('be'), p('nt'), p('et'), p('ahat'),
                                      n, mid, V, ld, P, E, st), 'dsgcn_dynadj_fwd')
    native.check(lib.dsgcn_dynadj_bwd(p('proj'), p('alpha'), p('beta'), p('we'), p('be'), p('nt'), p('et'), p('dah'), p('dd'),
                                      p('dproj'), p('ppar'), stride + pad, n, mid, V, ld, P, E, st), 'dsgcn_dynadj_bwd')
    torch.cuda.synchronize()
    assert torch.equal(o['ppar'].bits[:, stride:], before[:, stride:])           # the slack of each partial row: untouched
    assert torch.equal(o['proj'].bits, proj.view(torch.int32))                   # (bits: the pad columns may hold NaN)
    for k, b in list(o.items()) + list(ops.items()):
        assert b.fences_intact(), k
    return o, stride


@pytest.mark.parametrize('case', [(2, 7, 5, 11, 3, 7), (2, 8, 16, 8, 2, 4), (2, 8, 9, 25, 7, 33)], ids=C.case_id)
def test_c_abi_row_strides_one_writer_zero_pads(case):
    """The header's two claims about the backward's outputs: every element of dproj / ppar has exactly one writer (the
    result does not depend on what the buffers held: zeros or NaN), and the pad columns of dproj are written as zeros —
    at the padded stride the package uses (32), at ld = V and at an odd ld = V + 3 whose input pad columns hold NaN."""
    n, Ci, mid, V, P, E = case
    proj32, ops = _abi_operands(case)
    projV = proj32[..., :V].contiguous()
    projP = torch.full((n, proj32.shape[1], V + 3), float('nan'), device=DEV)
    projP[..., :V] = projV
    runs = [_abi_run(case, proj, ops, ld, fill)
            for proj, ld, fill in ((proj32, 32, 0.0), (projV, V, float('nan')), (projP, V + 3, float('nan')))]
    (o0, stride), others = runs[0], runs[1:]
    for o, _ in runs:
        for k in ('ahat', 'dd', 'dproj', 'ppar'):
            body = o[k].t[..., :V] if k == 'dproj' else (o[k].t[:, :stride] if k == 'ppar' else o[k].t)
            assert bool(torch.isfinite(body).all()), k
        assert not bool(o['dproj'].bits[..., V:].any())                          # pad columns: +0.0 exactly
    for o, _ in others:
        assert torch.equal(o['ahat'].t, o0['ahat'].t) and torch.equal(o['dd'].t, o0['dd'].t)
        assert torch.equal(o['dproj'].t[..., :V], o0['dproj'].t[..., :V])
        assert torch.equal(o['ppar'].t[:, :stride], o0['ppar'].t[:, :stride])
    # ... and what the package's autograd node returns from the same operands
    leaf = {k: ops[k].t.clone().requires_grad_() for k in ('A', 'alpha', 'beta', 'we', 'be')}
    pl = proj32.detach().clone().requires_grad_()
    out = K._DynAdj.apply(pl, leaf['A'], leaf['alpha'], leaf['beta'], leaf['we'], leaf['be'], ops['nt'].t, ops['et'].t,
                          False, None)
    out.backward(ops['dah'].t)
    assert torch.equal(out.detach(), o0['ahat'].t)
    assert torch.equal(pl.grad[..., :V], o0['dproj'].t[..., :V]) and not bool(pl.grad[..., V:].any())
    sums = K.colsum(o0['ppar'].t[:, :stride].contiguous())
    grads = torch.cat([leaf[k].grad.reshape(-1) for k in ('A', 'alpha', 'beta', 'we', 'be')])
    assert torch.equal(sums, grads)


def test_return_codes_before_any_launch():
    """Real buffers, arguments out of range: the code comes back and no output byte changes."""
    case = (2, 7, 5, 11, 3, 7)
    n, Ci, mid, V, P, E = case
    proj, ops = _abi_operands(case)
    lib = native.lib()
    st = torch.cuda.current_stream().cuda_stream
    stride = lib.dsgcn_dynadj_partial_stride(mid, V, E)
    wide = Fenced((n, (4 + P) * 65, 40), fill=0.25)                   # large enough for every shape asked below
    outs = {k: Fenced((n, 3 * 65, 33, 33), fill=float('nan')) for k in ('ahat', 'dd')}
    outs['dproj'] = Fenced(wide.t.shape, fill=float('nan'))
    outs['ppar'] = Fenced((n, lib.dsgcn_dynadj_partial_stride(65, 33, E)), fill=float('nan'))
    we = Fenced((E * 65, 65), fill=0.1)
    p = lambda k: ops[k].ptr()

    def fwd(n_, mid_, V_, ld_):
        return lib.dsgcn_dynadj_fwd(wide.ptr(), p('A'), p('alpha'), p('beta'), we.ptr(), we.ptr(), p('nt'), p('et'),
                                    outs['ahat'].ptr(), n_, mid_, V_, ld_, P, E, st)

    def bwd(n_, mid_, V_, ld_, ps):
        return lib.dsgcn_dynadj_bwd(wide.ptr(), p('alpha'), p('beta'), we.ptr(), we.ptr(), p('nt'), p('et'), outs['ahat'].ptr(),
                                    outs['dd'].ptr(), outs['dproj'].ptr(), outs['ppar'].ptr(), ps, n_, mid_, V_, ld_, P, E, st)
    big = 10 ** 7
    assert fwd(n, mid, 33, 40) == EUNSUPPORTED and bwd(n, mid, 33, 40, big) == EUNSUPPORTED
    assert fwd(n, 65, V, 32) == EUNSUPPORTED and bwd(n, 65, V, 32, big) == EUNSUPPORTED
    assert fwd(n, mid, V, V - 1) == EUNSUPPORTED and bwd(n, mid, V, V - 1, big) == EUNSUPPORTED
    assert bwd(n, 64, 25, 32, big) == EUNSUPPORTED                   # the forward's range is the wider one
    assert bwd(n, mid, V, 32, stride - 1) == EINVAL
    assert fwd(0, mid, V, 32) == EINVAL and bwd(0, mid, V, 32, stride) == EINVAL
    torch.cuda.synchronize()
    for k, b in outs.items():
        assert bool((b.bits == NAN_BITS).all()) and b.fences_intact(), k


# ---- the forward no longer depends on the batch size --------------------------------------------------------------------

@pytest.mark.parametrize('case', C.FORWARD_CASES, ids=C.case_id)
def test_forward_past_128_samples(case):
    """Inference only (torch.no_grad): mid = 40 takes one window as before; mid = 50 does not fit one window and was
    refused past 128 samples — it now takes the two windows it takes at n <= 128.  With gradients the backward's range
    decides, before anything is launched."""
    n, Ci, mid, V, P, E = case
    t, nt, et = C.dyn_inputs(*case, seed=C.case_seed(case))
    assert C.fwd_windows(n, mid, V, E) == (1 if mid == 40 else 2) and not C.supported(n, mid, V, 32, E, 1)

    def run(mod, dt, dev):
        with torch.no_grad():
            return mod.dynadj(*[v.to(dev, dt) for v in t.values()], nt.to(dev), et.to(dev))
    got = run(K, torch.float32, DEV)
    want = run(R, torch.float64, ref_dev(n))
    print(f'{C.case_id(case)}: forward {rel(got, want):.2e}')
    assert rel(got, want) < 2e-6, rel(got, want)
    assert torch.equal(got, run(K, torch.float32, DEV))
    with pytest.raises(NotImplementedError, match=f'mid = {mid} at V = 25 joints, E = 15 .*mid <= 37'):
        K.dynadj(*[v.to(DEV).requires_grad_() for v in t.values()], nt.to(DEV), et.to(DEV))
