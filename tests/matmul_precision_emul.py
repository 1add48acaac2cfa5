"""fp64 emulation of the bf16-term products of csrc/common.h, shared by test_matmul_precision_host.py / _gpu.py.

An fp32 operand x is split with torch's round-to-nearest-even bf16 cast exactly as the kernels split it (x0 = bf16(x),
x1 = bf16(x - x0), x2 = x - x0 - x1: the subtractions are exact in fp32); a product form is then a sum of fp64 evaluations
of a BILINEAR op on pairs of terms:

    'high'    (3 products): a0*b0 + a0*b1 + a1*b0                      (terms i + j <= 1)
    'highest' (6 products): the same + a0*b2 + a1*b1 + a2*b0           (terms i + j <= 2)

What remains between such an emulation and the kernel is the kernel's fp32 accumulation alone."""
import torch

PAIRS = {3: ((0, 0), (0, 1), (1, 0)), 6: ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0))}
# the bound of the three-product form: every cast is off by at most 2^-8 relative, so |x - x0 - x1| <= 2^-16 |x| and the
# dropped part of a*b (a1*b1 + a*(b - b0 - b1) + (a - a0 - a1)*b up to higher order) is at most 3 * 2^-16 |a||b|
HIGH_BOUND = 3 * 2.0 ** -16


def split_terms(x, nterms=3):
    """fp32 tensor -> its first ``nterms`` bf16 terms as fp64 tensors."""
    assert x.dtype == torch.float32
    terms, r = [], x.clone()
    for _ in range(nterms):
        t = r.to(torch.bfloat16).to(torch.float32)
        terms.append(t.double())
        r = r - t
    return terms


def term_product(op, a, b, products):
    """``op`` (bilinear, evaluated in fp64) on fp32 operands a, b the way a kernel with ``products`` bf16 products per fp32
    product forms it; products 0 (an fp32 MFMA form): the plain fp64 value."""
    if products not in PAIRS:
        return op(a.double(), b.double())
    at, bt = split_terms(a), split_terms(b)
    out = None
    for i, j in reversed(PAIRS[products]):          # smallest first
        v = op(at[i], bt[j])
        out = v if out is None else out + v
    return out


def fma32(x, s, h):
    """fp32 fmaf(x, s, h) of fp32 tensors: x*s is exact in fp64, one rounding to fp32 follows."""
    return (x.double() * s.double() + h.double()).float()
