"""Matmul precision level of the kernels that carry an fp32 product on bf16 terms.

'highest' (default): six bf16 MFMAs per fp32 product on the exact three-way bf16 split of both operands (csrc/common.h,
B3): fp32-class error.  'high': the three products a0*b0 + a0*b1 + a1*b0 on the first two terms of each operand, fp32
accumulate: |error| <= 3 * 2^-16 sum|a||b| elementwise (between TF32 and fp32), half the MFMAs and two thirds of the split.

The level lives in the library — one atomic integer, read on the host by the call that launches (include/dsgcn.h) — and is
process-wide: a captured hipGraph keeps the kernels it was captured with; ``TrainEngine`` / ``InferEngine`` fix theirs at
construction and run every step under it.  ``kernels.py`` reads DSGCN_MATMUL_PRECISION for the level a process starts at."""
from . import native

MATMUL_PRECISIONS = ('highest', 'high')


def precision_level(name, what='matmul precision'):
    if name not in MATMUL_PRECISIONS:
        raise ValueError(f'{what}: {name!r} is not one of {MATMUL_PRECISIONS}')
    return MATMUL_PRECISIONS.index(name)


def set_matmul_precision(name):
    """'highest' | 'high' for every launch of this process from now on (captured graphs keep theirs)."""
    native.check(native.lib().dsgcn_set_matmul_precision(precision_level(name)), 'dsgcn_set_matmul_precision')


def get_matmul_precision():
    return MATMUL_PRECISIONS[native.lib().dsgcn_get_matmul_precision()]


class matmul_precision:
    """``with matmul_precision('high'): ...`` — the level inside the block, the previous one restored on exit (also when
    the block raises)."""

    def __init__(self, name):
        self.level = precision_level(name)

    def __enter__(self):
        lib = native.lib()
        self.before = lib.dsgcn_get_matmul_precision()
        native.check(lib.dsgcn_set_matmul_precision(self.level), 'dsgcn_set_matmul_precision')
        return self

    def __exit__(self, *exc):
        native.check(native.lib().dsgcn_set_matmul_precision(self.before), 'dsgcn_set_matmul_precision')
        return False
