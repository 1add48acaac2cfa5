"""Shared pieces of the layout / alignment tests: a model whose flat parameter buffer starts k floats late, copies of a
tensor at a chosen 4-byte alignment class, and a patch that hands every kernel operand over at that class.

``FlatParams`` lays the parameters out back to back without padding, so a parameter's address is 4-byte aligned and
nothing more; activations and gradients come from the caching allocator (512-byte aligned) unless they are views.  The
kernels cast operand pointers to 16-byte vector types in many places: these helpers put operands at the other three
classes (address mod 16 = 4, 8, 12)."""
import importlib

import torch

MODULES = ('kernels', 'kernels_plain', 'kernels_head', 'kernels_flags')       # every module that binds the name `_f32c`
# (kernels_infer reaches it as `kernels._f32c` at call time: covered by the first entry)

# Operands that a wrapper WRITES THROUGH after taking them from `_f32c` would lose the write to the shifted copy and have
# to be passed by identity.  The 83 call sites were gone through for this: every tensor that goes through `_f32c` is read
# only (activations, weights, biases, BatchNorm coefficients, adjacencies, incoming gradients, targets); everything a
# launch writes (outputs, partial rows, BatchNorm buffers, running statistics, the step counter of the fused dropout, the
# `OutSlot` slices of `pwconv(out=...)`, the coefficient rows of `BNCtx`) is allocated by the wrapper or handed over by
# `data_ptr()` without passing `_f32c`.  The list is therefore empty.
WRITTEN_THROUGH = ()


def with_pad(model, k):
    """Registers k in 1..3 floats of padding as the model's FIRST parameter (the recognizers own no parameter themselves, so
    a parameter of the top module precedes every submodule's in ``parameters()``): every slice of ``FlatParams(model)``
    starts k floats later.  k = 0: the model as it is.  The pad takes no part in the forward and never gets a gradient."""
    if not 0 <= k <= 3:
        raise ValueError(k)
    if k:
        if model._parameters:
            raise ValueError('with_pad: the top module has parameters of its own, the pad would not come first')
        model._align_pad = torch.nn.Parameter(torch.zeros(k, device=next(model.parameters()).device))
        assert next(model.parameters()) is model._align_pad
    return model


def shifted(t, k):
    """A contiguous copy of t whose address is 4*k mod 16 (k in 0..3), inside a buffer of numel + 8 elements; the Python
    attributes of t (``_dsgcn_bn``, ``_dsgcn_sink``) travel with it."""
    if t.element_size() != 4:
        raise TypeError(f'shifted: 4-byte elements expected, got {t.dtype}')
    with torch.no_grad():
        buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
        first = ((4 * k - buf.data_ptr()) % 16) // 4
        assert buf.data_ptr() % 4 == 0 and 0 <= first < 4
        out = buf[first:first + t.numel()].view(t.shape)
        out.copy_(t)
    assert out.data_ptr() % 16 == 4 * k and out.is_contiguous()
    for name, value in vars(t).items():
        setattr(out, name, value)
    return out


class Moved:
    """How many operands the patch of ``shifted_operands`` moved (a case that moved none tested nothing)."""

    def __init__(self):
        self.count = 0


def shifted_operands(monkeypatch, k):
    """Until monkeypatch undoes it, every operand that a kernel wrapper takes through `_f32c` is a copy at alignment class
    k.  -> a ``Moved`` counter."""
    mods = [importlib.import_module('dsgcn_amd.' + name) for name in MODULES]
    original = mods[0]._f32c
    moved = Moved()

    def f32c_shifted(t):
        t = original(t)
        if t is None:
            return t
        moved.count += 1
        return shifted(t, k)

    for mod in mods:
        assert mod._f32c is original, mod.__name__
        monkeypatch.setattr(mod, '_f32c', f32c_shifted)
    return moved


def alignment_classes(flat):
    """[count of parameter tensors at flat offset mod 4 == c for c in 0..3]"""
    out = [0, 0, 0, 0]
    for off, _ in flat.slices:
        out[off % 4] += 1
    return out
