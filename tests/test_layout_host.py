"""CPU: the helpers of the layout tests (tests/layout_cases.py) do what the GPU tests rely on — the pad parameter comes
first and moves every slice of the flat buffer, an engine step does not notice it, a step at rate 0 leaves the parameters
bit-unchanged, and a shifted copy has the promised address, the values and the attributes of the original."""
import pytest
import torch

import dsgcn_amd as D
import torch_ops
from bench import ds_cfg, other_cfg
from grad_accum_fp64 import SGD, micro_batches, reduced_model
from layout_cases import alignment_classes, shifted, shifted_operands, with_pad

CONFIGS = {'dsstgcn_ntu60': lambda: ds_cfg(60), 'dsstgcn_ntu120': lambda: ds_cfg(120),
           'dsstgcn_k400_coco': lambda: ds_cfg(400, 'coco'), 'ctrgcn_ntu60': lambda: other_cfg('ctrgcn'),
           'stgcn_ntu60': lambda: other_cfg('stgcn'), 'stgcnpp_ntu60': lambda: other_cfg('stgcnpp'),
           'ctrgcn_shipped_ntu60': lambda: other_cfg('ctrgcn_shipped'), 'stgcn_shipped_ntu60': lambda: other_cfg('stgcn_shipped')}


@pytest.mark.parametrize('name', list(CONFIGS))
def test_pad_comes_first_and_moves_every_slice(name):
    torch.manual_seed(0)
    base = D.FlatParams(D.build_model(CONFIGS[name]()), gather=True)
    assert sum(alignment_classes(base)) == len(base.params)
    seen = set()
    for k in (1, 2, 3):
        m = with_pad(D.build_model(CONFIGS[name]()), k)
        names = [n for n, _ in m.named_parameters()]
        assert names[0] == '_align_pad'
        flat = D.FlatParams(m, gather=True)
        assert flat.slices[0] == (0, k) and flat.numel == base.numel + k
        assert [(off - k, n) for off, n in flat.slices[1:]] == base.slices            # every other slice moves by k floats
        assert all(p.data_ptr() == flat.flat_p.data_ptr() + 4 * off for p, (off, _) in zip(flat.params, flat.slices))
        cls, cls0 = alignment_classes(flat), alignment_classes(base)
        assert [cls[(c + k) % 4] - (1 if (c + k) % 4 == 0 else 0) for c in range(4)] == cls0     # the classes rotate
        seen.add(tuple(cls))
    with pytest.raises(ValueError):
        with_pad(torch.nn.Linear(2, 2), 1)                   # a top module with parameters of its own: the pad would not lead
    with pytest.raises(ValueError):
        with_pad(D.build_model(CONFIGS[name]()), 4)


def _run(k, steps=2, lr=None):
    eng = D.TrainEngine(with_pad(reduced_model(), k), use_graph=False, **SGD)
    losses, grads = [], []
    with D.kernels.use_ops(torch_ops):
        for kp, lb in micro_batches(steps):
            out = eng.step(kp, lb, lr=lr)
            losses.append(out['loss'].clone())
            grads.append(eng.flat.flat_g.clone())
    return eng, losses, grads


def test_engine_step_does_not_notice_the_pad():
    """The same operations on the same values at other offsets: losses, gradients and the parameters after two SGD steps
    are bit-equal with and without the pad; the pad's own slice stays zero (no gradient, zero weight decay term)."""
    e0, l0, g0 = _run(0)
    for k in (1, 2, 3):
        ek, lk, gk = _run(k)
        assert all(torch.equal(a, b) for a, b in zip(l0, lk))
        assert all(torch.equal(a, b[k:]) and not b[:k].any() for a, b in zip(g0, gk))
        assert torch.equal(e0.flat.flat_p, ek.flat.flat_p[k:]) and not ek.flat.flat_p[:k].any()
        assert torch.equal(e0.opt.buf, ek.opt.buf[k:])
        named = dict(ek.model.named_parameters())
        for n, p in e0.model.named_parameters():
            assert torch.equal(p, named[n]), n
    assert float(g0[0].abs().max()) > 0 and not torch.equal(g0[0], g0[1])


def test_step_at_rate_zero_leaves_the_parameters_bit_unchanged():
    """sgd_update ends in p + (-rate) * st: at rate 0 the parameters stay what they were (momentum and weight decay move
    the momentum buffer only), so every step of the GPU tests sees the same weights."""
    for k in (0, 2):
        eng = D.TrainEngine(with_pad(reduced_model(), k), use_graph=False, **SGD)
        p0 = eng.flat.flat_p.clone()
        with D.kernels.use_ops(torch_ops):
            for kp, lb in micro_batches(2):
                eng.step(kp, lb, lr=0.0)
        assert torch.equal(eng.flat.flat_p, p0)
        assert eng.opt.buf.any()                                        # the step did run
    e1, _, g1 = _run(1, lr=0.0)
    (kp, lb), = micro_batches(1)
    with D.kernels.use_ops(torch_ops):
        e1.step(kp, lb, lr=0.0)
    assert torch.equal(e1.flat.flat_g, g1[0])                           # same weights, same batch: the same gradient


@pytest.mark.parametrize('k', [0, 1, 2, 3])
@pytest.mark.parametrize('shape', [(1,), (7, 3), (2, 5, 4, 3), (64,)])
def test_shifted_copy(k, shape):
    t = torch.randn(shape)
    t._dsgcn_bn = marker = object()
    t._dsgcn_sink = sink = object()
    s = shifted(t, k)
    assert s.data_ptr() % 16 == 4 * k and s.is_contiguous() and s.shape == t.shape and s.dtype == t.dtype
    assert torch.equal(s, t) and s.data_ptr() != t.data_ptr()
    assert s._dsgcn_bn is marker and s._dsgcn_sink is sink
    assert s.untyped_storage().nbytes() == 4 * (t.numel() + 8)
    s2 = shifted(t.t() if t.dim() == 2 else t, k)                       # (non-contiguous input -> contiguous copy)
    assert s2.is_contiguous()
    with pytest.raises(TypeError):
        shifted(t.double(), k)


def test_shifted_operands_patches_every_module_and_counts(monkeypatch):
    from dsgcn_amd import kernels, kernels_flags, kernels_head, kernels_plain
    original = kernels._f32c
    moved = shifted_operands(monkeypatch, 3)
    f = kernels._f32c
    assert f is not original and all(m._f32c is f for m in (kernels_plain, kernels_head, kernels_flags))
    assert f(None) is None and moved.count == 0
    t = torch.randn(5, 3).t()
    t._dsgcn_sink = 'x'
    s = f(t)
    assert moved.count == 1 and s.data_ptr() % 16 == 12 and torch.equal(s, t) and s.is_contiguous()
    with pytest.raises(TypeError):
        f(torch.zeros(2, dtype=torch.float64))                          # the original's check still runs first
    monkeypatch.undo()
    assert kernels._f32c is original and kernels_head._f32c is original
