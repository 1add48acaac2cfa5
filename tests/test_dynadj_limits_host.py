"""CPU: the range of K-B (csrc/dynadj.hip) as the library states it (``dsgcn_dynadj_supported``, which both launches ask)
against the LDS carve restated in Python; that tests/dynadj_cases.RUNTIME_CASES still reaches the paths it exists for; that
the project's bars test the kernel and not the inputs at those cases (the fp32 STATEMENT's own error is at most a fifth of
each bar); and that a shipped-flag ``dgphgcn1`` whose backward cannot launch says so in forward instead of dying inside
autograd."""
import pytest
import torch

import dsgcn_amd as D
import dynadj_cases as C
import torch_ops
from dsgcn_amd import native
from test_dghgcn_host import graph_A

EUNSUPPORTED = -2
FWD_BAR, GRAD_BAR = 2e-6, 2e-5          # check_dynadj's bars (relative L2)


def test_predicate_is_the_lds_carve():
    ok = native.lib().dsgcn_dynadj_supported
    bad = []
    for backward in (0, 1):
        for E in (1, 15, 16, 17, 33):
            for n in (1, 128, 129):
                for V in range(1, 33):
                    for mid in range(1, 65):
                        got = ok(n, mid, V, 32, E, backward)
                        assert got in (0, EUNSUPPORTED)
                        if (got == 0) != C.supported(n, mid, V, 32, E, backward):
                            bad.append((n, mid, V, E, backward, got))
    assert not bad, bad[:10]
    # outside the loops' range: joints, width, row stride, empty dimensions
    for args in [(1, 8, 33, 40, 15, 0), (1, 65, 25, 32, 15, 0), (1, 8, 25, 24, 15, 1), (0, 8, 25, 32, 15, 0),
                 (1, 0, 25, 32, 15, 1), (1, 8, 0, 32, 15, 0), (1, 8, 25, 32, 0, 1)]:
        assert ok(*args) == EUNSUPPORTED and not C.supported(*args), args
    assert ok(1, 8, 25, 25, 15, 1) == 0 and ok(1, 8, 32, 32, 15, 0) == 0


def _largest_mid(n, V, E, backward):
    ok = native.lib().dsgcn_dynadj_supported
    return max(m for m in range(1, 65) if ok(n, m, V, 32, E, backward) == 0)


def test_pinned_limits():
    """The forward takes every mid <= 64 at any batch size (two windows where one does not fit); the backward's image is
    the larger one."""
    assert [_largest_mid(128, 25, 15, 0), _largest_mid(129, 25, 15, 0), _largest_mid(129, 25, 15, 1)] == [64, 64, 37]
    assert [_largest_mid(128, 32, 15, 0), _largest_mid(129, 32, 15, 0), _largest_mid(129, 32, 15, 1)] == [64, 64, 27]
    assert _largest_mid(1, 17, 15, 1) == 60
    # what the one-window forward held before: past it the launch takes two windows, below it the count is unchanged
    assert C.fwd_windows(129, 48, 25, 15) == 1 and C.fwd_windows(129, 49, 25, 15) == 2
    assert C.fwd_windows(129, 37, 32, 15) == 1 and C.fwd_windows(129, 38, 32, 15) == 2
    assert C.fwd_windows(128, 15, 25, 15) == 1 and C.fwd_windows(128, 16, 25, 15) == 2
    # the backward never runs a shape the forward refuses
    for V in range(1, 33):
        for mid in range(1, 65):
            for E in (1, 15, 33):
                assert C.supported(1, mid, V, 32, E, 0) or not C.supported(1, mid, V, 32, E, 1)


def test_table_reaches_the_paths_it_exists_for():
    cases = C.RUNTIME_CASES
    assert len(cases) == len(set(cases)) == 18 and set(C.LIMIT_CASES) <= set(cases)
    runtime = [c for c in cases if (c[3], c[2]) not in C.INSTANTIATED]
    assert len(runtime) == len(cases) - 2                                        # all but <25, 8> at E = 17 and at P = E = 1
    assert sum(C.ksplit(c[2], c[3]) == 1 for c in runtime) >= 2 and sum(C.ksplit(c[2], c[3]) == 2 for c in runtime) >= 2
    assert any(C.class_tiles(c[5]) >= 2 for c in cases) and any(C.class_tiles(c[5]) >= 3 for c in runtime)
    assert any(c[5] % 16 for c in cases if C.class_tiles(c[5]) >= 2)             # a partial last class tile
    uneven = [c for c in runtime if len(set(C.window_widths(c[2], C.fwd_windows(c[0], c[2], c[3], c[5])))) == 2]
    assert uneven and any(C.fwd_windows(c[0], c[2], c[3], c[5]) == 1 and c[2] >= 16 for c in runtime)
    assert any(min(C.launch_lds(c)) > 64 * 1024 for c in runtime)                # the opt-in of L(0, 0), each way
    assert any(c[2] % 4 for c in runtime) and any(c[2] % 16 and not c[2] % 4 for c in runtime)
    assert any(c[3] == 32 for c in runtime) and any(c[4] not in (1, 5) for c in runtime)
    for c in cases:
        n, _, mid, V, _, E = c
        assert C.supported(n, mid, V, 32, E, 0) and C.supported(n, mid, V, 32, E, 1), c
    for c in C.LIMIT_CASES:
        n, _, mid, V, _, E = c
        assert C.LDS_MAX - 4096 <= C.launch_lds(c)[1] <= C.LDS_MAX, c
        assert not C.supported(n, mid + 1, V, 32, E, 1), c


def test_inputs_for_any_graph():
    for case in C.RUNTIME_CASES:
        n, Ci, mid, V, P, E = case
        t, nt, et = C.dyn_inputs(*case, seed=C.case_seed(case))
        assert nt.dtype == et.dtype == torch.int32 and nt.tolist() == [v % P for v in range(V)] and et.shape == (V, V)
        assert 0 <= int(et.min()) and int(et.max()) < E
        if V * V >= E:
            assert len(set(et.flatten().tolist())) == E, case
        assert list(t) == ['xbar', 'A', 'alpha', 'beta', 'w1', 'b1', 'w2', 'b2', 'wse', 'bse', 'we', 'be']
        assert t['xbar'].shape == (n, Ci, V) and t['wse'].shape == (mid * P, Ci) and t['we'].shape == (E * mid, mid)


def _statement(case, dt):
    n, _, mid, V, _, _ = case
    t, nt, et = C.dyn_inputs(*case, seed=C.case_seed(case))
    tt = {k: v.to(dt).requires_grad_() for k, v in t.items()}
    out = torch_ops.dynadj(*tt.values(), nt, et)
    out.backward(C.dyn_cotangent(n, mid, V).to(dt))
    return out.detach(), {k: v.grad for k, v in tt.items()}


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


@pytest.mark.parametrize('case', C.RUNTIME_CASES, ids=C.case_id)
def test_bars_test_the_kernel_not_the_inputs(case):
    """The statement itself in fp32 against fp64, on the host: an input set under which plain fp32 arithmetic already
    spends the bar would make the GPU comparison a test of the inputs.  Measured with these seeds: forward <= 2.3e-7,
    gradients <= 2.7e-6 (beta at mid = 37)."""
    o32, g32 = _statement(case, torch.float32)
    o64, g64 = _statement(case, torch.float64)
    errs = {k: _rel(g32[k], g64[k]) for k in g64}
    worst = max(errs, key=errs.get)
    print(f'{C.case_id(case)}: fp32 statement forward {_rel(o32, o64):.2e}, worst gradient {worst} {errs[worst]:.2e}')
    assert _rel(o32, o64) <= FWD_BAR / 5
    assert errs[worst] <= GRAD_BAR / 5, (worst, errs[worst])


def test_forward_only_cases_same_condition():
    """8 samples of each forward-only case (the statement is per sample): fp32 against fp64 within a fifth of the bar."""
    for case in C.FORWARD_CASES:
        n, Ci, mid, V, P, E = case
        assert n > 128 and C.supported(n, mid, V, 32, E, 0) and not C.supported(n, mid, V, 32, E, 1)
        t, nt, et = C.dyn_inputs(*case, seed=C.case_seed(case))
        t['xbar'] = t['xbar'][:8]
        with torch.no_grad():
            o32 = torch_ops.dynadj(*t.values(), nt, et)
            o64 = torch_ops.dynadj(*[v.double() for v in t.values()], nt, et)
        assert _rel(o32, o64) <= FWD_BAR / 5, (case, _rel(o32, o64))
    assert [C.fwd_windows(*c[:1], c[2], c[3], c[5]) for c in C.FORWARD_CASES] == [1, 2]


def test_host_chunks_of_the_diagnosis_add_up():
    """check_dynadj's failure path (never taken by a passing run): the chunked host evaluation equals the statement in one
    piece, and the message carries the three comparisons."""
    from test_kernels_gpu import _dyn_diagnosis, _dyn_host_chunks
    case = (37, 8, 5, 11, 3, 7)
    n, _, mid, V, _, _ = case
    t, nt, et = C.dyn_inputs(*case, seed=3)
    dah = C.dyn_cotangent(n, mid, V)
    got = _dyn_host_chunks(t, nt, et, dah, list(t), True, chunk=16)
    tt = {k: v.double().requires_grad_() for k, v in t.items()}
    torch_ops.dynadj(*tt.values(), nt, et).backward(dah.double())
    for k, v in tt.items():
        assert _rel(got[k], v.grad) < 1e-13, k
    assert all(not v.requires_grad for v in t.values())
    assert _dyn_diagnosis('alpha', got['alpha'], got['alpha'], 16, None) == ()
    msg = _dyn_diagnosis('alpha', got['alpha'] * (1 + 1e-3), got['alpha'], 64, lambda: got)
    assert [m.split(' ')[0] for m in msg] == ['rel(kernel,', 'rel(gpu_ref,', 'rel(kernel,'] and '0.000e+00' in msg[1]


def _wide_unit():
    g = D.Graph(layout='nturgb+d', mode='spatial')
    torch.manual_seed(0)
    m = D.dgphgcn1(256, 256, graph_A(25), torch.tensor(g.edge_type), torch.tensor(g.node_type), ratio=0.25, decompose=True,
                   node_attention=True, edge_attention=True, subset_wise=True)
    assert m._shipped and m.mid_channels == 64
    return m


def test_untrainable_width_raises_in_forward_not_in_autograd():
    """ratio = 0.25 (the constructor default) at 256 channels is mid = 64: K-B's forward holds it, its backward does not."""
    m = _wide_unit().train()
    x = torch.randn(2, 256, 4, 25)
    with D.kernels.use_ops(torch_ops):
        with pytest.raises(NotImplementedError, match=r'mid = 64 at V = 25 joints, E = 15 .*mid <= 37'):
            m.forward_deferred(x)
        with torch.no_grad():
            y = m.forward_deferred(x)
        assert y.x1.shape == (2, 256, 4, 25)
        for p in m.parameters():
            p.requires_grad_(False)
        m.forward_deferred(x)                   # nothing to differentiate: nothing is refused
        with pytest.raises(NotImplementedError, match='dgphgcn1'):
            m.forward_deferred(x.requires_grad_())
    with pytest.raises(NotImplementedError, match='mid <= 37'):
        native.dynadj_require_backward(64, 25, 15)
    native.dynadj_require_backward(37, 25, 15)
    native.dynadj_require_backward(32, 25, 15, ld=25)


def test_shipped_width_is_not_refused():
    g = D.Graph(layout='nturgb+d', mode='spatial')
    m = D.dgphgcn1(64, 64, graph_A(25), torch.tensor(g.edge_type), torch.tensor(g.node_type), ratio=0.125, decompose=True,
                   node_attention=True, edge_attention=True, subset_wise=True).train()
    with D.kernels.use_ops(torch_ops):
        m.forward_deferred(torch.randn(2, 64, 4, 25)).x1.sum().backward()
    assert m._kb_trains is True


def test_return_codes_without_a_device():
    """Both launches ask the predicate before anything else that depends on the shape."""
    lib = native.lib()
    one = 1                                                                     # any non-NULL address
    for mid, V, ld in [(8, 33, 40), (65, 25, 32), (8, 25, 24), (64, 25, 32)]:
        assert lib.dsgcn_dynadj_bwd(*[one] * 11, 10 ** 6, 2, mid, V, ld, 5, 15, None) == EUNSUPPORTED, (mid, V, ld)
    for mid, V, ld in [(8, 33, 40), (65, 25, 32), (8, 25, 24)]:
        assert lib.dsgcn_dynadj_fwd(*[one] * 9, 2, mid, V, ld, 5, 15, None) == EUNSUPPORTED, (mid, V, ld)
    stride = lib.dsgcn_dynadj_partial_stride(8, 25, 15)
    assert stride == 3 * 625 + 6 + 15 * 64 + 15 * 8
    assert lib.dsgcn_dynadj_bwd(*[one] * 11, stride - 1, 2, 8, 25, 32, 5, 15, None) == -1
    assert lib.dsgcn_dynadj_bwd(*[one] * 11, stride, 0, 8, 25, 32, 5, 15, None) == -1
    assert lib.dsgcn_dynadj_fwd(*[one] * 9, 0, 8, 25, 32, 5, 15, None) == -1
