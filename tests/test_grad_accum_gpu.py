"""-m gpu: gradient accumulation on the device (csrc/accum.hip: dsgcn_grad_accum + dsgcn_grad_accum_finish) against the
numpy statement of the same fp32 operations, and TrainEngine(accumulate=k) eagerly and as replayed hipGraphs, against the
host statement, with clipping, and at k = 1."""
import functools

import numpy as np
import pytest
import torch

import dsgcn_amd as D
from dsgcn_amd import native
from grad_accum_fp64 import SGD, accum_ref, finish_ref, flat_of, grouped, host_statement, micro_batches, reduced_model, running_stats

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PAD = 8                                        # sentinel floats on either side of a buffer
SENTINEL = -12345.0
SIZES = [1, 3, 4, 1023, 4099]                  # below one vector, exactly one, a ragged block, more than one workgroup + tail
GRAD_REL_L2 = 2e-4                             # test_model_gpu.py::test_reduced_model_vs_golden: whole gradient, relative L2


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _case(n):
    gen = torch.Generator().manual_seed(500 + n)
    return torch.randn(n, generator=gen).numpy(), torch.randn(n, generator=gen).numpy(), torch.randn(n, generator=gen).numpy()


def _padded(values, offset):
    """values inside a sentinel-filled device buffer, starting ``offset`` floats past a 16-byte boundary -> (buffer, view)."""
    n = len(values)
    buf = torch.full((PAD + offset + n + PAD,), SENTINEL, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[PAD + offset:PAD + offset + n]
    view.copy_(torch.from_numpy(values))
    return buf, view


def _outside_untouched(buf, offset, n):
    return bool((buf[:PAD + offset] == SENTINEL).all()) and bool((buf[PAD + offset + n:] == SENTINEL).all())


@pytest.mark.parametrize('offsets', [(0, 0), (1, 1), (1, 0)])     # aligned; misaligned head; no common boundary (all scalar)
@pytest.mark.parametrize('n', SIZES)
def test_kernels_equal_the_fp32_statement(n, offsets):
    """acc += g twice, then finish with every factor: the results are the fp32 roundings of the same operations (exactly
    rounded adds and multiplies: equality), acc is zero after finish, nothing outside [0, n) is written."""
    lib = native.lib()
    a_h, g1_h, g2_h = _case(n)
    oa, og = offsets
    for factor in (1.0, 1.0 / 3.0, 1.0 / 8.0):
        abuf, acc = _padded(a_h, oa)
        gbuf, g = _padded(g1_h, og)
        assert acc.data_ptr() % 16 == 4 * oa and g.data_ptr() % 16 == 4 * og
        f = torch.full((1,), factor, device=DEV)
        assert lib.dsgcn_grad_accum(acc.data_ptr(), g.data_ptr(), n, _stream()) == 0
        want_acc = accum_ref(a_h, g1_h)
        assert np.array_equal(acc.cpu().numpy(), want_acc)
        assert np.array_equal(g.cpu().numpy(), g1_h)                          # a micro-iteration only reads g
        g.copy_(torch.from_numpy(g2_h))
        assert lib.dsgcn_grad_accum_finish(acc.data_ptr(), g.data_ptr(), f.data_ptr(), n, _stream()) == 0
        assert np.array_equal(g.cpu().numpy(), finish_ref(want_acc, g2_h, factor))
        assert not acc.any()
        assert _outside_untouched(abuf, oa, n) and _outside_untouched(gbuf, og, n)
        assert float(f) == float(np.float32(factor))


def test_kernels_at_the_flat_size_twice():
    """The DS-STGCN flat size (grid-stride rounds, whole chunks and a ragged one): equal to the statement, and to itself."""
    n = 1376950
    gen = torch.Generator().manual_seed(9)
    a_h, g_h = torch.randn(n, generator=gen).numpy(), torch.randn(n, generator=gen).numpy()
    f = torch.full((1,), 1.0 / 8.0, device=DEV)
    runs = []
    for _ in range(2):
        acc, g = torch.from_numpy(a_h).to(DEV), torch.from_numpy(g_h).to(DEV)
        assert native.lib().dsgcn_grad_accum(acc.data_ptr(), g.data_ptr(), n, _stream()) == 0
        mid = acc.cpu().numpy()
        assert native.lib().dsgcn_grad_accum_finish(acc.data_ptr(), g.data_ptr(), f.data_ptr(), n, _stream()) == 0
        assert not acc.any()
        runs.append((mid, g.cpu().numpy()))
    want = accum_ref(a_h, g_h)
    assert np.array_equal(runs[0][0], want) and np.array_equal(runs[0][1], finish_ref(want, g_h, 1.0 / 8.0))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


# ---- through the engine -------------------------------------------------------------------------------------------------

def _engine_run(n_iters, k, tail=True, lrs=None, **engine_kw):
    """The reduced DS-STGCN on ``n_iters`` different 2-clip micro-batches, flush for what is left over."""
    eng = D.TrainEngine(reduced_model().cuda(), warmup_eager=1, **dict(SGD, **engine_kw), **({} if k is None else dict(accumulate=k)))
    logs = []
    for i, (kp, lb) in enumerate(micro_batches(n_iters)):
        out = eng.step(kp.cuda(), lb.cuda(), lr=None if lrs is None else lrs[i])
        logs.append({name: v.clone() for name, v in out.items()})
    if tail and k not in (None, 1) and eng.pending:
        logs.append(eng.flush(eng.pending))
    torch.cuda.synchronize()
    return eng, logs


def _state(eng):
    return dict(p=eng.flat.flat_p.cpu(), buf=eng.opt.buf.cpu(), g=eng.flat.flat_g.cpu(), **running_stats(eng.model))


def test_engine_graphed_equals_eager_and_itself():
    """k = 3, two full groups and a tail of one: calls 2, 4, 5, 7 replay the micro-iteration's graph, call 6 the stepping
    one (each captured after one eager call of its kind).  Parameters, momentum, the last averaged gradient and every
    running statistic: the same bits eagerly, graphed, and graphed again."""
    kp, lb = micro_batches(7)[0]
    ea, la = _engine_run(7, 3, use_graph=False)
    eb, lb_ = _engine_run(7, 3, use_graph=True)
    ec, _ = _engine_run(7, 3, use_graph=True)
    assert eb.capture_error is None and eb.graphed(kp.cuda(), lb.cuda()) and not ea.graphed(kp.cuda(), lb.cuda())
    assert ea.iter == eb.iter == 7 and ea.pending == eb.pending == 0
    sa, sb, sc = _state(ea), _state(eb), _state(ec)
    for name in sa:
        assert torch.equal(sa[name], sb[name]) and torch.equal(sb[name], sc[name]), name
    assert [float(l['loss']) for l in la[:7]] == [float(l['loss']) for l in lb_[:7]]
    assert not ea.opt.acc.any() and not eb.opt.acc.any()


def test_engine_equals_the_host_statement():
    """k = 2 on the two micro-batches of the host test: the averaged gradient and the momentum buffer (= the gradient plus
    the weight decay after a first step) against the CPU statement at test_model_gpu.py's bound for this model's gradient;
    one update moved every parameter accordingly."""
    want = host_statement(micro_batches(2), [[0, 1]])
    for graph in (False, True):
        eng, _ = _engine_run(2, 2, use_graph=graph)
        for got, ref in ((eng.flat.flat_g, want['mean']), (eng.opt.buf, want['buf']), (eng.flat.flat_p, want['p'])):
            ref = flat_of(eng, ref)
            err = float((got.double().cpu() - ref).norm() / ref.norm())
            print('graph', graph, 'relative L2', err)
            assert err < GRAD_REL_L2


def test_engine_clips_the_averaged_gradient():
    """grad_clip with k = 3: the logged grad_norm is the norm of mean(g1, g2, g3), computed in fp64 from the micro-gradients
    of an eager engine that never moves its weights (rate 0), within 2 ulp (test_grad_clip_gpu.py's bound for the stored
    norm; the fp32 factor 1/3 adds 3e-8 relative, the three roundings per element average out); the flat buffer then
    holds that mean times the coefficient."""
    k, max_norm = 3, 1e-3
    probe = D.TrainEngine(reduced_model().cuda(), use_graph=False, **dict(SGD, lr=0.0))
    micro = []
    for kp, lb in micro_batches(k):
        probe.step(kp.cuda(), lb.cuda())
        micro.append(probe.flat.flat_g.double().cpu().numpy())
    mean64 = sum(micro) / k
    total = float(np.sqrt(np.sum(mean64 ** 2)))
    for graph in (False, True):
        eng, logs = _engine_run(2 * k if graph else k, k, use_graph=graph, grad_clip=dict(max_norm=max_norm))
        norms = [float(l['grad_norm']) for l in logs]
        ulp = float(np.spacing(np.float32(total)))
        print('graph', graph, 'grad_norm', norms, 'fp64', total, 'ulps', abs(norms[k - 1] - total) / ulp)
        assert norms[0] == norms[1] == 0.0 and total > max_norm              # refreshed by the update only
        assert abs(norms[k - 1] - total) <= 2 * ulp
        if graph:
            assert norms[k] == norms[k + 1] == norms[k - 1] and norms[2 * k - 1] != norms[k - 1]
            continue
        coef = max_norm / (total + 1e-6)
        got = eng.flat.flat_g.double().cpu().numpy()
        # three roundings per element, each below 2^-24 of sum |g_i| / k, and the coefficient's: 1e-6 is ample
        bound = 1e-6 * coef * sum(np.abs(g) for g in micro) / k
        assert np.all(np.abs(got - mean64 * coef) <= bound)
        assert float(np.sqrt(np.sum(got ** 2))) == pytest.approx(max_norm, rel=1e-3)


@pytest.mark.parametrize('graph', [False, True])
def test_accumulate_one_is_the_engine_without_the_argument(graph):
    ea, la = _engine_run(3, 1, use_graph=graph)
    eb, lb = _engine_run(3, None, use_graph=graph)
    assert ea.opt.acc is None and ea.opt.acc_factor is None and ea.accumulate == 1
    sa, sb = _state(ea), _state(eb)
    for name in sa:
        assert torch.equal(sa[name], sb[name]), name
    assert [float(l['loss']) for l in la] == [float(l['loss']) for l in lb]
    assert set(ea._graphs) == set(eb._graphs)                                 # the same captures under the same keys
