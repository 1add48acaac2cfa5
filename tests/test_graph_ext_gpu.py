"""GPU: the per-video learned adjacency at test time (``test_cfg['graph_ext']``): the pooling kernel (csrc/graphpool.hip)
against the fp64 mean of its own fp32 input, the taps of every unit type and the reduced model against fp64 statements,
InferEngine replays, ``test_model``.

Bars.  Kernel: elementwise ``|got - ref| <= R * 2^-24 * mean|a|`` with R = clips * M * mid values per mean — the fp32
summation bound for ANY order ((R - 1) u sum|a| before the division by R) plus the one rounding of the result
(u |mean| <= u sum|a| / R), u = 2^-24.  Units and model: relative L2 <= 2e-6, the project's K-B forward bar."""
import numpy as np
import pytest
import torch

import dggcn_plain_fp64 as P64
import dsgcn_amd as D
import graph_ext_ops as G
from dsgcn_amd import kernels as K
from test_graph_ext_host import graph_pool_argument_checks

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# (videos, clips, M, K, mid, V)
KERNEL_CASES = [(2, 3, 1, 3, 5, 17), (1, 2, 2, 8, 1, 25), (3, 1, 2, 3, 32, 25), (1, 10, 2, 3, 64, 32), (5, 1, 1, 16, 3, 32)]
_inputs = {}


def _ahat(case):
    """A real Ahat (videos*clips*M, K*mid, V, V), fp32, from the statement of the plain adjacency (any K, any V): A + alpha
    tanh(D) + beta softmax with alpha, beta ~ N(0, 0.5^2) of either sign — computed once per case, never written to."""
    if case not in _inputs:
        videos, clips, M, Ks, mid, V = case
        g = torch.Generator().manual_seed(1000 + KERNEL_CASES.index(case))
        n, Ci = videos * clips * M, 8
        r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
        a = P64.adjacency(r(n, Ci, V), r(Ks, V, V) * 0.1, r(Ks) * 0.5, r(Ks) * 0.5, r(Ks * mid, Ci) * 0.5, r(Ks * mid) * 0.1,
                          r(Ks * mid, Ci) * 0.5, r(Ks * mid) * 0.1)
        assert a.dtype == torch.float32 and bool((a < 0).any()) and bool((a > 0).any())
        _inputs[case] = a.contiguous()
    return _inputs[case]


def _reference(a, group, Ks):
    """fp64 mean of the fp32 input and the elementwise bound R * 2^-24 * mean|a|"""
    n, KM, V, _ = a.shape
    a6 = a.double().reshape(n // group, group, Ks, KM // Ks, V, V)
    R = group * (KM // Ks)
    return a6.mean((1, 3)), R * 2.0 ** -24 * a6.abs().mean((1, 3))


@pytest.mark.parametrize('case', KERNEL_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_kernel_against_the_fp64_mean_of_its_input(case):
    videos, clips, M, Ks, mid, V = case
    group = clips * M
    a = _ahat(case)
    ref, bound = _reference(a, group, Ks)
    assert float(bound.min()) > 0                                   # mixed-sign inputs: the bound is nowhere vacuous
    ad = a.to(DEV)
    L, layer = 3, 1
    out = torch.full((videos, L, Ks, V, V), -123.0, device=DEV)
    K.graph_pool(ad, group, Ks, out, layer)
    torch.cuda.synchronize()
    got = out[:, layer].double().cpu()
    err = (got - ref).abs()
    worst = float((err / bound).max())
    splits = K.native.lib().dsgcn_graph_pool_splits(videos, group, Ks, mid, V)
    print(f'graph_pool {case}: splits {splits}, max |err| / bound = {worst:.3f}, max |err| = {float(err.max()):.3e}')
    assert bool((err <= bound).all()), worst
    # only the layer's slice of the sentinel-filled buffer is written
    assert bool((out[:, 0] == -123.0).all()) and bool((out[:, 2] == -123.0).all())
    # a second run gives the same bits
    out2 = torch.full_like(out, 5.0)
    K.graph_pool(ad, group, Ks, out2, layer)
    assert torch.equal(out2[:, layer], out[:, layer])
    # the input at an odd float offset (4-byte, not 16-byte aligned), the output too
    flat = torch.empty(a.numel() + 1, device=DEV)
    shifted = flat[1:].view(a.shape)
    shifted.copy_(ad)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    oflat = torch.full((out.numel() + 3,), -123.0, device=DEV)
    out3 = oflat[3:].view(out.shape)
    K.graph_pool(shifted, group, Ks, out3, layer)
    assert torch.equal(out3[:, layer], out[:, layer])
    assert bool((oflat[:3] == -123.0).all()) and bool((out3[:, 0] == -123.0).all()) and bool((out3[:, 2] == -123.0).all())
    assert torch.equal(ad.cpu(), a)                                 # the input is read, never written


def test_both_launch_forms_are_among_the_cases():
    s = K.native.lib().dsgcn_graph_pool_splits
    forms = {s(v, c * m, k, mid, V) == 1 for v, c, m, k, mid, V in KERNEL_CASES}
    assert forms == {True, False}


def test_argument_checks_on_the_gpu():
    graph_pool_argument_checks()
    a = torch.zeros(6, 12, 25, 25, device=DEV)
    out = torch.zeros(2, 2, 3, 25, 25, device=DEV)
    for bad in (dict(group=4), dict(K=5), dict(layer=2), dict(layer=-1)):
        kw = dict(group=3, K=3, layer=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            K.graph_pool(a, kw['group'], kw['K'], out, kw['layer'])
    with pytest.raises(ValueError):
        K.graph_pool(a.transpose(2, 3), 3, 3, out, 0)               # it reads ahat where it lies: no silent copy
    with pytest.raises(ValueError):
        K.graph_pool(a, 3, 3, out.double(), 0)
    with pytest.raises(RuntimeError):
        K.graph_pool(a.cpu(), 3, 3, out, 0)
    assert not out.any()


def test_capturable_in_a_graph():
    """No allocation outside the caching allocator, no synchronisation: the two-launch form replays."""
    case = KERNEL_CASES[2]
    videos, clips, M, Ks, mid, V = case
    a = _ahat(case).to(DEV)
    eager = torch.zeros(videos, 1, Ks, V, V, device=DEV)
    K.graph_pool(a, clips * M, Ks, eager, 0)
    sa = a.clone()
    out = torch.zeros_like(eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode='thread_local'):
        K.graph_pool(sa, clips * M, Ks, out, 0)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ---- units ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V', [25, 17])
@pytest.mark.parametrize('kind', G.UNIT_KINDS)
def test_unit_taps_against_fp64(kind, V):
    u = G.make_unit(kind, V).to(DEV)
    Ks = u.num_subsets
    x = torch.randn(6, 32, 4, V, generator=torch.Generator().manual_seed(3)).to(DEV)       # 2 videos x 3 person-samples
    with torch.no_grad():
        y0 = u(x)
        for mode in ('ahat', 'ctr'):
            out = torch.full((2, 1, Ks, V, V), 9.0, device=DEV)
            with K.graph_collect(3, mode, out) as col:
                y = u(x)
            assert col.layer == 1
            assert torch.equal(y, y0)                               # the layer's own Ahat and output: the same bits
            want = G.pool64(G.unit_graph64(u, x.double().mean(2), mode), 3, Ks)
            rel = G.rel_l2(out[:, 0], want)
            print(f'{kind} V={V} {mode}: relative L2 {rel:.3e}')
            assert rel <= G.MODEL_BAR, (kind, V, mode, rel)
        assert torch.equal(u(x), y0)


# ---- the model ----------------------------------------------------------------------------------------------------------
_model_cache = {}


def _model():
    if 'm' not in _model_cache:
        _model_cache['m'] = G.fixture_model('ctr').to(DEV)
        _model_cache['x'] = G.fixture()['x'].to(DEV)
    m = _model_cache['m']
    m.test_cfg['graph_ext'] = 'ctr'
    return m, _model_cache['x']


def test_model_against_the_fixture_fp64():
    m, x = _model()
    got = m.forward_graphs(x)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 4, 3, 25, 25)
    rel = G.layer_rel(got, G.fixture()['g64'])
    print('model, ctr: per-layer relative L2 vs the reference fp64:', ['%.2e' % r for r in rel])
    assert max(rel) <= G.MODEL_BAR, rel
    one = m(keypoint=x[1:2], return_loss=False)
    assert isinstance(one, np.ndarray) and one.dtype == np.float32 and one.shape == (4, 3, 25, 25)
    assert G.rel_l2(one, got[1]) <= G.MODEL_BAR                     # every video is pooled by itself
    assert not m.training
    m.train()
    m.forward_graphs(x)
    assert m.training                                               # put to eval for the call only
    m.eval()


def test_ahat_mode_adds_the_softmax_term():
    m, x = _model()
    ctr = m.forward_graphs(x)
    m.test_cfg['graph_ext'] = 'ahat'
    ahat = m.forward_graphs(x)
    for layer, u in enumerate(m.graph_units()):
        cols = (ahat[:, layer].double() - ctr[:, layer].double()).sum(-2)
        assert torch.allclose(cols, u.beta.detach().double().view(1, 3, 1).expand_as(cols), atol=2e-5), layer


def test_engine_replay_equals_eager_and_scores_are_untouched():
    m, x = _model()
    eng = D.InferEngine(m, warmup_eager=1, strict_graph=True)
    m.test_cfg['graph_ext'] = False
    scores = [eng(x) for _ in range(3)]                             # eager, captured + replayed, replayed
    assert eng.replays == 2 and torch.equal(scores[0], scores[1]) and torch.equal(scores[0], scores[2])
    assert tuple(scores[0].shape) == (2, 12)
    for mode in ('ctr', 'ahat'):
        m.test_cfg['graph_ext'] = mode
        before = eng.replays
        graphs = [eng(x) for _ in range(3)]
        assert eng.capture_error is None and eng.graphed(x) and eng.replays == before + 2
        assert tuple(graphs[0].shape) == (2, 4, 3, 25, 25) and graphs[0].dtype == torch.float32 and graphs[0].is_cuda
        assert torch.equal(graphs[0], graphs[1]) and torch.equal(graphs[0], graphs[2])
        assert torch.equal(graphs[0], m.forward_graphs(x))
    m.test_cfg['graph_ext'] = 'ctr'
    assert not torch.equal(eng(x), graphs[0])                       # (graphs: 'ahat' by now) a captured graph per mode
    m.test_cfg['graph_ext'] = False
    after = eng(x)
    assert torch.equal(after, scores[0])                            # a scoring pass after the graph passes: the same bits
    assert len(eng._graphs) == 3
    # chunks of whole videos
    m.test_cfg['graph_ext'] = 'ctr'
    cut = D.InferEngine(m, use_graph=False, max_views=3)(x)
    assert tuple(cut.shape) == (2, 4, 3, 25, 25) and max(G.layer_rel(cut, G.fixture()['g64'])) <= G.MODEL_BAR


def test_test_model_returns_one_graph_stack_per_video(tmp_path):
    m, x = _model()
    g = torch.Generator().manual_seed(8)
    vids = torch.cat([x.cpu(), x.cpu()[:1] + 0.3 * torch.randn(3, 3, 2, 16, 25, 3, generator=g)])          # 5 videos
    labels = [0, 2, 0, 3, 2]
    data = [dict(keypoint=vids[i].numpy(), label=labels[i]) for i in range(5)]
    cfg = D.Config(dict(data=dict(test_dataloader=dict(videos_per_gpu=2)), work_dir=str(tmp_path)))
    out = str(tmp_path / 'graphs.pkl')
    res = D.test_model(m, data, cfg, out=out, metrics=('graph',))
    assert len(res['results']) == 5
    back = D.load_results(out)
    for i, (a, b) in enumerate(zip(res['results'], back)):
        assert a.dtype == b.dtype == np.float32 and a.shape == b.shape == (4, 3, 25, 25) and np.array_equal(a, b)
        want = m(keypoint=vids[i:i + 1].to(DEV), return_loss=False)
        assert G.rel_l2(a, want) <= G.MODEL_BAR, i
    assert G.rel_l2(np.stack(res['results'][:2]), G.fixture()['g64']) <= G.MODEL_BAR
    graphs = res['metrics']['graph']
    want = D.class_mean_graphs(res['results'], labels)
    assert list(res['metrics']) == ['graph'] and len(graphs) == 3           # classes 0, 1, 2; the last class (3) is left out
    assert np.isnan(graphs[1]).all()                                        # class 1 has no video
    for a, b in zip(graphs, want):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.allclose(graphs[0], (res['results'][0] + res['results'][2]) / 2, atol=1e-7)
    assert D.test_model(m, data, cfg)['metrics'] is None                    # the default metrics: nothing to rate
    with pytest.raises(ValueError, match='pkl'):
        D.test_model(m, data, cfg, out=str(tmp_path / 'graphs.json'))
