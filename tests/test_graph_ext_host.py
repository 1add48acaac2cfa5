"""CPU: the host side of the per-video learned adjacency at test time (``test_cfg['graph_ext']``): what the recognizer and
the engines accept and reject, one tap per unit and none without a collector, the fp32 statement of the whole chain
against the reference's fp64 (tests/golden/graph_ext.npz), ``class_mean_graphs`` with the reference loop's quirks, the
new entry point's declaration, binding, argument checks and code objects, the result files.  No GPU."""
import copy
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import dsgcn_amd as D
import graph_ext_ops as G
from dsgcn_amd import kernels as K
from dsgcn_amd import kernels_infer, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')


def _cfg(**test_cfg):
    cfg = copy.deepcopy(G.fixture()['cfg'])
    cfg['test_cfg'] = test_cfg
    return cfg


def _other_cfg(name):
    import json
    with open(os.path.join(GOLD, name + '_cfg.json')) as f:
        cfg = json.load(f)
    if 'tcn_ms_cfg' in cfg['backbone']:
        cfg['backbone']['tcn_ms_cfg'] = [tuple(c) if isinstance(c, list) else c for c in cfg['backbone']['tcn_ms_cfg']]
    return cfg


# ---- parsing and rejections ---------------------------------------------------------------------------------------------
def test_parse_graph_ext():
    assert K.parse_graph_ext(False) is None and K.parse_graph_ext(None) is None
    assert K.parse_graph_ext(True) == 'ctr' and K.parse_graph_ext('ctr') == 'ctr' and K.parse_graph_ext('ahat') == 'ahat'
    for bad in ('CTR', 'all', '', 1, 0, 2, 'true', ('ctr',)):
        with pytest.raises(ValueError, match='graph_ext'):
            K.parse_graph_ext(bad)


def test_recognizer_accepts_the_key():
    for value, mode in ((True, 'ctr'), ('ctr', 'ctr'), ('ahat', 'ahat'), (False, None)):
        m = D.build_model(_cfg(graph_ext=value))
        assert m.graph_extraction() == mode
        assert m.extraction() is None
        assert len(m.graph_units()) == 4
    m = D.build_model(_cfg())
    assert m.graph_extraction() is None and m.extraction() is None
    m.test_cfg['graph_ext'] = 'ahat'                              # read at every call, like the extraction keys
    assert m.graph_extraction() == 'ahat'


@pytest.mark.parametrize('bad', ['both', 1, 'Ahat', ['ctr']])
def test_recognizer_rejects_other_values(bad):
    with pytest.raises(ValueError, match='graph_ext'):
        D.build_model(_cfg(graph_ext=bad))


@pytest.mark.parametrize('key', ['feat_ext', 'score_ext'])
def test_graph_ext_does_not_go_with_extraction(key):
    with pytest.raises(ValueError, match='graph_ext'):
        D.build_model(_cfg(graph_ext=True, **{key: True, 'pool_opt': 'nm'}))
    m = D.build_model(_cfg(graph_ext='ahat'))
    m.test_cfg[key] = True
    m.test_cfg['pool_opt'] = 'nm'
    with pytest.raises(ValueError, match='graph_ext'):
        m.graph_extraction()


@pytest.mark.parametrize('name,backbone', [('model_reduced_stgcn', 'STGCN'), ('model_reduced_ctrgcn', 'CTRGCN'),
                                           ('model_reduced_aagcn', 'AAGCN')])
def test_backbones_without_dynamic_adjacency_raise(name, backbone):
    cfg = _other_cfg(name)
    cfg['test_cfg'] = dict(graph_ext=True)
    with pytest.raises(ValueError, match=backbone):
        D.build_model(cfg)
    cfg['test_cfg'] = dict(graph_ext=False)
    assert D.build_model(cfg).graph_extraction() is None


def test_extraction_is_unchanged():
    assert D.build_model(_cfg()).extraction() is None
    assert D.build_model(_cfg(feat_ext=True, pool_opt='nm')).extraction() == ('feat', 3)
    assert D.build_model(_cfg(score_ext=True)).extraction() == ('score', 15)
    assert D.build_model(_cfg(score_ext=True, feat_ext=True, pool_opt='none')).extraction() == ('score', 0)
    assert D.build_model(_cfg(graph_ext=False, feat_ext=True, pool_opt='tv')).extraction() == ('feat', 12)


def test_ensemble_engine_rejects_graph_ext():
    m = D.build_model(_cfg(graph_ext=True))
    with pytest.raises(ValueError, match='graph_ext'):
        D.EnsembleEngine([m], [1.0])


def test_test_model_rejects_before_the_pass(tmp_path):
    data = [dict(keypoint=None, label=0)] * 2
    m = D.build_model(_cfg(graph_ext=True))
    with pytest.raises(ValueError, match='pkl'):
        D.test_model(m, data, D.Config(dict()), out=str(tmp_path / 'graphs.json'), device='no such device')
    with pytest.raises(ValueError, match='graph'):
        D.test_model(m, data, D.Config(dict()), metrics=('graph', 'top_k_accuracy'), device='no such device')
    with pytest.raises(ValueError, match='graph'):
        D.test_model(m, data, D.Config(dict()), metrics=('confusion_matrix',), device='no such device')
    with pytest.raises(ValueError, match='graph_ext'):
        D.test_model(D.build_model(_cfg()), data, D.Config(dict()), metrics=('graph',), device='no such device')
    assert not list(tmp_path.iterdir())


# ---- the collector ------------------------------------------------------------------------------------------------------
def test_collector_needs_no_grad_and_eval():
    out = torch.zeros(1, 1, 3, 25, 25)
    with pytest.raises(RuntimeError, match='no_grad'):
        with K.graph_collect(1, 'ctr', out):
            pass
    with torch.no_grad():
        with pytest.raises(ValueError, match='mode'):
            with K.graph_collect(1, 'tanh', out):
                pass
        u = G.make_unit('dghgcn', 25).train()
        with K.use_ops(G.cpu_ops()), pytest.raises(RuntimeError, match='eval'):
            with K.graph_collect(1, 'ahat', out):
                u(torch.randn(1, 32, 4, 25))
        with K.graph_collect(1, 'ahat', out):                          # the failed collection was closed
            with pytest.raises(RuntimeError, match='already'):
                with K.graph_collect(1, 'ahat', out):
                    pass
    assert kernels_infer._graph is None


@pytest.mark.parametrize('V', [25, 17])
@pytest.mark.parametrize('kind', G.UNIT_KINDS + ('dggcn_k3',))
def test_every_unit_taps_once(kind, V):
    if kind == 'dggcn_k3':                                             # two K-B calls and a concatenation, still one tap
        np.random.seed(2)
        torch.manual_seed(2)
        A = torch.tensor(np.asarray(D.Graph(layout=G.LAYOUTS[V], mode='random', num_filter=3, init_off=.04,
                                            init_std=.02).A), dtype=torch.float32)
        u = D.dggcn(32, 32, A, ratio=0.125, subset_wise=True).eval()
        with torch.no_grad():
            u.alpha.normal_(0, 0.5)
            u.beta.normal_(0, 0.5)
        adj_calls = 2
    else:
        u = G.make_unit(kind, V)
        adj_calls = 1
    Ks = u.num_subsets
    x = torch.randn(6, 32, 4, V, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        calls = []
        with K.use_ops(G.cpu_ops(calls)):
            y0 = u(x)
        assert 'graph_pool' not in calls and len(calls) == adj_calls                   # no collector: nothing is tapped
        for mode in ('ahat', 'ctr'):
            calls = []
            out = torch.full((2, 3, Ks, V, V), 7.0)
            with K.use_ops(G.cpu_ops(calls)), K.graph_collect(3, mode, out) as col:
                col.layer = 1
                y = u(x)
            assert calls.count('graph_pool') == 1 and col.layer == 2
            assert len(calls) - 1 == adj_calls * (2 if mode == 'ctr' else 1)           # 'ctr': one more adjacency, beta = 0
            assert torch.equal(y, y0)
            assert bool((out[:, 0] == 7).all()) and bool((out[:, 2] == 7).all())       # only its layer's slice
            want = G.pool64(G.unit_graph64(u, x.mean(2), mode), 3, Ks)
            assert G.rel_l2(out[:, 1], want) < G.MODEL_BAR / 5, (kind, V, mode)
        # a buffer with too few layers
        out = torch.zeros(2, 1, Ks, V, V)
        with K.use_ops(G.cpu_ops()), K.graph_collect(3, 'ahat', out):
            u(x)
            with pytest.raises(RuntimeError, match='one more unit'):
                u(x)


# ---- the whole chain in fp32 against the reference's fp64 ---------------------------------------------------------------
def test_fixture_shapes_and_the_reference_own_error():
    fx = G.fixture()
    assert tuple(fx['x'].shape) == (2, 3, 2, 16, 25, 3)
    assert tuple(fx['g64'].shape) == tuple(fx['g32'].shape) == (2, 4, 3, 25, 25)
    assert fx['g64'].dtype == torch.float64 and fx['g32'].dtype == torch.float32
    rel = G.layer_rel(fx['g32'], fx['g64'])
    assert np.allclose(rel, fx['ref32_rel'], rtol=1e-6) and max(rel) < 1e-7 < G.MODEL_BAR / 5
    assert (fx['g64'] < 0).any() and (fx['g64'] > 0).any()
    assert os.path.getsize(G.GOLDEN) < 1 << 20


def test_fp32_statement_of_the_chain_is_within_a_fifth_of_the_model_bar():
    """The model on the CPU namespace, fp32, against the fixture's fp64: the bar of the GPU model test (2e-6) tests the
    kernels, not the inputs."""
    fx = G.fixture()
    m = G.fixture_model('ctr')
    with K.use_ops(G.cpu_ops()):
        got = m.forward_graphs(fx['x'])
        one = m(keypoint=fx['x'][1:2], return_loss=False)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 4, 3, 25, 25)
    rel = G.layer_rel(got, fx['g64'])
    print('fp32 CPU statement, per-layer relative L2 vs the reference fp64:', ['%.2e' % r for r in rel])
    assert max(rel) <= G.MODEL_BAR / 5, rel
    assert isinstance(one, np.ndarray) and one.dtype == np.float32 and one.shape == (4, 3, 25, 25)
    # every video is pooled by itself (the CPU matmuls block differently at another batch size: not bit for bit here)
    assert G.rel_l2(one, got[1]) < 1e-6


def test_ahat_mode_adds_the_softmax_term():
    """Ahat - (A + alpha tanh(D)) = beta_k softmax_u(...): every column of a softmax sums to 1, and so does their mean."""
    fx = G.fixture()
    m = G.fixture_model('ahat')
    with K.use_ops(G.cpu_ops()):
        ahat = m.forward_graphs(fx['x'])
        m.test_cfg['graph_ext'] = True
        ctr = m.forward_graphs(fx['x'])
    for layer, u in enumerate(m.graph_units()):
        cols = (ahat[:, layer].double() - ctr[:, layer].double()).sum(-2)              # (videos, K, V)
        want = u.beta.detach().double().view(1, 3, 1).expand_as(cols)
        assert torch.allclose(cols, want, atol=2e-5), layer


# ---- class_mean_graphs ----------------------------------------------------------------------------------------------------
def test_class_mean_graphs_against_numpy_with_both_quirks():
    rng = np.random.default_rng(4)
    labels = [0, 2, 2, 5, 0, 4, 5, 2]                                # classes 1 and 3 are empty; 5 is the last class
    graphs = [rng.standard_normal((4, 3, 5, 5)).astype(np.float32) for _ in labels]
    got = D.class_mean_graphs(graphs, labels)
    assert len(got) == 5                                             # range(max(label)): class 5 is left out
    arr, lab = np.stack(graphs).astype(np.float64), np.array(labels)
    for i, g in enumerate(got):
        assert g.dtype == np.float32 and g.shape == (4, 3, 5, 5)
        if i in (1, 3):
            assert np.isnan(g).all()                                 # the mean of nothing
        else:
            assert np.allclose(g, arr[lab == i].mean(0), rtol=0, atol=1e-6)
    assert D.class_mean_graphs(graphs[:1], [0]) == []                # one class: range(0)
    assert D.class_mean_graphs(graphs, np.array(labels)[:, None])[2].shape == (4, 3, 5, 5)
    with pytest.raises(ValueError):
        D.class_mean_graphs(graphs, labels[:-1])


# ---- the entry point ------------------------------------------------------------------------------------------------------
def test_entry_point_declared_exported_and_bound():
    from test_native_abi import declared_symbols
    path = native.build()
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r' T (dsgcn_\w+)', out))
    for name in ('dsgcn_graph_pool', 'dsgcn_graph_pool_splits'):
        assert name in declared_symbols() and name in native.SIGNATURES and name in exported, name
    assert len(native.SIGNATURES['dsgcn_graph_pool']) == 11
    for name in ('graph_pool', 'graph_collect', 'graph_tap', 'parse_graph_ext'):
        assert hasattr(K, name), name


def graph_pool_argument_checks():
    """Every DSGCN_EINVAL condition include/dsgcn.h lists, and the DSGCN_EUNSUPPORTED limits; all return before any launch
    (the pointers are never dereferenced).  Shared with tests/test_graph_ext_gpu.py."""
    f = native.lib().dsgcn_graph_pool
    p = 4096
    ok = dict(ahat=p, out=p, ws=p, videos=2, group=20, K=3, mid=8, V=25, L=10, layer=0)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a['ahat'], a['out'], a['ws'], a['videos'], a['group'], a['K'], a['mid'], a['V'], a['L'], a['layer'], None)

    assert call(ahat=None) == -1 and call(out=None) == -1
    assert call(ws=None) == -1                                       # this shape splits: the partial planes need a home
    for size in ('videos', 'group', 'K', 'mid', 'V', 'L'):
        assert call(**{size: 0}) == -1 and call(**{size: -3}) == -1, size
    assert call(layer=-1) == -1 and call(layer=10) == -1
    assert call(V=33) == -2 and call(mid=65) == -2 and call(K=17) == -2
    assert call(videos=1 << 20, group=1 << 10, K=16, mid=64) == -2    # 2^40 planes
    s = native.lib().dsgcn_graph_pool_splits
    assert s(2, 20, 3, 8, 25) > 1 and s(1, 1, 3, 2, 25) == 1
    assert s(2, 0, 3, 8, 25) == -1 and s(2, 20, 3, 8, 33) == -2 and s(2, 20, 3, 65, 25) == -2


def test_argument_checks_without_gpu():
    graph_pool_argument_checks()


def test_splits_fill_the_chip_at_one_video():
    """DS-STGCN NTU-60, one video of 10 clips x 2 persons: every layer's first launch has well over one workgroup per
    (video, subset), and no workgroup gets fewer than 4 planes."""
    s = native.lib().dsgcn_graph_pool_splits
    for mid in (8, 16, 32):
        splits = s(1, 20, 3, mid, 25)
        assert 3 * splits >= 100 and 20 * mid / splits >= 4, (mid, splits)
    assert 8 * 3 * s(8, 20, 3, 32, 25) >= 1024                        # 8 videos: about 1024 workgroups


def test_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import codeobj_report
    native.build()
    ks = {k: v for k, v in codeobj_report.kernels(native.LIB_PATH).items() if k.startswith('k_graph_pool')}
    assert sorted(ks) == ['k_graph_pool', 'k_graph_pool_finish']
    for name, k in ks.items():
        assert k.get('scratch_instructions', 0) == 0 and k.get('vgpr_spill_count', 0) == 0, (name, k)
        assert k.get('sgpr_spill_count', 0) == 0 and k.get('private_segment_fixed_size', 0) == 0, (name, k)


# ---- fixture and result files -----------------------------------------------------------------------------------------------
def test_fixture_regenerates_byte_identically_live(tmp_path):
    import ref_shim
    if not ref_shim.available():
        pytest.skip('the reference checkout is not on this machine')
    subprocess.run([sys.executable, os.path.join(GOLD, 'gen_golden_graph_ext.py'), '--out', str(tmp_path)], check=True,
                   capture_output=True)
    with open(G.GOLDEN, 'rb') as f, open(tmp_path / 'graph_ext.npz', 'rb') as g:
        assert f.read() == g.read()


def test_pkl_round_trip_of_graphs(tmp_path):
    rng = np.random.default_rng(6)
    graphs = [rng.standard_normal((4, 3, 25, 25)).astype(np.float32) for _ in range(5)]
    path = D.dump_results(graphs, str(tmp_path / 'sub' / 'graphs.pkl'))
    with open(path, 'rb') as f:
        raw = pickle.load(f)
    back = D.load_results(path)
    for a, b, c in zip(graphs, raw, back):
        assert b.dtype == c.dtype == np.float32 and b.shape == c.shape == (4, 3, 25, 25)
        assert np.array_equal(a, b) and np.array_equal(a, c)
