"""-m gpu: which kernel shapes and dispatch paths do the five BASELINE training steps run, and is each of them compared with
its fp64 statement at that size?

The census runs one eager train_step + backward per BASELINE config at its bench batch, with every public op of
dsgcn_amd.kernels wrapped by a recorder (monkeypatch on the module: the model reaches the ops through kernels.ops(), which
is the module itself — use_ops() would install a proxy namespace and change dispatch, backbones.py wants_prestrided).  A
record is a key of the arguments that decide the kernel and its tiling, plus the path the library took where an op has
more than one.  FULL_SIZE_CASES must hold exactly the recorded keys: a shape or path the steps start to run and no test
covers fails the census, and so does a table entry no step runs any more.  The fp64 comparisons below are parametrized
from the same table (the per-op helpers of tests/test_kernels_gpu.py, with the bars of the tests they came from)."""
import copy
import gc
import inspect

import numpy as np
import pytest
import torch

import dsgcn_amd
from dsgcn_amd import kernels as K
from dsgcn_amd import native

pytestmark = pytest.mark.gpu
DEV = 'cuda'


# ---------------------------------------------------------------------------------------------------------------------
# keys
# ---------------------------------------------------------------------------------------------------------------------

def _mode(a1, x2, a2, relu):
    """The input mode of a virtual-input op (pwconv / tconv_bn / fuse_out): the names test_kernels_gpu.py uses."""
    if x2 is not None:
        return ('res_affine' if a2 is not None else 'res_plain') if a1 is not None else ('res_x1' if a2 is None else 'res_a2')
    if a1 is None:
        return 'relu' if relu else 'plain'
    return 'affine_relu' if relu else 'affine'


def _shape(t):
    return tuple(int(s) for s in t.shape)


def _k_aggregate(a):
    n, KC, T, V = _shape(a['zp'])
    return (n, KC, T, V, bool(a['relu']), a['ap'] is not None)


def _k_aggregate_sum(a):
    n, KC, T, V = _shape(a['p'])
    Kk = int(a['K'])
    adj = a['adj']
    form = 'shared' if adj.dim() == 3 else ('per_sample' if a['per_sample'] else
                                            ('subset_major' if adj.dim() == 5 else 'per_channel'))
    return (n, Kk, KC // Kk, T, V, form, bool(a['want_bn']))


def _k_dynadj(a):
    n, Ci, ld = _shape(a['xbar'])
    V = int(a['A'].shape[-1])
    mid = int(a['we'].shape[1])
    key = (n, Ci, mid, V, ld, a['host'] is not None)
    # single_use=False (dggcn: A feeds two calls, the parameter sums are never deferred) extends the key; the default keeps
    # the key the BASELINE steps have always recorded
    return key if a['single_use'] else key + (False,)


def _k_dynadj_typed(a):
    n, Ci, ld = _shape(a['xbar'])
    V = int(a['A'].shape[-1])
    KM = int(a['w1'].shape[0]) // int(a['P'])
    E = int(a['we'].shape[0]) // KM if a['we'] is not None else 0
    return (n, Ci, KM, V, ld, int(a['P']), E, bool(a['add_type']) and E > 0, bool(a['single_use']))


def _pw_paths(n, Ci, Co, T, V, stride, aug):
    lib = native.lib()
    fwd = 'gemm_bf16' if lib.dsgcn_pwconv_wsplit_bytes(n, Ci, Co, T, V, stride) else 'direct'
    bwd = 'bwd64' if (not aug and lib.dsgcn_pwconv_bwd_rows(n, Ci, Co, T, V, stride) > 0) else 'dgrad_wgrad'
    return fwd, bwd


def _k_pwconv(a):
    n, Ci, T, V = _shape(a['x1'])
    Co = int(a['weight'].shape[0])
    stride, aug = int(a['stride']), bool(a['aug'])
    return ((n, Ci, Co, T, V, stride, aug, _mode(a['a1'], a['x2'], a['a2'], a['relu']), bool(a['want_bn']),
             a['bias'] is not None) + _pw_paths(n, Ci, Co, T, V, stride, aug))


def _k_pwconv_group(a):
    xs, ws = a['xs'], a['ws']
    n, Ci, T, V = _shape(xs[0])
    Co = int(ws[0].shape[0])
    ok = native.lib().dsgcn_pwconv_group_ok(n, Ci, Co, T, V) == 1
    return (len(xs), n, Ci, Co, T, V, a['affs'][0] is not None, 'grouped' if ok else 'one_by_one')


def _k_ctr_topology(a):
    n, Ci, V = _shape(a['xbar'])
    Kk = int(a['A'].shape[0])
    one_conv = (bool(a['subset_major']) and K.CTR_ONE_CONV and a['beta'] is None and not a['edge'] and
                a['alpha'].numel() == 1 and Kk <= 4)
    Rr = int(a['w1'].shape[0]) // Kk
    key = (n, Ci, int(a['w4'][0].shape[0]), V, Kk, Rr, bool(a['subset_major']), 'one_conv' if one_conv else 'per_subset')
    edge = a['edge'] or {}
    if a['alpha'].numel() == 1 and a['beta'] is None and not edge:
        return key                                  # the classic unit (unit_ctrgcn)
    # unit_ctrhgcn: + (alpha elements, Gram term, edge subsets, edge classes E)
    E = {int(we.shape[0]) // Rr for we, _, _ in edge.values()}
    assert len(E) <= 1, E
    return key + ((int(a['alpha'].numel()), a['beta'] is not None, tuple(sorted(edge)), E.pop() if E else 0),)


def _k_tconv_bn(a):
    n, Ci, T, V = _shape(a['x1'])
    Co, _, KT, _ = _shape(a['weight'])
    stride = int(a['stride'])
    return (n, Ci, Co, T, V, KT, _mode(a['a1'], a['x2'], a['a2'], a['relu']), stride, bool(a['want_bn']),
            K.tconv_gemm_ok(n, Ci, Co, T, V, KT, stride))


def _k_tconv(a):
    n, Ci, T, V = _shape(a['h'])
    Co, _, KT, _ = _shape(a['weight'])
    return (n, Ci, Co, T, V, int(a['stride']), KT, int(a['dilation']), bool(a['want_bn']))


def _cfg(branch_cfg):
    return tuple(c if isinstance(c, str) else tuple(c) for c in branch_cfg)


def _k_temporal(a, path):
    n, C, T, V = _shape(a['z'])
    return (n, C, T, V, int(a['stride']), _cfg(a['branch_cfg']), tuple(int(w) for w in a['widths']), int(a['n_act']),
            bool(a['want_bn']), path)


def _k_temporal_mlp(a):
    n, C, T, V = _shape(a['z'])
    return (n, C, T, V, int(a['stride']), _cfg(a['branch_cfg']), tuple(int(w) for w in a['widths']), int(a['n_act']),
            int(a['dw_w'].shape[1]), bool(a['merge_after']), bool(a['want_bn']))


def _k_temporal_unitmlp(a):
    n, C, T, V = _shape(a['h'])
    tw = a['tw']
    return (n, C, T, V, int(a['stride']), int(a['dw_w'].shape[1]), tuple(sorted({int(d) for d in a['dw_dil'].tolist()})),
            int(tw.shape[2]) if tw is not None else 0, int(a['tdil']) if tw is not None else 0, bool(a['merge_after']),
            bool(a['want_bn']))


def _k_gram(a):
    return _shape(a['a'])


def _k_gate(a):
    return _shape(a['y']) + (int(a['mode']), int(a['rmode']))


def _k_fuse_out(a):
    n, C, T, V = _shape(a['x1'])
    tm = a['want_tmean']
    return (n, C, T, V, _mode(a['a1'], a['x2'], a['a2'], False), int(a['relu']),
            0 if not tm else (V if tm is True else int(tm)), int(a['tee']), float(a['dropout']) > 0,
            K.prestrided_fits(T, V))


def _k_fuse_out_pool(a):
    n, C, T, V = _shape(a['x1'])
    return (n, C, T, V, _mode(a['a1'], a['x2'], a['a2'], False), int(a['relu']), float(a['dropout']) > 0)


def _k_head_loss(a):
    NM, C = _shape(a['feat'])
    P = int(a['persons'])
    return (NM // P, P, C, int(a['weight'].shape[0]), a['bias'] is not None)


def _k_data_bn(a):
    N, M, T, V, C = _shape(a['x'])
    bn = a['bn']
    return (N, M, T, V, C, a['bn_type'], bn.affine)


def _k_tmean(a):
    n, C, T, V = _shape(a['x'])
    ld = a['ld']
    return (n, C, T, V, V if ld is True else int(ld))


def _k_tee3(a):
    return (_shape(a['x']),)


def _k_bn_running_update(a):
    return (len(a['items']),)


def _k_strided_frames(a):
    return (_shape(a['x']), int(a['stride']))


KEYS = dict(aggregate=_k_aggregate, aggregate_sum=_k_aggregate_sum, dynadj=_k_dynadj, pwconv=_k_pwconv,
            pwconv_group=_k_pwconv_group, ctr_topology=_k_ctr_topology, tconv_bn=_k_tconv_bn, tconv=_k_tconv,
            temporal_ms=None, temporal_branches_bn=None, fuse_out=_k_fuse_out, fuse_out_pool=_k_fuse_out_pool,
            head_loss=_k_head_loss, data_bn=_k_data_bn, tmean=_k_tmean, tee3=_k_tee3,
            bn_running_update=_k_bn_running_update, strided_frames=_k_strided_frames, dynadj_typed=_k_dynadj_typed,
            gram=_k_gram, gate=_k_gate, temporal_mlp_bn=_k_temporal_mlp, temporal_unitmlp_bn=_k_temporal_unitmlp)
# The public functions of dsgcn_amd.kernels that the census does not wrap, and why.  KEYS and this table partition the
# module's public functions exactly (test_model_census_gpu.py::test_every_public_op_is_keyed_or_listed, no GPU needed):
# a new op fails that test until it is keyed here or listed with a reason.
UNWRAPPED = {
    'ops': 'returns the dispatch namespace; launches nothing',
    'use_ops': 'installs a dispatch namespace; launches nothing',
    'tconv_gemm_ok': 'host predicate; its answer is part of the tconv_bn key',
    'prestrided_fits': 'host predicate; its answer is part of the fuse_out key',
    'data_bn_eligible': 'host predicate deciding whether data_bn runs; launches nothing',
    'dropout_step_advance': 'host counter of the fused dropout streams; launches nothing',
    'dropout_mask': 'materialises a fused dropout mask for tests; the models never call it',
    'reset_leaf_uses': 'step bookkeeping (TrainEngine); launches nothing',
    'end_step': 'step bookkeeping (TrainEngine); launches nothing',
    'flush_param_sums': 'deferred column sums of TrainEngine; test_colsum / the bit-identical step tests check them',
    'param_colsum': 'ordered column sum inside the keyed ops; test_colsum checks its reduction at the census heights',
    'colsum': 'ordered column sum inside the keyed ops; test_colsum checks the one- and two-stage forms',
    'colsum_pair': 'two column sums sharing launches; test_colsum_pair checks every fold combination',
    'cat_rows': 'parameter concatenation, a view under FlatParams; its backward hands back row slices (no kernel)',
    'bn_finalize': 'BatchNorm finalize inside the keyed convs; their checks compare the statistics and affine it makes',
}


# ---------------------------------------------------------------------------------------------------------------------
# the census
# ---------------------------------------------------------------------------------------------------------------------

BASELINE_RUNS = (
    # (name, model, clips, T, V, classes, dropout kept?)
    ('stgcn', 'stgcn', 64, 64, 25, 60, False),
    ('stgcn_dropout', 'stgcn', 64, 64, 25, 60, True),       # config 1 with its shipped tcn_dropout = 0.5 (fused into fuse_out)
    ('ds', 'ds', 64, 64, 25, 60, False),
    ('ds120', 'ds120', 64, 64, 25, 120, False),
    ('ctrgcn', 'ctrgcn', 64, 64, 25, 60, False),
    ('ds_k400', 'ds_k400', 32, 100, 17, 400, False),
)


def _model_cfg(model, keep_drop):
    from bench import ds_cfg, other_cfg
    if model == 'ds':
        return ds_cfg()
    if model == 'ds120':
        return ds_cfg(120)
    if model == 'ds_k400':
        return ds_cfg(400, 'coco')
    return other_cfg(model, tcn_dropout=0.5) if keep_drop else other_cfg(model)


def public_functions(module=K):
    """The public functions defined in dsgcn_amd.kernels (no leading underscore)."""
    return {name for name, fn in inspect.getmembers(module, inspect.isfunction)
            if not name.startswith('_') and fn.__module__ == module.__name__}


BN_PAIRS = '_bn_feed_multi'        # the log entry of BatchNorm coefficient launches that name one BNCtx twice


def _watch_bn_feeds(mp, log):
    """Log every launch of BatchNorm coefficient jobs in which two jobs write one BNCtx's coef buffer — the second one
    accumulating into what the first one writes, in the same launch — as (the jobs' channel counts, jobs).  Covers the
    launches of kernels._bn_feed_multi and of the waiting jobs, and the jobs _bn_feed_multi hands to the caller's next
    (hosting) launch."""
    def same_ctx(jobs):
        coefs = [j.coef for j in jobs]
        if len(set(coefs)) < len(coefs):
            log.setdefault(BN_PAIRS, set()).add((tuple(int(j.C) for j in jobs), len(jobs)))

    def launch_coef(fn):
        def wrapped(jobs):
            same_ctx(jobs)
            return fn(jobs)
        return wrapped

    def feed_multi(fn):
        def wrapped(feeds, launch=True):
            out = fn(feeds, launch)
            same_ctx(out)
            return out
        return wrapped
    mp.setattr(K, '_launch_coef', launch_coef(K._launch_coef))
    mp.setattr(K, '_bn_feed_multi', feed_multi(K._bn_feed_multi))


# The ops whose dispatch reads grad mode or requires_grad: an eval record (_record_eval) extends their keys with EVAL, so
# a no-grad launch is never mistaken for the training launch of the same shape.  tee3 launches nothing for an input
# without history; data_bn normalises with the running statistics of an eval-mode BatchNorm (data_bn_eligible also
# reads requires_grad).
EVAL = 'eval'
GRAD_READING = ('tee3', 'data_bn')


def _install_recorders(mp, log, eval_keys=False):
    """Wrap every op of KEYS, the temporal dispatchers and the BatchNorm feeds: each call adds its key to ``log``."""
    path = {}

    def dispatcher(name, fn):
        def wrapped(*args, **kw):
            out = fn(*args, **kw)
            if out is not None:
                path.setdefault('taken', name)
            return out
        return wrapped

    def recorder(name, fn, keyfn):
        sig = inspect.signature(fn)
        extend = (EVAL,) if eval_keys and name in GRAD_READING else ()

        def wrapped(*args, **kw):
            b = sig.bind(*args, **kw)
            b.apply_defaults()
            if keyfn is None:                     # temporal_ms / temporal_branches_bn: the path is known after the call
                path.clear()
                out = fn(*args, **kw)
                taken = {'fused': 'fused', 'split': 'split'}.get(path.get('taken'), 'staged')
                log.setdefault(name, set()).add(_k_temporal(b.arguments, taken) + extend)
                return out
            log.setdefault(name, set()).add(keyfn(b.arguments) + extend)
            return fn(*args, **kw)
        return wrapped

    for name, keyfn in KEYS.items():
        mp.setattr(K, name, recorder(name, getattr(K, name), keyfn))
    mp.setattr(K, '_fused_temporal', dispatcher('fused', K._fused_temporal))
    mp.setattr(K, '_split_temporal', dispatcher('split', K._split_temporal))
    _watch_bn_feeds(mp, log)


def _build(model, keep_drop, cfg, gen):
    np.random.seed(0)
    torch.manual_seed(0)
    m = dsgcn_amd.build_model(copy.deepcopy(cfg) if cfg is not None else _model_cfg(model, keep_drop))
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith(('alpha', 'beta', 'add_coeff')):
                p.copy_(torch.randn(p.shape, generator=gen) * 0.5)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout) and not keep_drop:
            mod.p = 0.0
    return m


def fill_running_stats(m, gen):
    """Running statistics of every BatchNorm drawn from ``gen``, so that eval-mode affines are not the identity."""
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm) and mod.running_mean is not None:
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=gen) * 0.3)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=gen) + 0.5)


def _record_step(mp, model, clips, T, V, classes, keep_drop, cfg=None):
    """One eager train_step + backward of a BASELINE config (bench.py's model and inputs; or of the model dict ``cfg``)
    -> {op: set of keys}."""
    log = {}
    _install_recorders(mp, log)
    gen = torch.Generator().manual_seed(1)
    m = _build(model, keep_drop, cfg, gen)
    m = m.to(DEV).train()
    x = torch.randn(clips, 1, 2, T, V, 3, generator=gen).to(DEV)
    y = torch.randint(0, classes, (clips, 1), generator=gen).to(DEV)
    out = m.train_step(dict(keypoint=x, label=y), None)
    out['loss'].backward()
    torch.cuda.synchronize()
    assert np.isfinite(out['log_vars']['loss'])
    del m, x, y, out
    gc.collect()
    torch.cuda.empty_cache()
    return log


def _record_eval(mp, model, videos, clips, T, V, cfg=None):
    """One eval-mode forward_test (``model(keypoint=x, return_loss=False)``) of ``videos`` x ``clips`` clips of 2 persons,
    running statistics drawn from a seeded generator -> {op: set of keys}; the ops of GRAD_READING record EVAL keys."""
    log = {}
    _install_recorders(mp, log, eval_keys=True)
    gen = torch.Generator().manual_seed(1)
    m = _build(model, False, cfg, gen)
    fill_running_stats(m, gen)
    m = m.to(DEV).eval()
    x = torch.randn(videos, clips, 2, T, V, 3, generator=gen).to(DEV)
    probs = m(keypoint=x, return_loss=False)
    torch.cuda.synchronize()
    assert probs.shape[0] == videos and np.isfinite(probs).all()
    del m, x
    gc.collect()
    torch.cuda.empty_cache()
    return log


def _collect(runs, record):
    import os
    knobs = sorted(k for k in os.environ if k.startswith('DSGCN_'))
    assert not knobs, f'the census runs the default dispatch: unset {knobs}'
    seen = {}
    for run in runs:
        with pytest.MonkeyPatch.context() as mp:
            log = record(mp, *run[1:])
        for op, keys in log.items():
            for key in keys:
                seen.setdefault(op, {}).setdefault(key, []).append(run[0])
    return seen


def census(runs=BASELINE_RUNS, cfg_of=lambda model: None):
    """{op: {key: [the runs that recorded it]}} over the BASELINE steps (or ``runs``), default knobs.  The entry BN_PAIRS
    holds the coefficient launches that named one BatchNorm twice, if any."""
    return _collect(runs, lambda mp, model, *rest: _record_step(mp, model, *rest, cfg=cfg_of(model)))


def census_eval(runs, cfg_of=lambda model: None):
    """census() of eval-mode forward_test runs: ``runs`` holds (name, model, videos, clips per video, T, V)."""
    return _collect(runs, lambda mp, model, *rest: _record_eval(mp, model, *rest, cfg=cfg_of(model)))


# ---------------------------------------------------------------------------------------------------------------------
# the table: every key the BASELINE steps record, and nothing else (the comments name the runs that record each key)
# ---------------------------------------------------------------------------------------------------------------------

DGMSTCN = ((3, 1), (3, 2), (3, 3), (3, 4), ('max', 3), '1x1')      # DS-STGCN's dgmstcn branches
MSTCN = ((5, 1), (5, 2), ('max', 3), '1x1')                         # CTR-GCN's MSTCN branches

FULL_SIZE_CASES = {
    # (n, KC, T, V, relu, affine)
    'aggregate': [
        (128, 24, 64, 25, True, True),   # ds, ds120
        (128, 48, 32, 25, True, True),   # ds, ds120
        (128, 48, 64, 25, True, True),   # ds, ds120
        (128, 96, 16, 25, True, True),   # ds, ds120
        (128, 96, 32, 25, True, True),   # ds, ds120
        (64, 24, 100, 17, True, True),   # ds_k400
        (64, 48, 100, 17, True, True),   # ds_k400
        (64, 48, 50, 17, True, True),   # ds_k400
        (64, 96, 25, 17, True, True),   # ds_k400
        (64, 96, 50, 17, True, True),   # ds_k400
    ],
    # (n, K, Co, T, V, adjacency form, want_bn)
    'aggregate_sum': [
        (128, 3, 128, 32, 25, 'shared', True),   # stgcn, stgcn_dropout
        (128, 3, 128, 32, 25, 'subset_major', True),   # ctrgcn
        (128, 3, 128, 64, 25, 'shared', True),   # stgcn, stgcn_dropout
        (128, 3, 128, 64, 25, 'subset_major', True),   # ctrgcn
        (128, 3, 256, 16, 25, 'shared', True),   # stgcn, stgcn_dropout
        (128, 3, 256, 16, 25, 'subset_major', True),   # ctrgcn
        (128, 3, 256, 32, 25, 'shared', True),   # stgcn, stgcn_dropout
        (128, 3, 256, 32, 25, 'subset_major', True),   # ctrgcn
        (128, 3, 64, 64, 25, 'shared', True),   # stgcn, stgcn_dropout
        (128, 3, 64, 64, 25, 'subset_major', True),   # ctrgcn
    ],
    # (BatchNorms): one launch for every layer's running statistics; its arithmetic does not depend on a tile shape and is
    # checked against nn.BatchNorm2d by test_bn_running_update_matches_batch_norm
    'bn_running_update': [
        (22,),   # stgcn, stgcn_dropout
        (85,),   # ctrgcn
        (95,),   # ds, ds120, ds_k400
    ],
    # (n, Ci, Co, V, subsets, R, subset_major, path[, (alpha elements, beta, edge subsets, edge classes E)])
    'ctr_topology': [
        (128, 128, 128, 25, 3, 16, True, 'one_conv'),   # ctrgcn
        (128, 128, 256, 25, 3, 16, True, 'one_conv'),   # ctrgcn
        (128, 256, 256, 25, 3, 32, True, 'one_conv'),   # ctrgcn
        (128, 3, 64, 25, 3, 8, True, 'one_conv'),   # ctrgcn
        (128, 64, 128, 25, 3, 8, True, 'one_conv'),   # ctrgcn
        (128, 64, 64, 25, 3, 8, True, 'one_conv'),   # ctrgcn
    ],
    # (N, M, T, V, C, bn_type, affine)
    'data_bn': [
        (32, 2, 100, 17, 3, 'VC', True),   # ds_k400
        (64, 2, 64, 25, 3, 'MVC', True),   # ctrgcn
        (64, 2, 64, 25, 3, 'VC', True),   # stgcn, stgcn_dropout, ds, ds120
    ],
    # (n, Ci, mid, V, xbar row length, BatchNorm jobs hosted[, False: single_use=False])
    'dynadj': [
        (128, 128, 16, 25, 32, True),   # ds, ds120
        (128, 128, 32, 25, 32, True),   # ds, ds120
        (128, 256, 32, 25, 32, True),   # ds, ds120
        (128, 3, 8, 25, 32, True),   # ds, ds120
        (128, 64, 16, 25, 32, True),   # ds, ds120
        (128, 64, 8, 25, 32, True),   # ds, ds120
        (64, 128, 16, 17, 32, True),   # ds_k400
        (64, 128, 32, 17, 32, True),   # ds_k400
        (64, 256, 32, 17, 32, True),   # ds_k400
        (64, 3, 8, 17, 32, True),   # ds_k400
        (64, 64, 16, 17, 32, True),   # ds_k400
        (64, 64, 8, 17, 32, True),   # ds_k400
    ],
    # (n, C, T, V, mode, relu flags, time-mean ld (0: none), tee, dropout, prestrided_fits)
    'fuse_out': [
        (128, 128, 32, 25, 'res_affine', 1, 0, 1, False, True),   # stgcn
        (128, 128, 32, 25, 'res_affine', 1, 0, 1, True, True),   # stgcn_dropout
        (128, 128, 32, 25, 'res_affine', 1, 32, 1, False, True),   # ds, ds120
        (128, 128, 32, 25, 'res_affine', 3, 25, 1, False, True),   # ctrgcn
        (128, 128, 32, 25, 'res_plain', 1, 0, 1, False, True),   # stgcn
        (128, 128, 32, 25, 'res_plain', 1, 0, 1, True, True),   # stgcn_dropout
        (128, 128, 32, 25, 'res_plain', 1, 0, 2, False, True),   # stgcn
        (128, 128, 32, 25, 'res_plain', 1, 0, 2, True, True),   # stgcn_dropout
        (128, 128, 32, 25, 'res_plain', 1, 32, 1, False, True),   # ds, ds120
        (128, 128, 32, 25, 'res_plain', 1, 32, 2, False, True),   # ds, ds120
        (128, 128, 32, 25, 'res_plain', 3, 25, 1, False, True),   # ctrgcn
        (128, 128, 32, 25, 'res_plain', 3, 25, 2, False, True),   # ctrgcn
        (128, 256, 16, 25, 'res_affine', 1, 0, 1, False, True),   # stgcn
        (128, 256, 16, 25, 'res_affine', 1, 0, 1, True, True),   # stgcn_dropout
        (128, 256, 16, 25, 'res_affine', 1, 32, 1, False, True),   # ds, ds120
        (128, 256, 16, 25, 'res_affine', 3, 25, 1, False, True),   # ctrgcn
        (128, 256, 16, 25, 'res_plain', 1, 0, 1, False, True),   # stgcn
        (128, 256, 16, 25, 'res_plain', 1, 0, 1, True, True),   # stgcn_dropout
        (128, 256, 16, 25, 'res_plain', 1, 32, 1, False, True),   # ds, ds120
        (128, 256, 16, 25, 'res_plain', 3, 25, 1, False, True),   # ctrgcn
        (128, 3, 64, 25, 'plain', 0, 25, 0, False, True),   # ctrgcn
        (128, 3, 64, 25, 'plain', 0, 32, 0, False, True),   # ds, ds120
        (128, 64, 64, 25, 'affine', 1, 0, 1, False, True),   # stgcn, stgcn_dropout
        (128, 64, 64, 25, 'affine', 1, 32, 1, False, True),   # ds, ds120
        (128, 64, 64, 25, 'affine', 3, 25, 1, False, True),   # ctrgcn
        (128, 64, 64, 25, 'res_plain', 1, 0, 1, False, True),   # stgcn
        (128, 64, 64, 25, 'res_plain', 1, 0, 1, True, True),   # stgcn_dropout
        (128, 64, 64, 25, 'res_plain', 1, 0, 2, False, True),   # stgcn
        (128, 64, 64, 25, 'res_plain', 1, 0, 2, True, True),   # stgcn_dropout
        (128, 64, 64, 25, 'res_plain', 1, 32, 1, False, True),   # ds, ds120
        (128, 64, 64, 25, 'res_plain', 1, 32, 2, False, True),   # ds, ds120
        (128, 64, 64, 25, 'res_plain', 3, 25, 1, False, True),   # ctrgcn
        (128, 64, 64, 25, 'res_plain', 3, 25, 2, False, True),   # ctrgcn
        (64, 128, 50, 17, 'res_affine', 1, 32, 1, False, True),   # ds_k400
        (64, 128, 50, 17, 'res_plain', 1, 32, 1, False, True),   # ds_k400
        (64, 128, 50, 17, 'res_plain', 1, 32, 2, False, True),   # ds_k400
        (64, 256, 25, 17, 'res_affine', 1, 32, 1, False, True),   # ds_k400
        (64, 256, 25, 17, 'res_plain', 1, 32, 1, False, True),   # ds_k400
        (64, 3, 100, 17, 'plain', 0, 32, 0, False, True),   # ds_k400
        (64, 64, 100, 17, 'affine', 1, 32, 1, False, True),   # ds_k400
        (64, 64, 100, 17, 'res_plain', 1, 32, 1, False, True),   # ds_k400
        (64, 64, 100, 17, 'res_plain', 1, 32, 2, False, True),   # ds_k400
    ],
    # (n, C, T, V, mode, relu flags, dropout)
    'fuse_out_pool': [
        (128, 256, 16, 25, 'res_plain', 1, False),   # stgcn, ds, ds120
        (128, 256, 16, 25, 'res_plain', 1, True),   # stgcn_dropout
        (128, 256, 16, 25, 'res_plain', 3, False),   # ctrgcn
        (64, 256, 25, 17, 'res_plain', 1, False),   # ds_k400
    ],
    # (clips, persons, C, classes, bias)
    'head_loss': [
        (32, 2, 256, 400, True),   # ds_k400
        (64, 2, 256, 120, True),   # ds120
        (64, 2, 256, 60, True),   # stgcn, stgcn_dropout, ds, ctrgcn
    ],
    # (n, Ci, Co, T, V, stride, aug, mode, want_bn, bias, forward form, backward form)
    'pwconv': [
        (128, 128, 128, 32, 25, 1, False, 'affine_relu', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds, ds120
        (128, 128, 128, 32, 25, 1, False, 'res_plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ctrgcn
        (128, 128, 128, 32, 25, 1, True, 'res_plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds, ds120
        (128, 128, 128, 64, 25, 1, False, 'res_affine', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ctrgcn
        (128, 128, 128, 64, 25, 1, True, 'res_affine', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds, ds120
        (128, 128, 144, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds, ds120
        (128, 128, 256, 16, 25, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # stgcn, stgcn_dropout, ds, ds120, ctrgcn
        (128, 128, 256, 32, 25, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds, ds120, ctrgcn
        (128, 128, 288, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds, ds120
        (128, 128, 384, 32, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # stgcn, stgcn_dropout, ctrgcn
        (128, 128, 48, 32, 25, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds, ds120
        (128, 128, 768, 32, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # stgcn, stgcn_dropout, ctrgcn
        (128, 128, 96, 1, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn
        (128, 128, 96, 32, 25, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds, ds120
        (128, 24, 64, 64, 25, 1, False, 'plain', True, True, 'direct', 'bwd64'),   # ds, ds120
        (128, 256, 192, 1, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn
        (128, 256, 256, 16, 25, 1, False, 'affine_relu', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds, ds120
        (128, 256, 256, 16, 25, 1, False, 'res_plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ctrgcn
        (128, 256, 256, 16, 25, 1, True, 'res_plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds, ds120
        (128, 256, 256, 32, 25, 1, False, 'res_affine', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ctrgcn
        (128, 256, 256, 32, 25, 1, True, 'res_affine', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds, ds120
        (128, 256, 288, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds, ds120
        (128, 256, 768, 16, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # stgcn, stgcn_dropout, ctrgcn
        (128, 256, 96, 16, 25, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds, ds120
        (128, 3, 192, 64, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # stgcn, stgcn_dropout, ctrgcn
        (128, 3, 24, 64, 25, 1, False, 'plain', True, True, 'direct', 'bwd64'),   # ds, ds120
        (128, 3, 48, 1, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn
        (128, 3, 64, 64, 25, 1, False, 'plain', True, True, 'direct', 'bwd64'),   # ds, ds120, ctrgcn
        (128, 3, 72, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds, ds120
        (128, 48, 128, 32, 25, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds, ds120
        (128, 48, 128, 64, 25, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds, ds120
        (128, 64, 128, 32, 25, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # stgcn, stgcn_dropout, ds, ds120, ctrgcn
        (128, 64, 128, 64, 25, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds, ds120, ctrgcn
        (128, 64, 144, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds, ds120
        (128, 64, 192, 64, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # stgcn, stgcn_dropout, ctrgcn
        (128, 64, 24, 64, 25, 1, False, 'plain', True, True, 'direct', 'bwd64'),   # ds, ds120
        (128, 64, 384, 64, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # stgcn, stgcn_dropout, ctrgcn
        (128, 64, 48, 1, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn
        (128, 64, 48, 64, 25, 1, False, 'plain', True, True, 'direct', 'bwd64'),   # ds, ds120
        (128, 64, 64, 64, 25, 1, False, 'affine_relu', True, True, 'direct', 'bwd64'),   # ds, ds120
        (128, 64, 64, 64, 25, 1, False, 'res_affine', True, True, 'direct', 'bwd64'),   # ctrgcn
        (128, 64, 64, 64, 25, 1, False, 'res_plain', True, True, 'direct', 'bwd64'),   # ctrgcn
        (128, 64, 64, 64, 25, 1, True, 'res_affine', True, True, 'direct', 'dgrad_wgrad'),   # ds, ds120
        (128, 64, 64, 64, 25, 1, True, 'res_plain', True, True, 'direct', 'dgrad_wgrad'),   # ds, ds120
        (128, 64, 72, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds, ds120
        (128, 96, 256, 16, 25, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds, ds120
        (128, 96, 256, 32, 25, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds, ds120
        (64, 128, 128, 100, 17, 1, True, 'res_affine', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_k400
        (64, 128, 128, 50, 17, 1, False, 'affine_relu', True, True, 'direct', 'dgrad_wgrad'),   # ds_k400
        (64, 128, 128, 50, 17, 1, True, 'res_plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_k400
        (64, 128, 144, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_k400
        (64, 128, 256, 25, 17, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_k400
        (64, 128, 256, 50, 17, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_k400
        (64, 128, 288, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_k400
        (64, 128, 48, 50, 17, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_k400
        (64, 128, 96, 50, 17, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_k400
        (64, 24, 64, 100, 17, 1, False, 'plain', True, True, 'direct', 'bwd64'),   # ds_k400
        (64, 256, 256, 25, 17, 1, False, 'affine_relu', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_k400
        (64, 256, 256, 25, 17, 1, True, 'res_plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_k400
        (64, 256, 256, 50, 17, 1, True, 'res_affine', True, True, 'direct', 'dgrad_wgrad'),   # ds_k400
        (64, 256, 288, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_k400
        (64, 256, 96, 25, 17, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_k400
        (64, 3, 24, 100, 17, 1, False, 'plain', True, True, 'direct', 'bwd64'),   # ds_k400
        (64, 3, 64, 100, 17, 1, False, 'plain', True, True, 'direct', 'bwd64'),   # ds_k400
        (64, 3, 72, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_k400
        (64, 48, 128, 100, 17, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_k400
        (64, 48, 128, 50, 17, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_k400
        (64, 64, 128, 100, 17, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_k400
        (64, 64, 128, 50, 17, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_k400
        (64, 64, 144, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_k400
        (64, 64, 24, 100, 17, 1, False, 'plain', True, True, 'direct', 'bwd64'),   # ds_k400
        (64, 64, 48, 100, 17, 1, False, 'plain', True, True, 'direct', 'bwd64'),   # ds_k400
        (64, 64, 64, 100, 17, 1, False, 'affine_relu', True, True, 'direct', 'bwd64'),   # ds_k400
        (64, 64, 64, 100, 17, 1, True, 'res_affine', True, True, 'direct', 'dgrad_wgrad'),   # ds_k400
        (64, 64, 64, 100, 17, 1, True, 'res_plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_k400
        (64, 64, 72, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_k400
        (64, 96, 256, 25, 17, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_k400
        (64, 96, 256, 50, 17, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_k400
    ],
    # (convs, n, Ci, Co, T, V, input affine, path)
    'pwconv_group': [
        (3, 128, 10, 128, 25, 25, True, 'grouped'),   # ctrgcn
        (3, 128, 10, 64, 25, 25, True, 'grouped'),   # ctrgcn
        (3, 128, 18, 128, 25, 25, True, 'grouped'),   # ctrgcn
        (3, 128, 18, 256, 25, 25, True, 'grouped'),   # ctrgcn
        (3, 128, 34, 256, 25, 25, True, 'grouped'),   # ctrgcn
    ],
    # (n, Ci, Co, T, V, KT, mode, stride, want_bn, tconv_gemm_ok)
    'tconv_bn': [
        (128, 128, 128, 32, 25, 9, 'affine_relu', 1, True, True),   # stgcn, stgcn_dropout
        (128, 128, 128, 64, 25, 9, 'affine_relu', 2, True, True),   # stgcn, stgcn_dropout
        (128, 256, 256, 16, 25, 9, 'affine_relu', 1, True, True),   # stgcn, stgcn_dropout
        (128, 256, 256, 32, 25, 9, 'affine_relu', 2, True, True),   # stgcn, stgcn_dropout
        (128, 64, 64, 64, 25, 9, 'affine_relu', 1, True, True),   # stgcn, stgcn_dropout
    ],
    # (shape,): three aliases of the block input; their gradients meet in one dsgcn_add3 launch
    'tee3': [
        ((128, 3, 64, 25),),   # stgcn, stgcn_dropout, ds, ds120, ctrgcn
        ((64, 3, 100, 17),),   # ds_k400
    ],
    # (n, C, T, V, stride, branches, widths, n_act, want_bn, path)
    'temporal_branches_bn': [
        (128, 128, 32, 25, 1, MSTCN, (32, 32, 32, 32), 96, True, 'fused'),   # ctrgcn
        (128, 128, 64, 25, 2, MSTCN, (32, 32, 32, 32), 96, True, 'fused'),   # ctrgcn
        (128, 256, 16, 25, 1, MSTCN, (64, 64, 64, 64), 192, True, 'fused'),   # ctrgcn
        (128, 256, 32, 25, 2, MSTCN, (64, 64, 64, 64), 192, True, 'fused'),   # ctrgcn
        (128, 64, 64, 25, 1, MSTCN, (16, 16, 16, 16), 48, True, 'fused'),   # ctrgcn
    ],
    # (n, C, T, V, stride, branches, widths, n_act, want_bn, path)
    'temporal_ms': [
        (128, 128, 32, 25, 1, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, True, 'split'),   # ds, ds120
        (128, 128, 64, 25, 2, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, True, 'split'),   # ds, ds120
        (128, 256, 16, 25, 1, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, True, 'split'),   # ds, ds120
        (128, 256, 32, 25, 2, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, True, 'split'),   # ds, ds120
        (128, 64, 64, 25, 1, DGMSTCN, (14, 10, 10, 10, 10, 10), 54, True, 'split'),   # ds, ds120
        (64, 128, 100, 17, 2, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, True, 'staged'),   # ds_k400
        (64, 128, 50, 17, 1, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, True, 'staged'),   # ds_k400
        (64, 256, 25, 17, 1, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, True, 'staged'),   # ds_k400
        (64, 256, 50, 17, 2, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, True, 'staged'),   # ds_k400
        (64, 64, 100, 17, 1, DGMSTCN, (14, 10, 10, 10, 10, 10), 54, True, 'split'),   # ds_k400
    ],
    # (n, C, T, V, ld)
    'tmean': [
        (128, 3, 64, 25, 25),   # ctrgcn
        (128, 3, 64, 25, 32),   # ds, ds120
        (64, 3, 100, 17, 32),   # ds_k400
    ],
}


@pytest.fixture(scope='module')
def recorded():
    return census()


def _listing(keys):
    out = []
    for op in sorted(keys):
        out.append(f"    '{op}': [")
        out += [f'        {k!r},   # {", ".join(keys[op][k])}' for k in sorted(keys[op], key=repr)]
        out.append('    ],')
    return '\n'.join(out)


def test_census_every_kernel_call_is_in_the_table(recorded):
    missing = {op: {k: runs for k, runs in keys.items() if k not in FULL_SIZE_CASES.get(op, ())}
               for op, keys in recorded.items() if op != BN_PAIRS}
    missing = {op: keys for op, keys in missing.items() if keys}
    assert not missing, 'kernel calls of the BASELINE steps that FULL_SIZE_CASES lacks:\n' + _listing(missing)


def test_census_table_has_no_stale_entries(recorded):
    stale = {op: [k for k in keys if k not in recorded.get(op, {})] for op, keys in FULL_SIZE_CASES.items()}
    stale = {op: keys for op, keys in stale.items() if keys}
    assert not stale, f'FULL_SIZE_CASES entries no BASELINE step records: {stale!r}'
    assert all(len(set(keys)) == len(keys) for keys in FULL_SIZE_CASES.values())


def test_census_no_bn_coef_launch_writes_one_batchnorm_twice(recorded):
    """two jobs of one coefficient launch that name the same BNCtx race (the second accumulates into the coef
    buffer the first one writes)."""
    assert BN_PAIRS not in recorded, _listing({BN_PAIRS: recorded.get(BN_PAIRS, {})})


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 comparisons of the table's keys
# ---------------------------------------------------------------------------------------------------------------------
# Each key is mapped to the arguments of the check_* helper of tests/test_kernels_gpu.py that the op's own test runs, with
# that test's bars.  A key whose arguments are already one of that test's cases is not run twice.

import test_kernels_gpu as KG        # noqa: E402  (tests/ is on sys.path: tests/conftest.py)


def _existing(test):
    """The argument dicts of a test's parametrize lists (their product when stacked)."""
    import itertools
    marks = [m for m in getattr(test, 'pytestmark', []) if m.name == 'parametrize']
    lists = []
    for m in marks:
        names = [a.strip() for a in m.args[0].split(',')]
        lists.append([dict(zip(names, v if len(names) > 1 else (v,))) for v in m.args[1]])
    return [dict(kv for d in combo for kv in d.items()) for combo in itertools.product(*lists)]


def _cases(op, to_args, test=None, keep=lambda key: True, table=None):
    have = _existing(test) if test is not None else []
    out = []
    for key in (FULL_SIZE_CASES if table is None else table)[op]:
        if not keep(key):
            continue
        args = to_args(key)
        if args not in have:
            out.append(pytest.param(key, args, id=repr(key)))
    return out


class _Path:
    """Which temporal dispatcher answered (kernels._fused_temporal / _split_temporal, else the staged chain)."""

    def __init__(self, mp):
        self.taken = []
        for name, tag in (('_fused_temporal', 'fused'), ('_split_temporal', 'split')):
            mp.setattr(K, name, self._wrap(getattr(K, name), tag))

    def _wrap(self, fn, tag):
        def wrapped(*a, **kw):
            out = fn(*a, **kw)
            if out is not None:
                self.taken.append(tag)
            return out
        return wrapped

    def path(self):
        return self.taken[0] if self.taken else 'staged'


@pytest.mark.parametrize('key,args', _cases('aggregate', lambda k: dict(zip(('n', 'KC', 'T', 'V', 'relu', 'affine'), k)),
                                            KG.test_aggregate))
def test_aggregate_census(key, args):
    KG.check_aggregate(**args)


def _aggsum_args(k):
    n, Kk, Co, T, V, form, bn = k
    assert form in ('shared', 'subset_major'), form
    # subset-major adjacency: the fp64 check runs the (n, K*Co, V, V) layout; the subset-major launches are pinned to it
    # bit for bit by test_aggregate_sum_subset_major_census below
    return dict(n=n, K=Kk, Co=Co, T=T, V=V, shared=form == 'shared', bn=bn)


@pytest.mark.parametrize('key,args', _cases('aggregate_sum', _aggsum_args, KG.test_aggregate_sum))
def test_aggregate_sum_census(key, args):
    KG.check_aggregate_sum(**args)


@pytest.mark.parametrize('key,args', _cases('aggregate_sum', lambda k: dict(zip(('n', 'K', 'Co', 'T', 'V'), k[:5])),
                                            KG.test_aggregate_sum_subset_major_adjacency,
                                            keep=lambda k: k[5] == 'subset_major'))
def test_aggregate_sum_subset_major_census(key, args):
    assert key[6]               # the helper's calls take the BatchNorm statistics, as the step's do
    KG.check_aggregate_sum_subset_major_adjacency(**args)


def _ctr_args(k):
    n, Ci, Co, V, Kk, Rr, subset_major, path = k[:8]
    n_alpha, beta, edge, E = k[8] if len(k) > 8 else (1, False, (), 0)
    # check_ctr_topology builds three subsets of R = 8 (Ci <= 16) / Ci // 8 channels, as unit_ctrgcn does; with
    # subset_major it asserts the (K, n, Co, V, V) result of the one-conv form, which the library takes exactly for the
    # classic unit (one alpha, no Gram term, no edge subsets)
    classic = n_alpha == 1 and not beta and not edge
    assert Kk == 3 and Rr == (8 if Ci <= 16 else Ci // 8) and n_alpha in (1, Kk), k
    assert path == ('one_conv' if subset_major and classic else 'per_subset'), k
    args = dict(n=n, Ci=Ci, Co=Co, V=V, subset_major=subset_major)
    if not classic:
        args.update(alpha_per_subset=n_alpha == Kk, beta=beta, edge=edge, E=E)
    return args


@pytest.mark.parametrize('key,args', _cases('ctr_topology', _ctr_args, KG.test_ctr_topology))
def test_ctr_topology_census(key, args):
    KG.check_ctr_topology(**args)


@pytest.mark.parametrize('key,args', _cases('data_bn', lambda k: dict(zip(('N', 'M', 'T', 'V', 'C', 'bn_type', 'affine'), k)),
                                            KG.test_data_bn))
def test_data_bn_census(key, args):
    KG.check_data_bn(**args)


def _dyn_args(k):
    n, Ci, mid, V, ld, hosted = k[:6]
    single_use = len(k) == 6
    # ld = 32: the step hands xbar over zero-padded to 32 joints (fuse_out's time mean); dynadj pads an unpadded xbar to
    # the same tensor before its first launch, so the helper's unpadded input (ld = V) runs the same launches.  hosted:
    # BatchNorm finalize jobs ride in K-B's launches, bit-identical to the plain call
    # (test_bn_jobs_batched_and_hosted_are_bit_identical)
    assert ld in (32, V) and V < 32
    args = dict(n=n, Ci=Ci, mid=mid, V=V, layout={25: 'nturgb+d', 17: 'coco'}[V])
    if not single_use:
        args['single_use'] = False
    return args


@pytest.mark.parametrize('key,args', _cases('dynadj', _dyn_args, KG.test_dynadj))
def test_dynadj_census(key, args):
    KG.check_dynadj(**args)


def _fuse_args(k):
    n, C, T, V, mode, flags, ld, tee, drop, fits = k
    assert fits or tee != 2
    if drop:
        # tee = 1 hands out three aliases of the one output (no launch of its own): the dropout check runs the plain form
        assert ld == 0
        return dict(n=n, C=C, T=T, V=V, mode=mode, flags=flags, form='tee2' if tee == 2 else 'plain', p=0.5)
    args = dict(n=n, C=C, T=T, V=V, mode=mode, tmean=False if ld == 0 else (True if ld == V else ld), flags=flags)
    if tee:
        args['tee'] = tee
    return args


@pytest.mark.parametrize('key,args', _cases('fuse_out', _fuse_args, KG.test_fuse_out, keep=lambda k: not k[8]))
def test_fuse_out_census(key, args):
    KG.check_fuse_out(**args)


@pytest.mark.parametrize('key,args', _cases('fuse_out', _fuse_args, KG.test_fuse_out_dropout, keep=lambda k: k[8]))
def test_fuse_out_dropout_census(key, args):
    KG.check_fuse_out_dropout(**args)


def _pool_args(k):
    n, C, T, V, mode, flags, drop = k
    if drop:
        return dict(n=n, C=C, T=T, V=V, mode=mode, flags=flags, form='pool', p=0.5)
    return dict(n=n, C=C, T=T, V=V, mode=mode, flags=flags)


@pytest.mark.parametrize('key,args', _cases('fuse_out_pool', _pool_args, KG.test_fuse_out_pool, keep=lambda k: not k[6]))
def test_fuse_out_pool_census(key, args):
    KG.check_fuse_out_pool(**args)


@pytest.mark.parametrize('key,args', _cases('fuse_out_pool', _pool_args, KG.test_fuse_out_dropout, keep=lambda k: k[6]))
def test_fuse_out_pool_dropout_census(key, args):
    KG.check_fuse_out_dropout(**args)


@pytest.mark.parametrize('key,args', _cases('head_loss', lambda k: dict(N=k[0], M=k[1], C=k[2], K=k[3], lw=1.0, bias=k[4]),
                                            KG.test_head_loss))
def test_head_loss_census(key, args):
    KG.check_head_loss(**args)


def _pw_args(k):
    n, Ci, Co, T, V, stride, aug, mode, want_bn, bias, fwd, bwd = k
    args = dict(n=n, Ci=Ci, Co=Co, T=T, V=V, stride=stride, aug=aug, mode=mode)
    if not want_bn:
        args['want_bn'] = False
    if not bias:
        args['bias'] = False
    return args


@pytest.mark.parametrize('key,args', _cases('pwconv', _pw_args, KG.test_pwconv))
def test_pwconv_census(key, args):
    # the forward / backward forms are the library's own answers for the shape (dsgcn_pwconv_wsplit_bytes,
    # dsgcn_pwconv_bwd_rows): the helper's call at the same shape and mode takes the same ones
    assert key[-2:] == _pw_paths(*key[:7])
    KG.check_pwconv(**args)


@pytest.mark.parametrize('key,args', _cases('pwconv_group', lambda k: dict(zip(('Kk', 'n', 'Ci', 'Co', 'T', 'V', 'affine'), k))))
def test_pwconv_group_census(key, args):
    assert key[-1] == 'grouped'
    KG.check_pwconv_group(**args)


def _tcg_args(k):
    n, Ci, Co, T, V, KT, mode, stride, want_bn, ok = k
    assert want_bn and ok, k         # a shape tconv_gemm_ok declines runs no kernel here (the unit falls back to tconv)
    return dict(n=n, Ci=Ci, Co=Co, T=T, V=V, KT=KT, mode=mode, stride=stride)


@pytest.mark.parametrize('key,args', _cases('tconv_bn', _tcg_args, KG.test_tconv_gemm))
def test_tconv_gemm_census(key, args):
    KG.check_tconv_gemm(**args)


def _ms_args(k):
    n, C, T, V, stride, cfg, widths, n_act, want_bn, path = k
    mid = C // 6
    # check_temporal_ms builds dgmstcn's branch table the way the unit does: five branches of C // 6 channels
    assert cfg == DGMSTCN and widths == (C - 5 * mid,) + (mid,) * 5 and n_act == C - mid and want_bn, k
    return dict(n=n, C=C, T=T, V=V, stride=stride, fused={'fused': '1', 'split': 'split', 'staged': '0'}[path])


@pytest.mark.parametrize('key,args', _cases('temporal_ms', _ms_args))
def test_temporal_ms_census(key, args, monkeypatch):
    p = _Path(monkeypatch)
    KG.check_temporal_ms(**args, monkeypatch=monkeypatch)
    assert set(p.taken) <= {p.path()} and p.path() == key[-1], (p.taken, key[-1])


def _tb_args(k):
    n, C, T, V, stride, cfg, widths, n_act, want_bn, path = k
    ks = cfg[0][0]
    args = dict(n=n, C=C, T=T, V=V, stride=stride, ks=ks, fused={'fused': 'auto', 'staged': '0'}[path])
    assert want_bn, k
    if cfg == DGMSTCN:
        # ST-GCN++'s mstcn: dgmstcn's six branches, C // 6 channels each, the remainder on the first
        mid = C // 6
        assert widths == (C - 5 * mid,) + (mid,) * 5 and n_act == C - mid, k
        return dict(args, cfg=cfg)
    bc = C // 4
    assert cfg == ((ks, 1), (ks, 2), ('max', 3), '1x1') and widths == (bc, bc, bc, C - 3 * bc) and n_act == 3 * bc, k
    return args


@pytest.mark.parametrize('key,args', _cases('temporal_branches_bn', _tb_args))
def test_temporal_branches_bn_census(key, args, monkeypatch):
    p = _Path(monkeypatch)
    KG.check_temporal_branches_bn(**args, monkeypatch=monkeypatch)
    assert set(p.taken) <= {p.path()} and p.path() == key[-1], (p.taken, key[-1])


@pytest.mark.parametrize('key,args', _cases('tmean', lambda k: dict(n=k[0], C=k[1], T=k[2], V=k[3],
                                                                     ld=True if k[4] == k[3] else k[4])))
def test_tmean_census(key, args):
    KG.check_tmean(**args)


@pytest.mark.parametrize('key', FULL_SIZE_CASES['tee3'], ids=repr)
def test_tee3_census(key):
    """The three aliases are the input itself; the backward sums their gradients in one launch (dsgcn_add3): fp64 sum."""
    shape = key[0]
    g = torch.Generator().manual_seed(3)
    x = torch.randn(*shape, generator=g).to(DEV).requires_grad_()
    gs = [torch.randn(*shape, generator=g) for _ in range(3)]
    a, b, c = K.tee3(x)
    assert all(t.data_ptr() == x.data_ptr() for t in (a, b, c))
    ((a * gs[0].to(DEV)).sum() + (b * gs[1].to(DEV)).sum() + (c * gs[2].to(DEV)).sum()).backward()
    want = sum(t.double() for t in gs)
    assert KG.rel(x.grad, want) < 1e-7, KG.rel(x.grad, want)
