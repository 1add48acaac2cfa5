"""-m gpu: the dynamic-adjacency projections as GUEST workgroups of the `pre` conv's launches (csrc/pw4.hip: P4Guest).
Through the C ABI: host + guest in one call against the same two convs launched separately, every output pre-filled with
NaN — the same bits everywhere and no NaN left; against an fp64 torch conv at the tolerance tests/test_kernels_gpu.py
(check_pwconv) uses for these kernels.  Then the unit and the engine with kernels.PROJ_GUEST on and off."""
import ctypes

import pytest
import torch

import dsgcn_amd as D
from dsgcn_amd import kernels as K
from dsgcn_amd import native

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')

# (Ci -> Co_pre, guest rows) of DS-STGCN's ten blocks
SHAPES = [(3, 24, 72), (64, 24, 72), (64, 48, 144), (128, 48, 144), (128, 96, 288), (256, 96, 288)]


def _ptr(t):
    return None if t is None else t.data_ptr()


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _rand(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV, dtype=torch.float32)


def _wide_n(Ci, Co, T, V, n0):
    """the smallest n >= n0 at which the conv takes the fragment-image kernels (k_pwg3); n0 for the narrow convs"""
    lib = native.lib()
    if Co <= 64:
        assert lib.dsgcn_pwconv_wsplit_bytes(n0, Ci, Co, T, V, 1) == 0
        return n0
    for n in range(n0, 257):
        if lib.dsgcn_pwconv_wsplit_bytes(n, Ci, Co, T, V, 1):
            return n
    raise AssertionError('no batch size takes the GEMM form')


def _ws(w, n, Ci, Co, T, V):
    lib = native.lib()
    nb = lib.dsgcn_pwconv_wsplit_bytes(n, Ci, Co, T, V, 1)
    if not nb:
        return None
    ws = torch.empty(nb, device=DEV, dtype=torch.uint8)
    native.check(lib.dsgcn_pwconv_wsplit(_ptr(w), Ci, Co, _ptr(ws), None), 'dsgcn_pwconv_wsplit')
    return ws


def _guest(x, w, b, out):
    g = native.GuestConv(_ptr(x), _ptr(w), _ptr(b), _ptr(out), x.shape[0], x.shape[1], w.shape[0], x.shape[-1])
    g._keep = (x, w, b, out)
    return g


def _fwd_case(n, Ci, Co, R, T, V, seed, a1=None, relu=False):
    """-> dict of the tensors of one forward pair: host x (n, Ci, T, V) -> z (n, Co, T, V) with statistics rows, guest
    xbar (n, Ci, 1, 32) -> proj (n, R, 1, 32)"""
    g = torch.Generator().manual_seed(seed)
    lib = native.lib()
    c = dict(n=n, Ci=Ci, Co=Co, R=R, T=T, V=V, a1=a1, relu=relu)
    c['x'] = _rand(g, n, Ci, T, V)
    c['w'] = _rand(g, Co, Ci, scale=Ci ** -0.5)
    c['b'] = _rand(g, Co, scale=0.1)
    c['xbar'] = _rand(g, n, Ci, 1, 32)
    c['xbar'][..., V:] = 0                      # the padded joints of fuse_out(want_tmean=32)
    c['wp'] = _rand(g, R, Ci, scale=Ci ** -0.5)
    c['bp'] = _rand(g, R, scale=0.1)
    c['ws'] = _ws(c['w'], n, Ci, Co, T, V)
    c['rows'] = lib.dsgcn_pwconv_partial_rows(n, Ci, Co, T, V, 1, 0)
    return c


def _run_fwd(c, together):
    """together: one dsgcn_pwconv_fwd_ws_guest call; else the host's and the guest's own dsgcn_pwconv_fwd_ws calls.
    -> (z, partial, proj, hosted)"""
    lib = native.lib()
    n, Ci, Co, R, T, V = (c[k] for k in ('n', 'Ci', 'Co', 'R', 'T', 'V'))
    s1, h1 = c['a1'] if c['a1'] is not None else (None, None)
    z, partial, proj = _nan(n, Co, T, V), _nan(c['rows'], Co, 2), _nan(n, R, 1, 32)
    hosted = ctypes.c_int(-1)
    if together:
        g = _guest(c['xbar'], c['wp'], c['bp'], proj)
        rc = lib.dsgcn_pwconv_fwd_ws_guest(_ptr(c['x']), _ptr(s1), _ptr(h1), None, None, None, int(c['relu']), _ptr(c['w']),
                                           _ptr(c['b']), _ptr(z), None, _ptr(partial), n, Ci, Co, T, V, 1, 0, 1,
                                           _ptr(c['ws']), ctypes.addressof(g), ctypes.byref(hosted), None)
        native.check(rc, 'dsgcn_pwconv_fwd_ws_guest')
    else:
        rc = lib.dsgcn_pwconv_fwd_ws(_ptr(c['x']), _ptr(s1), _ptr(h1), None, None, None, int(c['relu']), _ptr(c['w']),
                                     _ptr(c['b']), _ptr(z), None, _ptr(partial), n, Ci, Co, T, V, 1, 0, 1, _ptr(c['ws']), None)
        native.check(rc, 'dsgcn_pwconv_fwd_ws')
        rc = lib.dsgcn_pwconv_fwd_ws(_ptr(c['xbar']), None, None, None, None, None, 0, _ptr(c['wp']), _ptr(c['bp']),
                                     _ptr(proj), None, None, n, Ci, R, 1, 32, 1, 0, 0, None, None)
        native.check(rc, 'dsgcn_pwconv_fwd_ws')
    torch.cuda.synchronize()
    return z, partial, proj, hosted.value


def _conv64(x, w, b):
    return torch.einsum('oc,nctv->notv', w.double(), x.double()) + b.double().view(1, -1, 1, 1)


def _check_fwd(c, want_hosted=1):
    z0, p0, q0, _ = _run_fwd(c, False)
    z1, p1, q1, hosted = _run_fwd(c, True)
    assert hosted == want_hosted
    g = _guest(c['xbar'], c['wp'], c['bp'], q1)
    if c['a1'] is None:
        assert native.lib().dsgcn_pwconv_guest_hosted(0, c['n'], c['Ci'], c['Co'], c['T'], c['V'], 1, ctypes.addressof(g)) == hosted
    for name, a, b in (('z', z0, z1), ('partial', p0, p1), ('proj', q0, q1)):
        assert not torch.isnan(b).any(), name
        assert torch.equal(a, b), name
    # fp32 MFMA / bf16-term dot products over <= 256 channels: the bound of check_pwconv (tests/test_kernels_gpu.py)
    assert rel(q1, _conv64(c['xbar'], c['wp'], c['bp'])) < 2e-5
    if c['a1'] is None:
        assert rel(z1, _conv64(c['x'], c['w'], c['b'])) < 2e-5


@pytest.mark.parametrize('Ci,Co,R', SHAPES)
def test_forward_pair_bit_equal(Ci, Co, R):
    """n = 3 persons, T = 8, V = 25 (the wide hosts at the smallest n that takes k_pwg3): blocks 1-7 on
    k_pw4<1, 4, 0, 8, 0, false>, blocks 8-10 on k_pwg3<0, 0, 1>."""
    n = _wide_n(Ci, Co, 8, 25, 3)
    _check_fwd(_fwd_case(n, Ci, Co, R, 8, 25, seed=Ci * 7 + Co))


@pytest.mark.parametrize('Ci,Co,R,T', [(64, 24, 72, 64), (256, 96, 288, 16)])
def test_forward_pair_full_size(Ci, Co, R, T):
    """n = 128 person-samples, one case per host family: tile-shape changes in K-C have escaped small batches before."""
    _check_fwd(_fwd_case(128, Ci, Co, R, T, 25, seed=T))


def test_forward_ragged_planes():
    """V = 17 (K400's joints), T = 4: 68-position planes"""
    _check_fwd(_fwd_case(3, 64, 24, 72, 4, 17, seed=17))


def test_forward_pair_not_hosted_still_written():
    """a host with an affine + ReLU operand is not one of the `pre` conv's kernels: the guest goes out alone from the same
    call (hosted = 0) and its output is written all the same"""
    g = torch.Generator().manual_seed(5)
    a1 = ((torch.rand(64, generator=g) + 0.5).to(DEV), _rand(g, 64, scale=0.3))
    _check_fwd(_fwd_case(3, 64, 24, 72, 8, 25, seed=3, a1=a1, relu=True), want_hosted=0)


def test_forward_no_guest_is_todays_entry_point():
    c = _fwd_case(3, 64, 24, 72, 8, 25, seed=9)
    lib = native.lib()
    z0, p0, _, _ = _run_fwd(c, False)
    z, partial = _nan(3, 24, 8, 25), _nan(c['rows'], 24, 2)
    hosted = ctypes.c_int(-1)
    rc = lib.dsgcn_pwconv_fwd_ws_guest(_ptr(c['x']), None, None, None, None, None, 0, _ptr(c['w']), _ptr(c['b']), _ptr(z), None,
                                       _ptr(partial), 3, 64, 24, 8, 25, 1, 0, 1, None, None, ctypes.byref(hosted), None)
    native.check(rc, 'dsgcn_pwconv_fwd_ws_guest')
    torch.cuda.synchronize()
    assert hosted.value == 0 and torch.equal(z, z0) and torch.equal(partial, p0)


# ---- backward: the projection's data gradient in the `pre` conv's backward launch ---------------------------------------------

def _bwd_case(n, Ci, Co, R, T, V, seed, a1=None, relu=False):
    """host: the backward of x (n, Ci, T, V) -> z (n, Co, T, V) with batch-statistics terms (A0, B0); guest: dproj
    (n, R, 1, 32) -> dxbar (n, Ci, 1, 32)"""
    g = torch.Generator().manual_seed(seed)
    lib = native.lib()
    c = dict(n=n, Ci=Ci, Co=Co, R=R, T=T, V=V, a1=a1, relu=relu)
    c['x'] = _rand(g, n, Ci, T, V)
    c['w'] = _rand(g, Co, Ci, scale=Ci ** -0.5)
    c['z'] = _rand(g, n, Co, T, V)
    c['gz'] = _rand(g, n, Co, T, V)
    c['A0'] = _rand(g, Co, scale=0.1)
    c['B0'] = _rand(g, Co, scale=0.1)
    c['dproj'] = _rand(g, n, R, 1, 32)
    c['wp'] = _rand(g, R, Ci, scale=Ci ** -0.5)
    c['xbar'] = _rand(g, n, Ci, 1, 32)
    c['ws'] = _ws(c['w'], n, Ci, Co, T, V)
    c['rows'] = lib.dsgcn_pwconv_bwd_rows(n, Ci, Co, T, V, 1)          # > 0: the one-pass narrow backward
    c['irows'] = lib.dsgcn_pwconv_ipart_rows(n, Ci, Co, T, V, 1)
    return c


def _run_bwd(c, together):
    """-> (dict of the host's outputs, dxbar, hosted)"""
    lib = native.lib()
    n, Ci, Co, R, T, V = (c[k] for k in ('n', 'Ci', 'Co', 'R', 'T', 'V'))
    s1, h1 = c['a1'] if c['a1'] is not None else (None, None)
    dx, dxbar = _nan(n, Ci, T, V), _nan(n, Ci, 1, 32)
    ipart = _nan(c['rows'] if c['rows'] else c['irows'], Ci, 3) if s1 is not None else None
    outs = dict(dx=dx)
    if ipart is not None:
        outs['ipart'] = ipart
    hosted = ctypes.c_int(-1)
    g = _guest(c['dproj'], c['wp'], None, dxbar)
    g.Ci, g.Co = Ci, R
    tail = (ctypes.addressof(g), ctypes.byref(hosted), None) if together else (None,)
    if c['rows']:
        pstride = Co * Ci + Co
        wpart = _nan(c['rows'], pstride)
        outs['wpart'] = wpart
        fn = lib.dsgcn_pwconv_bwd_guest if together else lib.dsgcn_pwconv_bwd
        rc = fn(_ptr(c['x']), _ptr(s1), _ptr(h1), None, None, None, int(c['relu']), _ptr(c['w']), _ptr(c['z']), _ptr(c['gz']),
                _ptr(c['A0']), _ptr(c['B0']), _ptr(dx), None, _ptr(ipart), wpart.data_ptr(), wpart.data_ptr() + 4 * Co * Ci,
                pstride, n, Ci, Co, T, V, *tail)
    else:
        fn = lib.dsgcn_pwconv_dgrad_ws_guest if together else lib.dsgcn_pwconv_dgrad_ws
        rc = fn(_ptr(c['x']), _ptr(s1), _ptr(h1), None, None, None, int(c['relu']), _ptr(c['w']), _ptr(c['z']), None,
                _ptr(c['gz']), None, _ptr(c['A0']), _ptr(c['B0']), _ptr(dx), None, _ptr(ipart), n, Ci, Co, T, V, 1, 0,
                _ptr(c['ws']), *tail)
    native.check(rc, 'host backward')
    if not together:
        rc = lib.dsgcn_pwconv_dgrad_ws(_ptr(c['xbar']), None, None, None, None, None, 0, _ptr(c['wp']), None, None,
                                       _ptr(c['dproj']), None, None, None, _ptr(dxbar), None, None, n, Ci, R, 1, 32, 1, 0,
                                       None, None)
        native.check(rc, 'dsgcn_pwconv_dgrad_ws')
    torch.cuda.synchronize()
    return outs, dxbar, hosted.value


def _check_bwd(c, want_hosted):
    o0, q0, _ = _run_bwd(c, False)
    o1, q1, hosted = _run_bwd(c, True)
    assert hosted == want_hosted
    if c['a1'] is None:
        g = _guest(c['dproj'], c['wp'], None, q1)
        g.Ci, g.Co = c['Ci'], c['R']
        assert native.lib().dsgcn_pwconv_guest_hosted(1, c['n'], c['Ci'], c['Co'], c['T'], c['V'], 1, ctypes.addressof(g)) == hosted
    for name in o0:
        assert not torch.isnan(o1[name]).any(), name
        assert torch.equal(o0[name], o1[name]), name
    assert not torch.isnan(q1).any() and torch.equal(q0, q1)
    # the bound of check_pwconv (tests/test_kernels_gpu.py) for a data gradient
    assert rel(q1, torch.einsum('oc,notv->nctv', c['wp'].double(), c['dproj'].double())) < 2e-5
    if c['a1'] is None:
        dz = c['gz'].double() + c['A0'].double().view(1, -1, 1, 1) + c['B0'].double().view(1, -1, 1, 1) * c['z'].double()
        assert rel(o1['dx'], torch.einsum('oc,notv->nctv', c['w'].double(), dz)) < 2e-5


# 128 -> 48 at n = 3: too few position groups for two row tiles per wave, so the data gradient runs on k_pw4<1, 4, 2, 8, 1>,
# which no shipped step uses for a `pre` conv and which hosts nothing (its full-size launch is hosted: the case below)
@pytest.mark.parametrize('Ci,Co,R,hosted', [s + (0 if s[:2] == (128, 48) else 1,) for s in SHAPES])
def test_backward_pair_bit_equal(Ci, Co, R, hosted):
    """n = 3, T = 8, V = 25: k_bwd64<true, false, false> (3 -> 24), k_bwd64b<true, false> (64 -> 24 / 48),
    k_pwg3<2, 1, 1> (128 -> 96), k_pwg3<2, 1, 2> (256 -> 96)"""
    n = _wide_n(Ci, Co, 8, 25, 3)
    _check_bwd(_bwd_case(n, Ci, Co, R, 8, 25, seed=Ci * 5 + Co), hosted)


@pytest.mark.parametrize('Ci,Co,R,T', [(64, 24, 72, 64), (256, 96, 288, 16), (128, 48, 144, 32)])
def test_backward_pair_full_size(Ci, Co, R, T):
    """n = 128, one case per host family; 128 -> 48 at T = 32 is block 6's launch on k_pw4<2, 4, 2, 8, 1, false>"""
    _check_bwd(_bwd_case(128, Ci, Co, R, T, 25, seed=T + 1), 1)


def test_backward_ragged_planes():
    """V = 17 (K400's joints), T = 4"""
    _check_bwd(_bwd_case(3, 64, 24, 72, 4, 17, seed=18), 1)


def test_backward_pair_not_hosted_still_written():
    """a narrow host whose input carries an affine + ReLU runs k_bwd64b<true, true>, none of the `pre` conv's kernels:
    hosted = 0, dxbar written by a launch of its own from the same call"""
    g = torch.Generator().manual_seed(6)
    a1 = ((torch.rand(64, generator=g) + 0.5).to(DEV), _rand(g, 64, scale=0.3))
    _check_bwd(_bwd_case(3, 64, 24, 72, 8, 25, seed=4, a1=a1, relu=True), 0)


def test_backward_no_guest_is_todays_entry_point():
    lib = native.lib()
    for Ci, Co in ((64, 24), (256, 96)):
        c = _bwd_case(3, Ci, Co, 72, 8, 25, seed=10)
        o0, _, _ = _run_bwd(c, False)
        dx = _nan(3, Ci, 8, 25)
        hosted = ctypes.c_int(-1)
        if c['rows']:
            pstride = Co * Ci + Co
            wpart = _nan(c['rows'], pstride)
            rc = lib.dsgcn_pwconv_bwd_guest(_ptr(c['x']), None, None, None, None, None, 0, _ptr(c['w']), _ptr(c['z']),
                                            _ptr(c['gz']), _ptr(c['A0']), _ptr(c['B0']), _ptr(dx), None, None, wpart.data_ptr(),
                                            wpart.data_ptr() + 4 * Co * Ci, pstride, 3, Ci, Co, 8, 25, None,
                                            ctypes.byref(hosted), None)
        else:
            rc = lib.dsgcn_pwconv_dgrad_ws_guest(_ptr(c['x']), None, None, None, None, None, 0, _ptr(c['w']), _ptr(c['z']), None,
                                                 _ptr(c['gz']), None, _ptr(c['A0']), _ptr(c['B0']), _ptr(dx), None, None, 3, Ci,
                                                 Co, 8, 25, 1, 0, _ptr(c['ws']), None, ctypes.byref(hosted), None)
        native.check(rc, 'guest entry point without a guest')
        torch.cuda.synchronize()
        assert hosted.value == 0 and torch.equal(dx, o0['dx'])
        if c['rows']:
            assert torch.equal(wpart, o0['wpart'])


# ---- unit level ------------------------------------------------------------------------------------------------------------

def _unit_run(i, switch):
    from oracle import dsgcn_oracle as O
    from test_oracle_golden import load, sd_of
    z = load('unit_dgphgcn1.npz')
    tag = f'u{i}_'
    sd = sd_of(z, tag + 'sd_', torch.float32)
    Co, Ci = sd['post.weight'].shape[0], sd['pre.0.weight'].shape[1]
    gc = O.graph_constants('nturgb+d')
    m = D.dgphgcn1(Ci, Co, sd['A'].clone(), torch.as_tensor(gc['edge_type']).float(), torch.as_tensor(gc['node_type']),
                   ratio=0.125, decompose=True, node_attention=True, edge_attention=True, subset_wise=True, ctr='T', ada='T')
    m.load_state_dict(sd)
    m = m.cuda().train()
    x = torch.from_numpy(z[tag + 'x']).cuda().requires_grad_()
    old, before = K.PROJ_GUEST, dict(K.PROJ_GUEST_COUNTS)
    K.PROJ_GUEST = switch
    try:
        y = m(x)
        (y * torch.from_numpy(z[tag + 'R']).cuda()).sum().backward()
        torch.cuda.synchronize()
    finally:
        K.PROJ_GUEST = old
    out = dict(y=y.detach().cpu(), dx=x.grad.cpu())
    out.update({k: p.grad.cpu() for k, p in m.named_parameters() if p.grad is not None})
    return out, _counts_since(before)


def _counts_since(before):
    return {k: v - before[k] for k, v in K.PROJ_GUEST_COUNTS.items()}


def _expected_counts(switch, units):
    """what `units` forward + backward passes of a shipped dgphgcn1 must leave in kernels.PROJ_GUEST_COUNTS: every
    projection hosted in the directions that are on, nothing launched beside its host, nothing left to the fence"""
    f, b = (units if switch & 1 else 0), (units if switch & 2 else 0)
    return dict(fwd_hosted=f, fwd_alone=0, dgrad_parked=b, dgrad_hosted=b, dgrad_alone=0, dgrad_flushed=0)


@pytest.mark.parametrize('i', [0, 1, 2])
def test_unit_bit_equal_across_the_switch(i):
    """dgphgcn1 forward + backward on tests/golden/unit_dgphgcn1.npz: output, input gradient and every parameter gradient
    carry the same bits with PROJ_GUEST = 3 / 1 / 2 / 0"""
    base, counts = _unit_run(i, 0)
    assert len(base) >= 8 and counts == _expected_counts(0, 1)
    for switch in (3, 1, 2):
        got, counts = _unit_run(i, switch)
        # the path under test ran: the `pre` conv's launches carried the projection, the backward parked and hosted it
        assert counts == _expected_counts(switch, 1), (switch, counts)
        assert got.keys() == base.keys()
        for k in base:
            assert torch.equal(got[k], base[k]), (switch, k)


# ---- engine level ----------------------------------------------------------------------------------------------------------

def _engine_params(switch, use_graph):
    from grad_accum_fp64 import SGD, micro_batches, reduced_model
    old, before = K.PROJ_GUEST, dict(K.PROJ_GUEST_COUNTS)
    K.PROJ_GUEST = switch
    try:
        eng = D.TrainEngine(reduced_model().cuda(), warmup_eager=1, use_graph=use_graph, **SGD)
        for kp, lb in micro_batches(2):
            eng.step(kp.cuda(), lb.cuda())
        torch.cuda.synchronize()
        assert eng.capture_error is None
    finally:
        K.PROJ_GUEST = old
    # every dgphgcn1 of the model hosts its projections' forward, once per Python pass over it (eager steps and captures;
    # replays make no calls).  The reduced model's projections are narrow enough (rows <= 64) for the one-pass backward,
    # which computes their data gradient with the weight gradient: nothing is parked there — what IS parked must be
    # hosted, and nothing may go out beside its host or be left to the fence
    units = sum(isinstance(m, D.dgphgcn1) for m in eng.model.modules())
    got = _counts_since(before)
    assert units > 0 and got['fwd_hosted'] == (2 * units if switch & 1 else 0), got
    assert got['dgrad_hosted'] == got['dgrad_parked'] and (switch & 2 or not got['dgrad_parked']), got
    assert got['fwd_alone'] == got['dgrad_alone'] == got['dgrad_flushed'] == 0, got
    return eng.flat.flat_p.cpu()


@pytest.mark.parametrize('use_graph', [False, True])
def test_engine_steps_bit_equal_across_the_switch(use_graph):
    """the reduced DS-STGCN, two TrainEngine steps, eager and graphed: the parameters after them are the same bits with
    the guests on and off.  At this level only the FORWARD guest path is shown to be alive (exact counts in
    _engine_params): the reduced model's projections have at most 64 rows, so their backward is the one-pass kernel and
    no data gradient is ever parked — the count check there holds with 0 = 0.  That the backward path parks and hosts is
    asserted with exact counts by test_unit_bit_equal_across_the_switch, whose units have 72-row projections."""
    assert torch.equal(_engine_params(3, use_graph), _engine_params(0, use_graph))
