"""CPU: the guest entry points (dsgcn_pwconv_fwd_ws_guest / _dgrad_ws_guest / _bwd_guest) reject bad records before any
launch, and dsgcn_pwconv_guest_hosted answers which (host, guest) pairs share a launch — host-side code only, nothing here
touches a device (the pointers of the eligibility queries are never dereferenced)."""
import ctypes

import pytest

from dsgcn_amd import kernels as K
from dsgcn_amd import native

P = 0x1000          # a non-NULL "device pointer" for calls that must fail, or only plan, before touching memory

# (Ci -> Co_pre, guest rows) of DS-STGCN's ten blocks
SHAPES = [(3, 24, 72), (64, 24, 72), (64, 48, 144), (128, 48, 144), (128, 96, 288), (256, 96, 288)]


def guest(inp=P, w=P, out=P, n=3, Ci=64, Co=72, L=32):
    return native.GuestConv(inp, w, None, out, n, Ci, Co, L)


BAD = [dict(inp=None), dict(w=None), dict(out=None), dict(n=0), dict(Ci=0), dict(Co=-1), dict(L=0)]


@pytest.mark.parametrize('bad', BAD)
def test_bad_guest_records_are_rejected_before_any_launch(bad):
    lib = native.lib()
    g = guest(**bad)
    hosted = ctypes.c_int(7)
    rc = lib.dsgcn_pwconv_fwd_ws_guest(P, None, None, None, None, None, 0, P, None, P, None, None, 3, 64, 24, 8, 25, 1, 0, 0, None,
                                       ctypes.addressof(g), ctypes.byref(hosted), None)
    assert rc == -1 and hosted.value == 0
    rc = lib.dsgcn_pwconv_dgrad_ws_guest(P, None, None, None, None, None, 0, P, P, None, P, None, P, P, P, None, None, 3, 128, 96, 8,
                                         25, 1, 0, None, ctypes.addressof(g), ctypes.byref(hosted), None)
    assert rc == -1 and hosted.value == 0
    rc = lib.dsgcn_pwconv_bwd_guest(P, None, None, None, None, None, 0, P, P, P, P, P, P, None, None, P, P, 64 * 24 + 24, 3, 64, 24,
                                    8, 25, ctypes.addressof(g), ctypes.byref(hosted), None)
    assert rc == -1 and hosted.value == 0
    for d in (0, 1):
        assert lib.dsgcn_pwconv_guest_hosted(d, 3, 64, 24, 8, 25, 1, ctypes.addressof(g)) == 0


def test_bad_host_arguments_are_rejected_as_without_a_guest():
    lib = native.lib()
    g = guest()
    # NULL host operands / sizes: DSGCN_EINVAL exactly as dsgcn_pwconv_fwd_ws / _dgrad_ws / _bwd give it
    assert lib.dsgcn_pwconv_fwd_ws_guest(None, None, None, None, None, None, 0, P, None, P, None, None, 3, 64, 24, 8, 25, 1, 0, 0,
                                         None, ctypes.addressof(g), None, None) == -1
    assert lib.dsgcn_pwconv_fwd_ws_guest(P, None, None, None, None, None, 0, P, None, P, None, None, 0, 64, 24, 8, 25, 1, 0, 0,
                                         None, None, None, None) == -1
    assert lib.dsgcn_pwconv_dgrad_ws_guest(P, None, None, None, None, None, 0, P, None, None, P, None, P, None, P, None, None, 3,
                                           128, 96, 8, 25, 1, 0, None, ctypes.addressof(g), None, None) == -1      # A0 without B0
    assert lib.dsgcn_pwconv_bwd_guest(P, None, None, None, None, None, 0, P, P, None, P, P, P, None, None, P, P, 64 * 24 + 24, 3,
                                      64, 24, 8, 25, ctypes.addressof(g), None, None) == -1                        # no gz
    assert lib.dsgcn_pwconv_bwd_guest(P, None, None, None, None, None, 0, P, P, P, P, P, P, None, None, P, P, 5, 3, 64, 24, 8, 25,
                                      ctypes.addressof(g), None, None) == -1                                       # pstride too small


@pytest.mark.parametrize('Ci,Co,R', SHAPES)
def test_the_model_shapes_are_hosted(Ci, Co, R):
    """at the shipped batch (n = 128 person-samples) every `pre` conv hosts its block's projections, both ways"""
    lib = native.lib()
    T = 64 if Ci <= 64 else (32 if Ci == 128 else 16)          # frames at that block
    g = guest(n=128, Ci=Ci, Co=R)
    assert lib.dsgcn_pwconv_guest_hosted(0, 128, Ci, Co, T, 25, 1, ctypes.addressof(g)) == 1
    assert lib.dsgcn_pwconv_guest_hosted(1, 128, Ci, Co, T, 25, 1, ctypes.addressof(g)) == 1


def test_pairs_that_are_not_hosted():
    lib = native.lib()
    g = guest()
    assert lib.dsgcn_pwconv_guest_hosted(0, 3, 64, 24, 8, 25, 1, ctypes.addressof(g)) == 1
    assert lib.dsgcn_pwconv_guest_hosted(0, 3, 64, 24, 8, 25, 2, ctypes.addressof(g)) == 0      # strided host: first-generation kernel
    big_g = guest(n=128, Ci=32)
    assert lib.dsgcn_pwconv_guest_hosted(0, 128, 32, 64, 64, 25, 1, ctypes.addressof(big_g)) == 0   # two row tiles: k_pw4<2, 4, 0, ...>
    assert lib.dsgcn_pwconv_guest_hosted(2, 3, 64, 24, 8, 25, 1, ctypes.addressof(g)) == 0      # no such direction
    big = guest(L=200)                                                                          # not a tiny-plane conv
    assert lib.dsgcn_pwconv_guest_hosted(0, 3, 64, 24, 8, 25, 1, ctypes.addressof(big)) == 0
    assert lib.dsgcn_pwconv_guest_hosted(1, 3, 64, 24, 8, 25, 1, ctypes.addressof(big)) == 0
    odd = guest(L=25)
    assert lib.dsgcn_pwconv_guest_hosted(0, 3, 64, 24, 8, 25, 1, ctypes.addressof(odd)) == 0


def test_switch_and_request_on_the_host():
    import torch
    assert K.PROJ_GUEST == 3                       # both directions on by default
    # operands the kernels cannot read in place (here: host tensors) give a request without an output slot: nothing is
    # hosted or parked, the projection's own call reuses the prepared operands
    xbar = torch.zeros(2, 8, 32)
    w, b = [torch.zeros(4, 8)], [torch.zeros(4)]
    req = K._proj_guest_request(xbar, 25, w, b)
    assert req.t is None and req.token is None and req.x.shape == (2, 8, 1, 32) and req.w is w[0]
    old = K.PROJ_GUEST
    K.PROJ_GUEST = 0
    try:
        assert K._proj_guest_request(xbar, 25, w, b) is None
    finally:
        K.PROJ_GUEST = old
    before = dict(K.PROJ_GUEST_COUNTS)
    tok = K._GuestToken()
    ran = []
    tok.job = (None, lambda: ran.append(1))
    tok.flush()
    tok.flush()
    assert ran == [1] and tok.job is None          # a parked job goes out exactly once
    assert K.PROJ_GUEST_COUNTS['dgrad_flushed'] == before['dgrad_flushed'] + 1
