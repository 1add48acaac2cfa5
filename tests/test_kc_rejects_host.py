"""CPU: K-C's host layer (csrc/pwconv.hip and the reductions of csrc/reduce.hip) answers as it did before its entry points
were regrouped.  Two tables, both RECORDED by running this file's calls against the library built from the commit before
that change — never taken from the code under test:

  * REJECTS: calls an entry point refuses before any launch (nothing here touches a device; the non-NULL "device pointers"
    are never dereferenced) and the code it returns: -1 DSGCN_EINVAL, -2 DSGCN_EUNSUPPORTED;
  * QUERIES: the pure shape queries (partial-row counts, split counts, weight-image bytes, bf16 term counts, grouped /
    hosted eligibility, column-sum blocks) at a handful of shapes, stride 1 and 2 where the query takes a stride."""
import ctypes

import pytest

from dsgcn_amd import native

P = 0x1000          # a non-NULL, 16-byte aligned "device pointer"
N, CI, CO, T, V = 2, 64, 64, 8, 25


def guest(**kw):
    f = dict(inp=P, w=P, bias=None, out=P, n=3, Ci=64, Co=72, L=32)
    f.update(kw)
    return native.GuestConv(f['inp'], f['w'], f['bias'], f['out'], f['n'], f['Ci'], f['Co'], f['L'])


def coef_job(**kw):
    f = dict(part=P, mean=P, var=P, gamma=None, coef=P, count=100.0, eps=1e-5, R=8, C=64, k=3, i_ds=0, i_dh=1, c_affine=64,
             accumulate=0)
    f.update(kw)
    return native.BnCoefJob(*[f[name] for name, _ in native.BnCoefJob._fields_])


def fin_job(**kw):
    f = dict(partial=P, gamma=None, beta=None, mean=P, var=P, scale=P, shift=P, count=100.0, eps=1e-5, nblk=8, C=64, c_affine=64)
    f.update(kw)
    return native.BnFinJob(*[f[name] for name, _ in native.BnFinJob._fields_])


# every builder returns (entry point, argument list) of a call that is VALID up to the launch; a case overrides one or two
# of its named operands
def fwd(guest_rec=False, **kw):
    f = dict(x1=P, s1=None, h1=None, x2=None, s2=None, h2=None, relu=0, w=P, bias=None, z=P, zaug=None, partial=None, n=N, Ci=CI,
             Co=CO, T=T, V=V, stride=1, aug=0, stats=0, ws=None)
    f.update(kw)
    args = [f[k] for k in ('x1', 's1', 'h1', 'x2', 's2', 'h2', 'relu', 'w', 'bias', 'z', 'zaug', 'partial', 'n', 'Ci', 'Co', 'T', 'V',
                           'stride', 'aug', 'stats', 'ws')]
    if guest_rec is False:
        return 'dsgcn_pwconv_fwd_ws', args + [None]
    return 'dsgcn_pwconv_fwd_ws_guest', args + [guest_rec, None, None]


def dgrad(guest_rec=False, **kw):
    f = dict(x1=P, s1=None, h1=None, x2=None, s2=None, h2=None, relu=0, w=P, z=P, zaug=None, gz=P, gzaug=None, A0=None, B0=None,
             dx1=P, dx2=None, ipart=None, n=N, Ci=CI, Co=CO, T=T, V=V, stride=1, aug=0, ws=None)
    f.update(kw)
    args = [f[k] for k in ('x1', 's1', 'h1', 'x2', 's2', 'h2', 'relu', 'w', 'z', 'zaug', 'gz', 'gzaug', 'A0', 'B0', 'dx1', 'dx2',
                           'ipart', 'n', 'Ci', 'Co', 'T', 'V', 'stride', 'aug', 'ws')]
    if guest_rec is False:
        return 'dsgcn_pwconv_dgrad_ws', args + [None]
    return 'dsgcn_pwconv_dgrad_ws_guest', args + [guest_rec, None, None]


def wgrad(jobs=None, **kw):
    arr = (native.BnCoefJob * len(jobs))(*jobs) if jobs else None
    f = dict(x1=P, s1=None, h1=None, x2=None, s2=None, h2=None, relu=0, z=P, zaug=None, gz=P, gzaug=None, A0=None, B0=None, dwp=P,
             dbp=P, pstride=CO * CI + CO, n=N, Ci=CI, Co=CO, T=T, V=V, stride=1, aug=0, jobs=arr, njobs=len(jobs) if jobs else 0)
    f.update(kw)
    return 'dsgcn_pwconv_wgrad_jobs', [f[k] for k in (
        'x1', 's1', 'h1', 'x2', 's2', 'h2', 'relu', 'z', 'zaug', 'gz', 'gzaug', 'A0', 'B0', 'dwp', 'dbp', 'pstride', 'n', 'Ci', 'Co',
        'T', 'V', 'stride', 'aug', 'jobs', 'njobs')] + [None]


def bwd(guest_rec=False, **kw):
    f = dict(x1=P, s1=None, h1=None, x2=None, s2=None, h2=None, relu=0, w=P, z=P, gz=P, A0=None, B0=None, dx1=P, dx2=None,
             ipart=None, dwp=P, dbp=P, pstride=CO * CI + CO, n=N, Ci=CI, Co=CO, T=T, V=V)
    f.update(kw)
    args = [f[k] for k in ('x1', 's1', 'h1', 'x2', 's2', 'h2', 'relu', 'w', 'z', 'gz', 'A0', 'B0', 'dx1', 'dx2', 'ipart', 'dwp', 'dbp',
                           'pstride', 'n', 'Ci', 'Co', 'T', 'V')]
    if guest_rec is False:
        return 'dsgcn_pwconv_bwd', args + [None]
    return 'dsgcn_pwconv_bwd_guest', args + [guest_rec, None, None]


def colsum(src=P, R=8, C=64, out=P):
    return 'dsgcn_colsum', [src, R, C, out, None]


def colsum2(**kw):
    f = dict(src_a=P, Ra=8, Ca=64, inner_a=1, out_a=P, src_b=P, Rb=8, Cb=66, inner_b=3, out_b=P)
    f.update(kw)
    return 'dsgcn_colsum2', [f[k] for k in ('src_a', 'Ra', 'Ca', 'inner_a', 'out_a', 'src_b', 'Rb', 'Cb', 'inner_b', 'out_b')] + [None]


def bn_finalize(**kw):
    f = dict(partial=P, nblk=8, C=64, count=100.0, gamma=None, beta=None, eps=1e-5, mean=P, var=P, scale=P, shift=P, c_affine=64)
    f.update(kw)
    return 'dsgcn_bn_finalize', [f[k] for k in ('partial', 'nblk', 'C', 'count', 'gamma', 'beta', 'eps', 'mean', 'var', 'scale',
                                                'shift', 'c_affine')] + [None]


def bn_coef_rows(**kw):
    f = dict(part=P, R=8, C=64, k=3, i_ds=0, i_dh=1, mean=P, var=P, gamma=None, eps=1e-5, count=100.0, c_affine=64, coef=P,
             accumulate=0)
    f.update(kw)
    return 'dsgcn_bn_coef_rows', [f[k] for k in ('part', 'R', 'C', 'k', 'i_ds', 'i_dh', 'mean', 'var', 'gamma', 'eps', 'count',
                                                 'c_affine', 'coef', 'accumulate')] + [None]


def multi(name, jobs, njobs=None):
    arr = (type(jobs[0]) * len(jobs))(*jobs) if jobs else None
    return name, [arr, len(jobs) if njobs is None else njobs, None]


G0 = guest()
BAD_GUESTS = [guest(n=0), guest(Ci=0), guest(Co=0), guest(L=0)]

# (what, call, return code recorded at the parent commit)
REJECTS = [
    # a NULL required pointer
    ('fwd: x1 NULL', fwd(x1=None), -1),
    ('fwd: w NULL', fwd(w=None), -1),
    ('fwd: z NULL', fwd(z=None), -1),
    ('fwd: aug without zaug', fwd(aug=1), -1),
    ('fwd: stats without partial', fwd(stats=1), -1),
    ('fwd_guest: x1 NULL', fwd(G0, x1=None), -1),
    ('fwd_guest: guest in NULL', fwd(guest(inp=None)), -1),
    ('fwd_guest: guest w NULL', fwd(guest(w=None)), -1),
    ('fwd_guest: guest out NULL', fwd(guest(out=None)), -1),
    ('dgrad: x1 NULL', dgrad(x1=None), -1),
    ('dgrad: w NULL', dgrad(w=None), -1),
    ('dgrad: dx1 NULL', dgrad(dx1=None), -1),
    ('dgrad_guest: dx1 NULL', dgrad(G0, dx1=None), -1),
    ('dgrad_guest: guest out NULL', dgrad(guest(out=None)), -1),
    ('wgrad_jobs: x1 NULL', wgrad(x1=None), -1),
    ('wgrad_jobs: dwp NULL', wgrad(dwp=None), -1),
    ('wgrad_jobs: dbp NULL', wgrad(dbp=None), -1),
    ('wgrad_jobs: jobs NULL with njobs 1', wgrad(njobs=1), -1),
    ('wgrad_jobs: a job without coef', wgrad(jobs=[coef_job(coef=None)]), -1),
    ('wgrad_jobs: a job with i_ds >= k', wgrad(jobs=[coef_job(i_ds=3)]), -1),
    ('bwd: x1 NULL', bwd(x1=None), -1),
    ('bwd: w NULL', bwd(w=None), -1),
    ('bwd: gz NULL', bwd(gz=None), -1),
    ('bwd: dx1 NULL', bwd(dx1=None), -1),
    ('bwd: dwp NULL', bwd(dwp=None), -1),
    ('bwd: dbp NULL', bwd(dbp=None), -1),
    ('bwd_guest: gz NULL', bwd(G0, gz=None), -1),
    ('bwd_guest: guest w NULL', bwd(guest(w=None)), -1),
    ('colsum: src NULL', colsum(src=None), -1),
    ('colsum: out NULL', colsum(out=None), -1),
    ('colsum: R 0', colsum(R=0), -1),
    ('colsum: C 0', colsum(C=0), -1),
    ('colsum2: src_b NULL', colsum2(src_b=None), -1),
    ('colsum2: out_a NULL', colsum2(out_a=None), -1),
    ('colsum2: inner_a 0', colsum2(inner_a=0), -1),
    ('colsum2: Cb not a multiple of inner_b', colsum2(Cb=64), -1),
    ('bn_finalize: partial NULL', bn_finalize(partial=None), -1),
    ('bn_finalize: shift NULL', bn_finalize(shift=None), -1),
    ('bn_finalize: nblk 0', bn_finalize(nblk=0), -1),
    ('bn_finalize: C 0', bn_finalize(C=0), -1),
    ('bn_coef_rows: part NULL', bn_coef_rows(part=None), -1),
    ('bn_coef_rows: coef NULL', bn_coef_rows(coef=None), -1),
    ('bn_coef_rows: k 0', bn_coef_rows(k=0), -1),
    ('bn_coef_rows: i_dh >= k', bn_coef_rows(i_dh=3), -1),
    ('bn_coef_rows: i_ds < 0', bn_coef_rows(i_ds=-1), -1),
    ('bn_finalize_multi: jobs NULL', ('dsgcn_bn_finalize_multi', [None, 1, None]), -1),
    ('bn_finalize_multi: a job without mean', multi('dsgcn_bn_finalize_multi', [fin_job(), fin_job(mean=None)]), -1),
    ('bn_finalize_multi: a job with C 0', multi('dsgcn_bn_finalize_multi', [fin_job(C=0)]), -1),
    ('bn_coef_rows_multi: jobs NULL', ('dsgcn_bn_coef_rows_multi', [None, 1, None]), -1),
    ('bn_coef_rows_multi: a job without part', multi('dsgcn_bn_coef_rows_multi', [coef_job(part=None)]), -1),
    ('bn_coef_rows_multi: a job with R 0', multi('dsgcn_bn_coef_rows_multi', [coef_job(), coef_job(R=0)]), -1),
    # s1 without h1 (the data gradient does not look at the pair)
    ('fwd: s1 without h1', fwd(s1=P), -1),
    ('fwd: s2 without h2', fwd(x2=P, s2=P), -1),
    ('fwd_guest: s1 without h1', fwd(G0, s1=P), -1),
    ('bwd: s1 without h1', bwd(s1=P), -1),
    ('bwd: s2 without h2', bwd(x2=P, dx2=P, s2=P), -1),
    ('bwd_guest: s1 without h1', bwd(G0, s1=P), -1),
    # x2 without dx2
    ('dgrad: x2 without dx2', dgrad(x2=P), -1),
    ('dgrad_guest: x2 without dx2', dgrad(G0, x2=P), -1),
    ('bwd: x2 without dx2', bwd(x2=P), -1),
    ('bwd_guest: x2 without dx2', bwd(G0, x2=P), -1),
    # A0 without B0 / z
    ('dgrad: A0 without B0', dgrad(A0=P), -1),
    ('dgrad: A0 without z', dgrad(A0=P, B0=P, z=None), -1),
    ('dgrad: aug with A0 and no zaug', dgrad(A0=P, B0=P, aug=1), -1),
    ('dgrad_guest: A0 without B0', dgrad(G0, A0=P), -1),
    ('wgrad_jobs: A0 without B0', wgrad(A0=P), -1),
    ('wgrad_jobs: A0 without z', wgrad(A0=P, B0=P, z=None), -1),
    ('wgrad_jobs: aug with A0 and no zaug', wgrad(A0=P, B0=P, aug=1), -1),
    ('bwd: A0 without B0', bwd(A0=P), -1),
    ('bwd: A0 without z', bwd(A0=P, B0=P, z=None), -1),
    ('bwd_guest: A0 without B0', bwd(G0, A0=P), -1),
    # ipart with a NULL gz
    ('dgrad: ipart with gz NULL', dgrad(gz=None, ipart=P), -1),
    ('dgrad_guest: ipart with gz NULL', dgrad(G0, gz=None, ipart=P), -1),
    # pstride < Co*Ci
    ('wgrad_jobs: pstride too small', wgrad(pstride=CO * CI - 1), -1),
    ('wgrad_jobs: pstride too small, strided', wgrad(pstride=CO * CI - 1, stride=2), -1),
    ('wgrad_jobs: pstride too small, wide', wgrad(pstride=256 * 128 - 1, Ci=128, Co=256), -1),
    ('bwd: pstride too small', bwd(pstride=CO * CI - 1), -1),
    ('bwd_guest: pstride too small', bwd(G0, pstride=5), -1),
    # a guest record with a zero dimension
    *[(f'fwd_guest: guest record {i} with a zero dimension', fwd(g), -1) for i, g in enumerate(BAD_GUESTS)],
    *[(f'dgrad_guest: guest record {i} with a zero dimension', dgrad(g), -1) for i, g in enumerate(BAD_GUESTS)],
    *[(f'bwd_guest: guest record {i} with a zero dimension', bwd(g), -1) for i, g in enumerate(BAD_GUESTS)],
    # njobs out of range
    ('wgrad_jobs: njobs -1', wgrad(njobs=-1), -1),
    ('wgrad_jobs: njobs 5', wgrad(jobs=[coef_job()] * 5), -1),
    ('bn_finalize_multi: njobs 0', multi('dsgcn_bn_finalize_multi', [fin_job()], 0), -1),
    ('bn_finalize_multi: njobs 5', multi('dsgcn_bn_finalize_multi', [fin_job()] * 5), -1),
    ('bn_coef_rows_multi: njobs 0', multi('dsgcn_bn_coef_rows_multi', [coef_job()], 0), -1),
    ('bn_coef_rows_multi: njobs -1', multi('dsgcn_bn_coef_rows_multi', [coef_job()], -1), -1),
    ('bn_coef_rows_multi: njobs 5', multi('dsgcn_bn_coef_rows_multi', [coef_job()] * 5), -1),
    # stride <= 0, and the other sizes
    ('fwd: stride 0', fwd(stride=0), -1),
    ('fwd: stride -1', fwd(stride=-1), -1),
    ('fwd_guest: stride 0', fwd(G0, stride=0), -1),
    ('dgrad: stride 0', dgrad(stride=0), -1),
    ('dgrad_guest: stride -2', dgrad(G0, stride=-2), -1),
    ('wgrad_jobs: stride 0', wgrad(stride=0), -1),
    ('fwd: n 0', fwd(n=0), -1),
    ('dgrad: Ci 0', dgrad(Ci=0), -1),
    ('wgrad_jobs: Co 0', wgrad(Co=0), -1),
    ('bwd: T 0', bwd(T=0), -1),
    ('bwd_guest: V 0', bwd(G0, V=0), -1),
    # what no kernel of the family takes: refused as unsupported, still before any launch
    ('fwd: strided tensor past 32-bit byte offsets', fwd(n=1024, T=64, V=128, stride=2), -2),
    ('wgrad_jobs: strided tensor past 32-bit byte offsets', wgrad(n=1024, T=64, V=128, stride=2), -2),
    ('wgrad_jobs: strided, 4 frames of V = 30 past the chunk', wgrad(V=30, stride=2), -2),
    ('bwd: a shape the one-pass backward does not cover', bwd(Ci=128, pstride=128 * CO + CO), -2),
    ('bwd_guest: a shape the one-pass backward does not cover', bwd(G0, Co=96, pstride=96 * CI + 96), -2),
]


def _run(lib, call):
    name, args = call
    args = [ctypes.addressof(a) if isinstance(a, (ctypes.Structure, ctypes.Array)) else a for a in args]
    return getattr(lib, name)(*args)


@pytest.mark.parametrize('what,call,expected', REJECTS, ids=[r[0] for r in REJECTS])
def test_refused_before_any_launch(what, call, expected):
    assert _run(native.lib(), call) == expected


def test_the_table_covers_every_entry_point():
    names = {call[0] for _, call, _ in REJECTS}
    assert names == {'dsgcn_pwconv_fwd_ws', 'dsgcn_pwconv_fwd_ws_guest', 'dsgcn_pwconv_dgrad_ws', 'dsgcn_pwconv_dgrad_ws_guest',
                     'dsgcn_pwconv_wgrad_jobs', 'dsgcn_pwconv_bwd', 'dsgcn_pwconv_bwd_guest', 'dsgcn_colsum', 'dsgcn_colsum2',
                     'dsgcn_bn_finalize', 'dsgcn_bn_coef_rows', 'dsgcn_bn_finalize_multi', 'dsgcn_bn_coef_rows_multi'}


def test_a_refused_guest_call_reports_nothing_hosted():
    lib = native.lib()
    for build in (fwd, dgrad, bwd):
        name, args = build(BAD_GUESTS[0])
        hosted = ctypes.c_int(7)
        args = args[:-2] + [ctypes.byref(hosted), None]
        assert _run(lib, (name, args)) == -1 and hosted.value == 0


# ---- the pure queries ------------------------------------------------------------------------------------------
SHAPES = [(2, 64, 64, 8, 25), (2, 128, 256, 8, 25), (2, 256, 96, 4, 25), (1, 3, 64, 8, 25), (2, 64, 64, 7, 17)]


def queries(lib, n, Ci, Co, T, V):
    """every query at one shape, in a fixed order: stride 1 then 2 where the query takes a stride"""
    g = guest(n=n, Ci=Ci, Co=72, L=32)
    out = []
    for s in (1, 2):
        out += [lib.dsgcn_pwconv_partial_rows(n, Ci, Co, T, V, s, 0), lib.dsgcn_pwconv_partial_rows(n, Ci, Co, T, V, s, 1),
                lib.dsgcn_pwconv_ipart_rows(n, Ci, Co, T, V, s), lib.dsgcn_pwconv_wgrad_splits(n, Ci, Co, T, V, s),
                lib.dsgcn_pwconv_bwd_rows(n, Ci, Co, T, V, s), lib.dsgcn_pwconv_wsplit_bytes(n, Ci, Co, T, V, s)]
        out += [lib.dsgcn_pwconv_terms(d, n, Ci, Co, T, V, s) for d in (0, 1, 2)]
        out += [lib.dsgcn_pwconv_guest_hosted(d, n, Ci, Co, T, V, s, ctypes.addressof(g)) for d in (0, 1)]
    out += [lib.dsgcn_pwconv_group_ok(n, Ci, Co, T, V), lib.dsgcn_colsum_blocks(P, Co * Ci + Co), lib.dsgcn_colsum_blocks(P + 4, Co * Ci + Co),
            lib.dsgcn_colsum_blocks(P, Co)]
    return out


# recorded at the parent commit (matmul precision 'highest', the library's initial level)
QUERIES = {
    (2, 64, 64, 8, 25): [1, 3, 1, 4, 8, 0, 0, 6, 6, 1, 1, 2, 4, 2, 2, 0, 0, 0, 0, 0, 0, 0, 1, 33, 130, 2],
    (2, 128, 256, 8, 25): [4, 6, 4, 26, 0, 589824, 6, 6, 6, 0, 1, 2, 4, 2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 258, 1032, 2],
    (2, 256, 96, 4, 25): [1, 3, 1, 14, 0, 0, 0, 0, 6, 1, 0, 2, 4, 2, 2, 0, 0, 0, 0, 0, 0, 0, 1, 193, 771, 3],
    (1, 3, 64, 8, 25): [1, 2, 1, 2, 4, 0, 0, 0, 0, 1, 1, 1, 2, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 2, 8, 2],
    (2, 64, 64, 7, 17): [1, 3, 1, 2, 0, 0, 0, 0, 0, 1, 0, 2, 4, 2, 2, 0, 0, 0, 0, 0, 0, 0, 1, 33, 130, 2],
}


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_pure_queries_answer_as_recorded(shape):
    lib = native.lib()
    assert lib.dsgcn_get_matmul_precision() == 0
    assert queries(lib, *shape) == QUERIES[shape]


if __name__ == '__main__':        # prints both tables as the loaded library answers them (how the recorded values were taken)
    lib = native.lib()
    for what, call, _ in REJECTS:
        print(f'{_run(lib, call):3d}  {what}')
    for shape in SHAPES:
        print(f'    {shape}: {queries(lib, *shape)},')
