"""Shared by tests/golden/gen_golden_featext.py (which writes tests/golden/featext.npz from the imported reference) and the
feat_ext tests (which read it): the table of kernel cases, the names of the fixture entries and their decoding.

A kernel case is one activation x (videos, clips, M, C, T, V) with fc_cls weights (K, C) [+ bias], run through the
reference's forward_test branch video by video at each (mode, pool_opt) of ``runs(case)``.  Entries of the archive:

    <case>_x          int16 numerators of x = n / 1024 (multiples of 2^-10 in [-2, 2]); float32 for the 'inf' case
    <case>_w, _b      float32 fc_cls.weight / fc_cls.bias (no _b: the head has no bias)
    <case>_<mode>_<pool>_r16   what the reference returns (float16), videos stacked on axis 0
    ..._r32                    the same run before its cast to float16 (float32)
    ..._d64                    int16: (r64 - r32) in steps of ``d64_steps[key]`` = max|r64 - r32| / 32767, r64 = the run with
                               everything .double().  r64 = r32 + step * d64 to 2^-16 of the reference's own fp32 error (a
                               float64 array costs four times as much for nothing more)
    d64_steps                  json: key -> step (float.hex)
``_r16`` is left out above R16_MAX elements: the generator asserts that it is r32.astype(float16) bit for bit.

Model cases: <model>_<mode>_<pool>_{r16,r32,d64} for the reduced models of tests/golden/<model>.npz on ``model_x``."""
import numpy as np

LETTERS = 'nmtv'


def pool_name(mask):
    return ''.join(c for i, c in enumerate(LETTERS) if mask >> i & 1) or 'none'


ALL_POOLS = [pool_name(m) for m in range(16)]

# name: videos, clips, M, C, T, V, K, bias, pools run in both modes, extra (mode, pool) runs
CASES = {
    # every mask, both modes
    'all': dict(videos=2, clips=3, M=2, C=8, T=3, V=5, K=7, bias=True, pools=ALL_POOLS),
    # C no multiple of 4 (nor 8: scalar weight loads on the matrix-core form), 100 positions = 3 tiles + 4; (T, V) planes
    # of 100 elements for the plane reduction
    'c70': dict(videos=1, clips=1, M=1, C=70, T=4, V=25, K=11, bias=True, pools=['t', 'tv'], extra=[('score', 'none')]),
    # K crosses the 128 classes the four waves take per round (and is no multiple of 32); 33 positions; 11 positions
    'k130': dict(videos=1, clips=1, M=1, C=12, T=3, V=11, K=130, bias=True, pools=['none', 't']),
    'v17t1': dict(videos=1, clips=2, M=2, C=8, T=1, V=17, K=7, bias=True, pools=['none', 'v', 'nm', 'mv']),
    'clips10': dict(videos=1, clips=10, M=1, C=8, T=2, V=5, K=7, bias=True, pools=['n', 'none', 'nmtv', 'nt']),
    'videos5': dict(videos=5, clips=2, M=1, C=8, T=2, V=3, K=7, bias=True, pools=['n', 'none', 'tv']),
    # 31 / 32 / 33 positions per video: below one tile (dot products), exactly one, one and a column
    'p31': dict(videos=2, clips=1, M=1, C=16, T=1, V=31, K=7, bias=True, pools=['none']),
    'p32': dict(videos=2, clips=1, M=1, C=16, T=4, V=8, K=7, bias=True, pools=['none']),
    'p33': dict(videos=2, clips=1, M=1, C=16, T=3, V=11, K=7, bias=True, pools=['none']),
    # plane-mean input (T = V = 1)
    'planes': dict(videos=2, clips=3, M=2, C=40, T=1, V=1, K=7, bias=True, pools=['none', 'nm', 'n', 'tv', 'nmtv']),
    'nobias': dict(videos=1, clips=2, M=2, C=8, T=3, V=5, K=7, bias=False, pools=['none', 'nm', 'tv']),
    # whole (T, V) planes of 45 elements under every combination with the outer axes
    'wave': dict(videos=2, clips=3, M=2, C=8, T=5, V=9, K=7, bias=True, pools=['tv', 'ntv', 'mtv', 'nmtv']),
    # feature mode, every pooled extent a power of two: every mean is exact in fp32
    'exact': dict(videos=1, clips=2, M=2, C=8, T=4, V=8, K=None, bias=False, pools=ALL_POOLS, modes=('feat',)),
    # |x| above the float16 range
    'inf': dict(videos=1, clips=1, M=1, C=2, T=1, V=4, K=None, bias=False, pools=['none', 'v'], modes=('feat',)),
}
EXACT = ('exact', 'inf')            # cases whose float16 result must equal the reference's bit for bit

MODELS = ('model_reduced', 'model_reduced_stgcn')
MODEL_RUNS = [('feat', 'nmtv'), ('feat', 'tv'), ('feat', 'none'), ('score', 'none'), ('score', 'nm')]
MODEL_CLIPS, MODEL_M = 3, 2
R16_MAX = 4096


def runs(name):
    c = CASES[name]
    out = [(mode, pool) for pool in c['pools'] for mode in c.get('modes', ('feat', 'score'))]
    return out + list(c.get('extra', []))


def key(name, mode, pool):
    return f'{name}_{mode}_{pool}'


def case_x(z, name):
    """x (videos, clips, M, C, T, V) float32 of a kernel case"""
    x = z[name + '_x']
    return x.astype(np.float32) / np.float32(1024) if x.dtype == np.int16 else x


def steps(z):
    import json
    return {k: float.fromhex(v) for k, v in json.loads(str(z['d64_steps'])).items()}


def delta64(z, k):
    return z[k + '_d64'].astype(np.float64) * steps(z)[k]


def ref64(z, k):
    return z[k + '_r32'].astype(np.float64) + delta64(z, k)


def ref16(z, k):
    return z[k + '_r16'] if k + '_r16' in z else z[k + '_r32'].astype(np.float16)


def errors(got32, z, k):
    """(error of got32, error of the reference's fp32 run, bar): error(a) = max|a - r64| / max|r64|; the bar is twice the
    reference's own error — one fp32 ulp of max|r64| where that error is 0."""
    r64 = ref64(z, k)
    top = np.abs(r64).max()
    if top == 0:
        top = 1.0
    e_got = np.abs(np.asarray(got32, dtype=np.float64) - r64).max() / top
    e_ref = np.abs(delta64(z, k)).max() / top
    bar = 2 * e_ref if e_ref > 0 else float(np.spacing(np.float32(top))) / top
    return e_got, e_ref, bar
