"""The kernel census (tests/test_kernel_census_gpu.py) applied to the models the library ships outside BASELINE: one eager
train_step + backward of each at 64 clips of 2 x 64 frames x 25 joints, 60 classes, with every public op of
dsgcn_amd.kernels wrapped by the same recorders.  MODEL_CASES holds the keys these runs record that FULL_SIZE_CASES (the
BASELINE steps) lacks, and nothing else; every one of them is compared with its fp64 statement at that size by the
check_* helpers of tests/test_kernels_gpu.py.

The partition test at the top needs no GPU: KEYS (the wrapped ops) and UNWRAPPED (the public functions that launch no
kernel of their own, with the reason) must cover the public functions of dsgcn_amd.kernels exactly."""
import pytest

from dsgcn_amd import kernels as K
import test_kernel_census_gpu as KC
from test_kernel_census_gpu import DGMSTCN, FULL_SIZE_CASES, KEYS, UNWRAPPED, _Path, _listing
import test_dghgcn_gpu as TDG
import test_kernels_gpu as KG


def test_every_public_op_is_keyed_or_listed():
    public = KC.public_functions()
    keyed, listed = set(KEYS), set(UNWRAPPED)
    assert not keyed & listed, f'ops both keyed and listed as unwrapped: {sorted(keyed & listed)}'
    new = public - keyed - listed
    assert not new, (f'public functions of dsgcn_amd.kernels outside the census: {sorted(new)} — give each a key in '
                     'test_kernel_census_gpu.KEYS (and fp64 checks of the keys the models record), or list it in UNWRAPPED '
                     'with the reason it launches no kernel of its own')
    gone = (keyed | listed) - public
    assert not gone, f'KEYS / UNWRAPPED name functions dsgcn_amd.kernels no longer has: {sorted(gone)}'


# ---------------------------------------------------------------------------------------------------------------------
# the model runs
# ---------------------------------------------------------------------------------------------------------------------

MODEL_RUNS = (
    # (name, model, clips, T, V, classes, dropout kept?)
    ('stgcn_shipped', 'stgcn_shipped', 64, 64, 25, 60, False),    # unit_gcn + unitmlp (k = 9)
    ('ctrgcn_shipped', 'ctrgcn_shipped', 64, 64, 25, 60, False),  # unit_ctrhgcn + msmlp
    ('stgcnpp', 'stgcnpp', 64, 64, 25, 60, False),                # mstcn with the 6-branch cfg
    ('aagcn', 'aagcn', 64, 64, 25, 60, False),
    ('dggcn', 'dggcn', 64, 64, 25, 60, False),
    ('dghgcn', 'dghgcn', 64, 64, 25, 60, False),                  # DGSTGCN's default gcn_type
)


def _model_cfg(model):
    from bench import other_cfg
    if model == 'dghgcn':
        from test_dghgcn_gpu import DGH_CFG          # not ds_cfg(): that carries dgphgcn1's flags (gcn_decompose, ...)
        return DGH_CFG
    return other_cfg(model)


MODEL_CASES = {
    # (n, K, Co, T, V, adjacency form, want_bn)
    'aggregate_sum': [
        (128, 3, 128, 32, 25, 'per_channel', True),   # ctrgcn_shipped
        (128, 3, 128, 32, 25, 'per_sample', True),   # aagcn
        (128, 3, 128, 64, 25, 'per_channel', True),   # ctrgcn_shipped
        (128, 3, 128, 64, 25, 'per_sample', True),   # aagcn
        (128, 3, 256, 16, 25, 'per_channel', True),   # ctrgcn_shipped
        (128, 3, 256, 16, 25, 'per_sample', True),   # aagcn
        (128, 3, 256, 32, 25, 'per_channel', True),   # ctrgcn_shipped
        (128, 3, 256, 32, 25, 'per_sample', True),   # aagcn
        (128, 3, 64, 64, 25, 'per_channel', True),   # ctrgcn_shipped
        (128, 3, 64, 64, 25, 'per_sample', True),   # aagcn
    ],
    # (BatchNorms): one launch for every layer's running statistics (test_bn_running_update_matches_batch_norm)
    'bn_running_update': [
        (25,),   # aagcn
    ],
    # (n, Ci, Co, V, subsets, R, subset_major, path, (alpha elements, beta, edge subsets, edge classes E))
    'ctr_topology': [
        (128, 128, 128, 25, 3, 16, False, 'per_subset', (3, True, (0,), 15)),   # ctrgcn_shipped
        (128, 128, 256, 25, 3, 16, False, 'per_subset', (3, True, (0,), 15)),   # ctrgcn_shipped
        (128, 256, 256, 25, 3, 32, False, 'per_subset', (3, True, (0,), 15)),   # ctrgcn_shipped
        (128, 3, 64, 25, 3, 8, False, 'per_subset', (3, True, (0,), 15)),   # ctrgcn_shipped
        (128, 64, 128, 25, 3, 8, False, 'per_subset', (3, True, (0,), 15)),   # ctrgcn_shipped
        (128, 64, 64, 25, 3, 8, False, 'per_subset', (3, True, (0,), 15)),   # ctrgcn_shipped
    ],
    # (n, Ci, mid, V, xbar row length, BatchNorm jobs hosted, False: single_use=False)
    'dynadj': [
        (128, 128, 16, 25, 32, False, False),   # dggcn
        (128, 128, 32, 25, 32, False, False),   # dggcn
        (128, 256, 32, 25, 32, False, False),   # dggcn
        (128, 3, 8, 25, 25, False, False),   # dggcn
        (128, 64, 16, 25, 32, False, False),   # dggcn
        (128, 64, 8, 25, 32, False, False),   # dggcn
    ],
    # (n, Ci, 3*mid, V, xbar row length, node types P, edge classes E, add_type, single_use)
    'dynadj_typed': [
        (128, 128, 48, 25, 32, 5, 15, False, True),   # dghgcn
        (128, 128, 96, 25, 32, 5, 15, False, True),   # dghgcn
        (128, 256, 96, 25, 32, 5, 15, False, True),   # dghgcn
        (128, 3, 24, 25, 32, 5, 15, False, True),   # dghgcn
        (128, 64, 24, 25, 32, 5, 15, False, True),   # dghgcn
        (128, 64, 48, 25, 32, 5, 15, False, True),   # dghgcn
    ],
    # (n, C, T, V, mode, relu flags, time-mean ld (0: none), tee, dropout, prestrided_fits)
    'fuse_out': [
        (128, 128, 32, 25, 'affine', 1, 0, 0, False, True),   # stgcn_shipped
        (128, 128, 32, 25, 'res_affine', 1, 25, 1, False, True),   # ctrgcn_shipped
        (128, 128, 32, 25, 'res_plain', 1, 25, 0, False, True),   # aagcn
        (128, 128, 32, 25, 'res_plain', 1, 25, 1, False, True),   # ctrgcn_shipped
        (128, 128, 32, 25, 'res_plain', 1, 25, 2, False, True),   # ctrgcn_shipped
        (128, 128, 32, 25, 'res_x1', 0, 0, 0, False, True),   # stgcn_shipped, ctrgcn_shipped
        (128, 128, 64, 25, 'affine', 1, 0, 0, False, True),   # stgcn_shipped
        (128, 128, 64, 25, 'res_affine', 1, 25, 0, False, True),   # aagcn
        (128, 256, 16, 25, 'affine', 1, 0, 0, False, True),   # stgcn_shipped
        (128, 256, 16, 25, 'res_affine', 1, 25, 1, False, True),   # ctrgcn_shipped
        (128, 256, 16, 25, 'res_plain', 1, 25, 0, False, True),   # aagcn
        (128, 256, 16, 25, 'res_plain', 1, 25, 1, False, True),   # ctrgcn_shipped
        (128, 256, 16, 25, 'res_x1', 0, 0, 0, False, True),   # stgcn_shipped, ctrgcn_shipped
        (128, 256, 32, 25, 'affine', 1, 0, 0, False, True),   # stgcn_shipped
        (128, 256, 32, 25, 'res_affine', 1, 25, 0, False, True),   # aagcn
        (128, 64, 64, 25, 'affine', 1, 0, 0, False, True),   # stgcn_shipped
        (128, 64, 64, 25, 'affine', 1, 25, 1, False, True),   # ctrgcn_shipped
        (128, 64, 64, 25, 'res_affine', 1, 25, 0, False, True),   # aagcn
        (128, 64, 64, 25, 'res_plain', 1, 25, 0, False, True),   # aagcn
        (128, 64, 64, 25, 'res_plain', 1, 25, 1, False, True),   # ctrgcn_shipped
        (128, 64, 64, 25, 'res_plain', 1, 25, 2, False, True),   # ctrgcn_shipped
        (128, 64, 64, 25, 'res_x1', 0, 0, 0, False, True),   # stgcn_shipped, ctrgcn_shipped
    ],
    # (n, C, T, V, gate mode, mean mode)
    'gate': [
        (128, 128, 32, 25, 0, 1),   # aagcn
        (128, 128, 32, 25, 1, 2),   # aagcn
        (128, 128, 32, 25, 2, 0),   # aagcn
        (128, 128, 64, 25, 0, 1),   # aagcn
        (128, 128, 64, 25, 1, 2),   # aagcn
        (128, 128, 64, 25, 2, 0),   # aagcn
        (128, 256, 16, 25, 0, 1),   # aagcn
        (128, 256, 16, 25, 1, 2),   # aagcn
        (128, 256, 16, 25, 2, 0),   # aagcn
        (128, 256, 32, 25, 0, 1),   # aagcn
        (128, 256, 32, 25, 1, 2),   # aagcn
        (128, 256, 32, 25, 2, 0),   # aagcn
        (128, 64, 64, 25, 0, 1),   # aagcn
        (128, 64, 64, 25, 1, 2),   # aagcn
        (128, 64, 64, 25, 2, 0),   # aagcn
    ],
    # (n, C, T, V)
    'gram': [
        (384, 16, 1, 25),   # ctrgcn_shipped
        (384, 16, 64, 25),   # aagcn
        (384, 32, 1, 25),   # ctrgcn_shipped
        (384, 32, 32, 25),   # aagcn
        (384, 32, 64, 25),   # aagcn
        (384, 64, 16, 25),   # aagcn
        (384, 64, 32, 25),   # aagcn
        (384, 8, 1, 25),   # ctrgcn_shipped
    ],
    # (n, Ci, Co, T, V, stride, aug, mode, want_bn, bias, forward form, backward form)
    'pwconv': [
        (128, 128, 128, 32, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # stgcn_shipped, ctrgcn_shipped
        (128, 128, 160, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # dggcn
        (128, 128, 192, 32, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # aagcn
        (128, 128, 384, 32, 25, 1, False, 'plain', False, False, 'gemm_bf16', 'dgrad_wgrad'),   # aagcn
        (128, 128, 480, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # dghgcn
        (128, 128, 768, 32, 25, 1, False, 'plain', False, False, 'gemm_bf16', 'dgrad_wgrad'),   # aagcn
        (128, 128, 80, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # dggcn
        (128, 128, 96, 32, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # aagcn
        (128, 128, 960, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # dghgcn
        (128, 16, 128, 25, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped
        (128, 16, 240, 25, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped
        (128, 16, 256, 25, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped
        (128, 24, 360, 2, 32, 1, False, 'plain', False, False, 'direct', 'dgrad_wgrad'),   # dghgcn
        (128, 256, 160, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # dggcn
        (128, 256, 192, 16, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # aagcn
        (128, 256, 256, 16, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # stgcn_shipped, ctrgcn_shipped
        (128, 256, 768, 16, 25, 1, False, 'plain', False, False, 'gemm_bf16', 'dgrad_wgrad'),   # aagcn
        (128, 256, 960, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # dghgcn
        (128, 3, 192, 64, 25, 1, False, 'plain', False, False, 'direct', 'dgrad_wgrad'),   # aagcn
        (128, 3, 240, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # dghgcn
        (128, 3, 40, 1, 32, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # dggcn
        (128, 3, 48, 64, 25, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # aagcn
        (128, 32, 256, 25, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped
        (128, 32, 480, 25, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped
        (128, 48, 720, 2, 32, 1, False, 'plain', False, False, 'direct', 'dgrad_wgrad'),   # dghgcn
        (128, 64, 192, 64, 25, 1, False, 'plain', False, False, 'gemm_bf16', 'dgrad_wgrad'),   # aagcn
        (128, 64, 240, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # dghgcn
        (128, 64, 384, 64, 25, 1, False, 'plain', False, False, 'gemm_bf16', 'dgrad_wgrad'),   # aagcn
        (128, 64, 40, 1, 32, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # dggcn
        (128, 64, 48, 64, 25, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # aagcn
        (128, 64, 480, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # dghgcn
        (128, 64, 64, 64, 25, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # stgcn_shipped, ctrgcn_shipped
        (128, 64, 80, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # dggcn
        (128, 64, 96, 64, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # aagcn
        (128, 8, 120, 25, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped
        (128, 8, 128, 25, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped
        (128, 8, 64, 25, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped
        (128, 96, 1440, 2, 32, 1, False, 'plain', False, False, 'direct', 'dgrad_wgrad'),   # dghgcn
    ],
    # (n, Ci, Co, T, V, stride, KT, dilation, want_bn)
    'tconv': [
        (128, 128, 128, 32, 25, 1, 9, 1, False),   # stgcn_shipped
        (128, 128, 128, 64, 25, 2, 9, 1, False),   # stgcn_shipped
        (128, 256, 256, 16, 25, 1, 9, 1, False),   # stgcn_shipped
        (128, 256, 256, 32, 25, 2, 9, 1, False),   # stgcn_shipped
        (128, 64, 64, 64, 25, 1, 9, 1, False),   # stgcn_shipped
    ],
    # (n, Ci, Co, T, V, KT, mode, stride, want_bn, tconv_gemm_ok)
    'tconv_bn': [
        (128, 128, 128, 32, 25, 9, 'plain', 1, True, True),   # aagcn
        (128, 128, 128, 64, 25, 9, 'plain', 2, True, True),   # aagcn
        (128, 256, 256, 16, 25, 9, 'plain', 1, True, True),   # aagcn
        (128, 256, 256, 32, 25, 9, 'plain', 2, True, True),   # aagcn
        (128, 64, 64, 64, 25, 9, 'plain', 1, True, True),   # aagcn
    ],
    # (n, C, T, V, stride, branches, widths, n_act, want_bn, path)
    'temporal_branches_bn': [
        (128, 128, 32, 25, 1, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, True, 'staged'),   # stgcnpp
        (128, 128, 64, 25, 2, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, True, 'staged'),   # stgcnpp
        (128, 256, 16, 25, 1, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, True, 'staged'),   # stgcnpp
        (128, 256, 32, 25, 2, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, True, 'staged'),   # stgcnpp
        (128, 64, 64, 25, 1, DGMSTCN, (14, 10, 10, 10, 10, 10), 54, True, 'staged'),   # stgcnpp
    ],
    # (n, C, T, V, stride, branches, widths, n_act, causal taps KM, merge_after, want_bn)
    'temporal_mlp_bn': [
        (128, 128, 32, 25, 1, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, 2, True, True),   # ctrgcn_shipped
        (128, 128, 64, 25, 2, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, 2, True, True),   # ctrgcn_shipped
        (128, 256, 16, 25, 1, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, 2, True, True),   # ctrgcn_shipped
        (128, 256, 32, 25, 2, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, 2, True, True),   # ctrgcn_shipped
        (128, 64, 64, 25, 1, DGMSTCN, (14, 10, 10, 10, 10, 10), 54, 2, True, True),   # ctrgcn_shipped
    ],
    # (n, C, T, V, stride, causal taps KM, dilations, dense KT, dense dilation, merge_after, want_bn)
    'temporal_unitmlp_bn': [
        (128, 128, 32, 25, 1, 5, (1,), 9, 1, True, True),   # stgcn_shipped
        (128, 128, 64, 25, 2, 5, (1,), 9, 1, True, True),   # stgcn_shipped
        (128, 256, 16, 25, 1, 5, (1,), 9, 1, True, True),   # stgcn_shipped
        (128, 256, 32, 25, 2, 5, (1,), 9, 1, True, True),   # stgcn_shipped
        (128, 64, 64, 25, 1, 5, (1,), 9, 1, True, True),   # stgcn_shipped
    ],
}


@pytest.fixture(scope='module')
def recorded():
    return KC.census(MODEL_RUNS, _model_cfg)


@pytest.mark.gpu
def test_model_census_every_kernel_call_is_in_the_tables(recorded):
    missing = {op: {k: runs for k, runs in keys.items()
                    if k not in FULL_SIZE_CASES.get(op, ()) and k not in MODEL_CASES.get(op, ())}
               for op, keys in recorded.items() if op != KC.BN_PAIRS}
    missing = {op: keys for op, keys in missing.items() if keys}
    assert not missing, 'kernel calls of the model runs that FULL_SIZE_CASES and MODEL_CASES lack:\n' + _listing(missing)


@pytest.mark.gpu
def test_model_census_table_has_no_stale_entries(recorded):
    stale = {op: [k for k in keys if k not in recorded.get(op, {})] for op, keys in MODEL_CASES.items()}
    stale = {op: keys for op, keys in stale.items() if keys}
    assert not stale, f'MODEL_CASES entries no model run records: {stale!r}'
    assert all(len(set(keys)) == len(keys) for keys in MODEL_CASES.values())


def test_model_cases_and_full_size_cases_are_disjoint():
    both = {op: [k for k in keys if k in FULL_SIZE_CASES.get(op, ())] for op, keys in MODEL_CASES.items()}
    both = {op: keys for op, keys in both.items() if keys}
    assert not both, f'MODEL_CASES entries that FULL_SIZE_CASES already holds: {both!r}'
    assert set(MODEL_CASES) <= set(KEYS), sorted(set(MODEL_CASES) - set(KEYS))


@pytest.mark.gpu
def test_model_census_no_bn_coef_launch_writes_one_batchnorm_twice(recorded):
    assert KC.BN_PAIRS not in recorded, _listing({KC.BN_PAIRS: recorded.get(KC.BN_PAIRS, {})})


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 comparisons of MODEL_CASES
# ---------------------------------------------------------------------------------------------------------------------
# As in test_kernel_census_gpu.py: each key goes to the check_* helper of tests/test_kernels_gpu.py that the op's own test
# runs, with that test's bars; a key whose arguments are already one of that test's cases is not run twice.
# bn_running_update has no tile shape (see FULL_SIZE_CASES).

def _cases(op, to_args, test=None, keep=lambda key: True):
    return KC._cases(op, to_args, test, keep, table=MODEL_CASES)


def test_model_cases_map_to_their_checks():
    """Every MODEL_CASES key maps to the arguments of its check (no GPU needed: the mappings assert what they assume), and
    every dynadj_typed key is one of test_typed_kb_full_size_vs_fp64's cases, which compare it at this size already."""
    maps = dict(aggregate_sum=_aggsum_args, ctr_topology=KC._ctr_args, dynadj=KC._dyn_args, fuse_out=KC._fuse_args,
                pwconv=KC._pw_args, tconv=_tconv_args, tconv_bn=KC._tcg_args, temporal_branches_bn=KC._tb_args,
                temporal_mlp_bn=_mlp_args, temporal_unitmlp_bn=_unitmlp_args, dynadj_typed=_typed_args,
                gram=lambda k: k, gate=lambda k: k, bn_running_update=lambda k: k)
    assert set(MODEL_CASES) <= set(maps), sorted(set(MODEL_CASES) - set(maps))
    for op, keys in MODEL_CASES.items():
        for key in keys:
            maps[op](key)
    have = KC._existing(TDG.test_typed_kb_full_size_vs_fp64)
    assert all(_typed_args(k) in have for k in MODEL_CASES['dynadj_typed'])


def _aggsum_args(k):
    n, Kk, Co, T, V, form, bn = k
    assert form in ('per_channel', 'per_sample') and bn, k
    return dict(n=n, K=Kk, Co=Co, T=T, V=V)


@pytest.mark.gpu
@pytest.mark.parametrize('key,args', _cases('aggregate_sum', _aggsum_args, keep=lambda k: k[5] == 'per_channel'))
def test_aggregate_sum_per_channel_model_census(key, args):
    KG.check_aggregate_sum(**args, shared=False, bn=True)


@pytest.mark.gpu
@pytest.mark.parametrize('key,args', _cases('aggregate_sum', _aggsum_args, keep=lambda k: k[5] == 'per_sample'))
def test_aggregate_sum_per_sample_model_census(key, args):
    a = dict(args)
    KG.check_aggregate_sum_per_sample(a['n'], a['K'], a['Co'], a['T'], a['V'])


@pytest.mark.gpu
@pytest.mark.parametrize('key,args', _cases('ctr_topology', KC._ctr_args, KG.test_ctr_topology))
def test_ctr_topology_model_census(key, args):
    KG.check_ctr_topology(**args)


@pytest.mark.gpu
@pytest.mark.parametrize('key,args', _cases('dynadj', KC._dyn_args, KG.test_dynadj))
def test_dynadj_model_census(key, args):
    KG.check_dynadj(**args)


def _typed_args(k):
    n, Ci, KM, V, ld, P, E, add_type, single_use = k
    # dghgcn at DGH_CFG's ratio 0.125: mid = Co / 8 (Ahat depends on Co through mid only); ld = 32 is the padded row the
    # check's unpadded xbar is padded to before the first launch (as in dynadj)
    assert (n, V, ld, P, E, add_type, single_use) == (128, 25, 32, 5, 15, False, True) and KM % 3 == 0, k
    return dict(case=(Ci, 8 * (KM // 3), 0.125), flags='node_edge')


@pytest.mark.gpu
@pytest.mark.parametrize('key,args', _cases('fuse_out', KC._fuse_args, KG.test_fuse_out, keep=lambda k: not k[8]))
def test_fuse_out_model_census(key, args):
    KG.check_fuse_out(**args)


@pytest.mark.gpu
@pytest.mark.parametrize('key', MODEL_CASES['gate'], ids=repr)
def test_gate_model_census(key):
    KG.check_gate(*key)


@pytest.mark.gpu
@pytest.mark.parametrize('key', MODEL_CASES['gram'], ids=repr)
def test_gram_model_census(key):
    KG.check_gram(*key)


@pytest.mark.gpu
@pytest.mark.parametrize('key,args', _cases('pwconv', KC._pw_args, KG.test_pwconv))
def test_pwconv_model_census(key, args):
    assert key[-2:] == KC._pw_paths(*key[:7])
    KG.check_pwconv(**args)


def _tconv_args(k):
    n, Ci, Co, T, V, stride, KT, dil, want_bn = k
    return dict(n=n, Ci=Ci, Co=Co, T=T, V=V, stride=stride, ks=KT, dil=dil, bn=want_bn)


@pytest.mark.gpu
@pytest.mark.parametrize('key,args', _cases('tconv', _tconv_args, KG.test_tconv_dense))
def test_tconv_dense_model_census(key, args):
    KG.check_tconv_dense(**args)


@pytest.mark.gpu
@pytest.mark.parametrize('key,args', _cases('tconv_bn', KC._tcg_args, KG.test_tconv_gemm))
def test_tconv_gemm_model_census(key, args):
    KG.check_tconv_gemm(**args)


@pytest.mark.gpu
@pytest.mark.parametrize('key,args', _cases('temporal_branches_bn', KC._tb_args))
def test_temporal_branches_bn_model_census(key, args, monkeypatch):
    p = _Path(monkeypatch)
    KG.check_temporal_branches_bn(**args, monkeypatch=monkeypatch)
    assert set(p.taken) <= {p.path()} and p.path() == key[-1], (p.taken, key[-1])


def _mlp_args(k):
    n, C, T, V, stride, cfg, widths, n_act, KM, merge_after, want_bn = k
    # check_temporal_mlp_bn builds msmlp's operands the way the unit does: widths, n_act and the causal taps from cfg
    assert widths == tuple(KG._ms_widths(C, cfg)) and n_act == C - widths[-1] and want_bn, k
    assert KM == (cfg[0][0] + 1) // 2, k
    return dict(n=n, C=C, T=T, V=V, stride=stride, cfg=cfg, merge_after=merge_after)


@pytest.mark.gpu
@pytest.mark.parametrize('key,args', _cases('temporal_mlp_bn', _mlp_args, KG.test_temporal_mlp_bn))
def test_temporal_mlp_bn_model_census(key, args):
    KG.check_temporal_mlp_bn(**args)


def _unitmlp_args(k):
    n, C, T, V, stride, KM, dils, KT, tdil, merge_after, want_bn = k
    # unitmlp: one dilation for the causal taps and the dense conv, (KT + 1) / 2 taps
    assert len(dils) == 1 and KM == (KT + 1) // 2 and tdil == dils[0] and KT > 0 and want_bn, k
    return dict(n=n, C=C, T=T, V=V, stride=stride, ks=KT, dil=tdil, add_tcn=True, merge_after=merge_after,
                zero_dil=False)


@pytest.mark.gpu
@pytest.mark.parametrize('key,args', _cases('temporal_unitmlp_bn', _unitmlp_args, KG.test_temporal_unitmlp_bn))
def test_temporal_unitmlp_bn_model_census(key, args):
    KG.check_temporal_unitmlp_bn(**args)
