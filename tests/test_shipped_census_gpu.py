"""The kernel census (tests/test_kernel_census_gpu.py) at the shapes of the shipped configs, which the BASELINE and model
censuses (T = 64, 64 clips) do not reach: clip lengths 60 and 100 at V = 25 (frames 60 -> 30 -> 15 and 100 -> 50 -> 25),
128 videos per GPU in training, 32 videos x 10 clips in the test and 128 x 1 in validation, and the odd-sized last batch
of an epoch (drop_last is False).  The training runs are one eager train_step + backward (KC.census); the eval runs are
one eval-mode forward_test (KC.census_eval) with seeded running statistics, the no-grad path no other census records.

SHIPPED_CASES holds the keys these runs record that FULL_SIZE_CASES and MODEL_CASES lack, and nothing else; each of them
is compared with its fp64 statement at that size by the check_* helpers of tests/test_kernels_gpu.py, with the bars of
the tests they came from.  Below them, forward_test of the full-width models at the shipped clip lengths against the
oracle in fp64."""
import numpy as np
import pytest
import torch

from dsgcn_amd import kernels as K

import test_kernel_census_gpu as KC
from test_kernel_census_gpu import DGMSTCN, EVAL, FULL_SIZE_CASES, KEYS, _Path, _listing
from test_model_census_gpu import MODEL_CASES
import test_kernels_gpu as KG


# ---------------------------------------------------------------------------------------------------------------------
# the runs
# ---------------------------------------------------------------------------------------------------------------------

TRAIN_RUNS = (
    # (name, model, videos, T, V, classes, dropout kept?)
    ('ds_t60', 'ds', 128, 60, 25, 60, False),                          # dsstgcn/ntu60_xsub_3dkp/j.py
    ('ds_t100', 'ds', 128, 100, 25, 60, False),                        # dsstgcn/ntu60_xsub_3dkp/{jm,b,bm}.py
    ('ds_t60_tail', 'ds', 27, 60, 25, 60, False),                      # the last, partial batch of an epoch
    ('ctrgcn_shipped_t60', 'ctrgcn_shipped', 128, 60, 25, 60, False),  # ctrgcn/CTRGCN_model.py
    ('stgcn_shipped_t60', 'stgcn_shipped', 128, 60, 25, 60, False),    # stgcn/STGCN_model.py
)

EVAL_RUNS = (
    # (name, model, videos, clips per video, T, V): n = videos * clips * 2 persons
    ('ds_t60_test', 'ds', 32, 10, 60, 25),
    ('ds_t100_test', 'ds', 32, 10, 100, 25),
    ('ds_t60_val', 'ds', 128, 1, 60, 25),
    ('ds_t60_test_tail', 'ds', 7, 10, 60, 25),
    ('ctrgcn_shipped_t60_test', 'ctrgcn_shipped', 32, 10, 60, 25),
    ('stgcn_shipped_t60_test', 'stgcn_shipped', 32, 10, 60, 25),
)


def _model_cfg(model):
    from bench import ds_cfg, other_cfg
    return ds_cfg() if model == 'ds' else other_cfg(model)


# the keys the runs record that FULL_SIZE_CASES and MODEL_CASES lack, and nothing else (the comments name the runs)
SHIPPED_CASES = {
    # (n, KC, T, V, relu, affine)
    'aggregate': [
        (140, 24, 60, 25, True, True),   # ds_t60_test_tail
        (140, 48, 30, 25, True, True),   # ds_t60_test_tail
        (140, 48, 60, 25, True, True),   # ds_t60_test_tail
        (140, 96, 15, 25, True, True),   # ds_t60_test_tail
        (140, 96, 30, 25, True, True),   # ds_t60_test_tail
        (256, 24, 100, 25, True, True),   # ds_t100
        (256, 24, 60, 25, True, True),   # ds_t60, ds_t60_val
        (256, 48, 100, 25, True, True),   # ds_t100
        (256, 48, 30, 25, True, True),   # ds_t60, ds_t60_val
        (256, 48, 50, 25, True, True),   # ds_t100
        (256, 48, 60, 25, True, True),   # ds_t60, ds_t60_val
        (256, 96, 15, 25, True, True),   # ds_t60, ds_t60_val
        (256, 96, 25, 25, True, True),   # ds_t100
        (256, 96, 30, 25, True, True),   # ds_t60, ds_t60_val
        (256, 96, 50, 25, True, True),   # ds_t100
        (54, 24, 60, 25, True, True),   # ds_t60_tail
        (54, 48, 30, 25, True, True),   # ds_t60_tail
        (54, 48, 60, 25, True, True),   # ds_t60_tail
        (54, 96, 15, 25, True, True),   # ds_t60_tail
        (54, 96, 30, 25, True, True),   # ds_t60_tail
        (640, 24, 100, 25, True, True),   # ds_t100_test
        (640, 24, 60, 25, True, True),   # ds_t60_test
        (640, 48, 100, 25, True, True),   # ds_t100_test
        (640, 48, 30, 25, True, True),   # ds_t60_test
        (640, 48, 50, 25, True, True),   # ds_t100_test
        (640, 48, 60, 25, True, True),   # ds_t60_test
        (640, 96, 15, 25, True, True),   # ds_t60_test
        (640, 96, 25, 25, True, True),   # ds_t100_test
        (640, 96, 30, 25, True, True),   # ds_t60_test
        (640, 96, 50, 25, True, True),   # ds_t100_test
    ],
    # (n, K, Co, T, V, adjacency form, want_bn)
    'aggregate_sum': [
        (256, 3, 128, 30, 25, 'per_channel', True),   # ctrgcn_shipped_t60
        (256, 3, 128, 30, 25, 'shared', True),   # stgcn_shipped_t60
        (256, 3, 128, 60, 25, 'per_channel', True),   # ctrgcn_shipped_t60
        (256, 3, 128, 60, 25, 'shared', True),   # stgcn_shipped_t60
        (256, 3, 256, 15, 25, 'per_channel', True),   # ctrgcn_shipped_t60
        (256, 3, 256, 15, 25, 'shared', True),   # stgcn_shipped_t60
        (256, 3, 256, 30, 25, 'per_channel', True),   # ctrgcn_shipped_t60
        (256, 3, 256, 30, 25, 'shared', True),   # stgcn_shipped_t60
        (256, 3, 64, 60, 25, 'per_channel', True),   # ctrgcn_shipped_t60
        (256, 3, 64, 60, 25, 'shared', True),   # stgcn_shipped_t60
        (640, 3, 128, 30, 25, 'per_channel', False),   # ctrgcn_shipped_t60_test
        (640, 3, 128, 30, 25, 'shared', False),   # stgcn_shipped_t60_test
        (640, 3, 128, 60, 25, 'per_channel', False),   # ctrgcn_shipped_t60_test
        (640, 3, 128, 60, 25, 'shared', False),   # stgcn_shipped_t60_test
        (640, 3, 256, 15, 25, 'per_channel', False),   # ctrgcn_shipped_t60_test
        (640, 3, 256, 15, 25, 'shared', False),   # stgcn_shipped_t60_test
        (640, 3, 256, 30, 25, 'per_channel', False),   # ctrgcn_shipped_t60_test
        (640, 3, 256, 30, 25, 'shared', False),   # stgcn_shipped_t60_test
        (640, 3, 64, 60, 25, 'per_channel', False),   # ctrgcn_shipped_t60_test
        (640, 3, 64, 60, 25, 'shared', False),   # stgcn_shipped_t60_test
    ],
    # (n, Ci, Co, V, subsets, R, subset_major, path, (alpha elements, beta, edge subsets, edge classes E))
    'ctr_topology': [
        (256, 128, 128, 25, 3, 16, False, 'per_subset', (3, True, (0,), 15)),   # ctrgcn_shipped_t60
        (256, 128, 256, 25, 3, 16, False, 'per_subset', (3, True, (0,), 15)),   # ctrgcn_shipped_t60
        (256, 256, 256, 25, 3, 32, False, 'per_subset', (3, True, (0,), 15)),   # ctrgcn_shipped_t60
        (256, 3, 64, 25, 3, 8, False, 'per_subset', (3, True, (0,), 15)),   # ctrgcn_shipped_t60
        (256, 64, 128, 25, 3, 8, False, 'per_subset', (3, True, (0,), 15)),   # ctrgcn_shipped_t60
        (256, 64, 64, 25, 3, 8, False, 'per_subset', (3, True, (0,), 15)),   # ctrgcn_shipped_t60
        (640, 128, 128, 25, 3, 16, False, 'per_subset', (3, True, (0,), 15)),   # ctrgcn_shipped_t60_test
        (640, 128, 256, 25, 3, 16, False, 'per_subset', (3, True, (0,), 15)),   # ctrgcn_shipped_t60_test
        (640, 256, 256, 25, 3, 32, False, 'per_subset', (3, True, (0,), 15)),   # ctrgcn_shipped_t60_test
        (640, 3, 64, 25, 3, 8, False, 'per_subset', (3, True, (0,), 15)),   # ctrgcn_shipped_t60_test
        (640, 64, 128, 25, 3, 8, False, 'per_subset', (3, True, (0,), 15)),   # ctrgcn_shipped_t60_test
        (640, 64, 64, 25, 3, 8, False, 'per_subset', (3, True, (0,), 15)),   # ctrgcn_shipped_t60_test
    ],
    # (N, M, T, V, C, bn_type, affine[, EVAL: an eval-mode BatchNorm on the running statistics])
    'data_bn': [
        (128, 2, 100, 25, 3, 'VC', True),   # ds_t100
        (128, 2, 60, 25, 3, 'MVC', True),   # ctrgcn_shipped_t60
        (128, 2, 60, 25, 3, 'VC', True),   # ds_t60, stgcn_shipped_t60
        (128, 2, 60, 25, 3, 'VC', True, EVAL),   # ds_t60_val
        (27, 2, 60, 25, 3, 'VC', True),   # ds_t60_tail
        (320, 2, 100, 25, 3, 'VC', True, EVAL),   # ds_t100_test
        (320, 2, 60, 25, 3, 'MVC', True, EVAL),   # ctrgcn_shipped_t60_test
        (320, 2, 60, 25, 3, 'VC', True, EVAL),   # ds_t60_test, stgcn_shipped_t60_test
        (70, 2, 60, 25, 3, 'VC', True, EVAL),   # ds_t60_test_tail
    ],
    # (n, Ci, mid, V, xbar row length, BatchNorm jobs hosted)
    'dynadj': [
        (140, 128, 16, 25, 32, True),   # ds_t60_test_tail
        (140, 128, 32, 25, 32, True),   # ds_t60_test_tail
        (140, 256, 32, 25, 32, True),   # ds_t60_test_tail
        (140, 3, 8, 25, 32, True),   # ds_t60_test_tail
        (140, 64, 16, 25, 32, True),   # ds_t60_test_tail
        (140, 64, 8, 25, 32, True),   # ds_t60_test_tail
        (256, 128, 16, 25, 32, True),   # ds_t60, ds_t100, ds_t60_val
        (256, 128, 32, 25, 32, True),   # ds_t60, ds_t100, ds_t60_val
        (256, 256, 32, 25, 32, True),   # ds_t60, ds_t100, ds_t60_val
        (256, 3, 8, 25, 32, True),   # ds_t60, ds_t100, ds_t60_val
        (256, 64, 16, 25, 32, True),   # ds_t60, ds_t100, ds_t60_val
        (256, 64, 8, 25, 32, True),   # ds_t60, ds_t100, ds_t60_val
        (54, 128, 16, 25, 32, True),   # ds_t60_tail
        (54, 128, 32, 25, 32, True),   # ds_t60_tail
        (54, 256, 32, 25, 32, True),   # ds_t60_tail
        (54, 3, 8, 25, 32, True),   # ds_t60_tail
        (54, 64, 16, 25, 32, True),   # ds_t60_tail
        (54, 64, 8, 25, 32, True),   # ds_t60_tail
        (640, 128, 16, 25, 32, True),   # ds_t60_test, ds_t100_test
        (640, 128, 32, 25, 32, True),   # ds_t60_test, ds_t100_test
        (640, 256, 32, 25, 32, True),   # ds_t60_test, ds_t100_test
        (640, 3, 8, 25, 32, True),   # ds_t60_test, ds_t100_test
        (640, 64, 16, 25, 32, True),   # ds_t60_test, ds_t100_test
        (640, 64, 8, 25, 32, True),   # ds_t60_test, ds_t100_test
    ],
    # (n, C, T, V, mode, relu flags, time-mean ld (0: none), tee, dropout, prestrided_fits)
    'fuse_out': [
        (140, 128, 30, 25, 'res_affine', 1, 32, 1, False, True),   # ds_t60_test_tail
        (140, 128, 30, 25, 'res_plain', 1, 32, 1, False, True),   # ds_t60_test_tail
        (140, 128, 30, 25, 'res_plain', 1, 32, 2, False, True),   # ds_t60_test_tail
        (140, 256, 15, 25, 'res_affine', 1, 32, 1, False, True),   # ds_t60_test_tail
        (140, 256, 15, 25, 'res_plain', 1, 0, 0, False, True),   # ds_t60_test_tail
        (140, 256, 15, 25, 'res_plain', 1, 32, 1, False, True),   # ds_t60_test_tail
        (140, 3, 60, 25, 'plain', 0, 32, 0, False, True),   # ds_t60_test_tail
        (140, 64, 60, 25, 'affine', 1, 32, 1, False, True),   # ds_t60_test_tail
        (140, 64, 60, 25, 'res_plain', 1, 32, 1, False, True),   # ds_t60_test_tail
        (140, 64, 60, 25, 'res_plain', 1, 32, 2, False, True),   # ds_t60_test_tail
        (256, 128, 30, 25, 'affine', 1, 0, 0, False, True),   # stgcn_shipped_t60
        (256, 128, 30, 25, 'res_affine', 1, 0, 1, False, True),   # stgcn_shipped_t60
        (256, 128, 30, 25, 'res_affine', 1, 25, 1, False, True),   # ctrgcn_shipped_t60
        (256, 128, 30, 25, 'res_affine', 1, 32, 1, False, True),   # ds_t60, ds_t60_val
        (256, 128, 30, 25, 'res_plain', 1, 0, 1, False, True),   # stgcn_shipped_t60
        (256, 128, 30, 25, 'res_plain', 1, 0, 2, False, True),   # stgcn_shipped_t60
        (256, 128, 30, 25, 'res_plain', 1, 25, 1, False, True),   # ctrgcn_shipped_t60
        (256, 128, 30, 25, 'res_plain', 1, 25, 2, False, True),   # ctrgcn_shipped_t60
        (256, 128, 30, 25, 'res_plain', 1, 32, 1, False, True),   # ds_t60, ds_t60_val
        (256, 128, 30, 25, 'res_plain', 1, 32, 2, False, True),   # ds_t60, ds_t60_val
        (256, 128, 30, 25, 'res_x1', 0, 0, 0, False, True),   # ctrgcn_shipped_t60, stgcn_shipped_t60
        (256, 128, 50, 25, 'res_affine', 1, 32, 1, False, True),   # ds_t100
        (256, 128, 50, 25, 'res_plain', 1, 32, 1, False, True),   # ds_t100
        (256, 128, 50, 25, 'res_plain', 1, 32, 2, False, True),   # ds_t100
        (256, 128, 60, 25, 'affine', 1, 0, 0, False, True),   # stgcn_shipped_t60
        (256, 256, 15, 25, 'affine', 1, 0, 0, False, True),   # stgcn_shipped_t60
        (256, 256, 15, 25, 'res_affine', 1, 0, 1, False, True),   # stgcn_shipped_t60
        (256, 256, 15, 25, 'res_affine', 1, 25, 1, False, True),   # ctrgcn_shipped_t60
        (256, 256, 15, 25, 'res_affine', 1, 32, 1, False, True),   # ds_t60, ds_t60_val
        (256, 256, 15, 25, 'res_plain', 1, 0, 0, False, True),   # ds_t60_val
        (256, 256, 15, 25, 'res_plain', 1, 0, 1, False, True),   # stgcn_shipped_t60
        (256, 256, 15, 25, 'res_plain', 1, 25, 1, False, True),   # ctrgcn_shipped_t60
        (256, 256, 15, 25, 'res_plain', 1, 32, 1, False, True),   # ds_t60, ds_t60_val
        (256, 256, 15, 25, 'res_x1', 0, 0, 0, False, True),   # ctrgcn_shipped_t60, stgcn_shipped_t60
        (256, 256, 25, 25, 'res_affine', 1, 32, 1, False, True),   # ds_t100
        (256, 256, 25, 25, 'res_plain', 1, 32, 1, False, True),   # ds_t100
        (256, 256, 30, 25, 'affine', 1, 0, 0, False, True),   # stgcn_shipped_t60
        (256, 3, 100, 25, 'plain', 0, 32, 0, False, True),   # ds_t100
        (256, 3, 60, 25, 'plain', 0, 25, 0, False, True),   # ctrgcn_shipped_t60
        (256, 3, 60, 25, 'plain', 0, 32, 0, False, True),   # ds_t60, ds_t60_val
        (256, 64, 100, 25, 'affine', 1, 32, 1, False, True),   # ds_t100
        (256, 64, 100, 25, 'res_plain', 1, 32, 1, False, True),   # ds_t100
        (256, 64, 100, 25, 'res_plain', 1, 32, 2, False, True),   # ds_t100
        (256, 64, 60, 25, 'affine', 1, 0, 0, False, True),   # stgcn_shipped_t60
        (256, 64, 60, 25, 'affine', 1, 0, 1, False, True),   # stgcn_shipped_t60
        (256, 64, 60, 25, 'affine', 1, 25, 1, False, True),   # ctrgcn_shipped_t60
        (256, 64, 60, 25, 'affine', 1, 32, 1, False, True),   # ds_t60, ds_t60_val
        (256, 64, 60, 25, 'res_plain', 1, 0, 1, False, True),   # stgcn_shipped_t60
        (256, 64, 60, 25, 'res_plain', 1, 0, 2, False, True),   # stgcn_shipped_t60
        (256, 64, 60, 25, 'res_plain', 1, 25, 1, False, True),   # ctrgcn_shipped_t60
        (256, 64, 60, 25, 'res_plain', 1, 25, 2, False, True),   # ctrgcn_shipped_t60
        (256, 64, 60, 25, 'res_plain', 1, 32, 1, False, True),   # ds_t60, ds_t60_val
        (256, 64, 60, 25, 'res_plain', 1, 32, 2, False, True),   # ds_t60, ds_t60_val
        (256, 64, 60, 25, 'res_x1', 0, 0, 0, False, True),   # ctrgcn_shipped_t60, stgcn_shipped_t60
        (54, 128, 30, 25, 'res_affine', 1, 32, 1, False, True),   # ds_t60_tail
        (54, 128, 30, 25, 'res_plain', 1, 32, 1, False, True),   # ds_t60_tail
        (54, 128, 30, 25, 'res_plain', 1, 32, 2, False, True),   # ds_t60_tail
        (54, 256, 15, 25, 'res_affine', 1, 32, 1, False, True),   # ds_t60_tail
        (54, 256, 15, 25, 'res_plain', 1, 32, 1, False, True),   # ds_t60_tail
        (54, 3, 60, 25, 'plain', 0, 32, 0, False, True),   # ds_t60_tail
        (54, 64, 60, 25, 'affine', 1, 32, 1, False, True),   # ds_t60_tail
        (54, 64, 60, 25, 'res_plain', 1, 32, 1, False, True),   # ds_t60_tail
        (54, 64, 60, 25, 'res_plain', 1, 32, 2, False, True),   # ds_t60_tail
        (640, 128, 30, 25, 'affine', 1, 0, 0, False, True),   # stgcn_shipped_t60_test
        (640, 128, 30, 25, 'res_affine', 1, 0, 1, False, True),   # stgcn_shipped_t60_test
        (640, 128, 30, 25, 'res_affine', 1, 25, 1, False, True),   # ctrgcn_shipped_t60_test
        (640, 128, 30, 25, 'res_affine', 1, 32, 1, False, True),   # ds_t60_test
        (640, 128, 30, 25, 'res_plain', 1, 0, 1, False, True),   # stgcn_shipped_t60_test
        (640, 128, 30, 25, 'res_plain', 1, 0, 2, False, True),   # stgcn_shipped_t60_test
        (640, 128, 30, 25, 'res_plain', 1, 25, 1, False, True),   # ctrgcn_shipped_t60_test
        (640, 128, 30, 25, 'res_plain', 1, 25, 2, False, True),   # ctrgcn_shipped_t60_test
        (640, 128, 30, 25, 'res_plain', 1, 32, 1, False, True),   # ds_t60_test
        (640, 128, 30, 25, 'res_plain', 1, 32, 2, False, True),   # ds_t60_test
        (640, 128, 30, 25, 'res_x1', 0, 0, 0, False, True),   # ctrgcn_shipped_t60_test, stgcn_shipped_t60_test
        (640, 128, 50, 25, 'res_affine', 1, 32, 1, False, True),   # ds_t100_test
        (640, 128, 50, 25, 'res_plain', 1, 32, 1, False, True),   # ds_t100_test
        (640, 128, 50, 25, 'res_plain', 1, 32, 2, False, True),   # ds_t100_test
        (640, 128, 60, 25, 'affine', 1, 0, 0, False, True),   # stgcn_shipped_t60_test
        (640, 256, 15, 25, 'affine', 1, 0, 0, False, True),   # stgcn_shipped_t60_test
        (640, 256, 15, 25, 'res_affine', 1, 0, 1, False, True),   # stgcn_shipped_t60_test
        (640, 256, 15, 25, 'res_affine', 1, 25, 1, False, True),   # ctrgcn_shipped_t60_test
        (640, 256, 15, 25, 'res_affine', 1, 32, 1, False, True),   # ds_t60_test
        (640, 256, 15, 25, 'res_plain', 1, 0, 0, False, True),   # ds_t60_test, ctrgcn_shipped_t60_test, stgcn_shipped_t60_test
        (640, 256, 15, 25, 'res_plain', 1, 0, 1, False, True),   # stgcn_shipped_t60_test
        (640, 256, 15, 25, 'res_plain', 1, 25, 1, False, True),   # ctrgcn_shipped_t60_test
        (640, 256, 15, 25, 'res_plain', 1, 32, 1, False, True),   # ds_t60_test
        (640, 256, 15, 25, 'res_x1', 0, 0, 0, False, True),   # ctrgcn_shipped_t60_test, stgcn_shipped_t60_test
        (640, 256, 25, 25, 'res_affine', 1, 32, 1, False, True),   # ds_t100_test
        (640, 256, 25, 25, 'res_plain', 1, 0, 0, False, True),   # ds_t100_test
        (640, 256, 25, 25, 'res_plain', 1, 32, 1, False, True),   # ds_t100_test
        (640, 256, 30, 25, 'affine', 1, 0, 0, False, True),   # stgcn_shipped_t60_test
        (640, 3, 100, 25, 'plain', 0, 32, 0, False, True),   # ds_t100_test
        (640, 3, 60, 25, 'plain', 0, 25, 0, False, True),   # ctrgcn_shipped_t60_test
        (640, 3, 60, 25, 'plain', 0, 32, 0, False, True),   # ds_t60_test
        (640, 64, 100, 25, 'affine', 1, 32, 1, False, True),   # ds_t100_test
        (640, 64, 100, 25, 'res_plain', 1, 32, 1, False, True),   # ds_t100_test
        (640, 64, 100, 25, 'res_plain', 1, 32, 2, False, True),   # ds_t100_test
        (640, 64, 60, 25, 'affine', 1, 0, 0, False, True),   # stgcn_shipped_t60_test
        (640, 64, 60, 25, 'affine', 1, 0, 1, False, True),   # stgcn_shipped_t60_test
        (640, 64, 60, 25, 'affine', 1, 25, 1, False, True),   # ctrgcn_shipped_t60_test
        (640, 64, 60, 25, 'affine', 1, 32, 1, False, True),   # ds_t60_test
        (640, 64, 60, 25, 'res_plain', 1, 0, 1, False, True),   # stgcn_shipped_t60_test
        (640, 64, 60, 25, 'res_plain', 1, 0, 2, False, True),   # stgcn_shipped_t60_test
        (640, 64, 60, 25, 'res_plain', 1, 25, 1, False, True),   # ctrgcn_shipped_t60_test
        (640, 64, 60, 25, 'res_plain', 1, 25, 2, False, True),   # ctrgcn_shipped_t60_test
        (640, 64, 60, 25, 'res_plain', 1, 32, 1, False, True),   # ds_t60_test
        (640, 64, 60, 25, 'res_plain', 1, 32, 2, False, True),   # ds_t60_test
        (640, 64, 60, 25, 'res_x1', 0, 0, 0, False, True),   # ctrgcn_shipped_t60_test, stgcn_shipped_t60_test
    ],
    # (n, C, T, V, mode, relu flags, dropout)
    'fuse_out_pool': [
        (256, 256, 15, 25, 'res_plain', 1, False),   # ds_t60, ctrgcn_shipped_t60, stgcn_shipped_t60
        (256, 256, 25, 25, 'res_plain', 1, False),   # ds_t100
        (54, 256, 15, 25, 'res_plain', 1, False),   # ds_t60_tail
    ],
    # (n, C, T, V)
    'gram': [
        (1920, 16, 1, 25),   # ctrgcn_shipped_t60_test
        (1920, 32, 1, 25),   # ctrgcn_shipped_t60_test
        (1920, 8, 1, 25),   # ctrgcn_shipped_t60_test
        (768, 16, 1, 25),   # ctrgcn_shipped_t60
        (768, 32, 1, 25),   # ctrgcn_shipped_t60
        (768, 8, 1, 25),   # ctrgcn_shipped_t60
    ],
    # (clips, persons, C, classes, bias)
    'head_loss': [
        (128, 2, 256, 60, True),   # ds_t60, ds_t100, ctrgcn_shipped_t60, stgcn_shipped_t60
        (27, 2, 256, 60, True),   # ds_t60_tail
    ],
    # (n, Ci, Co, T, V, stride, aug, mode, want_bn, bias, forward form, backward form)
    'pwconv': [
        (140, 128, 128, 30, 25, 1, False, 'affine_relu', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test_tail
        (140, 128, 128, 30, 25, 1, True, 'res_plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test_tail
        (140, 128, 128, 60, 25, 1, True, 'res_affine', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_test_tail
        (140, 128, 144, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test_tail
        (140, 128, 256, 15, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_test_tail
        (140, 128, 256, 30, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test_tail
        (140, 128, 288, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test_tail
        (140, 128, 48, 30, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test_tail
        (140, 128, 96, 30, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test_tail
        (140, 24, 64, 60, 25, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # ds_t60_test_tail
        (140, 256, 256, 15, 25, 1, False, 'affine_relu', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_test_tail
        (140, 256, 256, 15, 25, 1, True, 'res_plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_test_tail
        (140, 256, 256, 30, 25, 1, True, 'res_affine', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test_tail
        (140, 256, 288, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test_tail
        (140, 256, 96, 15, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_test_tail
        (140, 3, 24, 60, 25, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # ds_t60_test_tail
        (140, 3, 64, 60, 25, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # ds_t60_test_tail
        (140, 3, 72, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test_tail
        (140, 48, 128, 30, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test_tail
        (140, 48, 128, 60, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test_tail
        (140, 64, 128, 30, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test_tail
        (140, 64, 128, 60, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_test_tail
        (140, 64, 144, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test_tail
        (140, 64, 24, 60, 25, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # ds_t60_test_tail
        (140, 64, 48, 60, 25, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # ds_t60_test_tail
        (140, 64, 64, 60, 25, 1, False, 'affine_relu', False, True, 'direct', 'bwd64'),   # ds_t60_test_tail
        (140, 64, 64, 60, 25, 1, True, 'res_affine', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test_tail
        (140, 64, 64, 60, 25, 1, True, 'res_plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test_tail
        (140, 64, 72, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test_tail
        (140, 96, 256, 15, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_test_tail
        (140, 96, 256, 30, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test_tail
        (256, 128, 128, 100, 25, 1, True, 'res_affine', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t100
        (256, 128, 128, 30, 25, 1, False, 'affine_relu', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_val
        (256, 128, 128, 30, 25, 1, False, 'affine_relu', True, True, 'direct', 'dgrad_wgrad'),   # ds_t60, ctrgcn_shipped_t60
        (256, 128, 128, 30, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60, stgcn_shipped_t60
        (256, 128, 128, 30, 25, 1, False, 'res_plain', True, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60
        (256, 128, 128, 30, 25, 1, True, 'res_plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_val
        (256, 128, 128, 30, 25, 1, True, 'res_plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t60
        (256, 128, 128, 50, 25, 1, False, 'affine_relu', True, True, 'direct', 'dgrad_wgrad'),   # ds_t100
        (256, 128, 128, 50, 25, 1, True, 'res_plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t100
        (256, 128, 128, 60, 25, 1, False, 'res_affine', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ctrgcn_shipped_t60
        (256, 128, 128, 60, 25, 1, True, 'res_affine', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_val
        (256, 128, 128, 60, 25, 1, True, 'res_affine', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60
        (256, 128, 144, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60, ds_t100, ds_t60_val
        (256, 128, 256, 15, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_val
        (256, 128, 256, 15, 25, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60, ctrgcn_shipped_t60, stgcn_shipped_t60
        (256, 128, 256, 25, 25, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t100
        (256, 128, 256, 30, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_val
        (256, 128, 256, 30, 25, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t60, ctrgcn_shipped_t60
        (256, 128, 256, 50, 25, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t100
        (256, 128, 288, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60, ds_t100, ds_t60_val
        (256, 128, 384, 30, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60, stgcn_shipped_t60
        (256, 128, 48, 30, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_val
        (256, 128, 48, 30, 25, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t60
        (256, 128, 48, 50, 25, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t100
        (256, 128, 768, 30, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60, stgcn_shipped_t60
        (256, 128, 96, 1, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60
        (256, 128, 96, 30, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_val
        (256, 128, 96, 30, 25, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t60
        (256, 128, 96, 50, 25, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t100
        (256, 16, 128, 25, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60
        (256, 16, 240, 25, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60
        (256, 16, 256, 25, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60
        (256, 24, 64, 100, 25, 1, False, 'plain', True, True, 'direct', 'bwd64'),   # ds_t100
        (256, 24, 64, 60, 25, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # ds_t60_val
        (256, 24, 64, 60, 25, 1, False, 'plain', True, True, 'direct', 'bwd64'),   # ds_t60
        (256, 256, 192, 1, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60
        (256, 256, 256, 15, 25, 1, False, 'affine_relu', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_val
        (256, 256, 256, 15, 25, 1, False, 'affine_relu', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60, ctrgcn_shipped_t60
        (256, 256, 256, 15, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ctrgcn_shipped_t60, stgcn_shipped_t60
        (256, 256, 256, 15, 25, 1, False, 'res_plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ctrgcn_shipped_t60
        (256, 256, 256, 15, 25, 1, True, 'res_plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_val
        (256, 256, 256, 15, 25, 1, True, 'res_plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60
        (256, 256, 256, 25, 25, 1, False, 'affine_relu', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t100
        (256, 256, 256, 25, 25, 1, True, 'res_plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t100
        (256, 256, 256, 30, 25, 1, False, 'res_affine', True, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60
        (256, 256, 256, 30, 25, 1, True, 'res_affine', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_val
        (256, 256, 256, 30, 25, 1, True, 'res_affine', True, True, 'direct', 'dgrad_wgrad'),   # ds_t60
        (256, 256, 256, 50, 25, 1, True, 'res_affine', True, True, 'direct', 'dgrad_wgrad'),   # ds_t100
        (256, 256, 288, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60, ds_t100, ds_t60_val
        (256, 256, 768, 15, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ctrgcn_shipped_t60, stgcn_shipped_t60
        (256, 256, 96, 15, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_val
        (256, 256, 96, 15, 25, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60
        (256, 256, 96, 25, 25, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t100
        (256, 3, 192, 60, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60, stgcn_shipped_t60
        (256, 3, 24, 100, 25, 1, False, 'plain', True, True, 'direct', 'bwd64'),   # ds_t100
        (256, 3, 24, 60, 25, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # ds_t60_val
        (256, 3, 24, 60, 25, 1, False, 'plain', True, True, 'direct', 'bwd64'),   # ds_t60
        (256, 3, 48, 1, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60
        (256, 3, 64, 100, 25, 1, False, 'plain', True, True, 'direct', 'bwd64'),   # ds_t100
        (256, 3, 64, 60, 25, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # ds_t60_val
        (256, 3, 64, 60, 25, 1, False, 'plain', True, True, 'direct', 'bwd64'),   # ds_t60, ctrgcn_shipped_t60
        (256, 3, 72, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60, ds_t100, ds_t60_val
        (256, 32, 256, 25, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60
        (256, 32, 480, 25, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60
        (256, 48, 128, 100, 25, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t100
        (256, 48, 128, 30, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_val
        (256, 48, 128, 30, 25, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t60
        (256, 48, 128, 50, 25, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t100
        (256, 48, 128, 60, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_val
        (256, 48, 128, 60, 25, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t60
        (256, 64, 128, 100, 25, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t100
        (256, 64, 128, 30, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_val
        (256, 64, 128, 30, 25, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t60, ctrgcn_shipped_t60, stgcn_shipped_t60
        (256, 64, 128, 50, 25, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t100
        (256, 64, 128, 60, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_val
        (256, 64, 128, 60, 25, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60, ctrgcn_shipped_t60
        (256, 64, 144, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60, ds_t100, ds_t60_val
        (256, 64, 192, 60, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ctrgcn_shipped_t60, stgcn_shipped_t60
        (256, 64, 24, 100, 25, 1, False, 'plain', True, True, 'direct', 'bwd64'),   # ds_t100
        (256, 64, 24, 60, 25, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # ds_t60_val
        (256, 64, 24, 60, 25, 1, False, 'plain', True, True, 'direct', 'bwd64'),   # ds_t60
        (256, 64, 384, 60, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ctrgcn_shipped_t60, stgcn_shipped_t60
        (256, 64, 48, 1, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60
        (256, 64, 48, 100, 25, 1, False, 'plain', True, True, 'direct', 'bwd64'),   # ds_t100
        (256, 64, 48, 60, 25, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # ds_t60_val
        (256, 64, 48, 60, 25, 1, False, 'plain', True, True, 'direct', 'bwd64'),   # ds_t60
        (256, 64, 64, 100, 25, 1, False, 'affine_relu', True, True, 'direct', 'bwd64'),   # ds_t100
        (256, 64, 64, 100, 25, 1, True, 'res_affine', True, True, 'direct', 'dgrad_wgrad'),   # ds_t100
        (256, 64, 64, 100, 25, 1, True, 'res_plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t100
        (256, 64, 64, 60, 25, 1, False, 'affine_relu', False, True, 'direct', 'bwd64'),   # ds_t60_val
        (256, 64, 64, 60, 25, 1, False, 'affine_relu', True, True, 'direct', 'bwd64'),   # ds_t60, ctrgcn_shipped_t60
        (256, 64, 64, 60, 25, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # ctrgcn_shipped_t60, stgcn_shipped_t60
        (256, 64, 64, 60, 25, 1, False, 'res_affine', True, True, 'direct', 'bwd64'),   # ctrgcn_shipped_t60
        (256, 64, 64, 60, 25, 1, False, 'res_plain', True, True, 'direct', 'bwd64'),   # ctrgcn_shipped_t60
        (256, 64, 64, 60, 25, 1, True, 'res_affine', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_val
        (256, 64, 64, 60, 25, 1, True, 'res_affine', True, True, 'direct', 'dgrad_wgrad'),   # ds_t60
        (256, 64, 64, 60, 25, 1, True, 'res_plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_val
        (256, 64, 64, 60, 25, 1, True, 'res_plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t60
        (256, 64, 72, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60, ds_t100, ds_t60_val
        (256, 8, 120, 25, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60
        (256, 8, 128, 25, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60
        (256, 8, 64, 25, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60
        (256, 96, 256, 15, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_val
        (256, 96, 256, 15, 25, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60
        (256, 96, 256, 25, 25, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t100
        (256, 96, 256, 30, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_val
        (256, 96, 256, 30, 25, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t60
        (256, 96, 256, 50, 25, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t100
        (54, 128, 128, 30, 25, 1, False, 'affine_relu', True, True, 'direct', 'dgrad_wgrad'),   # ds_t60_tail
        (54, 128, 128, 30, 25, 1, True, 'res_plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t60_tail
        (54, 128, 128, 60, 25, 1, True, 'res_affine', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_tail
        (54, 128, 144, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_tail
        (54, 128, 256, 15, 25, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_tail
        (54, 128, 256, 30, 25, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t60_tail
        (54, 128, 288, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_tail
        (54, 128, 48, 30, 25, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t60_tail
        (54, 128, 96, 30, 25, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t60_tail
        (54, 24, 64, 60, 25, 1, False, 'plain', True, True, 'direct', 'bwd64'),   # ds_t60_tail
        (54, 256, 256, 15, 25, 1, False, 'affine_relu', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_tail
        (54, 256, 256, 15, 25, 1, True, 'res_plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_tail
        (54, 256, 256, 30, 25, 1, True, 'res_affine', True, True, 'direct', 'dgrad_wgrad'),   # ds_t60_tail
        (54, 256, 288, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_tail
        (54, 256, 96, 15, 25, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_tail
        (54, 3, 24, 60, 25, 1, False, 'plain', True, True, 'direct', 'bwd64'),   # ds_t60_tail
        (54, 3, 64, 60, 25, 1, False, 'plain', True, True, 'direct', 'bwd64'),   # ds_t60_tail
        (54, 3, 72, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_tail
        (54, 48, 128, 30, 25, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t60_tail
        (54, 48, 128, 60, 25, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t60_tail
        (54, 64, 128, 30, 25, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t60_tail
        (54, 64, 128, 60, 25, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_tail
        (54, 64, 144, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_tail
        (54, 64, 24, 60, 25, 1, False, 'plain', True, True, 'direct', 'bwd64'),   # ds_t60_tail
        (54, 64, 48, 60, 25, 1, False, 'plain', True, True, 'direct', 'bwd64'),   # ds_t60_tail
        (54, 64, 64, 60, 25, 1, False, 'affine_relu', True, True, 'direct', 'bwd64'),   # ds_t60_tail
        (54, 64, 64, 60, 25, 1, True, 'res_affine', True, True, 'direct', 'dgrad_wgrad'),   # ds_t60_tail
        (54, 64, 64, 60, 25, 1, True, 'res_plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t60_tail
        (54, 64, 72, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_tail
        (54, 96, 256, 15, 25, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_tail
        (54, 96, 256, 30, 25, 1, False, 'plain', True, True, 'direct', 'dgrad_wgrad'),   # ds_t60_tail
        (640, 128, 128, 100, 25, 1, True, 'res_affine', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t100_test
        (640, 128, 128, 30, 25, 1, False, 'affine_relu', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test, ctrgcn_shipped_t60_test
        (640, 128, 128, 30, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60_test, stgcn_shipped_t60_test
        (640, 128, 128, 30, 25, 1, False, 'res_plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60_test
        (640, 128, 128, 30, 25, 1, True, 'res_plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test
        (640, 128, 128, 50, 25, 1, False, 'affine_relu', False, True, 'direct', 'dgrad_wgrad'),   # ds_t100_test
        (640, 128, 128, 50, 25, 1, True, 'res_plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t100_test
        (640, 128, 128, 60, 25, 1, False, 'res_affine', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ctrgcn_shipped_t60_test
        (640, 128, 128, 60, 25, 1, True, 'res_affine', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_test
        (640, 128, 144, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test, ds_t100_test
        (640, 128, 256, 15, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_test, ctrgcn_shipped_t60_test, stgcn_shipped_t60_test
        (640, 128, 256, 25, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t100_test
        (640, 128, 256, 30, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test, ctrgcn_shipped_t60_test
        (640, 128, 256, 50, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t100_test
        (640, 128, 288, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test, ds_t100_test
        (640, 128, 384, 30, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60_test, stgcn_shipped_t60_test
        (640, 128, 48, 30, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test
        (640, 128, 48, 50, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t100_test
        (640, 128, 768, 30, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60_test, stgcn_shipped_t60_test
        (640, 128, 96, 1, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60_test
        (640, 128, 96, 30, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test
        (640, 128, 96, 50, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t100_test
        (640, 16, 128, 25, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60_test
        (640, 16, 240, 25, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60_test
        (640, 16, 256, 25, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60_test
        (640, 24, 64, 100, 25, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # ds_t100_test
        (640, 24, 64, 60, 25, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # ds_t60_test
        (640, 256, 192, 1, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60_test
        (640, 256, 256, 15, 25, 1, False, 'affine_relu', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_test, ctrgcn_shipped_t60_test
        (640, 256, 256, 15, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ctrgcn_shipped_t60_test, stgcn_shipped_t60_test
        (640, 256, 256, 15, 25, 1, False, 'res_plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ctrgcn_shipped_t60_test
        (640, 256, 256, 15, 25, 1, True, 'res_plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_test
        (640, 256, 256, 25, 25, 1, False, 'affine_relu', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t100_test
        (640, 256, 256, 25, 25, 1, True, 'res_plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t100_test
        (640, 256, 256, 30, 25, 1, False, 'res_affine', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60_test
        (640, 256, 256, 30, 25, 1, True, 'res_affine', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test
        (640, 256, 256, 50, 25, 1, True, 'res_affine', False, True, 'direct', 'dgrad_wgrad'),   # ds_t100_test
        (640, 256, 288, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test, ds_t100_test
        (640, 256, 768, 15, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ctrgcn_shipped_t60_test, stgcn_shipped_t60_test
        (640, 256, 96, 15, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_test
        (640, 256, 96, 25, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t100_test
        (640, 3, 192, 60, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60_test, stgcn_shipped_t60_test
        (640, 3, 24, 100, 25, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # ds_t100_test
        (640, 3, 24, 60, 25, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # ds_t60_test
        (640, 3, 48, 1, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60_test
        (640, 3, 64, 100, 25, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # ds_t100_test
        (640, 3, 64, 60, 25, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # ds_t60_test, ctrgcn_shipped_t60_test
        (640, 3, 72, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test, ds_t100_test
        (640, 32, 256, 25, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60_test
        (640, 32, 480, 25, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60_test
        (640, 48, 128, 100, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t100_test
        (640, 48, 128, 30, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test
        (640, 48, 128, 50, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t100_test
        (640, 48, 128, 60, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test
        (640, 64, 128, 100, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t100_test
        (640, 64, 128, 30, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test, ctrgcn_shipped_t60_test, stgcn_shipped_t60_test
        (640, 64, 128, 50, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t100_test
        (640, 64, 128, 60, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_test, ctrgcn_shipped_t60_test
        (640, 64, 144, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test, ds_t100_test
        (640, 64, 192, 60, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ctrgcn_shipped_t60_test, stgcn_shipped_t60_test
        (640, 64, 24, 100, 25, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # ds_t100_test
        (640, 64, 24, 60, 25, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # ds_t60_test
        (640, 64, 384, 60, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ctrgcn_shipped_t60_test, stgcn_shipped_t60_test
        (640, 64, 48, 1, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60_test
        (640, 64, 48, 100, 25, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # ds_t100_test
        (640, 64, 48, 60, 25, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # ds_t60_test
        (640, 64, 64, 100, 25, 1, False, 'affine_relu', False, True, 'direct', 'bwd64'),   # ds_t100_test
        (640, 64, 64, 100, 25, 1, True, 'res_affine', False, True, 'direct', 'dgrad_wgrad'),   # ds_t100_test
        (640, 64, 64, 100, 25, 1, True, 'res_plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t100_test
        (640, 64, 64, 60, 25, 1, False, 'affine_relu', False, True, 'direct', 'bwd64'),   # ds_t60_test, ctrgcn_shipped_t60_test
        (640, 64, 64, 60, 25, 1, False, 'plain', False, True, 'direct', 'bwd64'),   # ctrgcn_shipped_t60_test, stgcn_shipped_t60_test
        (640, 64, 64, 60, 25, 1, False, 'res_affine', False, True, 'direct', 'bwd64'),   # ctrgcn_shipped_t60_test
        (640, 64, 64, 60, 25, 1, False, 'res_plain', False, True, 'direct', 'bwd64'),   # ctrgcn_shipped_t60_test
        (640, 64, 64, 60, 25, 1, True, 'res_affine', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test
        (640, 64, 64, 60, 25, 1, True, 'res_plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test
        (640, 64, 72, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test, ds_t100_test
        (640, 8, 120, 25, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60_test
        (640, 8, 128, 25, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60_test
        (640, 8, 64, 25, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ctrgcn_shipped_t60_test
        (640, 96, 256, 15, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t60_test
        (640, 96, 256, 25, 25, 1, False, 'plain', False, True, 'gemm_bf16', 'dgrad_wgrad'),   # ds_t100_test
        (640, 96, 256, 30, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t60_test
        (640, 96, 256, 50, 25, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),   # ds_t100_test
    ],
    # (n, Ci, Co, T, V, stride, KT, dilation, want_bn)
    'tconv': [
        (256, 128, 128, 30, 25, 1, 9, 1, False),   # stgcn_shipped_t60
        (256, 128, 128, 60, 25, 2, 9, 1, False),   # stgcn_shipped_t60
        (256, 256, 256, 15, 25, 1, 9, 1, False),   # stgcn_shipped_t60
        (256, 256, 256, 30, 25, 2, 9, 1, False),   # stgcn_shipped_t60
        (256, 64, 64, 60, 25, 1, 9, 1, False),   # stgcn_shipped_t60
        (640, 128, 128, 30, 25, 1, 9, 1, False),   # stgcn_shipped_t60_test
        (640, 128, 128, 60, 25, 2, 9, 1, False),   # stgcn_shipped_t60_test
        (640, 256, 256, 15, 25, 1, 9, 1, False),   # stgcn_shipped_t60_test
        (640, 256, 256, 30, 25, 2, 9, 1, False),   # stgcn_shipped_t60_test
        (640, 64, 64, 60, 25, 1, 9, 1, False),   # stgcn_shipped_t60_test
    ],
    # (shape,[ EVAL: an input without history, three aliases and no launch])
    'tee3': [
        ((140, 3, 60, 25), EVAL),   # ds_t60_test_tail
        ((256, 3, 100, 25),),   # ds_t100
        ((256, 3, 60, 25), EVAL),   # ds_t60_val
        ((256, 3, 60, 25),),   # ds_t60, ctrgcn_shipped_t60, stgcn_shipped_t60
        ((54, 3, 60, 25),),   # ds_t60_tail
        ((640, 3, 100, 25), EVAL),   # ds_t100_test
        ((640, 3, 60, 25), EVAL),   # ds_t60_test, ctrgcn_shipped_t60_test, stgcn_shipped_t60_test
    ],
    # (n, C, T, V, stride, branches, widths, n_act, causal taps KM, merge_after, want_bn)
    'temporal_mlp_bn': [
        (256, 128, 30, 25, 1, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, 2, True, True),   # ctrgcn_shipped_t60
        (256, 128, 60, 25, 2, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, 2, True, True),   # ctrgcn_shipped_t60
        (256, 256, 15, 25, 1, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, 2, True, True),   # ctrgcn_shipped_t60
        (256, 256, 30, 25, 2, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, 2, True, True),   # ctrgcn_shipped_t60
        (256, 64, 60, 25, 1, DGMSTCN, (14, 10, 10, 10, 10, 10), 54, 2, True, True),   # ctrgcn_shipped_t60
        (640, 128, 30, 25, 1, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, 2, True, False),   # ctrgcn_shipped_t60_test
        (640, 128, 60, 25, 2, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, 2, True, False),   # ctrgcn_shipped_t60_test
        (640, 256, 15, 25, 1, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, 2, True, False),   # ctrgcn_shipped_t60_test
        (640, 256, 30, 25, 2, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, 2, True, False),   # ctrgcn_shipped_t60_test
        (640, 64, 60, 25, 1, DGMSTCN, (14, 10, 10, 10, 10, 10), 54, 2, True, False),   # ctrgcn_shipped_t60_test
    ],
    # (n, C, T, V, stride, branches, widths, n_act, want_bn, path)
    'temporal_ms': [
        (140, 128, 30, 25, 1, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, False, 'staged'),   # ds_t60_test_tail
        (140, 128, 60, 25, 2, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, False, 'staged'),   # ds_t60_test_tail
        (140, 256, 15, 25, 1, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, False, 'staged'),   # ds_t60_test_tail
        (140, 256, 30, 25, 2, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, False, 'staged'),   # ds_t60_test_tail
        (140, 64, 60, 25, 1, DGMSTCN, (14, 10, 10, 10, 10, 10), 54, False, 'split'),   # ds_t60_test_tail
        (256, 128, 100, 25, 2, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, True, 'staged'),   # ds_t100
        (256, 128, 30, 25, 1, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, False, 'staged'),   # ds_t60_val
        (256, 128, 30, 25, 1, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, True, 'staged'),   # ds_t60
        (256, 128, 50, 25, 1, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, True, 'staged'),   # ds_t100
        (256, 128, 60, 25, 2, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, False, 'staged'),   # ds_t60_val
        (256, 128, 60, 25, 2, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, True, 'staged'),   # ds_t60
        (256, 256, 15, 25, 1, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, False, 'staged'),   # ds_t60_val
        (256, 256, 15, 25, 1, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, True, 'staged'),   # ds_t60
        (256, 256, 25, 25, 1, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, True, 'staged'),   # ds_t100
        (256, 256, 30, 25, 2, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, False, 'staged'),   # ds_t60_val
        (256, 256, 30, 25, 2, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, True, 'staged'),   # ds_t60
        (256, 256, 50, 25, 2, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, True, 'staged'),   # ds_t100
        (256, 64, 100, 25, 1, DGMSTCN, (14, 10, 10, 10, 10, 10), 54, True, 'staged'),   # ds_t100
        (256, 64, 60, 25, 1, DGMSTCN, (14, 10, 10, 10, 10, 10), 54, False, 'split'),   # ds_t60_val
        (256, 64, 60, 25, 1, DGMSTCN, (14, 10, 10, 10, 10, 10), 54, True, 'split'),   # ds_t60
        (54, 128, 30, 25, 1, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, True, 'staged'),   # ds_t60_tail
        (54, 128, 60, 25, 2, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, True, 'staged'),   # ds_t60_tail
        (54, 256, 15, 25, 1, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, True, 'staged'),   # ds_t60_tail
        (54, 256, 30, 25, 2, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, True, 'staged'),   # ds_t60_tail
        (54, 64, 60, 25, 1, DGMSTCN, (14, 10, 10, 10, 10, 10), 54, True, 'split'),   # ds_t60_tail
        (640, 128, 100, 25, 2, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, False, 'staged'),   # ds_t100_test
        (640, 128, 30, 25, 1, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, False, 'staged'),   # ds_t60_test
        (640, 128, 50, 25, 1, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, False, 'staged'),   # ds_t100_test
        (640, 128, 60, 25, 2, DGMSTCN, (23, 21, 21, 21, 21, 21), 107, False, 'staged'),   # ds_t60_test
        (640, 256, 15, 25, 1, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, False, 'staged'),   # ds_t60_test
        (640, 256, 25, 25, 1, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, False, 'staged'),   # ds_t100_test
        (640, 256, 30, 25, 2, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, False, 'staged'),   # ds_t60_test
        (640, 256, 50, 25, 2, DGMSTCN, (46, 42, 42, 42, 42, 42), 214, False, 'staged'),   # ds_t100_test
        (640, 64, 100, 25, 1, DGMSTCN, (14, 10, 10, 10, 10, 10), 54, False, 'staged'),   # ds_t100_test
        (640, 64, 60, 25, 1, DGMSTCN, (14, 10, 10, 10, 10, 10), 54, False, 'split'),   # ds_t60_test
    ],
    # (n, C, T, V, stride, causal taps KM, dilations, dense KT, dense dilation, merge_after, want_bn)
    'temporal_unitmlp_bn': [
        (256, 128, 30, 25, 1, 5, (1,), 9, 1, True, True),   # stgcn_shipped_t60
        (256, 128, 60, 25, 2, 5, (1,), 9, 1, True, True),   # stgcn_shipped_t60
        (256, 256, 15, 25, 1, 5, (1,), 9, 1, True, True),   # stgcn_shipped_t60
        (256, 256, 30, 25, 2, 5, (1,), 9, 1, True, True),   # stgcn_shipped_t60
        (256, 64, 60, 25, 1, 5, (1,), 9, 1, True, True),   # stgcn_shipped_t60
        (640, 128, 30, 25, 1, 5, (1,), 9, 1, True, False),   # stgcn_shipped_t60_test
        (640, 128, 60, 25, 2, 5, (1,), 9, 1, True, False),   # stgcn_shipped_t60_test
        (640, 256, 15, 25, 1, 5, (1,), 9, 1, True, False),   # stgcn_shipped_t60_test
        (640, 256, 30, 25, 2, 5, (1,), 9, 1, True, False),   # stgcn_shipped_t60_test
        (640, 64, 60, 25, 1, 5, (1,), 9, 1, True, False),   # stgcn_shipped_t60_test
    ],
    # (n, C, T, V, ld)
    'tmean': [
        (140, 3, 60, 25, 32),   # ds_t60_test_tail
        (256, 3, 100, 25, 32),   # ds_t100
        (256, 3, 60, 25, 25),   # ctrgcn_shipped_t60
        (256, 3, 60, 25, 32),   # ds_t60, ds_t60_val
        (54, 3, 60, 25, 32),   # ds_t60_tail
        (640, 3, 100, 25, 32),   # ds_t100_test
        (640, 3, 60, 25, 25),   # ctrgcn_shipped_t60_test
        (640, 3, 60, 25, 32),   # ds_t60_test
    ],
}


@pytest.fixture(scope='module')
def recorded():
    seen = KC.census(TRAIN_RUNS, _model_cfg)
    for op, keys in KC.census_eval(EVAL_RUNS, _model_cfg).items():
        for key, runs in keys.items():
            seen.setdefault(op, {}).setdefault(key, []).extend(runs)
    return seen


@pytest.mark.gpu
def test_shipped_census_every_kernel_call_is_in_the_tables(recorded):
    missing = {op: {k: runs for k, runs in keys.items() if k not in FULL_SIZE_CASES.get(op, ())
                    and k not in MODEL_CASES.get(op, ()) and k not in SHIPPED_CASES.get(op, ())}
               for op, keys in recorded.items() if op != KC.BN_PAIRS}
    missing = {op: keys for op, keys in missing.items() if keys}
    assert not missing, ('kernel calls of the shipped-config runs that FULL_SIZE_CASES, MODEL_CASES and SHIPPED_CASES '
                         'lack:\n' + _listing(missing))


@pytest.mark.gpu
def test_shipped_census_table_has_no_stale_entries(recorded):
    stale = {op: [k for k in keys if k not in recorded.get(op, {})] for op, keys in SHIPPED_CASES.items()}
    stale = {op: keys for op, keys in stale.items() if keys}
    assert not stale, f'SHIPPED_CASES entries no shipped-config run records: {stale!r}'
    assert all(len(set(keys)) == len(keys) for keys in SHIPPED_CASES.values())


@pytest.mark.gpu
def test_shipped_census_no_bn_coef_launch_writes_one_batchnorm_twice(recorded):
    assert KC.BN_PAIRS not in recorded, _listing({KC.BN_PAIRS: recorded.get(KC.BN_PAIRS, {})})


def test_shipped_cases_are_disjoint_from_the_other_tables():
    both = {op: [k for k in keys if k in FULL_SIZE_CASES.get(op, ()) or k in MODEL_CASES.get(op, ())]
            for op, keys in SHIPPED_CASES.items()}
    both = {op: keys for op, keys in both.items() if keys}
    assert not both, f'SHIPPED_CASES entries that FULL_SIZE_CASES or MODEL_CASES already holds: {both!r}'
    assert set(SHIPPED_CASES) <= set(KEYS), sorted(set(SHIPPED_CASES) - set(KEYS))


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 comparisons of SHIPPED_CASES
# ---------------------------------------------------------------------------------------------------------------------
# As in the other censuses: each key goes to the check_* helper of tests/test_kernels_gpu.py that the op's own test runs,
# with that test's bars; a key whose arguments are already one of that test's cases is not run twice.  A key only the
# eval runs record (_eval_only) is checked the way those runs call it: under torch.no_grad() on inputs without history,
# outputs against fp64.  That needs a forward-only form of the helper; the ops whose helpers have none (aggregate,
# dynadj, ctr_topology, fuse_out, gram, tmean) do not read grad mode (KC.GRAD_READING), so the helper's forward is the
# launch the eval runs make, and its backward is checked besides.

EVAL_BATCHES = (640, 140)        # n of the 10-clip test runs (32 and 7 videos x 10 clips x 2 persons); no training run's
FORWARD_ONLY = ('aggregate_sum', 'pwconv', 'tconv', 'temporal_ms', 'temporal_mlp_bn', 'temporal_unitmlp_bn')


def _eval_only(op, k):
    """Does only an eval run record this key?  (test_shipped_census_eval_only_keys_are_eval_records checks the rule)"""
    if op == 'tee3':
        return k[-1] == EVAL
    if op == 'data_bn':
        return k[-1] == EVAL
    if k[0] in EVAL_BATCHES:
        return True
    # the statistics-free forms of the stages that feed a BatchNorm: the eval runs' (validation at n = 256 included)
    return op in ('temporal_ms', 'temporal_mlp_bn', 'temporal_unitmlp_bn', 'aggregate_sum') and not _want_bn(op, k)


def _want_bn(op, k):
    return k[-2] if op == 'temporal_ms' else k[-1] if op != 'aggregate_sum' else k[6]


@pytest.mark.gpu
def test_shipped_census_eval_only_keys_are_eval_records(recorded):
    """A key checked forward-only must not be a training launch too (its backward would go unchecked)."""
    evals = {name for name, *_ in EVAL_RUNS}
    wrong = {op: [k for k in keys if _eval_only(op, k) and not set(recorded[op][k]) <= evals]
             for op, keys in SHIPPED_CASES.items() if op in recorded}
    wrong = {op: keys for op, keys in wrong.items() if keys}
    assert not wrong, f'keys taken as eval-only that a training run records: {wrong!r}'


def _cases(op, to_args, test=None, keep=lambda key: True):
    return KC._cases(op, lambda k: to_args(k), test, keep, table=SHIPPED_CASES)


def _fwd(op, args, k):
    """The helper's forward-only mode for an eval-only key of FORWARD_ONLY."""
    if op in FORWARD_ONLY and _eval_only(op, k):
        return dict(args, **({'want_bn': False} if op.startswith('temporal') else {'grad': False}))
    return args


def _aggsum_args(k):
    n, Kk, Co, T, V, form, bn = k
    assert form in ('shared', 'per_channel'), k
    return _fwd('aggregate_sum', dict(n=n, K=Kk, Co=Co, T=T, V=V, shared=form == 'shared', bn=bn), k)


def _data_bn_args(k):
    # check_data_bn compares the training form and then the eval form on the running statistics: one check for both keys
    return dict(zip(('N', 'M', 'T', 'V', 'C', 'bn_type', 'affine'), k[:7]))


def _pw_args(k):
    return _fwd('pwconv', KC._pw_args(k), k)


def _tconv_args(k):
    n, Ci, Co, T, V, stride, KT, dil, want_bn = k
    return _fwd('tconv', dict(n=n, Ci=Ci, Co=Co, T=T, V=V, stride=stride, ks=KT, dil=dil, bn=want_bn), k)


def _ms_args(k):
    n, C, T, V, stride, cfg, widths, n_act, want_bn, path = k
    mid = C // 6
    assert cfg == DGMSTCN and widths == (C - 5 * mid,) + (mid,) * 5 and n_act == C - mid, k
    args = dict(n=n, C=C, T=T, V=V, stride=stride, fused={'fused': '1', 'split': 'split', 'staged': '0'}[path])
    return _fwd('temporal_ms', args, k) if not want_bn else args


def _mlp_args(k):
    n, C, T, V, stride, cfg, widths, n_act, KM, merge_after, want_bn = k
    assert widths == tuple(KG._ms_widths(C, cfg)) and n_act == C - widths[-1] and KM == (cfg[0][0] + 1) // 2, k
    args = dict(n=n, C=C, T=T, V=V, stride=stride, cfg=cfg, merge_after=merge_after)
    return _fwd('temporal_mlp_bn', args, k) if not want_bn else args


def _unitmlp_args(k):
    n, C, T, V, stride, KM, dils, KT, tdil, merge_after, want_bn = k
    assert len(dils) == 1 and KM == (KT + 1) // 2 and tdil == dils[0] and KT > 0, k
    args = dict(n=n, C=C, T=T, V=V, stride=stride, ks=KT, dil=tdil, add_tcn=True, merge_after=merge_after,
                zero_dil=False)
    return _fwd('temporal_unitmlp_bn', args, k) if not want_bn else args


MAPS = dict(aggregate=lambda k: dict(zip(('n', 'KC', 'T', 'V', 'relu', 'affine'), k)), aggregate_sum=_aggsum_args,
            ctr_topology=KC._ctr_args, data_bn=_data_bn_args, dynadj=KC._dyn_args, fuse_out=KC._fuse_args,
            fuse_out_pool=KC._pool_args, gram=lambda k: k,
            head_loss=lambda k: dict(N=k[0], M=k[1], C=k[2], K=k[3], lw=1.0, bias=k[4]), pwconv=_pw_args,
            tconv=_tconv_args, tee3=lambda k: k, temporal_ms=_ms_args, temporal_mlp_bn=_mlp_args,
            temporal_unitmlp_bn=_unitmlp_args,
            tmean=lambda k: dict(n=k[0], C=k[1], T=k[2], V=k[3], ld=True if k[4] == k[3] else k[4]))


def test_shipped_cases_map_to_their_checks():
    """Every SHIPPED_CASES key maps to the arguments of its check (no GPU needed: the mappings assert what they assume);
    no key records dropout (the shipped configs train with tcn_dropout = 0), and every want_bn False form of a stage that
    feeds a BatchNorm is an eval-only key, compared forward-only."""
    assert set(SHIPPED_CASES) <= set(MAPS), sorted(set(SHIPPED_CASES) - set(MAPS))
    for op, keys in SHIPPED_CASES.items():
        for key in keys:
            MAPS[op](key)
    assert not any(k[8] for k in SHIPPED_CASES['fuse_out']) and not any(k[6] for k in SHIPPED_CASES['fuse_out_pool'])
    for op in ('temporal_ms', 'temporal_mlp_bn', 'temporal_unitmlp_bn', 'aggregate_sum'):
        for k in SHIPPED_CASES[op]:
            assert _want_bn(op, k) != _eval_only(op, k) or k[0] in EVAL_BATCHES, (op, k)


@pytest.mark.gpu
@pytest.mark.parametrize('key,args', _cases('aggregate', MAPS['aggregate'], KG.test_aggregate))
def test_aggregate_shipped_census(key, args):
    KG.check_aggregate(**args)


@pytest.mark.gpu
@pytest.mark.parametrize('key,args', _cases('aggregate_sum', _aggsum_args, KG.test_aggregate_sum))
def test_aggregate_sum_shipped_census(key, args):
    KG.check_aggregate_sum(**args)


@pytest.mark.gpu
@pytest.mark.parametrize('key,args', _cases('ctr_topology', KC._ctr_args, KG.test_ctr_topology))
def test_ctr_topology_shipped_census(key, args):
    KG.check_ctr_topology(**args)


@pytest.mark.gpu
@pytest.mark.parametrize('key,args', _cases('data_bn', _data_bn_args, KG.test_data_bn))
def test_data_bn_shipped_census(key, args):
    KG.check_data_bn(**args)


@pytest.mark.gpu
@pytest.mark.parametrize('key,args', _cases('dynadj', KC._dyn_args, KG.test_dynadj))
def test_dynadj_shipped_census(key, args):
    KG.check_dynadj(**args)


@pytest.mark.gpu
@pytest.mark.parametrize('key,args', _cases('fuse_out', KC._fuse_args, KG.test_fuse_out))
def test_fuse_out_shipped_census(key, args):
    KG.check_fuse_out(**args)


@pytest.mark.gpu
@pytest.mark.parametrize('key,args', _cases('fuse_out_pool', KC._pool_args, KG.test_fuse_out_pool))
def test_fuse_out_pool_shipped_census(key, args):
    KG.check_fuse_out_pool(**args)


@pytest.mark.gpu
@pytest.mark.parametrize('key', SHIPPED_CASES['gram'], ids=repr)
def test_gram_shipped_census(key):
    KG.check_gram(*key)


@pytest.mark.gpu
@pytest.mark.parametrize('key,args', _cases('head_loss', MAPS['head_loss'], KG.test_head_loss))
def test_head_loss_shipped_census(key, args):
    KG.check_head_loss(**args)


@pytest.mark.gpu
@pytest.mark.parametrize('key,args', _cases('pwconv', _pw_args, KG.test_pwconv))
def test_pwconv_shipped_census(key, args):
    assert key[-2:] == KC._pw_paths(*key[:7])
    KG.check_pwconv(**args)


@pytest.mark.gpu
@pytest.mark.parametrize('key,args', _cases('tconv', _tconv_args, KG.test_tconv_dense))
def test_tconv_dense_shipped_census(key, args):
    KG.check_tconv_dense(**args)


@pytest.mark.gpu
@pytest.mark.parametrize('key', SHIPPED_CASES['tee3'], ids=repr)
def test_tee3_shipped_census(key):
    """Training: the three aliases' gradients meet in one dsgcn_add3 launch (fp64 sum).  EVAL: an input without history
    comes back three times as itself, no launch and no autograd node."""
    shape = key[0]
    g = torch.Generator().manual_seed(3)
    x = torch.randn(*shape, generator=g).to(KC.DEV)
    if key[-1] == EVAL:
        with torch.no_grad():
            outs = K.tee3(x)
        assert all(t is x for t in outs)
        return
    x.requires_grad_()
    gs = [torch.randn(*shape, generator=g) for _ in range(3)]
    a, b, c = K.tee3(x)
    assert all(t.data_ptr() == x.data_ptr() for t in (a, b, c))
    ((a * gs[0].to(KC.DEV)).sum() + (b * gs[1].to(KC.DEV)).sum() + (c * gs[2].to(KC.DEV)).sum()).backward()
    want = sum(t.double() for t in gs)
    assert KG.rel(x.grad, want) < 1e-7, KG.rel(x.grad, want)


@pytest.mark.gpu
@pytest.mark.parametrize('key,args', _cases('temporal_ms', _ms_args))
def test_temporal_ms_shipped_census(key, args, monkeypatch):
    p = _Path(monkeypatch)
    KG.check_temporal_ms(**args, monkeypatch=monkeypatch)
    assert set(p.taken) <= {p.path()} and p.path() == key[-1], (p.taken, key[-1])


@pytest.mark.gpu
@pytest.mark.parametrize('key,args', _cases('temporal_mlp_bn', _mlp_args, KG.test_temporal_mlp_bn))
def test_temporal_mlp_bn_shipped_census(key, args):
    KG.check_temporal_mlp_bn(**args)


@pytest.mark.gpu
@pytest.mark.parametrize('key,args', _cases('temporal_unitmlp_bn', _unitmlp_args, KG.test_temporal_unitmlp_bn))
def test_temporal_unitmlp_bn_shipped_census(key, args):
    KG.check_temporal_unitmlp_bn(**args)


@pytest.mark.gpu
@pytest.mark.parametrize('key,args', _cases('tmean', MAPS['tmean']))
def test_tmean_shipped_census(key, args):
    KG.check_tmean(**args)


# ---------------------------------------------------------------------------------------------------------------------
# forward_test of the full-width models at the shipped clip lengths against the oracle in fp64
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('model,T,fuse', [('ds', 60, False), ('ds', 100, False), ('ds', 60, True), ('ds', 100, True),
                                          ('ctrgcn_shipped', 60, False), ('stgcn_shipped', 60, False)])
def test_forward_test_vs_oracle_at_shipped_clip_lengths(model, T, fuse):
    """model(keypoint=x, return_loss=False) of 2 videos x 10 clips (n = 40) in eval mode, running statistics from a
    train-mode forward moved by a seeded draw, against the oracle's training=False forward in fp64 on the host: averaged
    probabilities rel < 1e-5, per-clip scores rel < 1e-4 (the bars of test_eval_mode_vs_reference_fixture).  fuse: the same after checkpoint.fuse_conv_bn."""
    import dsgcn_amd
    from oracle import dsgcn_oracle as O
    V, videos, clips = 25, 2, 10
    np.random.seed(0)
    torch.manual_seed(0)
    m = dsgcn_amd.build_model(_model_cfg(model))
    gen = torch.Generator().manual_seed(5)
    # DS-STGCN as test_full_model_vs_oracle sets it up; the other two as test_full_other_backbones_vs_oracle (alpha only:
    # CTR-GCN's Gram term at beta = randn * 0.5 compounds over ten blocks and overflows fp64 in eval mode)
    drawn = ('alpha', 'beta', 'add_coeff') if model == 'ds' else ('alpha',)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith(drawn):
                p.copy_(torch.randn(p.shape, generator=gen) * 0.5)
    m = m.to(KC.DEV)
    x = torch.randn(videos, clips, 2, T, V, 3, generator=gen)
    # running statistics: one train-mode forward's batch statistics (momentum 1), then moved by a seeded draw, so that the
    # affines are neither the identity nor the batch's (uncalibrated draws blow up CTR-GCN's Gram term in eval mode)
    bns = [mod for mod in m.modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)]
    for bn in bns:
        bn.momentum = 1.0
    m.train().extract_feat(x.to(KC.DEV).flatten(0, 1))
    with torch.no_grad():
        for bn in bns:
            bn.momentum = 0.1
            sd_ = bn.running_var.sqrt()
            bn.running_mean.add_(torch.randn(bn.running_mean.shape, generator=gen).to(KC.DEV) * 0.1 * sd_)
            bn.running_var.mul_(torch.exp(torch.randn(bn.running_var.shape, generator=gen) * 0.2).to(KC.DEV))
    m = m.cpu().eval()
    sd = {k: (v.detach().double() if v.is_floating_point() else v.detach()).clone() for k, v in m.state_dict().items()}
    xs = x.double().flatten(0, 1)[:, None]
    y = torch.zeros(videos * clips, 1, dtype=torch.long)
    if model == 'ds':
        gcs = O.graph_constants('nturgb+d')
        ref, _ = O.recognizer_forward_train(xs, y, sd, gcs['node_type'], gcs['edge_type'], O.dgstgcn_plan(),
                                            training=False)
    else:
        plan = O.ctrgcn_plan() if model == 'ctrgcn_shipped' else O.dgstgcn_plan()
        ref, _ = O.recognizer_forward_train_backbone(model, xs, y, sd, plan, training=False)
    ref = ref.view(videos, clips, -1)
    if fuse:
        dsgcn_amd.fuse_conv_bn(m)
    m = m.to(KC.DEV)
    probs = m(keypoint=x.to(KC.DEV), return_loss=False)
    assert isinstance(probs, np.ndarray) and probs.shape == (videos, ref.shape[-1])
    assert KG.rel(torch.from_numpy(probs), ref.softmax(-1).mean(1)) < 1e-5
    with torch.no_grad():
        scores = m.cls_head(m.extract_feat(x.to(KC.DEV).flatten(0, 1))).view(videos, clips, -1)
    assert KG.rel(scores.cpu(), ref) < 1e-4
