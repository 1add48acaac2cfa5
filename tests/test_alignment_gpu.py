"""-m gpu: every kernel family against its own fp64 statement with every operand at an address that is 4, 8 or 12 mod 16.

The bodies are the existing ``check_*`` / ``test_*`` functions, run unchanged — their references, their tolerances, their
bit-equality assertions between two launches (both launches then run shifted) — under ``layout_cases.shifted_operands``,
which hands every tensor that passes ``kernels._f32c`` (activations, weights, BatchNorm coefficients, incoming gradients)
to the kernel as a copy at the chosen alignment class.  The parameters of a trained model live at such addresses
(FlatParams packs them without padding); many kernels read their operands through 16-byte vector types and decide that
from sizes alone, a few choose their summation order from the address.  The cases are the smallest existing ones that
reach each kernel family.  A case whose body moved no operand fails: it tested nothing."""
import pytest
import torch

import test_dggcn_plain_gpu as TP
import test_dghgcn_gpu as TH
import test_dgphgcn1_flags_gpu as TF
import test_ensemble_gpu as TE
import test_feat_ext_gpu as TX
import test_head_target_gpu as TT
import test_infer_gpu as TI
import test_kernels_gpu as TK
from dsgcn_amd import kernels as K
from layout_cases import shifted, shifted_operands

pytestmark = pytest.mark.gpu
KS = [1, 2, 3]


def run_shifted(monkeypatch, k, body, *args):
    moved = shifted_operands(monkeypatch, k)
    body(*args)
    assert moved.count > 0, 'vacuous: no operand went through _f32c'
    return moved.count


PWCONV = [(1, 5, 7, 9, 18, 2, True, 'affine_relu'),           # direct form, ragged everything
          (2, 64, 24, 64, 25, 1, False, 'res_affine'),        # one-pass backward (csrc/bwd64.hip)
          (2, 64, 128, 8, 16, 1, False, 'plain'),             # three-term GEMM form, smallest eligible plane
          (3, 128, 160, 12, 25, 1, False, 'res_affine'),      # three-term GEMM form, tiles straddle samples
          (2, 64, 64, 25, 17, 1, False, 'res_affine')]        # odd plane length (425)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('case', PWCONV, ids=repr)
def test_pwconv(case, k, monkeypatch):
    run_shifted(monkeypatch, k, TK.check_pwconv, *case)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('case', [(1, 5, 7, 25, True, True), (2, 10, 25, 17, True, True)], ids=repr)
def test_aggregate(case, k, monkeypatch):
    run_shifted(monkeypatch, k, TK.check_aggregate, *case)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('case', [(3, 3, 8, 25, 'nturgb+d'), (2, 64, 8, 17, 'coco')], ids=repr)
def test_dynadj(case, k, monkeypatch):
    run_shifted(monkeypatch, k, TK.check_dynadj, *case)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('case', [(2, 16, 24, 8, 25, 3, 'res_affine', 1), (2, 16, 16, 12, 18, 3, 'plain', 2)], ids=repr)
def test_tconv_gemm(case, k, monkeypatch):
    run_shifted(monkeypatch, k, TK.check_tconv_gemm, *case)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('case', [(1, 5, 7, 18, 'plain', True, 1), (2, 32, 16, 25, 'res_affine', False, 3)], ids=repr)
def test_fuse_out(case, k, monkeypatch):
    run_shifted(monkeypatch, k, TK.check_fuse_out, *case)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('case', [(2, 64, 16, 25, 'res_plain', 1, 'plain', 0.5), (3, 12, 9, 25, 'res_affine', 1, 'tmean', 0.1)],
                         ids=repr)
def test_fuse_out_dropout(case, k, monkeypatch):
    run_shifted(monkeypatch, k, TK.check_fuse_out_dropout, *case)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('case', [(1, 5, 7, 18, 'plain', 1), (2, 16, 8, 25, 'res_affine', 0)], ids=repr)
def test_fuse_out_pool(case, k, monkeypatch):
    run_shifted(monkeypatch, k, TK.check_fuse_out_pool, *case)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('case', [(3, 8, 9, 25, 3), (2, 12, 7, 17, 2)], ids=repr)
def test_fuse_out_even_frame_output(case, k, monkeypatch):
    run_shifted(monkeypatch, k, TK.test_fuse_out_even_frame_output, *case)


# all three forms on shapes the split layout takes (V odd, T % 4 == 0; stride 2: T % 8 == 0): a single 4-frame unit, the
# smallest joint count, a stride-2 stage; the fused and the staged form also on a ragged shape the split layout refuses
TEMPORAL_MS = [(c, f) for c in [(1, 64, 4, 25, 1), (2, 36, 8, 5, 1), (2, 128, 32, 25, 2)] for f in ('1', '0', 'split')]
TEMPORAL_MS += [((1, 12, 9, 18, 2), '1'), ((1, 12, 9, 18, 2), '0')]


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('case,fused', TEMPORAL_MS, ids=repr)
def test_temporal_ms(case, fused, k, monkeypatch):
    run_shifted(monkeypatch, k, TK.check_temporal_ms, *case, fused, monkeypatch)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('case', [(1, 2, 5, 7, 18, False, False), (2, 3, 64, 16, 25, True, True)], ids=repr)
def test_aggregate_sum(case, k, monkeypatch):
    run_shifted(monkeypatch, k, TK.check_aggregate_sum, *case)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('case', [(2, 3, 64, 25, False), (2, 64, 64, 25, True)], ids=repr)
def test_ctr_topology(case, k, monkeypatch):
    run_shifted(monkeypatch, k, TK.check_ctr_topology, *case)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('case', [(1, 16, 9, 18, 1, 3, '1'), (2, 32, 21, 17, 2, 5, '0')], ids=repr)
def test_temporal_branches_bn(case, k, monkeypatch):
    run_shifted(monkeypatch, k, TK.check_temporal_branches_bn, *case, monkeypatch)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('case', [(1, 12, 4, 17, 1, TK.CFG6, True), (2, 18, 7, 18, 2, TK.CFG6, False)], ids=repr)
def test_temporal_mlp_bn(case, k, monkeypatch):
    run_shifted(monkeypatch, k, TK.check_temporal_mlp_bn, *case)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('case', [(1, 8, 6, 17, 1, 9, 2, False, False, False), (2, 12, 7, 18, 2, 5, 4, False, True, True)], ids=repr)
def test_temporal_unitmlp_bn(case, k, monkeypatch):
    run_shifted(monkeypatch, k, TK.check_temporal_unitmlp_bn, *case)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('case', [(2, 16, 16, 12, 18, 1, 3, 2, True), (2, 40, 72, 21, 17, 2, 9, 1, False)], ids=repr)
def test_tconv_dense(case, k, monkeypatch):
    run_shifted(monkeypatch, k, TK.check_tconv_dense, *case)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('R,C', [(1664, 192), (128, 48), (7, 3)])
def test_colsum(R, C, k):
    """test_colsum's body; colsum takes its input by address (no `_f32c`), so the input itself is the shifted copy.
    (1664, 192): C % 4 == 0 and C >= 128 — the address alone chooses between the 16-byte fast path and the scalar one."""
    t = torch.randn(R, C)
    s = shifted(t.cuda(), k)
    assert s.data_ptr() % 16 == 4 * k
    assert TK.rel(K.colsum(s).cpu(), t.double().sum(0)) < 1e-6


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('case', [(5, 1, 96, 3, 1.0, False), (7, 3, 70, 11, 2.0, True), (1, 2, 256, 60, 1.0, True)], ids=repr)
def test_head_loss(case, k, monkeypatch):
    run_shifted(monkeypatch, k, TK.check_head_loss, *case)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('case', [(5, 1, 7, 18, 2, 'MVC', True), (2, 3, 30, 25, 9, 'VC', False)], ids=repr)
def test_data_bn(case, k, monkeypatch):
    run_shifted(monkeypatch, k, TK.check_data_bn, *case)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('case', [(1, 5, 7, 18), (2, 64, 16, 25)], ids=repr)
def test_aagcn_gram_gates_and_per_sample_aggregate(case, k, monkeypatch):
    run_shifted(monkeypatch, k, TK.test_aagcn_gram_gates_and_per_sample_aggregate, *case)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('add_type', [False, True])
def test_typed_kb(add_type, k, monkeypatch):
    run_shifted(monkeypatch, k, TH.test_typed_kb_small_shapes_vs_fp64, (2, 8, 5, 17, 3, 4), add_type)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('case', [(2, 8, 7, 3, 11), (3, 64, 3, 21, 25)], ids=repr)
def test_plain_kb(case, k, monkeypatch):
    run_shifted(monkeypatch, k, TP.check_plain_kb, *case)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('word', [6, 17])
def test_flag_kb(word, k, monkeypatch):
    run_shifted(monkeypatch, k, TF.test_flag_kb_small_shapes_vs_fp64, (2, 8, 5, 17, 3, 4, 17), word)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('shape', [(1, 2, 256, 60), (7, 3, 70, 11)], ids=repr)
def test_head_target(shape, mode, k, monkeypatch):
    """(1, 2, 256, 60): C % 4 == 0, so the weight's address alone chooses the 16-byte loads or the scalar ones."""
    run_shifted(monkeypatch, k, TT.test_head_target_vs_fp64, shape, mode, True, True)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('mode', ['prob', None])
def test_head_test(mode, k, monkeypatch):
    run_shifted(monkeypatch, k, TI.test_head_test_vs_fp64, 5, 3, 1, 64, 7, True, mode)      # C = 64: the address decides


@pytest.mark.parametrize('k', KS)
def test_feat_ext(k, monkeypatch):
    run_shifted(monkeypatch, k, TX.test_kernel_case, 'all')                                 # C = 8: the address decides


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('mode', ['prob', 'score'])
def test_head_ensemble(mode, k, monkeypatch):
    run_shifted(monkeypatch, k, TE.test_head_ensemble_equals_head_launches_and_host_sum, (2, 3, 5, 64, 2, 4), mode)
