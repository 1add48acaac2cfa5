"""-m gpu: ``dggcn`` at numbers of subsets other than three on the HIP path — K-C projections + the plain K-B (csrc/
dynadj_plain.hip) — against the reference's fixtures (tests/golden/unit_dggcn_k.npz, model_reduced_dggcn_k8), against the
fp64 restatement (tests/dggcn_plain_fp64.py) at full batch, against the two-launch K = 3 form, and the K = 8 DG-STGCN
through the kernel census, a captured TrainEngine step, the InferEngine and a checkpoint round trip."""
import copy

import numpy as np
import pytest
import torch

import dsgcn_amd as D
from dsgcn_amd import kernels as K
import dggcn_plain_fp64 as F
import test_dggcn_plain_host as H
from test_dggcn_plain_host import CASES, Z, ZERO_GRAD_BIASES
from test_oracle_golden import rel, sd_of
import test_kernel_census_gpu as KC
import test_kernels_gpu as KG
from test_model_census_gpu import MODEL_CASES

pytestmark = pytest.mark.gpu
DEV = 'cuda'


# ---- 7. the unit against the reference's fixture -------------------------------------------------------------------------

@pytest.mark.parametrize('tag', CASES)
def test_dggcn_k_unit_vs_reference_fixture(tag):
    """The unit on the HIP path against the reference's fp64 output, input gradient and every parameter gradient
    (tests/golden/unit_dggcn_k.npz: whole arrays or their probes), and element by element against the fp64 restatement
    of the same weights (pinned to the reference by tests/test_dggcn_plain_host.py)."""
    m, c = H.make_unit(tag)
    p64 = {k: v.detach().double().cuda().requires_grad_() for k, v in m.named_parameters()}
    m = m.cuda().train()
    x32, r32 = H.unit_inputs(tag)
    x = x32.cuda().requires_grad_()
    y = m(x)
    (y * r32.cuda()).sum().backward()
    x64 = x32.double().cuda().requires_grad_()
    y64 = F.unit_forward(p64, x64, c['subset_wise'])
    (y64 * r32.double().cuda()).sum().backward()
    for got, want, key, bar in ((y, y64, '_y', 1e-5), (x.grad, x64.grad, '_dx', 5e-5)):
        e_fix = F.fixture_rel(Z, tag + key, got.detach().cpu().numpy())
        e_ful = rel(got.detach().cpu(), want.detach().cpu())
        print(f'{tag}{key}: fixture {e_fix:.2e}, fp64 {e_ful:.2e}')
        assert e_fix < bar and e_ful < bar, (key, e_fix, e_ful)
    par = dict(m.named_parameters())
    for k, p in par.items():
        key = tag + '_grad_' + k
        if k in ZERO_GRAD_BIASES:
            # the bias of a conv under a train-mode BatchNorm: the true gradient is exactly zero (so is the fixture's, to
            # fp64 rounding), a relative error does not exist.  The 1e-4 bar of the parameter gradients is applied to the
            # conv's gradient as a whole: what the bias holds is rounding noise of the sums that also make the weight's.
            assert np.abs(Z[key]).max() < 1e-10, k
            e = float(p.grad.norm() / par[k[:-4] + 'weight'].grad.norm()) if p.grad is not None else 0.0
            print(f'{tag} grad {k}: |db| / |dW| {e:.2e}')
            assert e < 1e-4, (k, e)
            continue
        if F.fixture_is_zero(Z, key):              # alpha[1:], beta[1:] are unused without subset_wise
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
        else:
            e_fix = F.fixture_rel(Z, key, p.grad.cpu().numpy())
            e_ful = rel(p.grad.cpu(), p64[k].grad.cpu())
            print(f'{tag} grad {k}: fixture {e_fix:.2e}, fp64 {e_ful:.2e}')
            assert e_fix < 1e-4 and e_ful < 1e-4, (k, e_fix, e_ful)


# ---- 8. the adjacency path at full size -----------------------------------------------------------------------------------

def plain_inputs(n, Ci, Kk, mid, V, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(
        xbar=torch.randn(n, Ci, V, generator=g),
        A=torch.randn(Kk, V, V, generator=g) * 0.02 + 0.04,
        alpha=torch.randn(Kk, generator=g) * 0.5, beta=torch.randn(Kk, generator=g) * 0.5,
        w1=torch.randn(Kk * mid, Ci, generator=g) / Ci ** 0.5, b1=torch.randn(Kk * mid, generator=g) * 0.1,
        w2=torch.randn(Kk * mid, Ci, generator=g) / Ci ** 0.5, b2=torch.randn(Kk * mid, generator=g) * 0.1)


def check_plain_kb(n, Ci, Kk, mid, V):
    """Ahat, d xbar and every parameter gradient of K-C projection + plain K-B against fp64 torch on the GPU, at the bars
    of test_kernels_gpu.check_dynadj; a second run is bit-identical."""
    t = plain_inputs(n, Ci, Kk, mid, V, seed=Ci + mid + Kk)
    dah = torch.randn(n, Kk * mid, V, V, generator=torch.Generator().manual_seed(7))
    order = list(t)

    def run(fn, dt):
        tt = {k: v.to(DEV, dt).requires_grad_() for k, v in t.items()}
        out = fn(*[tt[k] for k in order])
        out.backward(dah.to(DEV, dt))
        return out, {k: v.grad for k, v in tt.items()}

    out, grads = run(K.dynadj_plain, torch.float32)
    ro, rg = run(F.dynadj_plain, torch.float64)
    e = rel(out.detach().cpu(), ro.detach().cpu())
    print(f'Ahat {e:.2e}')
    assert e < 2e-6, e
    for k in order:
        e = rel(grads[k].cpu(), rg[k].cpu())
        print(f'd{k} {e:.2e}')
        assert e < 2e-5, (k, e)
    out2, grads2 = run(K.dynadj_plain, torch.float32)
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in order)


# (Ci, Co, K, ratio): the six (Ci, Co) of the 10-stage model at K = 8 ratio 0.125, the widest at 0.25 (mid = 64), and
# K = 5 at ratio=None (mid = 12)
FULL = [(3, 64, 8, 0.125), (64, 64, 8, 0.125), (64, 128, 8, 0.125), (128, 128, 8, 0.125), (128, 256, 8, 0.125),
        (256, 256, 8, 0.125), (256, 256, 8, 0.25), (60, 60, 5, None)]


@pytest.mark.parametrize('Ci,Co,Kk,ratio', FULL)
def test_plain_kb_full_size_vs_fp64(Ci, Co, Kk, ratio):
    check_plain_kb(128, Ci, Kk, int((1 / Kk if ratio is None else ratio) * Co), 25)


@pytest.mark.parametrize('V', [17, 18])
def test_plain_kb_other_joint_counts_vs_fp64(V):
    """17 joints (coco: its own instantiation) and 18 (openpose: the run-time form), K = 8, 64 -> 128."""
    check_plain_kb(128, 64, 8, 16, V)


@pytest.mark.parametrize('n,Ci,Kk,mid,V', [(3, 64, 3, 21, 25), (2, 16, 16, 5, 32), (5, 32, 1, 64, 32), (2, 8, 7, 3, 11)])
def test_plain_kb_odd_shapes_vs_fp64(n, Ci, Kk, mid, V):
    """mid * V * V not a multiple of 4 (the first and last 16-byte slot of a workgroup's rows are partial), the largest
    supported K, mid and V, and a small odd graph."""
    check_plain_kb(n, Ci, Kk, mid, V)


# ---- 9. the new kernel against the two-launch K = 3 form --------------------------------------------------------------------

def test_plain_kb_vs_two_launch_form_at_three_subsets():
    """``dynadj_plain`` at K = 3 and ``dggcn.adjacency`` (two dsgcn_dynadj launches + a concatenation) on the same weights
    and input: both are fp32 evaluations of one formula, so each one's error is measured against the fp64 restatement
    and the new kernel's may be at most 2x the old path's — forward and every gradient."""
    n, Ci, Co, V = 128, 64, 128, 25
    torch.manual_seed(5)
    m = D.dggcn(Ci, Co, H.graph_A('nturgb+d', 3), ratio=0.25, subset_wise=True)
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        m.alpha.copy_(torch.randn(3, generator=g) * 0.5)
        m.beta.copy_(torch.randn(3, generator=g) * 0.5)
        m.conv1.bias.copy_(torch.randn(m.conv1.bias.shape, generator=g) * 0.1)
        m.conv2.bias.copy_(torch.randn(m.conv2.bias.shape, generator=g) * 0.1)
    xbar = torch.randn(n, Ci, V, generator=g)
    dah = torch.randn(n, 3 * m.mid_channels, V, V, generator=g)
    names = ('A', 'alpha', 'beta', 'conv1.weight', 'conv1.bias', 'conv2.weight', 'conv2.bias')
    p64 = {k: dict(m.named_parameters())[k].detach().double().to(DEV).requires_grad_() for k in names}
    x64 = xbar.double().to(DEV).requires_grad_()
    F.adjacency(x64, *[p64[k] for k in names]).backward(dah.double().to(DEV))
    want64 = F.adjacency(x64.detach(), *[p64[k].detach() for k in names])
    m = m.to(DEV)
    par = dict(m.named_parameters())

    def run(new):
        m.zero_grad(set_to_none=True)
        x = xbar.to(DEV).requires_grad_()
        if new:
            out = K.dynadj_plain(x, m.A, m.alpha, m.beta, m.conv1.weight.flatten(1), m.conv1.bias,
                                 m.conv2.weight.flatten(1), m.conv2.bias)
        else:
            out = m.adjacency(x)
        out.backward(dah.to(DEV))
        err = {'Ahat': rel(out.detach().cpu(), want64.cpu()), 'dxbar': rel(x.grad.cpu(), x64.grad.cpu())}
        err.update({'d' + k: rel(par[k].grad.cpu(), p64[k].grad.cpu()) for k in names})
        return err

    old, new = run(False), run(True)
    for k in old:
        print(f'{k}: two-launch form {old[k]:.3e}, plain K-B {new[k]:.3e}')
    for k in old:
        assert new[k] <= 2 * old[k], (k, new[k], old[k])


# ---- 10. the other kernels of a K = 8 step ----------------------------------------------------------------------------------

K8_RUNS = (('dggcn_k8', 'dggcn_k8', 64, 64, 25, 60, False),)      # one eager 64-clip train step of the K = 8 DG-STGCN

# The keys that step records and neither FULL_SIZE_CASES (the BASELINE steps) nor MODEL_CASES (the other shipped models)
# holds, and nothing else.
K8_CASES = {
    # (n, KC, T, V, relu, affine): K-A over K * mid = 64 / 128 / 256 per-channel adjacencies
    'aggregate': [
        (128, 128, 32, 25, True, True),
        (128, 128, 64, 25, True, True),
        (128, 256, 16, 25, True, True),
        (128, 256, 32, 25, True, True),
        (128, 64, 64, 25, True, True),
    ],
    # (n, Ci, Co, T, V, stride, aug, input mode, want_bn, bias, forward form, backward form): the Ci -> 2 * Co projections
    # on the padded (n, Ci, 1, 32) time mean, and the `pre` convs Ci -> K * mid = Co that no other model has at T x 25
    'pwconv': [
        (128, 128, 128, 32, 25, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),
        (128, 128, 128, 64, 25, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),
        (128, 128, 256, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),
        (128, 128, 512, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),
        (128, 256, 256, 16, 25, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),
        (128, 256, 256, 32, 25, 1, False, 'plain', True, True, 'gemm_bf16', 'dgrad_wgrad'),
        (128, 256, 512, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),
        (128, 3, 128, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),
        (128, 64, 128, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),
        (128, 64, 256, 1, 32, 1, False, 'plain', False, True, 'direct', 'dgrad_wgrad'),
        (128, 64, 64, 64, 25, 1, False, 'plain', True, True, 'direct', 'bwd64'),
    ],
}


@pytest.fixture(scope='module')
def recorded_k8():
    return KC.census(runs=K8_RUNS, cfg_of=lambda model: H.k8_cfg())


def _known(op, key):
    return key in KC.FULL_SIZE_CASES.get(op, ()) or key in MODEL_CASES.get(op, ())


def test_k8_census_every_kernel_call_is_in_a_table(recorded_k8):
    missing = {op: {k: runs for k, runs in keys.items() if not _known(op, k) and k not in K8_CASES.get(op, ())}
               for op, keys in recorded_k8.items() if op != KC.BN_PAIRS}
    missing = {op: keys for op, keys in missing.items() if keys}
    assert not missing, 'kernel calls of the K = 8 step that no table holds:\n' + KC._listing(missing)
    assert KC.BN_PAIRS not in recorded_k8


def test_k8_census_table_has_no_stale_entries(recorded_k8):
    stale = {op: [k for k in keys if k not in recorded_k8.get(op, {}) or _known(op, k)] for op, keys in K8_CASES.items()}
    stale = {op: keys for op, keys in stale.items() if keys}
    assert not stale, f'K8_CASES entries the K = 8 step does not record, or another table already holds: {stale!r}'
    assert set(K8_CASES) <= {'aggregate', 'pwconv'}, 'give the new op its check below'


@pytest.mark.parametrize('key', K8_CASES.get('aggregate', []), ids=repr)
def test_aggregate_k8_census(key):
    KG.check_aggregate(*key)


@pytest.mark.parametrize('key', K8_CASES.get('pwconv', []), ids=repr)
def test_pwconv_k8_census(key):
    assert key[-2:] == KC._pw_paths(*key[:7])
    KG.check_pwconv(**KC._pw_args(key))


# ---- 11. the reduced K = 8 model against the reference -----------------------------------------------------------------------

def _reduced():
    z, cfg = H.reduced_k8()
    m = D.build_model(copy.deepcopy(cfg))
    m.load_state_dict(sd_of(z, 'sd_', torch.float32))
    assert all(type(b.gcn).__name__ == 'dggcn' and b.gcn.num_subsets == 8 for b in m.backbone.gcn)
    return z, m


def test_dggcn_k8_reduced_model_vs_golden():
    z, m = _reduced()
    m = m.cuda().train()
    x, y = torch.from_numpy(z['x']).cuda(), torch.from_numpy(z['label']).cuda()
    logits = m.cls_head(m.extract_feat(x[:, 0]))
    loss = m.cls_head.loss(logits, y.squeeze(-1))['loss_cls']
    loss.backward()
    e_log = rel(logits.detach().cpu(), z['logits_f64'])
    e_loss = abs(loss.item() - float(z['loss_f64'])) / abs(float(z['loss_f64']))
    num = den = num32 = 0.0
    for k, p in m.named_parameters():
        if 'g64_' + k in z:
            g64 = z['g64_' + k].astype(np.float64)
            num += float(((p.grad.double().cpu().numpy() - g64) ** 2).sum())
            num32 += float(((z['g32_' + k].astype(np.float64) - g64) ** 2).sum())
            den += float((g64 ** 2).sum())
    err, ref_err = (num / den) ** .5, (num32 / den) ** .5
    print(f'logits {e_log:.2e}, loss {e_loss:.2e}, gradient {err:.2e} (the reference in fp32: {ref_err:.2e})')
    assert e_log < 1e-4 and e_loss < 1e-4
    assert err < 2e-4, err                                    # whole-gradient relative L2 vs fp64 truth
    assert err <= 2 * ref_err, (err, ref_err)                 # ... and within 2x the reference's own fp32 error


def test_dggcn_k8_eval_logits_and_fuse_conv_bn():
    z, m = _reduced()
    m = m.cuda().eval()
    x = torch.from_numpy(z['x']).cuda()
    with torch.no_grad():
        logits = m.cls_head(m.extract_feat(x[:, 0]))
        e = rel(logits.cpu(), z['logits_eval_f64'])
        D.fuse_conv_bn(m)
        fused = m.cls_head(m.extract_feat(x[:, 0]))
    print(f'eval logits {e:.2e}, fused vs unfused {rel(fused.cpu(), logits.cpu()):.2e}')
    assert e < 1e-4, e
    assert rel(fused.cpu(), logits.cpu()) <= 1e-5, rel(fused.cpu(), logits.cpu())


# ---- 12. the engines on the full-width K = 8 DG-STGCN ---------------------------------------------------------------------

def _k8_model(seed=0):
    torch.manual_seed(seed)
    np.random.seed(seed)
    m = D.build_model(H.k8_cfg())
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith(('alpha', 'beta', 'add_coeff')):
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
    return m


def test_dggcn_k8_train_engine_step_graphed_bit_identical():
    """A 64-clip TrainEngine step of the K = 8 DG-STGCN, captured as a hipGraph: finite, and the gradients and parameters
    of two runs from the same weights are bit-identical (no float atomics on the new path)."""
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(64, 1, 2, 64, 25, 3, generator=gen).cuda()
    y = torch.randint(0, 60, (64, 1), generator=gen).cuda()
    sd = _k8_model().state_dict()
    runs = []
    for _ in range(2):
        m = D.build_model(H.k8_cfg())
        m.load_state_dict(sd)
        m = m.cuda().train()
        eng = D.TrainEngine(m, lr=0.05, use_graph=True, warmup_eager=2)
        for _ in range(3):
            logs = eng.step(x, y)
        torch.cuda.synchronize()
        assert eng.graphed(x, y), eng.capture_error
        assert torch.isfinite(logs['loss']).item()
        runs.append((eng.flat.flat_g.detach().clone(), eng.flat.flat_p.detach().clone()))
    assert torch.isfinite(runs[0][0]).all()
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])


def test_dggcn_k8_infer_engine_replay_is_the_eager_engine():
    m = _k8_model()
    KC.fill_running_stats(m, torch.Generator().manual_seed(2))
    m = m.cuda().eval()
    x = torch.randn(2, 3, 2, 32, 25, 3, generator=torch.Generator().manual_seed(4)).cuda()
    eager = D.InferEngine(m, use_graph=False)
    want = eager(x)
    assert eager.replays == 0 and not eager.graphed(x)
    eng = D.InferEngine(m, warmup_eager=1)
    for _ in range(eng.warmup_eager + 1):
        eng(x)
    before = eng.replays
    got = eng(x)
    assert eng.capture_error is None and eng.graphed(x) and eng.replays == before + 1
    assert torch.isfinite(got).all()
    assert torch.equal(got, want), rel(got.cpu(), want.cpu())


# ---- 13. checkpoint round trip ------------------------------------------------------------------------------------------------

def test_dggcn_k8_checkpoint_round_trip(tmp_path):
    m = _k8_model()
    KC.fill_running_stats(m, torch.Generator().manual_seed(2))
    path = str(tmp_path / 'k8.pth')
    D.save_checkpoint(m, path)
    fresh = D.build_model(H.k8_cfg())
    D.load_checkpoint(fresh, path, strict=True)
    assert tuple(fresh.backbone.gcn[0].gcn.A.shape) == (8, 25, 25)
    x = torch.randn(4, 2, 32, 25, 3, generator=torch.Generator().manual_seed(4)).cuda()
    with torch.no_grad():
        a = m.cuda().eval()
        b = fresh.cuda().eval()
        la = a.cls_head(a.extract_feat(x))
        lb = b.cls_head(b.extract_feat(x))
    assert torch.isfinite(la).all() and torch.equal(la, lb)
