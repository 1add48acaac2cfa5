"""CPU: the head's loss options (class weights, soft labels, multi-label BCE, label smoothing) against the reference's fp64
values (tests/golden/headloss.npz), the registry / config surface, what stays rejected, the new C-ABI entry points'
argument checks and the new kernels' code objects."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dsgcn_amd as D
import head_target_fp64 as H
from dsgcn_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
Z = H.fixture()
CASES = [str(c) for c in Z['cases']]
# Two fp64 evaluations of one formula: 1e-12 relative.  Observed: the torch path reproduces every fixture value bit for
# bit; over the forward_loss seam only ce_wsoft differs (the twin multiplies q, log p and w in another order): 3.5e-16 on
# the loss, below 1e-16 on the gradients.
BAR64 = 1e-12


def _head(cfg, t):
    """The package's GCNHead of a fixture case, its weights loaded through the reference's state_dict keys, fp64."""
    head = D.build_head(copy.deepcopy(cfg))
    assert sorted(head.state_dict()) == json.loads(str(t['sd_keys'])) == ['fc_cls.bias', 'fc_cls.weight']
    head.load_state_dict({'fc_cls.weight': t['fc_cls.weight'], 'fc_cls.bias': t['fc_cls.bias']}, strict=True)
    return head.double().train()


def _check(out, head, x, t, name, feat_grad=None):
    reports_acc = 'top1_acc64' in t
    assert set(out) == ({'top1_acc', 'top5_acc', 'loss_cls'} if reports_acc else {'loss_cls'}), (name, set(out))
    out['loss_cls'].backward()
    got = dict(loss=out['loss_cls'], dx=x.grad if feat_grad is None else feat_grad(x.grad), dw=head.fc_cls.weight.grad,
               db=head.fc_cls.bias.grad)
    errs = {k: H.rel(v, t[k + '64']) for k, v in got.items()}
    print(name, {k: f'{e:.1e}' for k, e in errs.items()})
    assert all(e < BAR64 for e in errs.values()), (name, errs)
    if reports_acc:
        assert float(out['top1_acc']) == float(t['top1_acc64']) and float(out['top5_acc']) == float(t['top5_acc64'])


@pytest.mark.parametrize('name', CASES)
def test_fixture_case_on_the_torch_path(name):
    """``head.loss(head(x), label)``: the loss modules themselves (the path of heads with dropout and of CPU runs)."""
    cfg, t = H.fixture_case(Z, name)
    head = _head(cfg, t)
    x = t['x'].double().requires_grad_()
    label = t['label'].double() if t['label'].is_floating_point() else t['label']
    _check(head.loss(head(x), label), head, x, t, name)


@pytest.mark.parametrize('name', CASES)
def test_fixture_case_through_forward_loss(name):
    """``head.forward_loss`` over the CPU seam: the mode the head picks, the label handling of heads/base.py:60-77 and the
    arguments it hands to ``head_target`` (the fp64 twin of the kernel stands in for it)."""
    cfg, t = H.fixture_case(Z, name)
    head = _head(cfg, t)
    x = t['x'].double().requires_grad_()
    label = t['label'].double() if t['label'].is_floating_point() else t['label']
    calls = []
    with D.kernels.use_ops(H.cpu_ops(calls)):
        out = head.forward_loss(x, label)
    assert calls == ['head_target']
    _check(out, head, x, t, name)


def test_forward_loss_picks_the_path():
    """No class weights + integer labels: today's ``head_loss`` call; everything else the issue lists: ``head_target``."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 2, 8, generator=g).double()
    hard, soft = torch.tensor([0, 4, 2]), torch.softmax(torch.randn(3, 5, generator=g), 1).double()
    seen = []

    def ns():
        ops = H.cpu_ops()
        real = ops.head_target
        ops.head_loss = (lambda f=ops.head_loss: lambda *a, **k: (seen.append(('head_loss',)), f(*a, **k))[1])()
        ops.head_target = lambda feat, w, b, tg, M, mode, cw=None, lw=1.0: (
            seen.append(('head_target', mode, cw is not None, lw)), real(feat, w, b, tg, M, mode, cw, lw))[1]
        return ops
    table = [
        (dict(), hard, ('head_loss',), True),
        (dict(loss_cls=dict(type='CrossEntropyLoss', class_weight=[1, 2, 3, 4, 5])), hard, ('head_target', 0, True, 1.0), True),
        (dict(loss_cls=dict(type='CrossEntropyLoss', loss_weight=0.5)), soft, ('head_target', 1, False, 0.5), False),
        (dict(loss_cls=dict(type='BCELossWithLogits'), multi_class=True), soft, ('head_target', 2, False, 1.0), False),
        (dict(multi_class=True), hard, ('head_loss',), False),          # base.py:66: a multi_class head reports no accuracy
    ]
    for kw, label, want, acc in table:
        head = D.build_head(dict(type='GCNHead', num_classes=5, in_channels=8, **kw)).double()
        del seen[:]
        with D.kernels.use_ops(ns()):
            out = head.forward_loss(x, label)
        assert seen == [want], (kw, seen)
        assert ('top1_acc' in out) == acc and ('top5_acc' in out) == acc and 'loss_cls' in out
    # a head with dropout takes loss(forward(x), label): the loss modules, no fused op
    head = D.build_head(dict(type='GCNHead', num_classes=5, in_channels=8, dropout=0.5,
                             loss_cls=dict(type='CrossEntropyLoss', class_weight=[1, 2, 3, 4, 5]))).double().eval()
    del seen[:]
    with D.kernels.use_ops(ns()):
        out = head.forward_loss(x, hard)
    want = torch.nn.functional.cross_entropy(head(x), hard, weight=torch.tensor([1., 2, 3, 4, 5]).double())
    assert seen == [] and torch.equal(out['loss_cls'], want)


def test_label_smoothing_only_on_multi_class_heads():
    """base.py:74-75: ``label_smooth_eps`` without ``multi_class`` changes nothing."""
    g = torch.Generator().manual_seed(1)
    score = torch.randn(4, 6, generator=g).double()
    q = (torch.rand(4, 6, generator=g) < 0.4).double()
    kw = dict(type='GCNHead', num_classes=6, in_channels=8, loss_cls=dict(type='BCELossWithLogits'))
    plain = D.build_head(dict(kw)).loss(score, q)['loss_cls']
    ignored = D.build_head(dict(kw, label_smooth_eps=0.1)).loss(score, q)['loss_cls']
    smoothed = D.build_head(dict(kw, label_smooth_eps=0.1, multi_class=True)).loss(score, q)['loss_cls']
    want = torch.nn.functional.binary_cross_entropy_with_logits(score, 0.9 * q + 0.1 / 6)
    assert torch.equal(plain, ignored) and not torch.equal(plain, smoothed)
    assert abs(float(smoothed) - float(want)) < 1e-15


def test_class_weight_is_a_buffer_outside_the_state_dict():
    for typ in ('CrossEntropyLoss', 'BCELossWithLogits'):
        loss = D.build_loss(dict(type=typ, loss_weight=0.5, class_weight=[1.0, 2.0, 0.0]))
        assert loss.loss_weight == 0.5 and loss.class_weight.tolist() == [1.0, 2.0, 0.0]
        assert dict(loss.named_buffers()).keys() == {'class_weight'} and not loss.state_dict()
        assert loss.double().class_weight.dtype == torch.float64          # follows .to() like any buffer
        assert D.build_loss(dict(type=typ)).class_weight is None
    with pytest.raises(ValueError):
        D.build_loss(dict(type='CrossEntropyLoss', class_weight=[1.0, 2.0]))(torch.zeros(2, 3), torch.tensor([0, 1]))


CFG = dict(type='RecognizerGCN',
           backbone=dict(type='DGSTGCN', gcn_type='dgphgcn1', gcn_ratio=0.125, gcn_node_attention=True,
                         gcn_edge_attention=True, gcn_decompose=True, gcn_subset_wise=True, gcn_ctr='T', gcn_ada='T',
                         tcn_type='dgmstcn', base_channels=16, num_stages=4, inflate_stages=[3], down_stages=[3],
                         graph_cfg=dict(layout='nturgb+d', mode='random', num_filter=3, init_off=.04, init_std=.02),
                         tcn_ms_cfg=[(3, 1), (3, 2), (3, 3), (3, 4), ('max', 3), '1x1']),
           cls_head=dict(type='GCNHead', num_classes=4, in_channels=32))
HEAD_OPTIONS = {
    'class_weight': dict(loss_cls=dict(type='CrossEntropyLoss', class_weight=[1.0, 4.0, 0.5, 2.0])),
    'loss_weight': dict(loss_cls=dict(type='CrossEntropyLoss', loss_weight=0.5)),
    'bce': dict(loss_cls=dict(type='BCELossWithLogits', class_weight=[1.0, 4.0, 0.5, 2.0]), multi_class=True),
    'bce_smooth': dict(loss_cls=dict(type='BCELossWithLogits'), multi_class=True, label_smooth_eps=0.1),
}


@pytest.mark.parametrize('opt', sorted(HEAD_OPTIONS))
def test_build_model_takes_each_option(opt):
    cfg = copy.deepcopy(CFG)
    cfg['cls_head'].update(copy.deepcopy(HEAD_OPTIONS[opt]))
    ref_keys = set(D.build_model(copy.deepcopy(CFG)).state_dict())
    m = D.build_model(cfg)
    want = HEAD_OPTIONS[opt]
    assert type(m.cls_head.loss_cls).__name__ == want['loss_cls']['type']
    assert m.cls_head.multi_class == want.get('multi_class', False)
    assert m.cls_head.label_smooth_eps == want.get('label_smooth_eps', 0.0)
    assert set(m.state_dict()) == ref_keys                      # the options add no checkpoint key
    assert 'BCELossWithLogits' in D.LOSSES and 'CrossEntropyLoss' in D.LOSSES


def test_what_stays_rejected(tmp_path):
    import pickle
    ann = tmp_path / 'ann.pkl'
    with open(ann, 'wb') as f:
        pickle.dump([dict(frame_dir='a', label=0, keypoint=np.zeros((1, 4, 25, 3), np.float32), total_frames=4)], f)
    D.PoseDataset(str(ann), pipeline=[])
    with pytest.raises(NotImplementedError):
        D.PoseDataset(str(ann), pipeline=[], multi_class=True)
    with pytest.raises(TypeError):                              # F.cross_entropy's extra kwargs
        D.build_loss(dict(type='CrossEntropyLoss'))(torch.zeros(2, 3), torch.tensor([0, 1]), label_smoothing=0.1)
    with pytest.raises(NotImplementedError):                    # BCE on integer labels
        D.build_loss(dict(type='BCELossWithLogits'))(torch.zeros(2, 3), torch.tensor([0, 1]))


def test_entry_points_declared_bound_and_checking_their_arguments():
    from test_native_abi import declared_symbols
    new = {'dsgcn_head_target_fwd', 'dsgcn_head_target_bwd'}
    assert new <= set(declared_symbols()) and new <= set(native.SIGNATURES)
    lib = native.lib()
    one = 16                                                    # any non-NULL, 16-byte aligned address: nothing is launched
    fwd = lambda **k: lib.dsgcn_head_target_fwd(  # noqa: E731
        k.get('feat', one), one, None, None, k.get('target', one), k.get('mode', 0), k.get('N', 4), 2, k.get('C', 64),
        k.get('K', 10), 1.0, one, one, one, one, one, k.get('den', one), k.get('acc', one), None)
    assert fwd(feat=None) == -1 and fwd(target=None) == -1 and fwd(den=None) == -1
    assert fwd(N=0) == -1 and fwd(K=-1) == -1 and fwd(mode=3) == -1 and fwd(mode=-1) == -1
    assert fwd(acc=None) == -1                                  # mode 0 writes the accuracies
    assert fwd(C=15000, K=400) == -2 and fwd(C=256, K=15200, mode=1, acc=None) == -2      # (C + K) floats > 60 KB
    bwd = lambda **k: lib.dsgcn_head_target_bwd(  # noqa: E731
        k.get('ds', one), one, one, one, k.get('den', one), k.get('N', 4), 2, 64, k.get('K', 10), 1.0, one, one, one, None)
    assert bwd(ds=None) == -1 and bwd(den=None) == -1 and bwd(N=0) == -1
    assert bwd(N=15361) == -2 and bwd(K=15361) == -2            # max(N, K) floats > 60 KB


def test_head_target_kernels_have_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import codeobj_report
    native.build()
    ks = {k: v for k, v in codeobj_report.kernels(native.LIB_PATH).items() if k.startswith('k_htarget')}
    assert sorted(ks) == ['k_htarget_bwd', 'k_htarget_fin', 'k_htarget_fwd<0>', 'k_htarget_fwd<1>', 'k_htarget_fwd<2>']
    for name, k in ks.items():
        assert k.get('scratch_instructions', 0) == 0 and k.get('vgpr_spill_count', 0) == 0, (name, k)
        assert k.get('sgpr_spill_count', 0) == 0 and k.get('private_segment_fixed_size', 0) == 0, (name, k)


def test_fixture_regenerates_byte_identically_live(tmp_path):
    import ref_shim
    if not ref_shim.available():
        pytest.skip('the reference checkout is not on this machine')
    subprocess.run([sys.executable, os.path.join(GOLD, 'gen_golden_headloss.py'), '--out', str(tmp_path)], check=True,
                   capture_output=True)
    with open(os.path.join(GOLD, 'headloss.npz'), 'rb') as f, open(tmp_path / 'headloss.npz', 'rb') as g:
        assert f.read() == g.read()
    assert os.path.getsize(os.path.join(GOLD, 'headloss.npz')) < 200_000
