"""-m gpu: the head with class weights, soft labels and multi-label BCE (csrc/head_target.hip) against its fp64 CPU twin
(tests/head_target_fp64.py) and the reference's fp64 values (tests/golden/headloss.npz), its determinism, its edge cases,
the untouched default path, and TrainEngine on soft-label / class-weighted batches eagerly and as replayed hipGraphs.

The bar on the loss and on each gradient (error against fp64 relative to the norm): the larger of head.hip's 2e-6
(test_kernels_gpu.check_head_loss) and twice the error of the same formula evaluated by torch in fp32 on the CPU.
Every case prints its errors beside that fp32 error; profiles/head_target/README.md is where the maxima are kept."""
import copy
import faulthandler
import functools

import numpy as np
import pytest
import torch

import dsgcn_amd as D
import head_target_fp64 as H
from dsgcn_amd import kernels as K_
from dsgcn_amd import native

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BAR = H.HEAD_LOSS_BAR
SHAPES = [(1, 2, 256, 60),          # one clip
          (5, 1, 96, 3),            # K < 5 for top-5, one partly filled class pass
          (7, 3, 70, 11),           # C % 4 != 0: the scalar path
          (9, 2, 260, 2),           # more than one 256-channel chunk, binary
          (6, 2, 256, 400),         # K > 256: block-stride loops
          (300, 1, 8, 5)]           # N > 256 in the backward's per-class blocks
GRADS = ('dfeat', 'dw', 'db')


def _run(mod, dt, dev, c, mode, use_cw, bias, lw):
    leaf = lambda t: t.detach().to(dev, dt).clone().requires_grad_()  # noqa: E731  (the cached inputs stay untouched)
    f, ww = leaf(c['feat']), leaf(c['w'])
    bb = leaf(c['b']) if bias else None
    tg = c['target'][mode].to(dev)
    tg = tg.to(dt) if tg.is_floating_point() else tg
    cw = c['cw'].to(dev, dt) if use_cw else None
    loss, acc, score = mod.head_target(f, ww, bb, tg, c['M'], mode, cw, lw)
    loss.backward(torch.tensor(0.7).to(dev, dt))
    out = dict(loss=loss.detach(), score=score, dfeat=f.grad, dw=ww.grad)
    if bias:
        out['db'] = bb.grad
    if acc is not None:
        out['acc'] = acc
    return out


@functools.lru_cache(maxsize=None)
def _inputs(N, M, C, K):
    g = torch.Generator().manual_seed(N * 31 + K)
    hard = torch.randint(0, K, (N,), generator=g)
    hard[0] = 0                                                  # a class of non-zero weight is present
    cw = torch.rand(K, generator=g) * 2 + 0.25
    cw[K - 1] = 0.0                                              # one class at weight 0
    return dict(M=M, feat=torch.randn(N * M, C, generator=g), w=torch.randn(K, C, generator=g) * 0.2,
                b=torch.randn(K, generator=g) * 0.1, cw=cw,
                target={0: hard, 1: torch.softmax(torch.randn(N, K, generator=g) * 2, 1),
                        2: (torch.rand(N, K, generator=g) < 0.3).float()})


@functools.lru_cache(maxsize=None)
def _reference(shape, mode, use_cw, bias):
    """fp64 on the CPU, and the error of the same torch formula in fp32 on the CPU: computed once, never modified."""
    c = _inputs(*shape)
    lw = 0.5 if use_cw else 1.0
    ref = _run(H, torch.float64, 'cpu', c, mode, use_cw, bias, lw)
    f32 = _run(H, torch.float32, 'cpu', c, mode, use_cw, bias, lw)
    return ref, {k: H.rel(f32[k], ref[k]) for k in ref if k not in ('acc', 'score')}, lw


@pytest.mark.parametrize('bias', [True, False])
@pytest.mark.parametrize('use_cw', [False, True])
@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('shape', SHAPES)
def test_head_target_vs_fp64(shape, mode, use_cw, bias):
    c = _inputs(*shape)
    ref, e32, lw = _reference(shape, mode, use_cw, bias)
    got = _run(K_, torch.float32, DEV, c, mode, use_cw, bias, lw)
    assert got['loss'].dtype == torch.float32 and got['loss'].dim() == 0
    assert ('acc' in got) == (mode == 0)
    if mode == 0:
        assert got['acc'].dtype == torch.float64 and torch.equal(got['acc'].cpu(), ref['acc']), (got['acc'], ref['acc'])
    errs = {k: H.rel(got[k], ref[k]) for k in e32}
    print('head_target', shape, mode, use_cw, bias, {k: f'{errs[k]:.2e} (torch fp32 {e32[k]:.2e})' for k in errs},
          f"score {H.rel(got['score'], ref['score']):.2e}")
    assert H.rel(got['score'], ref['score']) < BAR
    for k in errs:
        assert errs[k] <= max(BAR, 2 * e32[k]), (k, errs[k], e32[k])
    # twice the same launch: bit-identical (fixed-order sums)
    again = _run(K_, torch.float32, DEV, c, mode, use_cw, bias, lw)
    assert all(torch.equal(got[k], again[k]) for k in got)


@pytest.mark.parametrize('shape', [(7, 3, 70, 11), (6, 2, 256, 400), (64, 2, 256, 60)])
@pytest.mark.parametrize('ones', [False, True])
def test_mode0_with_unit_weights_is_head_loss(shape, ones):
    """No class weights (NULL) and all weights 1: scores and accuracies are head_loss's bits, loss and gradients its values
    within the bar."""
    N, M, C, K = shape
    c = _inputs(*shape)
    cw = torch.ones(K, device=DEV) if ones else None

    def run(fn):
        f, ww, bb = (t.detach().to(DEV).requires_grad_() for t in (c['feat'], c['w'], c['b']))
        loss, acc, score = fn(f, ww, bb, c['target'][0].to(DEV))
        loss.backward(torch.tensor(0.7, device=DEV))
        return dict(loss=loss.detach(), acc=acc, score=score, dfeat=f.grad, dw=ww.grad, db=bb.grad)
    a = run(lambda f, w, b, y: K_.head_loss(f, w, b, y, M, 0.5))
    b = run(lambda f, w, b, y: K_.head_target(f, w, b, y, M, 0, cw, 0.5))
    assert torch.equal(a['acc'], b['acc']) and torch.equal(a['score'], b['score'])
    for k in ('loss',) + GRADS:
        assert H.rel(b[k], a[k]) < BAR, (k, H.rel(b[k], a[k]))


def test_ties_and_bad_label_with_class_weights():
    """test_head_loss_ties_and_bad_label with class weights: the stable-argsort tie rule, and a label outside [0, K) gives a
    NaN loss with the accuracies unchanged — its class weight is never loaded, the run ends clean."""
    K = 8
    w = torch.zeros(K, 4, device=DEV)
    b = torch.tensor([1., 1., 1., 1., 1., 1., 0., 0.], device=DEV)           # six classes tie at the top
    cw = torch.arange(1, K + 1, device=DEV).float()
    feat = torch.zeros(6, 4, device=DEV)
    label = torch.tensor([0, 1, 4, 5, 6, 7], device=DEV)
    loss, acc, _ = K_.head_target(feat, w, b, label, 1, 0, cw)
    assert acc.tolist() == [1 / 6, 3 / 6] and bool(torch.isfinite(loss))
    _, acc_ref, _ = H.head_target(feat.cpu().double(), w.cpu().double(), b.cpu().double(), label.cpu(), 1, 0, cw.cpu())
    assert acc_ref.tolist() == acc.tolist()
    for bad in (99, -1, 2 ** 40):
        loss, acc, _ = K_.head_target(feat, w, b, torch.tensor([0, 1, 4, 5, 6, bad], device=DEV), 1, 0, cw)
        torch.cuda.synchronize()
        assert torch.isnan(loss) and acc.tolist() == [1 / 6, 3 / 6]


def test_all_present_classes_at_weight_zero_is_nan():
    g = torch.Generator().manual_seed(2)
    feat, w = torch.randn(4, 8, generator=g), torch.randn(5, 8, generator=g)
    label = torch.tensor([1, 3, 3, 1])
    cw = torch.tensor([1., 0., 2., 0., 1.])
    want = torch.nn.functional.cross_entropy(feat @ w.t(), label, weight=cw)
    loss, acc, _ = K_.head_target(feat.to(DEV), w.to(DEV), None, label.to(DEV), 1, 0, cw.to(DEV))
    assert torch.isnan(want) and torch.isnan(loss) and bool(torch.isfinite(acc).all())


Z = H.fixture()


@pytest.mark.parametrize('name', [str(c) for c in Z['cases']])
def test_fixture_case_on_the_device(name):
    """``GCNHead.forward_loss`` on the (N, M, C) plane means of a fixture case (exact in fp32: the fixture's x holds
    multiples of 2^-10) against the reference's fp64 values; the bar's second term is the reference's own fp32 run."""
    cfg, t = H.fixture_case(Z, name)
    head = D.build_head(copy.deepcopy(cfg))
    head.load_state_dict({'fc_cls.weight': t['fc_cls.weight'], 'fc_cls.bias': t['fc_cls.bias']}, strict=True)
    head = head.to(DEV).train()
    feat = t['x'].double().mean((-1, -2)).float()
    assert torch.equal(feat.double(), t['x'].double().mean((-1, -2)))
    feat = feat.to(DEV).requires_grad_()
    out = head.forward_loss(feat, t['label'].to(DEV))
    assert set(out) == ({'top1_acc', 'top5_acc', 'loss_cls'} if 'top1_acc64' in t else {'loss_cls'})
    out['loss_cls'].backward()
    got = dict(loss=out['loss_cls'], dx=feat.grad, dw=head.fc_cls.weight.grad, db=head.fc_cls.bias.grad)
    for k, v in got.items():
        want, ref32 = t[k + '64'], t[k + '32']
        if k == 'dx':                                            # d plane mean = the sum of d x over the plane
            want, ref32 = want.sum((-1, -2)), ref32.double().sum((-1, -2))
        err, e32 = H.rel(v, want), H.rel(ref32, want)
        print('fixture', name, k, f'{err:.2e} (reference fp32 {e32:.2e})')
        assert err <= max(BAR, 2 * e32), (name, k, err, e32)
    if 'top1_acc64' in t:
        assert float(out['top1_acc']) == float(t['top1_acc64']) and float(out['top5_acc']) == float(t['top5_acc64'])


class _Counting:
    """``native.lib()`` with a call counter per entry point."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


def test_default_config_stays_on_head_loss_bit_for_bit(monkeypatch):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(6, 2, 64, generator=g)
    y = torch.randint(0, 10, (6,), generator=g).to(DEV)
    torch.manual_seed(0)
    head = D.build_head(dict(type='GCNHead', num_classes=10, in_channels=64)).to(DEV).train()
    head.init_weights()
    with torch.no_grad():
        head.fc_cls.weight.mul_(20)
    counting = _Counting(native.lib())
    monkeypatch.setattr(native, '_lib', counting)
    f = x.to(DEV).requires_grad_()
    out = head.forward_loss(f, y)
    out['loss_cls'].backward()
    assert counting.calls == {'dsgcn_head_loss_fwd': 1, 'dsgcn_head_loss_bwd': 1}
    monkeypatch.undo()
    f2 = x.to(DEV).requires_grad_()
    w2, b2 = head.fc_cls.weight.detach().clone().requires_grad_(), head.fc_cls.bias.detach().clone().requires_grad_()
    loss, acc, _ = K_.head_loss(f2.reshape(12, 64), w2, b2, y, 2, 1.0)
    loss.backward()
    assert torch.equal(loss, out['loss_cls']) and torch.equal(acc[0], out['top1_acc']) and torch.equal(acc[1], out['top5_acc'])
    assert torch.equal(f.grad, f2.grad) and torch.equal(head.fc_cls.weight.grad, w2.grad)
    assert torch.equal(head.fc_cls.bias.grad, b2.grad)
    # ... and the weighted head of the same weights goes through the new entry points
    counting = _Counting(native.lib())
    monkeypatch.setattr(native, '_lib', counting)
    head.loss_cls = D.build_loss(dict(type='CrossEntropyLoss', class_weight=[1.0] * 9 + [2.0])).to(DEV)
    head.forward_loss(x.to(DEV).requires_grad_(), y)['loss_cls'].backward()
    assert counting.calls == {'dsgcn_head_target_fwd': 1, 'dsgcn_head_target_bwd': 1}


# ---- through the engine -------------------------------------------------------------------------------------------------

CFG = dict(type='RecognizerGCN',
           backbone=dict(type='DGSTGCN', gcn_type='dgphgcn1', gcn_ratio=0.125, gcn_node_attention=True,
                         gcn_edge_attention=True, gcn_decompose=True, gcn_subset_wise=True, gcn_ctr='T', gcn_ada='T',
                         tcn_type='dgmstcn', base_channels=16, num_stages=4, inflate_stages=[3], down_stages=[3],
                         graph_cfg=dict(layout='nturgb+d', mode='random', num_filter=3, init_off=.04, init_std=.02),
                         tcn_ms_cfg=[(3, 1), (3, 2), (3, 3), (3, 4), ('max', 3), '1x1']),
           cls_head=dict(type='GCNHead', num_classes=12, in_channels=32))


@pytest.fixture
def watchdog():
    """A per-test time limit: a step that hangs ends the run with a traceback instead of waiting for the outer limit."""
    faulthandler.dump_traceback_later(240, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _engine_run(head_kw, soft, steps, use_graph):
    torch.manual_seed(5)
    np.random.seed(5)
    cfg = copy.deepcopy(CFG)
    cfg['cls_head'].update(copy.deepcopy(head_kw))
    m = D.build_model(cfg).cuda().train()
    eng = D.TrainEngine(m, lr=0.05, momentum=0.9, weight_decay=5e-4, nesterov=True, warmup_eager=2, use_graph=use_graph)
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(4, 1, 2, 16, 25, 3, generator=gen).cuda()
    if soft:
        y = torch.softmax(torch.randn(4, 12, generator=gen) * 2, 1).cuda()
    else:
        y = torch.randint(0, 12, (4, 1), generator=gen).cuda()
    logs = [{k: v.clone() for k, v in eng.step(x, y).items()} for _ in range(steps)]
    torch.cuda.synchronize()
    return eng, x, y, logs


@pytest.mark.parametrize('kind', ['soft', 'class_weight'])
def test_engine_eager_and_replayed_agree(kind, watchdog):
    """The reduced DS-STGCN, 4 clips: five steps eagerly, and two eager + three replayed from the two hipGraphs, on a
    soft-label (N, K) batch and on a class-weighted hard-label batch: the same losses, the same parameters."""
    soft = kind == 'soft'
    head_kw = dict() if soft else dict(loss_cls=dict(type='CrossEntropyLoss', class_weight=[0.5 + 0.25 * i for i in range(12)]))
    ea, x, y, la = _engine_run(head_kw, soft, 5, use_graph=False)
    eb, _, _, lb = _engine_run(head_kw, soft, 5, use_graph=True)
    assert eb.capture_error is None and eb.graphed(x, y) and not ea.graphed(x, y)
    assert set(la[0]) == set(lb[0]) == ({'loss_cls', 'loss'} if soft else {'top1_acc', 'top5_acc', 'loss_cls', 'loss'})
    losses = [float(l['loss']) for l in la]
    print('engine', kind, losses)
    assert all(np.isfinite(losses)) and losses == [float(l['loss']) for l in lb] and len(set(losses)) == 5
    assert torch.equal(ea.flat.flat_p, eb.flat.flat_p) and torch.equal(ea.opt.buf, eb.opt.buf)
