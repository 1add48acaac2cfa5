"""-m gpu: TrainEngine — what bench.py times and train_model drives — at FULL width against the reference's fp64 fixtures,
with the flat parameter buffer starting 0..3 floats late.

FlatParams lays the parameters out back to back, so every weight, bias, gamma and adjacency the product trains with sits
at a 4-byte-aligned address and nothing more, and which of the four classes (address mod 16) a tensor lands in depends on
the sizes of all tensors before it.  The pad parameter of ``layout_cases.with_pad`` rotates the classes: k = 0 is the
shipped layout, k = 1, 2, 3 move every tensor through the other three.  Every step runs at rate 0 (sgd_update ends in
fmaf(-rate, st, pv): the parameters stay put), so every step of a case must reproduce the same gradient.

Observed on the MI355X (profiles/layout/README.md has the table): all 24 shifted cases are bit-identical to k = 0."""
import functools
import json

import numpy as np
import pytest
import torch

import dsgcn_amd as D
from dsgcn_amd.evaluation import top_k_accuracy
from layout_cases import with_pad
from test_model_gpu import GRAD_CLIPS, R2_CONFIGS, _load_running, _r2_model
from test_oracle_golden import load, rel

pytestmark = pytest.mark.gpu

# whole-selection error against fp64 over the reference's own fp32 error (`theirs` of
# test_full_width_gradients_vs_reference_fixture, not redefined): < 2.0, the existing bar — the unflattened ratios recorded
# in tests/golden/grad_ratio_marks.json are <= 1.33 for these seven.  The shipped CTR-GCN: five +-1-ulp draws of this model
# lie between 1.75 and 3.09 of 2.19e-3 (profiles/r05/gram_check.txt) = 1.38 .. 2.44 of today's yardstick 2.77e-3; 2.44 plus
# the 15 % tripwire margin = 2.8.  The engine's summation order (deferred sums, fused ends) is another such draw.
RATIO_BAR = {name: 2.0 for name in R2_CONFIGS}
RATIO_BAR['ctrgcn_shipped_ntu60'] = 2.8
ENGINE = dict(momentum=0.9, weight_decay=5e-4, nesterov=True, use_graph=True, warmup_eager=1)


def _buffers(m):
    return [b.detach().clone() for b in m.buffers()]


def _restore(m, saved):
    with torch.no_grad():
        for b, s in zip(m.buffers(), saved):
            b.copy_(s)                                   # in place: a captured graph holds the buffers' addresses


def _running_err(m, z):
    sd = m.state_dict()
    return max(rel(sd[k].cpu(), z[f'running_{i}']) for i, k in enumerate(json.loads(str(z['running_names']))))


def _ratio(grad_of, z):
    """ours / theirs exactly as test_full_width_gradients_vs_reference_fixture computes it; grad_of: name -> tensor."""
    num = den = 0.0
    for i, k in enumerate(json.loads(str(z['names']))):
        g64 = z[f'g64_{i}'].astype(np.float64)
        num += float(((grad_of(k).double().cpu().numpy() - g64) ** 2).sum())
        den += float((g64 ** 2).sum())
    ours, theirs = (num / den) ** .5, max(float(z['gerr32_set']), float(z['gnoise32_set']) / 2 ** .5)
    return ours / theirs, ours, theirs


@functools.lru_cache(maxsize=None)
def _input(name):
    from closed_form import counter_input
    mk, T, V = R2_CONFIGS[name]
    classes = mk()['cls_head']['num_classes']
    x, y = counter_input(GRAD_CLIPS, T, V, classes)
    return x.cuda(), y.cuda()


@functools.lru_cache(maxsize=None)
def engine_case(name, k):
    """The engine sequence of one (config, pad): logits, one eager step, the capture step, one replay.  -> the figures and
    the gradient per parameter name (host copies; computed once, read by every test that needs them, never modified)."""
    m, cfg, T, V = _r2_model(name)
    m = with_pad(m, k).cuda().train()
    eng = D.TrainEngine(m, **ENGINE)
    flat = eng.flat
    assert (not k or flat.slices[0] == (0, k)) and flat.flat_p.data_ptr() % 16 == 0
    x, y = _input(name)
    z = load(f'full_grads_{name}.npz')
    out = dict(name=name, k=k)
    initial = _buffers(m)
    p0 = flat.flat_p.clone()
    with torch.no_grad():
        logits = m.cls_head(m.extract_feat(x[:, 0]))
    _restore(m, initial)
    out['logits_err'] = rel(logits.cpu(), z['logits64'])
    # ---- one eager step
    logs = eng.step(x, y, lr=0.0)
    assert not eng.graphed(x, y)
    loss = logs['loss'].clone()
    out['loss_err'] = abs(loss.item() - float(z['loss64'])) / abs(float(z['loss64']))
    out['acc'] = (float(logs['top1_acc']), float(logs['top5_acc']))
    out['acc64'] = tuple(top_k_accuracy(z['logits64'], y.cpu().numpy(), (1, 5)))
    out['running_err_eager'] = _running_err(m, z)
    g_eager = flat.flat_g.clone()
    # ---- the capture step (captures, then replays once) and one more replay, each from the initial buffers
    out['graph_equal'], out['running_err_graph'] = [], []
    for _ in range(2):
        _restore(m, initial)
        logs = eng.step(x, y, lr=0.0)
        out['graph_equal'].append(bool(torch.equal(flat.flat_g, g_eager)) and bool(torch.equal(logs['loss'], loss)))
        out['running_err_graph'].append(_running_err(m, z))
    out['graphed'], out['capture_error'] = bool(eng.graphed(x, y)), eng.capture_error
    out['params_unchanged'] = bool(torch.equal(flat.flat_p, p0))
    g = g_eager.cpu()
    out['flat_g'] = g[k:]
    out['pad_grad_zero'] = not bool(g[:k].any())
    out['grads'] = {n: g[off:off + cnt].view(p.shape) for (n, p), (off, cnt) in zip(m.named_parameters(), flat.slices)
                    if n != '_align_pad'}
    out['ratio'], out['ours'], out['theirs'] = _ratio(out['grads'].__getitem__, z)
    print(f'layout {name} k={k}: ratio {out["ratio"]:.3f} (ours {out["ours"]:.3e}, reference fp32 {out["theirs"]:.3e})  logits '
          f'{out["logits_err"]:.2e}  loss {out["loss_err"]:.2e}  running {out["running_err_eager"]:.2e}')
    del eng, m
    return out


@functools.lru_cache(maxsize=None)
def unflattened_case(name):
    """The path of test_full_width_gradients_vs_reference_fixture: freshly allocated parameters, cls_head + cross_entropy,
    immediate parameter sums, no packing.  -> gradient per parameter name (None where none arrived), on the host."""
    m, cfg, T, V = _r2_model(name)
    m = m.cuda().train()
    x, y = _input(name)
    logits = m.cls_head(m.extract_feat(x[:, 0]))
    torch.nn.functional.cross_entropy(logits, y.squeeze(-1)).backward()
    return {n: (None if p.grad is None else p.grad.detach().cpu()) for n, p in m.named_parameters()}


def _distance(a, b):
    """-> (whole-buffer relative L2, largest per-tensor relative L2, its name) of gradient dict a against b"""
    num = den = 0.0
    worst = (0.0, None)
    for n, gb in b.items():
        e2, d2 = float((a[n].double() - gb.double()).pow(2).sum()), float(gb.double().pow(2).sum())
        num, den = num + e2, den + d2
        r = (e2 / d2) ** .5 if d2 > 0 else (0.0 if e2 == 0 else float('inf'))
        if r > worst[0]:
            worst = (r, n)
    return (num / den) ** .5, worst[0], worst[1]


def _check_engine_vs_fixture(c):
    name = c['name']
    assert c['logits_err'] < 1e-4 and c['loss_err'] < 1e-4, (c['logits_err'], c['loss_err'])        # north_star bars
    assert c['acc'] == c['acc64'], (c['acc'], c['acc64'])
    assert c['running_err_eager'] < 1e-4, c['running_err_eager']
    assert c['ratio'] < RATIO_BAR[name], (c['ratio'], c['ours'], c['theirs'])
    assert c['capture_error'] is None and c['graphed'], c['capture_error']
    assert c['graph_equal'] == [True, True]                  # capture step and replay: the eager step's bits
    assert max(c['running_err_graph']) < 1e-4, c['running_err_graph']
    assert c['params_unchanged'] and c['pad_grad_zero']


@pytest.mark.parametrize('name', list(R2_CONFIGS))
def test_engine_vs_reference_fixture(name):
    """The shipped layout (k = 0): logits, loss, accuracies, running statistics and the selected gradients of one engine step
    against the reference's fp64 run; the captured step and its replay bit-equal to the eager one; the whole flat gradient
    against the unflattened path's (another summation order of the same step: < 2e-2, test_full_size_properties' bar — a
    dropped deferred sum or a wrong slice is O(1)) with the same tensors dead on both sides."""
    c = engine_case(name, 0)
    _check_engine_vs_fixture(c)
    u = unflattened_case(name)
    assert set(u) == set(c['grads'])
    dead_u = {n for n, g in u.items() if g is None or not g.any()}
    dead_e = {n for n, g in c['grads'].items() if not g.any()}
    assert dead_u == dead_e, sorted(dead_u ^ dead_e)
    whole, worst, which = _distance(c['grads'], {n: (torch.zeros_like(c['grads'][n]) if g is None else g) for n, g in u.items()})
    print(f'layout {name}: engine vs unflattened whole {whole:.3e}, worst tensor {worst:.3e} ({which}); {len(dead_e)} dead')
    assert whole < 2e-2, whole


@pytest.mark.parametrize('k', [1, 2, 3])
@pytest.mark.parametrize('name', list(R2_CONFIGS))
def test_engine_at_shifted_layout(name, k):
    """Every parameter k floats later: the forward bars, the graph bit-equality and the ratio bar against fp64 hold as at
    k = 0, and the whole flat gradient is BIT-IDENTICAL to the k = 0 engine's — what the MI355X showed for all 24 cases
    (profiles/layout/README.md): no kernel of the training step chooses its arithmetic by a parameter's address (the ones
    that do — head_target, head_test, feat_ext, head_ensemble on the weight, colsum on its input — are not on this path or
    see allocator-aligned operands; tests/test_alignment_gpu.py holds them to their fp64 bars at every class).  The
    distances are printed first: a weight read one float off is O(1) in both."""
    c, c0 = engine_case(name, k), engine_case(name, 0)
    _check_engine_vs_fixture(c)
    whole, worst, which = _distance(c['grads'], c0['grads'])
    same = bool(torch.equal(c['flat_g'], c0['flat_g']))
    print(f'layout {name} k={k}: vs k=0 whole {whole:.3e}, worst tensor {worst:.3e} ({which}), bit-identical {same}')
    assert same, (whole, worst, which)


def test_weight_image_cache_keeps_no_autograd_history():
    """A wide conv whose weight is COMPUTED from parameters (msmlp's block-diagonal channel mix: the shipped CTR-GCN): the
    per-step cache of bf16 weight images must not keep that tensor's graph alive.  It did — the view of the weight made
    inside the conv's forward kept its base — so the parameters' AccumulateGrad nodes of one step, and the stream they were
    made on, lived into the next, and the capture of the shipped CTR-GCN's step died in hipStreamEndCapture.  No capture
    here: a hook on the first step's accumulator must not fire in the second step, and no cached weight has a base with
    history."""
    from dsgcn_amd import kernels as K, native
    n, Ci, Co, T, V = 2, 64, 128, 8, 16                                  # the smallest shape on the three-term GEMM form
    assert native.lib().dsgcn_pwconv_wsplit_bytes(n, Ci, Co, T, V, 1) > 0
    g = torch.Generator().manual_seed(0)
    p = torch.nn.Parameter((torch.randn(Co // 2, Ci // 2, generator=g) * 0.1).cuda())
    x = torch.randn(n, Ci, T, V, generator=g).cuda()
    fired = []

    def step(mark):
        K.reset_leaf_uses()
        try:
            w = torch.block_diag(p, p)
            if mark:
                p.view_as(p).grad_fn.next_functions[0][0].register_hook(lambda *a: fired.append(1))
            K.pwconv(x, None, None, None, False, w, None, 1, False)[0].sum().backward()
        finally:
            K.end_step()

    step(True)
    assert len(fired) == 1 and p.grad is not None
    p.grad = None
    step(False)
    assert len(fired) == 1, 'the first step\'s AccumulateGrad node was still alive in the second step'
    held = [j['w'] for j in K._wsplit_state['jobs'].values()]
    assert held and all(w.grad_fn is None and (w._base is None or w._base.grad_fn is None) for w in held)


@pytest.mark.parametrize('k', [0, 1, 2, 3])
@pytest.mark.parametrize('name', list(R2_CONFIGS))
def test_eval_mode_on_flat_parameters(name, k):
    """test_eval_mode_vs_reference_fixture's body on a model whose parameters live in the flat buffer, k floats late:
    the same bars (probabilities 1e-5, per-clip scores 1e-4 against the reference's fp64 run)."""
    from closed_form import EVAL_LIVEN, eval_clips
    m, cfg, T, V = _r2_model(name, EVAL_LIVEN.get(name, 0.5))
    z = load(f'eval_{name}.npz')
    _load_running(m, z)
    x = eval_clips(name, T, V).cuda()
    m = with_pad(m, k).cuda().eval()
    flat = D.FlatParams(m)
    assert flat.slices[0][0] == 0 and flat.slices[1 if k else 0][0] == k
    probs = m(keypoint=x, return_loss=False)
    assert isinstance(probs, np.ndarray) and probs.shape == z['probs64'].shape
    assert rel(probs, z['probs64']) < 1e-5, rel(probs, z['probs64'])
    with torch.no_grad():
        scores = m.cls_head(m.extract_feat(x.flatten(0, 1))).reshape(2, 10, -1)
    assert rel(scores.cpu(), z['scores64_clips']) < 1e-4, rel(scores.cpu(), z['scores64_clips'])
