"""Golden fixture for feature / score-map extraction at test time, generated from the IMPORTED reference (build container
only: needs the reference checkout, see ref_shim):

    python tests/golden/gen_golden_featext.py [--out DIR]

  featext.npz   the reference's own ``RecognizerGCN.forward_test`` (pyskl/models/recognizers/recognizergcn.py:53-93) under
                ``test_cfg = dict(feat_ext=True | score_ext=True, pool_opt=...)``, with explicit letter strings only (its
                default 'all' trips its own assertion).  Two groups (tests/feat_ext_cases.py names the entries):
                kernel cases   the recognizer over a stub backbone that returns the stored activation x and a head that
                               holds the stored fc_cls, one call per video (it asserts bs == 1);
                model cases    the reduced DS-STGCN / ST-GCN of model_reduced(.npz, _cfg.json) / model_reduced_stgcn in
                               eval mode on one seeded video of 3 clips x 2 persons (T = 16, V = 25).
                Every run once in fp32 — the float16 array it returns and the fp32 tensor before that cast — and once with
                everything ``.double()``, kept as its difference to the fp32 run in 16-bit steps (the arrays of the model
                cases at 'none' have 38400 elements: whole float64 copies would make an archive of several MB).

Data only.  The archive is written with fixed member times, so a second run gives a byte-identical file."""
import copy
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (ref_shim, extract_feat_f64)
from gen_golden_dghgcn import savez_det  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import feat_ext_cases as F  # noqa: E402  (the case table the tests read the archive by)

R = G.R
Recognizer = R.rec.RecognizerGCN


class Returns(nn.Module):
    """A backbone that returns a given activation whatever it is called with."""

    def __init__(self, x):
        super().__init__()
        self.x = x

    def forward(self, keypoint):
        return self.x


class Head(nn.Module):
    def __init__(self, w, b):
        super().__init__()
        K, C = w.shape
        self.fc_cls = nn.Linear(C, K, bias=b is not None).to(w.dtype)
        with torch.no_grad():
            self.fc_cls.weight.copy_(w)
            if b is not None:
                self.fc_cls.bias.copy_(b)


def before_cast(rec, keypoint):
    """forward_test's return value AND the tensor it casts: the cast is its last step (``.astype(np.float16)`` on
    ``x.data.cpu().numpy()``), so numpy's cast is watched for the array it is given."""
    seen = []
    real = np.ndarray.astype

    class Spy(np.ndarray):
        def astype(self, dtype, *a, **k):
            seen.append(np.array(self, copy=True).view(np.ndarray))
            return real(self.view(np.ndarray), dtype, *a, **k)

    to_numpy = torch.Tensor.numpy
    torch.Tensor.numpy = lambda t, *a, **k: to_numpy(t, *a, **k).view(Spy)
    try:
        with torch.no_grad():
            out = rec.forward_test(keypoint)
    finally:
        torch.Tensor.numpy = to_numpy
    assert len(seen) == 1 and out.dtype == np.float16
    return np.asarray(out), seen[0]


def stub_recognizer(x, w, b):
    """The reference's RecognizerGCN around a stub backbone / head (its constructor builds real ones from configs)."""
    rec = Recognizer.__new__(Recognizer)
    nn.Module.__init__(rec)
    rec.backbone = Returns(x)
    rec.cls_head = Head(w, b) if w is not None else None
    rec.feat_ext = True
    rec.train_cfg, rec.test_cfg = {}, {}
    return rec.eval()


def run_stub(x, w, b, mode, pool):
    """x (videos, clips, M, C, T, V) -> (r16, r32) of the reference, videos stacked on axis 0"""
    r16, r32 = [], []
    for xv in x:
        rec = stub_recognizer(xv, w, b)
        rec.test_cfg = {('score_ext' if mode == 'score' else 'feat_ext'): True, 'pool_opt': pool}
        keypoint = torch.zeros((1, xv.shape[0], xv.shape[1], 1, 1, 1), dtype=xv.dtype)
        a16, a32 = before_cast(rec, keypoint)
        if mode == 'feat':
            a16, a32 = a16[None], a32[None]
        r16.append(a16)
        r32.append(a32)
    return np.concatenate(r16), np.concatenate(r32)


def put(out, k, r16, r32, r64):
    assert r32.dtype == np.float32 and r64.dtype == np.float64 and r16.shape == r32.shape == r64.shape
    assert np.array_equal(r16.view(np.uint16), r32.astype(np.float16).view(np.uint16))
    out[k + '_r32'] = r32
    if r16.size <= F.R16_MAX:                   # (above: the reader takes r32.astype(float16), asserted equal just now)
        out[k + '_r16'] = r16
    d = r64 - r32.astype(np.float64)
    step = float(np.abs(d).max()) / 32767
    out[k + '_d64'] = np.round(d / step).astype(np.int16) if step else np.zeros(d.shape, np.int16)
    out['d64_steps'][k] = step.hex()


def case_inputs(i, name, c):
    g = torch.Generator().manual_seed(5200 + i)
    shape = (c['videos'], c['clips'], c['M'], c['C'], c['T'], c['V'])
    if name == 'inf':
        x = torch.tensor([[70000., -70000., 65520., 65519.], [-65520., 65504., 1e30, 1e30]]).reshape(shape)
        return x, None, None
    n = torch.randint(-2048, 2049, shape, generator=g, dtype=torch.int16)
    if name == 'exact':
        # channel 0: the mean over all 128 elements is 3 * 2^-17, a float16 subnormal; channels 1 / 2: 1 + 2^-11 and
        # 1 + 3 * 2^-11, exact ties between two float16 neighbours (round to even: down to 1, up to 1 + 2^-9)
        n[:, :, :, 0] = 0
        n[0, 0, 0, 0, 0, :3] = 1
        n[:, :, :, 1:3] = 1024
        n[0, 1, 0, 1, 2, 3] = 1024 + 64
        n[0, 0, 1, 2, 1, 5] = 1024 + 192
    w = b = None
    if c['K']:
        w = torch.randn(c['K'], c['C'], generator=g) * 0.2
        b = torch.randn(c['K'], generator=g) * 0.1 if c['bias'] else None
    return n, w, b


def kernel_cases(out):
    for i, (name, c) in enumerate(F.CASES.items()):
        n, w, b = case_inputs(i, name, c)
        out[name + '_x'] = n.numpy()
        x = n.float() / 1024 if n.dtype == torch.int16 else n
        if w is not None:
            out[name + '_w'] = w.numpy()
        if b is not None:
            out[name + '_b'] = b.numpy()
        for mode, pool in F.runs(name):
            r16, r32 = run_stub(x, w, b, mode, pool)
            _, r64 = run_stub(x.double(), None if w is None else w.double(), None if b is None else b.double(), mode, pool)
            put(out, F.key(name, mode, pool), r16, r32, r64)
        if name == 'exact':
            pooled = out[F.key(name, 'feat', 'nmtv') + '_r32'].reshape(-1)
            assert 0 < pooled[0] < 2.0 ** -14 and pooled[0] == 3 * 2.0 ** -17             # a float16 subnormal
            assert pooled[1] == 1 + 2.0 ** -11 and pooled[2] == 1 + 3 * 2.0 ** -11        # round-to-even ties
            assert np.float16(pooled[1]) == 1 and np.float16(pooled[2]) == 1 + 2.0 ** -9
            for mode, pool in F.runs(name):                                                # every mean exact in fp32
                assert not out[F.key(name, mode, pool) + '_d64'].any(), pool
        if name == 'inf':
            assert np.isinf(out[F.key(name, 'feat', 'none') + '_r16']).sum() == 6


def model_cases(out):
    g = torch.Generator().manual_seed(77)
    x = torch.randn(1, F.MODEL_CLIPS, F.MODEL_M, 16, 25, 3, generator=g)
    out['model_x'] = x.numpy()
    for name in F.MODELS:
        with open(os.path.join(HERE, name + '_cfg.json')) as f:
            cfg = json.load(f)
        if 'tcn_ms_cfg' in cfg['backbone']:
            cfg['backbone']['tcn_ms_cfg'] = [tuple(c) if isinstance(c, list) else c for c in cfg['backbone']['tcn_ms_cfg']]
        with np.load(os.path.join(HERE, name + '.npz')) as z:
            sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd_')}
        m = R.builder.build_model(copy.deepcopy(cfg))
        m.load_state_dict(sd)
        m.eval()
        m64 = R.builder.build_model(copy.deepcopy(cfg)).double()
        m64.load_state_dict({k: v.double() if v.dtype.is_floating_point else v for k, v in sd.items()})
        m64.eval()
        with torch.no_grad():
            # (the reference's STGCN casts its input to fp32: the fp64 activation comes from G.extract_feat_f64 and the
            # recognizer's own branch then runs on it)
            feat64 = G.extract_feat_f64(m64, x.double().flatten(0, 1))
        m64.backbone = Returns(feat64)
        for mode, pool in F.MODEL_RUNS:
            cfg_t = {('score_ext' if mode == 'score' else 'feat_ext'): True, 'pool_opt': pool}
            m.test_cfg, m64.test_cfg = dict(cfg_t), dict(cfg_t)
            r16, r32 = before_cast(m, x)
            _, r64 = before_cast(m64, x.double())
            put(out, F.key(name, mode, pool), r16, r32, r64)


def main(out_dir=HERE):
    out = {'cases': np.array(list(F.CASES)), 'models': np.array(list(F.MODELS)), 'd64_steps': {}}
    kernel_cases(out)
    model_cases(out)
    out['d64_steps'] = np.array(json.dumps(out['d64_steps'], sort_keys=True))
    path = os.path.join(out_dir, 'featext.npz')
    savez_det(path, **out)
    print(f'wrote featext.npz: {len(out)} entries, {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main(sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else HERE)
