"""Golden fixture for the head's loss options, generated from the IMPORTED reference (build container only: needs the
reference checkout, see ref_shim):

    python tests/golden/gen_golden_headloss.py [--out DIR]

  headloss.npz      the reference's own ``GCNHead`` (pyskl/models/heads/simple_head.py, heads/base.py:50-84) with each loss
                    config of CASES below (losses/cross_entropy_loss.py:11-123): ``head.loss(head(x), label)`` + backward
                    on seeded inputs, once in fp32 and once with everything ``.double()``.  Per case: the head's config
                    (json), x (N, M, C, T, V), label, fc_cls.weight / fc_cls.bias, and for both precisions the loss,
                    top1_acc / top5_acc where the reference reports them, and the gradients of x, fc_cls.weight and
                    fc_cls.bias.  x holds multiples of 2^-10: its (T, V) plane mean is exact in fp32, so a test may feed
                    the (N, M, C) plane means instead.

Data only.  The archive is written with fixed member times, so a second run gives a byte-identical file."""
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (ref_shim)
from gen_golden_dghgcn import savez_det  # noqa: E402

R = G.R

CW11 = [1.0, 0.5, 2.0, 0.0, 1.5, 1.0, 0.25, 3.0, 1.0, 0.75, 1.25]      # one class at weight 0
CW7 = [0.5, 2.0, 1.0, 1.5, 0.25, 1.0, 3.0]

# (name, N, M, C, K, label kind, head kwargs)
CASES = [
    ('ce_weight', 7, 2, 96, 11, 'hard', dict(loss_cls=dict(type='CrossEntropyLoss', class_weight=CW11))),
    ('ce_soft', 5, 1, 70, 11, 'soft', dict(loss_cls=dict(type='CrossEntropyLoss', loss_weight=0.5))),
    ('ce_wsoft', 5, 1, 70, 11, 'soft', dict(loss_cls=dict(type='CrossEntropyLoss', class_weight=CW11))),
    ('bce_plain', 6, 2, 64, 7, 'multi', dict(loss_cls=dict(type='BCELossWithLogits'), multi_class=True)),
    ('bce_smooth_weight', 6, 2, 64, 7, 'multi',
     dict(loss_cls=dict(type='BCELossWithLogits', loss_weight=2.0, class_weight=CW7), multi_class=True,
          label_smooth_eps=0.1)),
    ('bce_single_clip', 1, 2, 64, 7, 'multi1',
     dict(loss_cls=dict(type='BCELossWithLogits', class_weight=CW7), multi_class=True, label_smooth_eps=0.1)),
]
T, V = 2, 2


def inputs(i, N, M, C, K, kind):
    g = torch.Generator().manual_seed(4100 + i)
    x = torch.randint(-2048, 2049, (N, M, C, T, V), generator=g).float() / 1024
    w = torch.randn(K, C, generator=g) * 0.2
    b = torch.randn(K, generator=g) * 0.1
    if kind == 'hard':
        label = torch.randint(0, K, (N,), generator=g)
        label[0] = 3                                            # the class at weight 0 is present
    elif kind == 'soft':
        label = torch.softmax(torch.randn(N, K, generator=g) * 2, dim=1)
    else:
        label = (torch.rand(N, K, generator=g) < 0.3).float()
        label[:, 0] = 1.0
        if kind == 'multi1':
            label = label[0]                                    # (K,): heads/base.py:62-64 unsqueezes it
    return x, w, b, label


def run(cfg, x, w, b, label, dtype):
    head = R.builder.build_head(copy.deepcopy(cfg))
    with torch.no_grad():
        head.fc_cls.weight.copy_(w)
        head.fc_cls.bias.copy_(b)
    head = head.to(dtype).train()
    if head.loss_cls.class_weight is not None:                  # (a plain attribute there: .to() does not reach it)
        head.loss_cls.class_weight = head.loss_cls.class_weight.to(dtype)
    xx = x.detach().to(dtype).clone().requires_grad_()
    lab = label.to(dtype) if label.is_floating_point() else label
    out = head.loss(head(xx), lab)
    out['loss_cls'].backward()
    res = dict(loss=out['loss_cls'].detach().numpy(), dx=xx.grad.numpy(), dw=head.fc_cls.weight.grad.numpy(),
               db=head.fc_cls.bias.grad.numpy())
    for k in ('top1_acc', 'top5_acc'):
        if k in out:
            res[k] = np.asarray(out[k].detach().numpy(), dtype=np.float64)
    return res, sorted(head.state_dict())


def main(out_dir=HERE):
    out = {'cases': np.array([c[0] for c in CASES])}
    for i, (name, N, M, C, K, kind, kw) in enumerate(CASES):
        cfg = dict(type='GCNHead', num_classes=K, in_channels=C, **kw)
        x, w, b, label = inputs(i, N, M, C, K, kind)
        tag = name + '_'
        out[tag + 'cfg'] = np.array(json.dumps(cfg, sort_keys=True))
        out[tag + 'x'] = x.numpy()
        out[tag + 'label'] = label.numpy()
        out[tag + 'fc_cls.weight'] = w.numpy()
        out[tag + 'fc_cls.bias'] = b.numpy()
        for dtype, sfx in ((torch.float32, '32'), (torch.float64, '64')):
            res, keys = run(cfg, x, w, b, label, dtype)
            for k, v in res.items():
                out[tag + k + sfx] = v
        out[tag + 'sd_keys'] = np.array(json.dumps(keys))
    savez_det(os.path.join(out_dir, 'headloss.npz'), **out)
    print('wrote headloss.npz:', ', '.join(c[0] for c in CASES))


if __name__ == '__main__':
    main(sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else HERE)
