"""The window stage of ``dgmsmlp`` (``kernels.dgmlp_windows``: everything between branch_act and combine) with the
mlp-window kernel (csrc/mlpwin.hip) next to the staged launches it replaces (DSGCN_MLPWIN=0: dwcausal, the block-diagonal
1x1 conv, the add), at the three widths of DGSTGCN at the bench batch:

    n = 128 person-samples, V = 25 (26 columns), (C, T) = (64, 64), (128, 32), (256, 16), stride 1

for the class defaults (no dilated conv beside the taps) and for add_tcn + merge_after.  Forward alone (no_grad) and
forward + backward; the two sides alternate in one process; every call of a block takes the next of `--sets` operand sets
(h and the incoming gradient; 6 sets of 54.5 MB each way are more than the 256 MB Infinity Cache, so the operands come
from HBM); median of `--blocks` blocks with the spread (min .. max).  "bwd" is the difference of the two medians.

    python tools/mlpwin_bench.py [--blocks 7] [--sets 6] [--out FILE.json]
Prints one JSON document (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import dsgcn_amd  # noqa: F401
from dsgcn_amd import kernels as K

N, V1 = 128, 26
CFG = [(3, 1), (3, 2), (3, 3), (3, 4), ('max', 3), '1x1']
SHAPES = [(64, 64), (128, 32), (256, 16)]


def operands(C, T, add_tcn, sets):
    g = torch.Generator(device='cuda').manual_seed(C + T)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g, device='cuda') * scale)        # noqa: E731
    mid = C // len(CFG)
    widths = [C - mid * (len(CFG) - 1)] + [mid] * (len(CFG) - 1)
    mlp = [c != '1x1' and c[0] != 'max' for c in CFG]
    p = dict(cw=[], cb=[], w1=[], b1=[])
    rows_w, rows_b, dil = [], [], []
    for w, c, m in zip(widths, CFG, mlp):
        rows_w.append(rnd(w, 2, scale=0.5) if m else torch.zeros(w, 2, device='cuda'))
        rows_b.append(rnd(w, scale=0.1) if m else torch.zeros(w, device='cuda'))
        dil += [c[1] if m else 0] * w
        if m:
            p['w1'].append(rnd(w, w, scale=w ** -0.5).requires_grad_())
            p['b1'].append(rnd(w, scale=0.1).requires_grad_())
            if add_tcn:
                p['cw'].append(rnd(w, w, 3, 1, scale=(3 * w) ** -0.5).requires_grad_())
                p['cb'].append(rnd(w, scale=0.1).requires_grad_())
    p['dw_w'], p['dw_b'] = torch.cat(rows_w).requires_grad_(), torch.cat(rows_b).requires_grad_()
    p['dil'] = torch.tensor(dil, dtype=torch.int32, device='cuda')
    hs = [torch.relu(rnd(N, C, T, V1)).requires_grad_() for _ in range(sets)]
    dus = [rnd(N, C, T, V1) for _ in range(sets)]
    return widths, p, hs, dus


def side(kernel, widths, p, merge_after):
    def run(h):
        K.MLPWIN = kernel
        return K.dgmlp_windows(h, CFG, widths, p['cw'] or None, p['cb'] or None, p['dw_w'], p['dw_b'], p['dil'], p['w1'],
                               p['b1'], merge_after, 1)
    return run


def time_block(fn, hs, dus, backward):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for h, du in zip(hs, dus):
        if backward:
            h.grad = None
            fn(h).backward(du)
        else:
            with torch.no_grad():
                fn(h)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / len(hs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--sets', type=int, default=6)
    ap.add_argument('--out')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU'
    was = K.MLPWIN
    rows = []
    for add_tcn, merge_after in ((False, False), (True, True)):
        for C, T in SHAPES:
            widths, p, hs, dus = operands(C, T, add_tcn, args.sets)
            sides = {'kernel': side(True, widths, p, merge_after), 'staged': side(False, widths, p, merge_after)}
            out = {k: fn(hs[0]).detach() for k, fn in sides.items()}
            row = dict(C=C, T=T, add_tcn=add_tcn, merge_after=merge_after,
                       max_abs_diff=float((out['kernel'] - out['staged']).abs().max()))
            for backward in (False, True):
                for fn in sides.values():                       # warm-up of both sides at this shape
                    time_block(fn, hs, dus, backward)
                ms = {k: [] for k in sides}
                for _ in range(args.blocks):
                    for k, fn in sides.items():
                        ms[k].append(time_block(fn, hs, dus, backward))
                for k, v in ms.items():
                    row[f"{k}_{'fwd_bwd' if backward else 'fwd'}_ms"] = dict(median=statistics.median(v), min=min(v), max=max(v))
            for k in sides:
                row[f'{k}_bwd_ms'] = row[f'{k}_fwd_bwd_ms']['median'] - row[f'{k}_fwd_ms']['median']
            rows.append(row)
            del hs, dus
            torch.cuda.empty_cache()
    K.MLPWIN = was
    doc = dict(n=N, V1=V1, sets=args.sets, blocks=args.blocks, rows=rows)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
