"""``RecognizerGCN`` behind the reference's registry name, constructor and call conventions
(pyskl/models/recognizers/recognizergcn.py:16-148 over recognizers/base.py:21-205):

* ``model(keypoint=(N,1,M,T,V,C), label=(N,1), return_loss=True)`` -> ``dict(top1_acc, top5_acc, loss_cls)``;
* ``model(keypoint=(N,clips,M,T,V,C), return_loss=False)`` -> ``np.ndarray (N, classes)``: clip scores averaged as
  probabilities (``test_cfg['average_clips']`` = 'prob' default, 'score', or None for per-clip scores);
* ``model(keypoint=(1,clips,M,T,V,C), return_loss=False)`` under ``test_cfg['feat_ext']`` / ``['score_ext']``
  (recognizergcn.py:65-93) -> ``np.float16``: the last block's activation ``(n', m', C, t', v')``, averaged over the axes
  named in ``test_cfg['pool_opt']`` (letters of n m t v, 'all', 'none'), or with ``score_ext`` ``cls_head.fc_cls`` at every
  remaining position, ``(1, n', m', classes, t', v')`` — one launch, ``kernels.feat_ext``;
* ``model(keypoint=(1,clips,M,T,V,C), return_loss=False)`` under ``test_cfg['graph_ext']`` (True | 'ctr' | 'ahat'; the
  reference's hook tooling, core/hooks/feature_hook.py:13-142) -> ``np.float32 (L, K, V, V)``: the learned adjacency of
  every dynamic-adjacency layer, averaged over the video's clips, persons and channels — ``kernels.graph_collect``;
* ``model.train_step(data_batch, optimizer)`` -> ``dict(loss, losses, log_vars, num_samples)`` (what mmcv's runner
  calls, core/local_runner/epoch_based_sparse_runner.py:33-34).

Host-side differences that matter at MI355X step times (a step is ~15 ms; the reference spends four collectives and
four ``.item()`` syncs per step on its log scalars, base.py:150-156):

* ``train_step(..., sync_log_vars=True)`` (default, reference semantics): ONE packed all-reduce of all log scalars and
  ONE device->host read;
* ``train_step(..., sync_log_vars=False)``: no collective and no host read at all — ``log_vars`` are rank-local device
  tensors, safe inside a hipGraph capture; ``reduce_log_vars`` averages them over ranks whenever the caller logs.

Necks and multi-view test batching (``max_testing_views``) are not reached by the skeleton configs and raise."""
from collections import OrderedDict
from itertools import zip_longest

import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F

from . import builder, kernels
from .builder import RECOGNIZERS


def _dist_world():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def reduce_log_vars(log_vars, sync=True):
    """Average a dict of scalar device tensors over the ranks with one collective.  ``sync=True`` also reads them back
    (one device->host copy) and returns floats."""
    names = list(log_vars)
    packed = torch.stack([torch.as_tensor(log_vars[k]).detach().double() for k in names])
    world = _dist_world()
    if world > 1:
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('reduce_log_vars issues a collective: call it outside hipGraph capture '
                               '(use train_step(..., sync_log_vars=False) inside the captured step)')
        packed = packed / world
        dist.all_reduce(packed)
    vals = packed.tolist() if sync else list(packed.unbind(0))
    return OrderedDict(zip(names, vals))


@RECOGNIZERS.register_module()
class RecognizerGCN(nn.Module):

    def __init__(self, backbone, neck=None, cls_head=None, train_cfg=dict(), test_cfg=dict()):
        super().__init__()
        if neck:
            raise NotImplementedError('necks are outside the DS-GCN hot path (no skeleton config uses one)')
        self.backbone = builder.build_backbone(backbone)
        self.cls_head = builder.build_head(cls_head) if cls_head else None
        self.train_cfg = dict(train_cfg or {})
        self.test_cfg = dict(test_cfg or {})
        if self.test_cfg.get('max_testing_views'):
            raise NotImplementedError("test_cfg['max_testing_views'] is outside the hot path")
        ext = self.extraction()                # (AssertionError on a pool_opt letter outside n m t v, as the reference's)
        if ext is not None and ext[0] == 'score' and not hasattr(self.cls_head, 'fc_cls'):
            raise ValueError("test_cfg['score_ext'] projects with cls_head.fc_cls: the model has none")
        gmode = kernels.parse_graph_ext(self.test_cfg.get('graph_ext', False))       # (ValueError on any other value)
        if gmode is not None:
            if ext is not None:
                raise ValueError("test_cfg['graph_ext'] returns graphs only: it does not go with feat_ext / score_ext")
            if not self.graph_units():
                raise ValueError(f"test_cfg['graph_ext']: the backbone {type(self.backbone).__name__} has no "
                                 'dynamic-adjacency unit (dgphgcn1, dghgcn, dggcn): there is no per-sample graph to collect')
        mode = self.test_cfg.setdefault('average_clips', 'prob')
        if mode not in ('score', 'prob', None):
            raise ValueError(f'{mode} is not supported. Supported: ["score", "prob", None]')
        self.init_weights()

    with_cls_head = property(lambda self: self.cls_head is not None)

    def init_weights(self):
        self.backbone.init_weights()
        if self.cls_head is not None:
            self.cls_head.init_weights()

    def extract_feat(self, keypoint):
        return self.backbone(keypoint)

    # ---- training ------------------------------------------------------------------------------------------
    def forward_train(self, keypoint, label):
        assert self.cls_head is not None
        assert keypoint.shape[1] == 1, 'training batches carry one clip per sample'
        fused = hasattr(self.cls_head, 'forward_loss')
        # a pooling head only reads the plane means of the features: ask the backbone for those
        pool = (fused and kernels.FUSED_ENDS and getattr(self.backbone, 'supports_pool', False)
                and getattr(self.cls_head, 'mode', None) == 'GCN')
        x = keypoint[:, 0].float()
        feat = self.backbone(x, pool=True) if pool else self.extract_feat(x)
        if fused:
            return self.cls_head.forward_loss(feat, label.squeeze(-1))
        return self.cls_head.loss(self.cls_head(feat), label.squeeze(-1))

    def train_step(self, data_batch, optimizer=None, sync_log_vars=True, **_runner_kwargs):
        losses = self(**data_batch, return_loss=True)
        # (recognizers/base.py:128-143 `_parse_losses`; the mean of a scalar and the `0 +` of sum() are launches here)
        log_vars = OrderedDict((k, v if v.dim() == 0 else v.mean()) for k, v in losses.items())
        loss = None
        for k, v in log_vars.items():
            if 'loss' in k:
                loss = v if loss is None else loss + v
        log_vars['loss'] = loss
        if sync_log_vars:
            log_vars = reduce_log_vars(log_vars)
        else:
            log_vars = OrderedDict((k, v.detach()) for k, v in log_vars.items())
        return dict(loss=loss, losses=losses, log_vars=log_vars, num_samples=len(next(iter(data_batch.values()))))

    val_step = train_step

    # ---- inference -----------------------------------------------------------------------------------------
    def extraction(self):
        """``None`` when ``test_cfg`` asks for class scores, else ``(mode, pool mask)`` with mode 'score' or 'feat'
        (``score_ext`` wins when both are set) — read from ``test_cfg`` at every call, as the reference does."""
        score, feat = self.test_cfg.get('score_ext', False), self.test_cfg.get('feat_ext', False)
        if not (score or feat):
            return None
        return ('score' if score else 'feat'), kernels.parse_pool_opt(self.test_cfg.get('pool_opt', 'all'))

    def graph_units(self):
        """The backbone's dynamic-adjacency units (dgphgcn1, dghgcn, dggcn) in module order = call order."""
        from .gcn_units import dggcn, dghgcn, dgphgcn1
        return [m for m in self.backbone.modules() if isinstance(m, (dgphgcn1, dghgcn, dggcn))]

    def graph_extraction(self):
        """``None`` unless ``test_cfg['graph_ext']`` is set, else the mode: 'ctr' (True or 'ctr': ``A + alpha tanh(D)``, the
        reference hook's quantity) or 'ahat' (the whole adjacency the layer aggregates with) — read from ``test_cfg`` at
        every call, like ``extraction``.  ValueError on any other value, or together with feat_ext / score_ext."""
        mode = kernels.parse_graph_ext(self.test_cfg.get('graph_ext', False))
        if mode is not None and self.extraction() is not None:
            raise ValueError("test_cfg['graph_ext'] returns graphs only: it does not go with feat_ext / score_ext")
        return mode

    @torch.no_grad()
    def forward_graphs(self, keypoint):
        """The graph branch on the device: keypoint (N, clips, M, T, V, C) -> float32 (N, L, K, V, V): for each video and
        each of the L dynamic-adjacency layers the mean over the video's clips * M person-samples (a zero-padded second
        person counts, as in the reference) and over the layer's channels of ``A + alpha tanh(D)`` ('ctr') or of Ahat
        ('ahat').  The backbone runs once in eval mode (the model is put there for the call); its features are dropped."""
        mode = self.graph_extraction()
        units = self.graph_units()
        if mode is None or not units:
            raise ValueError("forward_graphs: test_cfg['graph_ext'] is not set, or the backbone has no dynamic-adjacency unit")
        K, V = units[0].num_subsets, units[0].A.shape[-1]
        if any(u.num_subsets != K or u.A.shape[-1] != V for u in units):
            raise ValueError('forward_graphs: the layers differ in their number of subsets or joints')
        N, clips, M = keypoint.shape[:3]
        x = keypoint.float().flatten(0, 1)
        out = torch.empty((N, len(units), K, V, V), device=x.device, dtype=torch.float32)
        was_training = self.training
        self.eval()
        try:
            with kernels.graph_collect(clips * M, mode, out) as col:
                if getattr(self.backbone, 'supports_pool', False):
                    self.backbone(x, pool=True)
                else:
                    self.extract_feat(x)
            if col.layer != len(units):
                raise RuntimeError(f'forward_graphs: {col.layer} of {len(units)} dynamic-adjacency units ran')
        finally:
            self.train(was_training)
        return out

    @torch.no_grad()
    def forward_extract(self, keypoint, want_fp32=False):
        """The extraction branch on the device: keypoint (N, clips, M, T, V, C) -> float16 (N, n', m', C | classes, t', v'),
        every video pooled by itself.  With frames and joints both pooled a backbone that can hand over plane means is asked
        for those (``backbone(x, pool=True)``): the activation is then never written."""
        mode, mask = self.extraction()
        N, clips, M = keypoint.shape[:3]
        x = keypoint.float().flatten(0, 1)
        if mask & 12 == 12 and getattr(self.backbone, 'supports_pool', False):
            feat = self.backbone(x, pool=True)
        else:
            feat = self.extract_feat(x)
        if isinstance(feat, (tuple, list)):
            feat = torch.cat(feat, dim=2)
        fc = self.cls_head.fc_cls if mode == 'score' else None
        return kernels.feat_ext(feat, N, clips, M, mask, None if fc is None else fc.weight, None if fc is None else fc.bias,
                                want_fp32=want_fp32)

    @torch.no_grad()
    def forward_test(self, keypoint):
        assert self.cls_head is not None or self.test_cfg.get('feat_ext', False) or self.test_cfg.get('graph_ext', False)
        N, clips = keypoint.shape[:2]
        if self.graph_extraction() is not None:
            assert N == 1, 'graph extraction takes one video per call (InferEngine batches videos)'
            return self.forward_graphs(keypoint)[0].cpu().numpy()               # (L, K, V, V)
        ext = self.extraction()
        if ext is not None:
            assert N == 1, 'feature / score extraction takes one video per call (InferEngine batches videos)'
            out = self.forward_extract(keypoint).cpu().numpy()
            return out if ext[0] == 'score' else out[0]          # (1, n', m', K, t', v') / (n', m', C, t', v')
        feats = self.extract_feat(keypoint.float().flatten(0, 1))
        scores = self.cls_head(feats).view(N, clips, -1)
        mode = self.test_cfg['average_clips']
        if mode == 'prob':
            scores = F.softmax(scores, dim=2).mean(1)
        elif mode == 'score':
            scores = scores.mean(1)
        return scores.cpu().numpy()

    def forward(self, keypoint, label=None, return_loss=True):
        if not return_loss:
            return self.forward_test(keypoint)
        if label is None:
            raise ValueError('Label should not be None.')
        return self.forward_train(keypoint, label)


def gather_results(part, size):
    """Inference results of all ranks in dataset order (what mmcv's ``multi_gpu_test`` hands tools/test.py:107):
    rank r holds samples r, r+world, ... (``DistributedSampler``, padded), so the parts are interleaved and cut to
    ``size``.  Every rank gets the full list."""
    world = _dist_world()
    if world == 1:
        return list(part)[:size]
    parts = [None] * world
    dist.all_gather_object(parts, list(part))
    return interleave_parts(parts, size)


def interleave_parts(parts, size):
    """parts[r] = the results of samples r, r + world, ... -> one list in dataset order, cut to ``size`` (the wrapped
    padding of the sampler falls off the end)."""
    hole = object()
    out = []
    for group in zip_longest(*parts, fillvalue=hole):
        out.extend(r for r in group if r is not hole)
    return out[:size]
