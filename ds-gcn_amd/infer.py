"""Multi-clip inference of a recognizer on one GPU, the MI355X way: the counterpart of ``engine.TrainEngine`` for the test
pass (reference: ``RecognizerGCN.forward_test``, pyskl/models/recognizers/recognizergcn.py:53-107, driven by mmcv's
``multi_gpu_test`` from tools/test.py:101-105).

``RecognizerGCN.forward_test`` here runs eagerly, asks the backbone for the whole last-block activation although a
``GCNHead`` only reads its plane means, does the head as ~8 framework launches and ends every batch with a blocking
``.cpu().numpy()``.  ``InferEngine`` is the same arithmetic as

    one hipGraph replay per batch shape:  weight images of the wide convs  ->  backbone(x, pool=True)  ->  head_test

Under ``test_cfg['feat_ext']`` / ``['score_ext']`` the tail of the graph is ``kernels.feat_ext`` instead (the pooled last
block when frames and joints are both averaged, the whole activation otherwise), any number of videos per call, each
pooled by itself.  Under ``test_cfg['graph_ext']`` the graph is the backbone with the units' adjacency taps
(``RecognizerGCN.forward_graphs``) and the result the per-video graphs (N, L, K, V, V).  Either way the engine hands back DEVICE tensors: nothing in a call waits for the GPU, the caller reads back when it wants to (``test_model``:
once per pass)."""
import torch

from . import kernels
from .heads import SimpleHead


class InferEngine:

    def __init__(self, model, use_graph=True, warmup_eager=1, strict_graph=False, max_views=None, matmul_precision=None):
        """use_graph: capture one hipGraph per input shape after ``warmup_eager`` eager calls of that shape and replay it
        from then on.  strict_graph: a failed capture raises instead of falling back to eager launches (``capture_error``
        keeps the reason either way; multi-GPU runs: ranks must not silently differ).  max_views: the largest number of
        clips (videos x clips) one forward may hold; a larger batch is cut into chunks of whole videos (a single video is
        never split), at most two chunk shapes, results concatenated.  matmul_precision: 'highest' | 'high' or None = the
        process level at this moment; fixed here for every eager call, capture and replay (see ``TrainEngine``).

        The captured graph contains the launches that build the bf16 weight images of the wide convs, so a replay after the
        parameters were changed IN PLACE (an optimizer step, ``load_state_dict``) computes with the new values.  Anything
        that changes tensor addresses or the module tree (``.to()``, ``fuse_conv_bn`` creating a bias, swapping a layer)
        needs ``reset()`` — or build the engine afterwards, as ``test_model`` does."""
        self.model = model
        self.matmul_precision = kernels.get_matmul_precision() if matmul_precision is None else matmul_precision
        kernels.matmul_precision(self.matmul_precision)        # (ValueError for an unknown name)
        self._want_graph = bool(use_graph)
        self.warmup_eager = int(warmup_eager)
        self.strict_graph = strict_graph
        self.max_views = None if not max_views else int(max_views)
        # the engine's OWN table of weight images (kernels.private_weight_images): entries pinned by a capture live and die
        # with this object, and a TrainEngine beside it never rebuilds them (nor this engine the TrainEngine's)
        self._images = {}
        self.reset()

    def reset(self):
        """Forget every captured graph, static buffer and weight image (after a structural change of the model)."""
        self._graphs = {}          # (shape, dtype, average_clips, extraction, graph mode) -> (graph, static input, static output)
        self._seen = {}            # same key -> eager calls taken
        self._images.clear()
        self.use_graph = self._want_graph
        self.capture_error = None
        self.replays = self.eager_calls = 0
        head, backbone = self.model.cls_head, self.model.backbone
        # the pooled last block + the one-launch head apply when the head is the plain 'GCN' pooling head; anything else
        # takes the module calls of forward_test (still on the device)
        self.fused_head = bool(getattr(backbone, 'supports_pool', False) and isinstance(head, SimpleHead)
                               and type(head).forward is SimpleHead.forward and head.mode == 'GCN' and head.dropout is None)

    # ---- pieces --------------------------------------------------------------------------------------------
    def _forward(self, x):
        model = self.model
        if model.graph_extraction() is not None:
            return model.forward_graphs(x)
        if model.extraction() is not None:
            return model.forward_extract(x)
        N, clips, M = x.shape[:3]
        mode = model.test_cfg['average_clips']
        head = model.cls_head
        if self.fused_head and kernels.head_test_fits(clips, head.in_c, head.num_classes):
            feat = model.backbone(x.float().flatten(0, 1), pool=True)                 # (N*clips, M, C) plane means
            return kernels.head_test(feat.reshape(N * clips * M, -1), head.fc_cls.weight, head.fc_cls.bias, N, clips, M, mode)
        scores = head(model.extract_feat(x.float().flatten(0, 1))).view(N, clips, -1)
        if mode == 'prob':
            scores = torch.softmax(scores, dim=2).mean(1)
        elif mode == 'score':
            scores = scores.mean(1)
        return scores

    def _capture(self, x):
        sx = x.clone()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        # one chain on the capturing stream: no side streams, no parallel branches
        with torch.cuda.graph(g, capture_error_mode='thread_local'):
            out = self._forward(sx)
        torch.cuda.synchronize()
        return g, sx, out

    def _key(self, x):
        return (tuple(x.shape), x.dtype, self.model.test_cfg['average_clips'], self.model.extraction(),
                self.model.graph_extraction())

    def _run(self, x):
        key = self._key(x)
        if self.use_graph and key not in self._graphs and self._seen.get(key, 0) >= self.warmup_eager:
            try:
                self._graphs[key] = self._capture(x)
            except Exception as exc:       # noqa: BLE001 — report and fall back (or raise) below
                self.capture_error = f'{type(exc).__name__}: {exc}'
                if self.strict_graph:
                    raise
                self.use_graph = False
        if self.use_graph and key in self._graphs:
            g, sx, out = self._graphs[key]
            sx.copy_(x)
            g.replay()
            self.replays += 1
            return out.clone()             # the static buffer is rewritten by the next replay
        out = self._forward(x)
        self._seen[key] = self._seen.get(key, 0) + 1
        self.eager_calls += 1
        return out

    def _chunks(self, N, clips):
        if self.max_views is None or N * clips <= self.max_views:
            return [(0, N)]
        per = max(1, self.max_views // clips)
        return [(a, min(a + per, N)) for a in range(0, N, per)]

    # ---- the call ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, keypoint):
        """keypoint (N, clips, M, T, V, C) on the device -> DEVICE tensor (N, classes) — (N, clips, classes) when the
        model's ``test_cfg['average_clips']`` is None; float16 (N, n', m', C | classes, t', v') under ``feat_ext`` /
        ``score_ext`` (row i: what ``forward_test`` returns for video i alone); float32 (N, L, K, V, V) under ``graph_ext``.
        No host synchronisation."""
        if keypoint.dim() != 6:
            raise ValueError(f'InferEngine expects (N, clips, M, T, V, C), got {tuple(keypoint.shape)}')
        if not keypoint.is_cuda:
            raise RuntimeError('InferEngine runs on the GPU only (there is no CPU path): move the batch to the device')
        model = self.model
        was_training = model.training
        if was_training:
            model.eval()
        try:
            with kernels.private_weight_images(self._images), kernels.matmul_precision(self.matmul_precision):
                parts = [self._run(keypoint[a:b]) for a, b in self._chunks(keypoint.shape[0], keypoint.shape[1])]
        finally:
            if was_training:
                model.train()
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def graphed(self, keypoint):
        return self._key(keypoint) in self._graphs


class EnsembleEngine:
    """The multi-stream test pass (joint + bone + joint motion + bone motion, configs/*/README.md note 2) of S recognizers
    that belong together, as

        one hipGraph replay per batch shape:  weight images of every model  ->  S x backbone(x_s, pool=True)  ->  head_ensemble

    — the S heads and the weighted sum of their scores are ONE launch (csrc/head_ensemble.hip) whose stream rows and sum
    have the bits of S ``InferEngine`` passes followed by ``testing.ensemble_results``."""

    MAX_SIDE_STREAMS = 4

    def __init__(self, models, weights, use_graph=True, warmup_eager=1, max_views=None, matmul_precision=None,
                 concurrent=False):
        """models: S ``RecognizerGCN``s with a 'GCN' pooling head, the same ``num_classes``, head ``in_channels`` and
        ``test_cfg['average_clips']`` ('prob' | 'score'), none of them extracting features (ValueError otherwise).
        weights: S stream weights; they live in a device tensor the head launch reads, so ``set_weights`` is followed by
        the next replay.  use_graph / warmup_eager / max_views / matmul_precision: as ``InferEngine`` — static buffers
        inside, copies out, parameters changed in place seen by the next replay, ``reset()`` after a structural change.
        concurrent: the backbones run as parallel branches on up to four side streams, forked from and joined to the
        calling stream (in a capture: graph edges); False: back to back on the calling stream."""
        from .recognizers import RecognizerGCN
        self.models = list(models)
        S = len(self.models)
        if not 1 <= S <= kernels.ENSEMBLE_MAX:
            raise ValueError(f'EnsembleEngine: {S} models; 1 to {kernels.ENSEMBLE_MAX} streams fit the head launch')
        weights = [float(w) for w in weights]
        if len(weights) != S:
            raise ValueError(f'EnsembleEngine: {S} models, {len(weights)} stream weights')
        for i, m in enumerate(self.models):
            head = getattr(m, 'cls_head', None)
            if not isinstance(m, RecognizerGCN) or not (
                    isinstance(head, SimpleHead) and type(head).forward is SimpleHead.forward and head.mode == 'GCN'
                    and head.dropout is None and getattr(m.backbone, 'supports_pool', False)):
                raise ValueError(f'EnsembleEngine: model {i} is not a RecognizerGCN with a GCNHead over a pooling backbone')
            if m.extraction() is not None:
                raise ValueError(f'EnsembleEngine: model {i}: test_cfg feat_ext / score_ext has no weighted sum')
            if m.graph_extraction() is not None:
                raise ValueError(f'EnsembleEngine: model {i}: test_cfg graph_ext has no weighted sum')
        h0 = self.models[0].cls_head
        for i, m in enumerate(self.models):
            if m.cls_head.num_classes != h0.num_classes or m.cls_head.in_c != h0.in_c:
                raise ValueError(f'EnsembleEngine: model {i}: head ({m.cls_head.in_c} channels, {m.cls_head.num_classes} '
                                 f'classes) differs from model 0 ({h0.in_c}, {h0.num_classes})')
        self._mode()
        self.matmul_precision = kernels.get_matmul_precision() if matmul_precision is None else matmul_precision
        kernels.matmul_precision(self.matmul_precision)
        self._want_graph = bool(use_graph)
        self.warmup_eager = int(warmup_eager)
        self.max_views = None if not max_views else int(max_views)
        self.concurrent = bool(concurrent)
        self.weights = torch.tensor(weights, dtype=torch.float32, device=next(self.models[0].parameters()).device)
        self._images = {}
        self._sides = []
        self.stream_scores = None
        self.reset()

    def _mode(self):
        modes = [m.test_cfg['average_clips'] for m in self.models]
        if any(md != modes[0] for md in modes) or modes[0] not in ('prob', 'score'):
            raise ValueError(f"EnsembleEngine: test_cfg['average_clips'] of the models is {modes}: one of 'prob' / 'score' "
                             'for all (per-clip score lists have no weighted sum)')
        return modes[0]

    def set_weights(self, weights):
        """New stream weights, in place: the next call — replayed or not — sums with them."""
        weights = [float(w) for w in weights]
        if len(weights) != len(self.models):
            raise ValueError(f'EnsembleEngine: {len(self.models)} models, {len(weights)} stream weights')
        self.weights.copy_(torch.tensor(weights, dtype=torch.float32))

    def reset(self):
        """Forget every captured graph, static buffer and weight image (after a structural change of a model)."""
        self._graphs = {}          # (shape, dtype, average_clips) -> (graph, static inputs, static sum, static stream scores)
        self._seen = {}
        self._images.clear()
        self.use_graph = self._want_graph
        self.capture_error = None
        self.replays = self.eager_calls = 0

    # ---- pieces --------------------------------------------------------------------------------------------
    def _backbones(self, xs):
        flat = [x.float().flatten(0, 1) for x in xs]
        if not self.concurrent or len(flat) == 1:
            return [m.backbone(x, pool=True) for m, x in zip(self.models, flat)]
        dev = flat[0].device
        main = torch.cuda.current_stream(dev)
        while len(self._sides) < min(len(flat), self.MAX_SIDE_STREAMS):
            self._sides.append(torch.cuda.Stream(device=dev))
        feats = []
        for s, (m, x) in enumerate(zip(self.models, flat)):
            side = self._sides[s % len(self._sides)]
            if s < len(self._sides):
                side.wait_stream(main)                    # fork (a fifth model queues behind the first on its stream)
            with torch.cuda.stream(side):
                feats.append(m.backbone(x, pool=True))
        for side in self._sides[:len(flat)]:
            main.wait_stream(side)                        # join
        for f in feats:
            f.record_stream(main)
        return feats

    def _forward(self, xs):
        N, clips, M = xs[0].shape[:3]
        feats = self._backbones(xs)
        heads = [(m.cls_head.fc_cls.weight, m.cls_head.fc_cls.bias) for m in self.models]
        return kernels.head_ensemble([f.reshape(N * clips * M, -1) for f in feats], heads, self.weights, N, clips, M,
                                     self._mode(), want_streams=True)

    def _capture(self, xs):
        sx = [x.clone() for x in xs]
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode='thread_local'):
            out, so = self._forward(sx)
        torch.cuda.synchronize()
        return g, sx, out, so

    def _key(self, xs):
        return tuple(xs[0].shape), xs[0].dtype, self._mode()

    def _run(self, xs):
        key = self._key(xs)
        if self.use_graph and key not in self._graphs and self._seen.get(key, 0) >= self.warmup_eager:
            try:
                self._graphs[key] = self._capture(xs)
            except Exception as exc:       # noqa: BLE001 — kept in capture_error; eager launches from here on
                self.capture_error = f'{type(exc).__name__}: {exc}'
                self.use_graph = False
        if self.use_graph and key in self._graphs:
            g, sx, out, so = self._graphs[key]
            for d, x in zip(sx, xs):
                d.copy_(x)
            g.replay()
            self.replays += 1
            return out.clone(), so.clone()     # the static buffers are rewritten by the next replay
        res = self._forward(xs)
        self._seen[key] = self._seen.get(key, 0) + 1
        self.eager_calls += 1
        return res

    def _chunks(self, N, clips):
        if self.max_views is None or N * clips <= self.max_views:
            return [(0, N)]
        per = max(1, self.max_views // clips)
        return [(a, min(a + per, N)) for a in range(0, N, per)]

    # ---- the call ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, keypoints):
        """keypoints: S tensors (N, clips, M, T, V, C) on the device, one per model, of one shape -> DEVICE tensor
        (N, classes), the weighted sum; ``stream_scores`` (S, N, classes) holds the models' own scores of this call.  No
        host synchronisation."""
        xs = list(keypoints)
        if len(xs) != len(self.models):
            raise ValueError(f'EnsembleEngine: {len(self.models)} models, {len(xs)} inputs')
        for x in xs:
            if x.dim() != 6:
                raise ValueError(f'EnsembleEngine expects (N, clips, M, T, V, C) per stream, got {tuple(x.shape)}')
            if not x.is_cuda:
                raise RuntimeError('EnsembleEngine runs on the GPU only (there is no CPU path): move the batch to the device')
            if x.shape != xs[0].shape or x.dtype != xs[0].dtype:
                raise ValueError(f'EnsembleEngine: the streams differ in shape: {[tuple(t.shape) for t in xs]}')
        was_training = [m.training for m in self.models]
        for m in self.models:
            m.eval()
        try:
            with kernels.private_weight_images(self._images), kernels.matmul_precision(self.matmul_precision):
                parts = [self._run([x[a:b] for x in xs]) for a, b in self._chunks(xs[0].shape[0], xs[0].shape[1])]
        finally:
            for m, t in zip(self.models, was_training):
                m.train(t)
        if len(parts) == 1:
            out, self.stream_scores = parts[0]
        else:
            out, self.stream_scores = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts], 1)
        return out

    def graphed(self, keypoints):
        return self._key(list(keypoints)) in self._graphs
