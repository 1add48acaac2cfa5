"""``test_model`` — the testing half of the reference's command line (tools/test.py:71-176 over mmcv's ``multi_gpu_test``)
with the call shape of ``apis.train_model``:

    load the checkpoint [-> fuse_conv_bn] -> InferEngine over the model
    every rank: samples rank, rank + world, ... in dataset order through the engine (one hipGraph replay per batch; the
                scores stay on the device; ONE read-back at the end of the pass)
    gather_results -> rank 0 writes ``out`` and evaluates the metrics

``dump_results`` / ``ensemble_results`` end the j / b / jm / bm workflow inside the package: the paper's headline rows are
sums of four such result files.  ``test_ensemble`` is that workflow as ONE pass: one plan and one input launch per batch
for all streams, one ``EnsembleEngine`` replay, the stream files and the weighted sum out of the same read-back."""
import json
import logging
import os
import pickle

import numpy as np

from collections import OrderedDict

from .apis import EvalLoop, _get, _rank_world, evaluate_scores
from .checkpoint import fuse_conv_bn, load_checkpoint
from .infer import EnsembleEngine, InferEngine
from .evaluation import class_mean_graphs
from .recognizers import gather_results


def test_batch_size(cfg):
    """``data.test_dataloader.videos_per_gpu``, else ``data.videos_per_gpu``, else 1 (tools/test.py:143-147)."""
    data = _get(cfg, 'data', None) or {}
    loader = data.get('test_dataloader', None) or {}
    return int(loader.get('videos_per_gpu', data.get('videos_per_gpu', 1)))


test_batch_size.__test__ = False          # (a library function, not a pytest case)


def dump_results(results, out):
    """What ``dataset.dump_results`` writes (datasets/base.py:240-242): the list of per-video score arrays as ``.pkl``
    (float32 arrays) or ``.json`` (nested lists), in dataset order.  Extracted features / score maps (float16 arrays,
    ``test_cfg['feat_ext']`` / ``['score_ext']``) keep their dtype and go to ``.pkl`` only."""
    half = any(np.asarray(r).dtype == np.float16 for r in results)
    if half and os.path.splitext(out)[1].lower() == '.json':
        raise ValueError(f'dump_results: {out!r}: extracted features / score maps are float16 arrays and are written as .pkl')
    results = [np.asarray(r) if half else np.asarray(r, dtype=np.float32) for r in results]
    folder = os.path.dirname(os.path.abspath(out))
    os.makedirs(folder, exist_ok=True)
    suffix = os.path.splitext(out)[1].lower()
    if suffix in ('.pkl', '.pickle'):
        with open(out, 'wb') as f:
            pickle.dump(results, f)
    elif suffix == '.json':
        with open(out, 'w') as f:
            json.dump([r.tolist() for r in results], f)
    else:
        raise ValueError(f'dump_results: {out!r}: the output file is .pkl or .json')
    return out


def load_results(path):
    """The list ``dump_results`` wrote: float32 score arrays; float16 features / score maps come back as float16."""
    suffix = os.path.splitext(path)[1].lower()
    if suffix in ('.pkl', '.pickle'):
        with open(path, 'rb') as f:
            data = pickle.load(f)
    elif suffix == '.json':
        with open(path) as f:
            data = json.load(f)
    else:
        raise ValueError(f'load_results: {path!r}: a result file is .pkl or .json')
    return [r if isinstance(r, np.ndarray) and r.dtype == np.float16 else np.asarray(r, dtype=np.float32) for r in data]


def ensemble_results(files_or_lists, weights=None, labels=None, metrics=('top_k_accuracy', 'mean_class_accuracy')):
    """Weighted sum of several result sets (file names or lists of per-video score arrays; the j + b + jm + bm rows of the
    paper's tables, weights 1 by default) -> ``dict(results=[(classes,) float32 ...], metrics=OrderedDict | None)``;
    the metrics are those of the summed scores and need ``labels``."""
    sets = [load_results(s) if isinstance(s, (str, os.PathLike)) else [np.asarray(r, dtype=np.float32) for r in s]
            for s in files_or_lists]
    if not sets:
        raise ValueError('ensemble_results: nothing to sum')
    weights = [1.0] * len(sets) if weights is None else [float(w) for w in weights]
    if len(weights) != len(sets):
        raise ValueError(f'ensemble_results: {len(sets)} result sets, {len(weights)} weights')
    if any(len(s) != len(sets[0]) for s in sets):
        raise ValueError(f'ensemble_results: the result sets differ in length: {[len(s) for s in sets]}')
    total = sum(np.stack(s).astype(np.float32) * np.float32(w) for s, w in zip(sets, weights))
    vals = evaluate_scores(total, labels, metrics) if labels is not None else None
    return dict(results=list(total), metrics=vals)


def test_model(model, dataset, cfg, checkpoint=None, fuse=False, out=None,
               metrics=('top_k_accuracy', 'mean_class_accuracy'), average_clips=None, device='cuda', use_graph=True):
    """Score ``dataset`` with ``model`` the way the reference's tools/test.py does for the skeleton configs.

    dataset: a map-style dataset of ``dict(keypoint=(clips, M, T, V, C), label)`` items, or a (``SkeletonStore``,
    ``SkeletonBatcher``) pair built from the test pipeline; ``None``: built from ``cfg.data.test`` with ``test_mode=True``.
    checkpoint: loaded with ``load_checkpoint``; ``None``: ``<cfg.work_dir>/latest.pth`` when it exists, else the model as
    it is.  fuse: ``fuse_conv_bn`` before the engine is built.  average_clips: 'prob' / 'score' override the model's
    ``test_cfg`` for this pass (``--average-clips``; ``None`` = keep it).  out: rank 0 writes the results there (.pkl / .json).

    -> ``dict(results=[...], metrics=OrderedDict | None)``: the scores of every video in dataset order on every rank
    (``(classes,)`` float32 arrays; ``(clips, classes)`` when the model's ``average_clips`` is None, which has no metrics);
    ``metrics`` on rank 0 only.  ``cfg.evaluation.metric_options`` is honoured.  The numpy RNG state is left as found.
    ``cfg.matmul_precision`` ('highest' | 'high'; absent = the process level) is the level of the pass, logged once.

    Under ``test_cfg['feat_ext']`` / ``['score_ext']`` ``results`` holds one float16 array per video — what
    ``forward_test`` returns for that video alone, ``(n', m', C, t', v')`` resp. ``(1, n', m', classes, t', v')`` — and
    ``metrics`` is None; ``out`` must be a ``.pkl`` (checked before the pass).

    Under ``test_cfg['graph_ext']`` (True | 'ctr' | 'ahat') ``results`` holds one float32 ``(L, K, V, V)`` array per video:
    the learned adjacency of every dynamic-adjacency layer, averaged over the video's clips, persons and channels
    (gathered over the ranks and dumped like the feature arrays; ``out`` must be a ``.pkl``).  The only metric of such a
    pass is ``metrics=('graph',)``: ``evaluation.class_mean_graphs(results, labels)`` under the key 'graph'; the default
    metric tuple gives ``metrics`` None, any other name raises ValueError (before the pass, like 'graph' without
    ``graph_ext``)."""
    rank, world = _rank_world()
    data = _get(cfg, 'data', None) or {}
    if dataset is None:
        from .pipeline import build_dataset
        test_cfg = dict(data['test'])
        test_cfg['test_mode'] = True
        dataset = build_dataset(test_cfg)
    if isinstance(dataset, list) and len(dataset) == 1:
        dataset = dataset[0]
    if average_clips not in (None, 'prob', 'score'):
        raise ValueError(f'average_clips={average_clips!r}: "prob", "score" or None (keep the model\'s test_cfg)')
    extraction = model.extraction()
    graph_mode = model.graph_extraction()
    metrics = [metrics] if isinstance(metrics, str) else list(metrics)
    if graph_mode is not None:
        if out is not None and os.path.splitext(out)[1].lower() not in ('.pkl', '.pickle'):
            raise ValueError(f'test_model: {out!r}: per-video graphs are (L, K, V, V) arrays and are written as .pkl')
        if metrics == ['top_k_accuracy', 'mean_class_accuracy']:          # the default: no class scores to rate
            metrics = []
        if any(m != 'graph' for m in metrics):
            raise ValueError(f"test_model: metrics {metrics}: a test_cfg['graph_ext'] pass has the metric 'graph' only")
    elif 'graph' in metrics:
        raise ValueError("test_model: the metric 'graph' needs test_cfg['graph_ext']")
    if extraction is not None and out is not None and os.path.splitext(out)[1].lower() == '.json':
        raise ValueError(f'test_model: {out!r}: extracted features / score maps are float16 arrays and are written as .pkl')
    work_dir = _get(cfg, 'work_dir', None)
    if checkpoint is None and work_dir and os.path.exists(os.path.join(work_dir, 'latest.pth')):
        checkpoint = os.path.join(work_dir, 'latest.pth')
    if checkpoint is not None:
        load_checkpoint(model, checkpoint, map_location='cpu')
    model = model.to(device)
    was_training = model.training
    model.eval()
    if fuse:
        fuse_conv_bn(model)
    mode_before = model.test_cfg['average_clips']
    if average_clips is not None:
        model.test_cfg['average_clips'] = average_clips
    try:
        # built AFTER the structural steps above (device move, conv + BatchNorm folding): its graphs hold addresses
        engine = InferEngine(model, use_graph=use_graph, strict_graph=world > 1,
                             matmul_precision=_get(cfg, 'matmul_precision', None))
        logging.getLogger('dsgcn_amd').info('test_model: matmul precision: %s', engine.matmul_precision)
        eval_cfg = _get(cfg, 'evaluation', None) or {}
        loop = EvalLoop(dataset, batch_size=test_batch_size(cfg), metrics=[] if graph_mode is not None else metrics,
                        metric_options=eval_cfg.get('metric_options'), save_best=None,
                        device=next(model.parameters()).device, engine=engine)
        part = loop.predict(model, rank, world)
        results = gather_results(part, len(loop.source))
        per_clip = model.test_cfg['average_clips'] is None or extraction is not None or graph_mode is not None
    finally:
        model.test_cfg['average_clips'] = mode_before
        model.train(was_training)
    vals = None
    if rank == 0:
        if out is not None:
            dump_results(results, out)
        if not per_clip:
            vals = loop.evaluate(np.stack(results), loop.labels())
        elif graph_mode is not None and 'graph' in metrics:
            vals = OrderedDict(graph=class_mean_graphs(results, loop.labels()))
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    return dict(results=results, metrics=vals)


test_model.__test__ = False


STREAM_WEIGHTS = {'two': (1, 1), 'four': (2, 2, 1, 1)}       # the two- and four-stream rows (configs/*/README.md note 2)


def parse_stream_weights(weights, streams=None):
    """'2:2:1:1' | a key of ``STREAM_WEIGHTS`` | a sequence -> tuple of floats; ``streams``: the length it must have."""
    if isinstance(weights, str):
        if weights in STREAM_WEIGHTS:
            vals = STREAM_WEIGHTS[weights]
        else:
            try:
                vals = [float(p) for p in weights.split(':')]
            except ValueError:
                raise ValueError(f'stream weights {weights!r}: numbers joined by ":" (e.g. "2:2:1:1") or one of '
                                 f'{sorted(STREAM_WEIGHTS)}') from None
    else:
        vals = list(weights)
    vals = tuple(float(v) for v in vals)
    if streams is not None and len(vals) != streams:
        raise ValueError(f'stream weights {weights!r}: {len(vals)} weights for {streams} streams')
    return vals


def _stream_dataset(cfgs, streams, device):
    """(SkeletonStore, StreamBatcher) from ``data.test`` of one config per stream: the pipelines may differ in the
    feature alone, the annotations not at all."""
    from .pipeline import SkeletonStore, StreamBatcher, build_dataset
    if len(cfgs) != streams:
        raise ValueError(f'test_ensemble(dataset=None): {streams} models need {streams} configs, got {len(cfgs)}')
    tests = [dict((_get(c, 'data', None) or {})['test']) for c in cfgs]
    batcher = StreamBatcher([t['pipeline'] for t in tests])
    for i, t in enumerate(tests):
        for key in sorted((set(t) | set(tests[0])) - {'pipeline'}):
            if t.get(key) != tests[0].get(key):
                raise ValueError(f'test_ensemble: data.test of config {i} differs from config 0: {key}: '
                                 f'{tests[0].get(key)} != {t.get(key)}')
    first = dict(tests[0], test_mode=True)
    ds = build_dataset(first)
    dec = batcher.batcher.decompress
    opt = None if dec is None else dict(squeeze=dec.squeeze, max_person=dec.max_person)
    return SkeletonStore(ds.video_infos, device=device, decompress=opt), batcher


def test_ensemble(models, dataset, cfg, checkpoints=None, fuse=False, weights='2:2:1:1', out=None, stream_out=None,
                  metrics=('top_k_accuracy', 'mean_class_accuracy'), average_clips=None, device='cuda', use_graph=True,
                  concurrent=False):
    """Score ``dataset`` with the S models of a multi-stream ensemble (joint, bone, joint motion, bone motion) in ONE pass:
    what S ``test_model`` runs, S result files and ``ensemble_results`` give, bit for bit.

    models: S recognizers (``EnsembleEngine``'s conditions).  dataset: a (``SkeletonStore``, ``StreamBatcher``) pair;
    ``None``: built from ``data.test`` of ``cfg``, then a list of S configs that differ in ``GenSkeFeat.feats`` alone.
    cfg: one config, or a list whose first entry gives the batch size (``test_batch_size``), ``evaluation.metric_options``
    and ``matmul_precision``.  checkpoints: S files (``None`` entries: the model as it is); ``None``: with S configs
    ``<work_dir>/latest.pth`` of each where it exists.  weights: a sequence or 'a:b:c:d' (``parse_stream_weights``).
    average_clips: 'prob' / 'score' for this pass, ``None`` = the models' (which must agree).  out / stream_out (S paths):
    rank 0 writes the summed and the per-stream results through ``dump_results`` — each stream file is what
    ``test_model`` writes for that model.  concurrent: ``EnsembleEngine(concurrent=...)``.

    -> ``dict(results, metrics, stream_results=[S lists], stream_metrics=[S dicts])``, every list in dataset order on
    every rank, the metrics on rank 0 only.  The numpy RNG state is left as found."""
    from .apis import _BatchSource, epoch_indices
    import torch
    rank, world = _rank_world()
    models = list(models)
    S = len(models)
    cfgs = list(cfg) if isinstance(cfg, (list, tuple)) else [cfg]
    cfg0 = cfgs[0]
    vals = parse_stream_weights(weights, S)
    if stream_out is not None and len(stream_out) != S:
        raise ValueError(f'test_ensemble: {S} models, {len(stream_out)} stream_out paths')
    if checkpoints is not None and len(checkpoints) != S:
        raise ValueError(f'test_ensemble: {S} models, {len(checkpoints)} checkpoints')
    if average_clips not in (None, 'prob', 'score'):
        raise ValueError(f'average_clips={average_clips!r}: "prob", "score" or None (keep the models\' test_cfg)')
    if dataset is None:
        dataset = _stream_dataset(cfgs, S, device)
    if not (isinstance(dataset, (tuple, list)) and len(dataset) == 2 and hasattr(dataset[1], 'plan')
            and len(dataset[1]) == S):
        raise ValueError(f'test_ensemble: dataset is a (SkeletonStore, StreamBatcher) pair with {S} streams')
    if checkpoints is None:
        checkpoints = [None] * S
        if len(cfgs) == S:
            for i, c in enumerate(cfgs):
                work_dir = _get(c, 'work_dir', None)
                if work_dir and os.path.exists(os.path.join(work_dir, 'latest.pth')):
                    checkpoints[i] = os.path.join(work_dir, 'latest.pth')
    was_training, modes_before = [m.training for m in models], [m.test_cfg['average_clips'] for m in models]
    for i, ckpt in enumerate(checkpoints):
        if ckpt is not None:
            load_checkpoint(models[i], ckpt, map_location='cpu')
        models[i] = models[i].to(device)
        models[i].eval()
        if fuse:
            fuse_conv_bn(models[i])
        if average_clips is not None:
            models[i].test_cfg['average_clips'] = average_clips
    try:
        # built AFTER the structural steps above (device move, conv + BatchNorm folding): its graphs hold addresses
        engine = EnsembleEngine(models, vals, use_graph=use_graph, matmul_precision=_get(cfg0, 'matmul_precision', None),
                                concurrent=concurrent)
        logging.getLogger('dsgcn_amd').info('test_ensemble: %d streams, weights %s, matmul precision: %s', S, vals,
                                            engine.matmul_precision)
        source = _BatchSource(dataset, next(models[0].parameters()).device)
        n, batch = len(source), test_batch_size(cfg0)
        order = epoch_indices(n, 0, 0, rank, world, shuffle=False)
        sums, streams = [], []
        rng = np.random.get_state()           # the test-mode sampler seeds numpy per clip: put the stream back afterwards
        try:
            for b in range(0, len(order), batch):
                kps, _ = source.batch(order[b:b + batch])
                sums.append(engine(kps))
                streams.append(engine.stream_scores)
        finally:
            np.random.set_state(rng)
        if world > 1 and engine.capture_error is not None:
            raise RuntimeError(f'test_ensemble: the capture failed on rank {rank}: {engine.capture_error}')
        packed = torch.cat([torch.cat(sums)[None], torch.cat(streams, 1)]).cpu().numpy()      # the pass's one read-back
    finally:
        for m, t, md in zip(models, was_training, modes_before):
            m.test_cfg['average_clips'] = md
            m.train(t)
    results = gather_results(list(packed[0]), n)
    stream_results = [gather_results(list(packed[1 + s]), n) for s in range(S)]
    vals_sum, stream_vals = None, [None] * S
    if rank == 0:
        if out is not None:
            dump_results(results, out)
        for s in range(S if stream_out is not None else 0):
            dump_results(stream_results[s], stream_out[s])
        eval_cfg = _get(cfg0, 'evaluation', None) or {}
        labels = [int(v) for v in dataset[0].labels]
        vals_sum = evaluate_scores(np.stack(results), labels, list(metrics), eval_cfg.get('metric_options'))
        stream_vals = [evaluate_scores(np.stack(r), labels, list(metrics), eval_cfg.get('metric_options'))
                       for r in stream_results]
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    return dict(results=results, metrics=vals_sum, stream_results=stream_results, stream_metrics=stream_vals)


test_ensemble.__test__ = False
