"""Accuracy metrics used on the training / validation path.  Contract: pyskl/core/evaluation.py:21-126 — ``top_k_accuracy``
(a sample counts when its label is among the k best scores), ``confusion_matrix`` (rows = true class, columns = predicted,
over the classes that OCCUR in either list, in sorted order), ``mean_class_accuracy`` (this fork returns the pair
(mean of the per-class recalls over those classes, confusion matrix); datasets/base.py:194,201 unpacks it).
``class_mean_graphs``: the reference's ``metric='graph'`` (datasets/base.py:214-223) over the per-video learned adjacencies of
``test_cfg['graph_ext']``."""
import numpy as np


def top_k_accuracy(scores, labels, topk=(1, )):
    """-> list, per k: the fraction of samples whose label is one of their k highest-scoring classes (ties resolved the
    way a stable ascending argsort resolves them: the later class wins)."""
    scores = np.asarray(scores)
    want = np.asarray(labels).reshape(-1, 1)
    ranked = np.argsort(scores, axis=1)                     # ascending: the best k are the last k columns
    return [float((ranked[:, max(scores.shape[1] - k, 0):] == want).any(axis=1).mean()) for k in topk]


def confusion_matrix(y_pred, y_real, normalize=None):
    """Counts[i, j] = samples of the i-th occurring class predicted as the j-th occurring class (classes = sorted union of
    both inputs).  ``normalize``: None | 'true' (rows sum to 1) | 'pred' (columns) | 'all'; empty rows / columns give 0."""
    if normalize not in ('true', 'pred', 'all', None):
        raise ValueError("normalize must be one of {'true', 'pred', 'all', None}")
    pred, real = np.asarray(y_pred), np.asarray(y_real)
    for name, a in (('y_pred', pred), ('y_real', real)):
        if not np.issubdtype(a.dtype, np.integer):
            raise TypeError(f'{name} must hold integer class ids, got {a.dtype}')
    classes, codes = np.unique(np.concatenate([real.ravel(), pred.ravel()]), return_inverse=True)
    k = len(classes)
    row, col = codes[:real.size], codes[real.size:]
    counts = np.zeros((k, k), dtype=np.int64)
    np.add.at(counts, (row, col), 1)
    if normalize is None:
        return counts
    total = {'true': counts.sum(1, keepdims=True), 'pred': counts.sum(0, keepdims=True), 'all': counts.sum()}[normalize]
    with np.errstate(all='ignore'):
        return np.nan_to_num(counts / total)


def mean_class_accuracy(scores, labels):
    """-> (mean over the occurring classes of hits / samples of that class — a class that only occurs as a prediction
    counts as 0 —, confusion matrix as float)."""
    counts = confusion_matrix(np.argmax(scores, axis=1), labels).astype(float)
    seen = counts.sum(axis=1)
    recall = np.divide(np.diag(counts), seen, out=np.zeros_like(seen), where=seen > 0)
    return float(recall.mean()), counts


def class_mean_graphs(results, labels):
    """The reference's ``evaluate(metric='graph')`` (datasets/base.py:214-223): ``results`` — one ``(L, K, V, V)`` array per
    video — and integer ``labels`` -> a list whose entry i is the mean graph of the videos of class i, float32.

    Two quirks of the reference loop ``for i in range(max(label))`` are kept: the list has ``max(labels)`` entries, so the
    LAST class (the largest label that occurs) is left out, and a class below it without a video gives an all-NaN entry
    (the mean of nothing), not a missing one."""
    graphs = np.stack([np.asarray(r, dtype=np.float32) for r in results])
    labels = np.asarray(labels).reshape(-1)
    if len(labels) != len(graphs):
        raise ValueError(f'class_mean_graphs: {len(graphs)} results, {len(labels)} labels')
    out = []
    for i in range(int(labels.max())):
        rows = graphs[labels == i]
        if len(rows):
            out.append(rows.mean(0, dtype=np.float32))
        else:
            out.append(np.full(graphs.shape[1:], np.nan, dtype=np.float32))
    return out
