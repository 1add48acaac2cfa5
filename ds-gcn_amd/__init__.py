"""dsgcn_amd — MI355X-native DS-GCN hot path behind the PYSKL registry/config API.

Drop-in names (reference: pyskl/models/builder.py, pyskl/models/gcns/*, recognizers/*, heads/*,
losses/*): ``build_model``, ``RecognizerGCN``, ``DGSTGCN``, ``STGCN``, ``CTRGCN``, ``GCNHead``,
``CrossEntropyLoss``, ``Graph``, ``Config``.
"""
from .registry import Registry, build_from_cfg
from .config import Config, ConfigDict
from .graph import Graph
from .builder import (MODELS, BACKBONES, HEADS, LOSSES, NECKS, RECOGNIZERS, build_backbone, build_head, build_loss,
                      build_model, build_recognizer)
from .evaluation import top_k_accuracy, mean_class_accuracy, confusion_matrix, class_mean_graphs
from .losses import CrossEntropyLoss
from .heads import GCNHead, SimpleHead
from .gcn_units import dggcn, dghgcn, dgphgcn1, unit_aagcn, unit_gcn, unit_ctrgcn, unit_ctrhgcn, CTRGC, CTRHGC, Deferred
from .tcn_units import dgmstcn, dgmsmlp, mstcn, msmlp, unitmlp, unit_tcn, MSTCN
from .backbones import DGSTGCN, STGCN, CTRGCN, AAGCN, DGBlock, STGCNBlock, CTRGCNBlock, AAGCNBlock
from .recognizers import RecognizerGCN, reduce_log_vars, gather_results
from . import kernels
from .kernels import set_matmul_precision, get_matmul_precision, matmul_precision
from . import pipeline
from .pipeline import PIPELINES, DATASETS, Compose, PoseDataset, SkeletonStore, SkeletonBatcher, StreamBatcher, build_dataset
from .data_parallel import FlatParams, FlatDataParallel, shard_batch
from .train import FlatAdam, FlatSGD, build_optimizer, cosine_lr
from .paramwise import param_rules
from .ema import FlatEMA, ema_momentum
from .checkpoint import load_checkpoint, save_checkpoint, resume, find_resume, fuse_conv_bn
from .engine import TrainEngine
from .apis import train_model, EpochRunner, EvalLoop, epoch_indices, evaluate_scores
from .infer import InferEngine, EnsembleEngine
from .testing import (test_model, dump_results, load_results, ensemble_results, test_ensemble, parse_stream_weights,
                      STREAM_WEIGHTS)

__version__ = '0.1.0'
