"""mmcv 1.x ``DefaultOptimizerConstructor`` for the flat optimizers: what ``build_optimizer(model, cfg.optimizer)`` of the
reference (pyskl/core/optimizer/optimizers_builder.py:94, pyskl/apis/train.py:110) turns an ``optimizer`` dict and its
``paramwise_cfg`` into — one (lr, weight_decay) pair per parameter tensor, in ``parameters()`` order.

Without ``paramwise_cfg`` mmcv hands ``model.parameters()`` to the optimizer: ONE param group.  With it ``add_params``
walks the module tree (a module's own parameters, then its children: the order of ``named_parameters()``) and makes one
param group PER TENSOR:

1. ``custom_keys``: the keys sorted alphabetically, then by length with the longest first; the first one that is a substring
   of the parameter's full name sets ``lr = base_lr * lr_mult`` and ``weight_decay = base_wd * decay_mult`` (each multiplier
   defaults to 1) and nothing below applies.
2. otherwise a ``bias`` that does not belong to a norm layer gets ``lr = base_lr * bias_lr_mult``, and the weight decay is
   ``base_wd`` times the first of: ``norm_decay_mult`` (the module is a _BatchNorm, _InstanceNorm, GroupNorm or LayerNorm),
   ``dwconv_decay_mult`` (an nn.Conv2d with groups == in_channels), ``bias_decay_mult`` (the parameter is named ``bias``).

A parameter with ``requires_grad=False`` keeps its slot (a group of its own with the optimizer's defaults) and is never
updated.  ``bypass_duplicate`` is accepted: the models here share no tensors.  ``dcn_offset_lr_mult`` and any other key
raise ``NotImplementedError``."""
from collections import namedtuple

import torch.nn as nn
from torch.nn.modules.batchnorm import _BatchNorm
from torch.nn.modules.instancenorm import _InstanceNorm

KEYS = ('custom_keys', 'bias_lr_mult', 'bias_decay_mult', 'norm_decay_mult', 'dwconv_decay_mult', 'bypass_duplicate')

# one per parameter tensor, in parameters() order; weight_decay None = the optimizer class's default
ParamRule = namedtuple('ParamRule', 'name param lr weight_decay')


def validate(paramwise_cfg, base_wd):
    """mmcv ``DefaultOptimizerConstructor._validate_cfg`` plus the keys this package implements."""
    if not isinstance(paramwise_cfg, dict):
        raise TypeError(f'paramwise_cfg should be None or a dict, but got {type(paramwise_cfg)}')
    for key in paramwise_cfg:
        if key not in KEYS:
            raise NotImplementedError(f'paramwise_cfg key {key!r} is not supported (supported: {", ".join(KEYS)})')
    custom_keys = paramwise_cfg.get('custom_keys', {})
    if not isinstance(custom_keys, dict):
        raise TypeError(f'If specified, custom_keys must be a dict, but got {type(custom_keys)}')
    if base_wd is None:
        if any('decay_mult' in custom_keys[key] for key in custom_keys) or \
                any(k in paramwise_cfg for k in ('bias_decay_mult', 'norm_decay_mult', 'dwconv_decay_mult')):
            raise ValueError('base_wd should not be None')


def param_rules(module, base_lr, base_wd=None, paramwise_cfg=None):
    """-> [ParamRule] for every parameter of ``module`` (frozen ones included), in ``parameters()`` order.  ``base_wd``:
    the ``weight_decay`` of the optimizer dict, None when it is absent (then every rule's ``weight_decay`` is None)."""
    if paramwise_cfg is None:
        return [ParamRule(name, p, base_lr, base_wd) for name, p in module.named_parameters()]
    validate(paramwise_cfg, base_wd)
    custom_keys = paramwise_cfg.get('custom_keys', {})
    sorted_keys = sorted(sorted(custom_keys.keys()), key=len, reverse=True)
    bias_lr_mult = paramwise_cfg.get('bias_lr_mult', 1.)
    bias_decay_mult = paramwise_cfg.get('bias_decay_mult', 1.)
    norm_decay_mult = paramwise_cfg.get('norm_decay_mult', 1.)
    dwconv_decay_mult = paramwise_cfg.get('dwconv_decay_mult', 1.)
    rules = []

    def add_params(mod, prefix):
        is_norm = isinstance(mod, (_BatchNorm, _InstanceNorm, nn.GroupNorm, nn.LayerNorm))
        is_dwconv = isinstance(mod, nn.Conv2d) and mod.in_channels == mod.groups
        for name, param in mod.named_parameters(recurse=False):
            full = f'{prefix}.{name}' if prefix else name
            lr, wd = base_lr, base_wd
            if param.requires_grad:
                for key in sorted_keys:
                    if key in f'{prefix}.{name}':
                        lr = base_lr * custom_keys[key].get('lr_mult', 1.)
                        if base_wd is not None:
                            wd = base_wd * custom_keys[key].get('decay_mult', 1.)
                        break
                else:
                    if name == 'bias' and not is_norm:
                        lr = base_lr * bias_lr_mult
                    if base_wd is not None:
                        if is_norm:
                            wd = base_wd * norm_decay_mult
                        elif is_dwconv:
                            wd = base_wd * dwconv_decay_mult
                        elif name == 'bias':
                            wd = base_wd * bias_decay_mult
            rules.append(ParamRule(full, param, lr, wd))
        for child_name, child in mod.named_children():
            add_params(child, f'{prefix}.{child_name}' if prefix else child_name)

    add_params(module, '')
    return rules
