"""Golden fixture for the per-video learned adjacency at test time (``test_cfg['graph_ext']``), generated from the IMPORTED
reference (build container only: needs the reference checkout, see ref_shim):

    python tests/golden/gen_golden_graph_ext.py [--out DIR]

  graph_ext.npz   the reduced DS-STGCN (the shipped DS kwargs at base 16, 4 stages: L = 4 layers, mid = 2, 2, 4, 4) with
                  alpha, beta, add_coeff ~ N(0, 0.5^2), in eval mode on 2 seeded videos of 3 clips x 2 persons (T = 16,
                  V = 25).  The reference's own ``HookTool.hook_fun`` (pyskl/core/hooks/feature_hook.py:13-142) is registered
                  on each block's ``gcn`` and rebuilds ``A + alpha tanh(D)`` per person-sample and channel — (12, 3, mid, 1,
                  25, 25) per layer —, which is then averaged over the channels and over the 6 person-samples of each video
                  (the clip / person average of the driver in pyskl/pyskl/core/engine/test.py:39-71 with the channel mean).
                  Entries: ``cfg`` (json), ``sd_*`` (the state_dict), ``input_seed`` / ``input_shape`` (x = randn of that
                  generator seed), ``g64`` — the pooled graphs (2, 4, 3, 25, 25) of a float64 run —, ``g32`` — of the
                  reference's own float32 run, pooled in float32 —, ``ref32_rel`` — the per-layer relative L2 error of
                  g32 against g64.

The hook module imports ``mmcv.parallel`` and ``mmcv.runner.HOOKS / Hook / OptimizerHook`` for code that is not run here:
stubs of those names are added to ref_shim's.  Data only.  The archive is written with fixed member times, so a second run
gives a byte-identical file."""
import copy
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (ref_shim, ds_cfg, liven, sd_np)
import ref_shim  # noqa: E402
from gen_golden_dghgcn import savez_det  # noqa: E402

R = G.R
INPUT_SEED = 4100
INPUT_SHAPE = (2, 3, 2, 16, 25, 3)


def hook_tool():
    """The reference's HookTool class, its module loaded from its file (the package around it pulls in mmcv's runner)."""
    par = types.ModuleType('mmcv.parallel')
    par.is_module_wrapper = lambda m: False
    sys.modules['mmcv.parallel'] = par
    runner = sys.modules['mmcv.runner']
    runner.HOOKS = ref_shim._Registry('hook')
    runner.Hook = object
    runner.OptimizerHook = object
    path = os.path.join(ref_shim.REF_ROOT, 'pyskl', 'core', 'hooks', 'feature_hook.py')
    spec = importlib.util.spec_from_file_location('dsgcn_ref_feature_hook', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.HookTool


def model_cfg():
    cfg = G.ds_cfg(num_classes=12, base_channels=16, num_stages=4, inflate_stages=[3], down_stages=[3])
    cfg['cls_head']['in_channels'] = 32
    return cfg


def pooled_graphs(model, x, HookTool):
    """x (videos, clips, M, T, V, C) -> (videos, L, K, V, V): the hook's A of every layer, channel mean, then the mean over
    the clips * M person-samples of each video (consecutive rows: ``keypoint.flatten(0, 1)`` leaves the person fastest)."""
    hooks = []
    handles = []
    for blk in model.backbone.gcn:
        h = HookTool()
        handles.append(blk.gcn.register_forward_hook(h.hook_fun))
        hooks.append(h)
    videos, clips, M = x.shape[:3]
    with torch.no_grad():
        model.extract_feat(x.flatten(0, 1))
    for h in handles:
        h.remove()
    out = []
    for h in hooks:
        A = h.A                                               # (videos*clips*M, K, mid, 1, V, V)
        assert A.dim() == 6 and A.shape[0] == videos * clips * M and A.shape[3] == 1, A.shape
        A = A[:, :, :, 0]
        out.append(A.reshape((videos, clips * M) + A.shape[1:]).mean((1, 3)))
    return torch.stack(out, 1)


def main(out_dir=HERE):
    HookTool = hook_tool()
    cfg = model_cfg()
    np.random.seed(14)
    torch.manual_seed(14)
    m = R.builder.build_model(copy.deepcopy(cfg))
    G.liven(m, 41)
    m.eval()
    g = torch.Generator().manual_seed(INPUT_SEED)
    x = torch.randn(INPUT_SHAPE, generator=g)
    out = {'cfg': np.array(json.dumps(cfg, sort_keys=True)), 'input_seed': np.array(INPUT_SEED),
           'input_shape': np.array(INPUT_SHAPE)}
    out.update({'sd_' + k: v for k, v in G.sd_np(m).items()})
    g32 = pooled_graphs(m, x, HookTool)
    m64 = R.builder.build_model(copy.deepcopy(cfg)).double()
    m64.load_state_dict({k: v.double() if v.dtype.is_floating_point else v for k, v in m.state_dict().items()})
    m64.eval()
    g64 = pooled_graphs(m64, x.double(), HookTool)
    assert g32.dtype == torch.float32 and g64.dtype == torch.float64 and g32.shape == g64.shape
    out['g32'] = g32.numpy()
    out['g64'] = g64.numpy()
    d = (g32.double() - g64).flatten(2).transpose(0, 1).flatten(1)
    rel = d.norm(dim=1) / g64.flatten(2).transpose(0, 1).flatten(1).norm(dim=1)
    out['ref32_rel'] = rel.numpy()
    path = os.path.join(out_dir, 'graph_ext.npz')
    savez_det(path, **out)
    print(f'wrote graph_ext.npz: graphs {tuple(g64.shape)}, {os.path.getsize(path)} bytes, reference fp32 relative L2 per '
          f'layer {[f"{v:.2e}" for v in rel.tolist()]}')


if __name__ == '__main__':
    main(sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else HERE)
