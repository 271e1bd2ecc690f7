"""Shared test helpers: the project's bounds, seeded model construction, the primitive-op fixture and checksum verification
against the golden fixtures."""
import copy

import numpy as np
import pytest
import torch

from calodiffusion_amd.configs import load_config
from calodiffusion_amd.unet import CondUnet, unet_kwargs_from_config

SEED = 1234

# Bounds, all relative L2.  north_star asks for <= 1e-4 of the reference CPU path; the reference's own fp32 reorder floor is
# 5.5e-7 per denoise call.
TOL_OP = 1e-5       # one kernel / one denoise call against the reference's goldens or the CPU oracle
TOL_TRAJ = 1e-4     # a multi-step trajectory: north_star's own figure
TOL_ORACLE = 1e-5   # a whole denoise call against the oracle (test_denoise_matches_reference's bound: TOL_OP by another name)
TOL_REASSOC = 2e-6  # per conv, for a changed fp32 summation order: two forms of one computation, both above the reorder floor
TOL_ROW = 2e-6      # a sample's rows in a batch against the same sample alone (the chunking follows the batch: a reorder again)
TOL_BWD = 2e-5      # one backward kernel's dx / dw / db against autograd through the oracle's op (test_gpu_backward.py)
TOL_GRAD = 5e-6     # all parameter gradients together against autograd through the fp32 oracle (test_gpu_train.py)


def seeded_model(name, over=None, seed=SEED):
    """CaloDiffusion of the shipped config `name`, or of a config dict (a private copy, `over` applied) with the parameters the reference gets for
    torch.manual_seed(seed).  The config is the model's `.config`."""
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    cfg = copy.deepcopy(load_config(name))
    cfg.update(over or {})
    torch.manual_seed(seed)
    return CaloDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"])


def seeded_model_cfg(name, over=None, seed=SEED):
    """(seeded_model(...), its config)."""
    m = seeded_model(name, over, seed)
    return m, m.config


@pytest.fixture(scope="module")
def ops():
    from calodiffusion_amd.engine import Ops
    return Ops()


def cl(ops, a):
    return ops.to_channels_last(t(a).cuda())


def back(ops, y_cl):
    return ops.to_ncdhw(y_cl).cpu().numpy()


def seeded_unet(cfg_name_or_kwargs, seed=SEED):
    """CondUnet whose parameters equal the reference's for torch.manual_seed(seed) (see oracle/gen_golden.py)."""
    kw = unet_kwargs_from_config(load_config(cfg_name_or_kwargs)) if isinstance(cfg_name_or_kwargs, str) else dict(cfg_name_or_kwargs)
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    net = CondUnet(**kw)
    torch.random.set_rng_state(state)
    return net


def verify_checksums(sd, g):
    keys = [str(k) for k in g["ck_keys"]]
    vals = g["ck_vals"]
    assert sorted(sd.keys()) == keys
    for k, (s1, s2) in zip(keys, vals):
        t = sd[k].double()
        assert abs(float(t.sum()) - s1) <= 1e-9 * max(1.0, abs(s1)), k
        assert abs(float((t * t).sum()) - s2) <= 1e-9 * max(1.0, abs(s2)), k


def d1grid_kwargs():
    return dict(out_dim=1, layer_sizes=[32, 32, 64, 96], channels=4, cond_dim=128, resnet_block_groups=8, mid_attn=True,
                block_attn=True, compress_Z=True, cylindrical=True, data_shape=[1, 4, 5, 10, 30], time_embed=False,
                cond_embed=False, cond_size=7)


def unet_kwargs(grid, sizes=(32, 32, 64, 32), channels=3, cond_size=9, **over):
    kw = dict(out_dim=1, layer_sizes=list(sizes), channels=channels, cond_dim=128, resnet_block_groups=8, mid_attn=True,
              block_attn=True, compress_Z=True, cylindrical=True, data_shape=[1, channels] + list(grid), time_embed=False,
              cond_embed=False, cond_size=cond_size)
    kw.update(over)
    return kw


def profiled_launches(fn):
    """Run fn() under the per-launch profiler and return {category: launches}."""
    from calodiffusion_amd import engine
    engine.profile_begin()
    fn()
    return {k: v["launches"] for k, v in engine.profile_end().items()}


def per_layer_worst(got, want):
    """Worst relative L2 over the (shower, layer) rows: an energy-weighted norm over the whole array hides the low-energy layers."""
    num = np.linalg.norm((got - want).reshape(got.shape[0], got.shape[1], -1), axis=-1)
    den = np.linalg.norm(want.reshape(got.shape[0], got.shape[1], -1), axis=-1)
    return float((num / np.maximum(den, 1e-30)).max())


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def attn_block_weights(C, gen, qscale=1.0, kscale=1.0, bias=0.0):
    """CPU state dict of one Residual(PreNorm(LinearAttention)) block at C channels, keyed as engine.Ops.linear_attention takes it:
    to_qkv / sqrt(C) (q rows x qscale, k rows x kscale), to_out / sqrt(32) with `bias` added to its bias, norm parameters
    1 + 0.1 randn / 0.1 randn.  The draws from `gen` come in a fixed order."""
    wqkv = torch.randn((96, C, 1, 1, 1), generator=gen) / C ** 0.5
    wqkv[:32] *= qscale
    wqkv[32:64] *= kscale
    return {"fn.norm.weight": 1 + 0.1 * torch.randn(C, generator=gen), "fn.norm.bias": 0.1 * torch.randn(C, generator=gen),
            "fn.fn.to_qkv.conv.weight": wqkv, "fn.fn.to_out.0.conv.weight": torch.randn((C, 32, 1, 1, 1), generator=gen) / 32 ** 0.5,
            "fn.fn.to_out.0.conv.bias": 0.1 * torch.randn(C, generator=gen) + bias,
            "fn.fn.to_out.1.weight": 1 + 0.1 * torch.randn(C, generator=gen), "fn.fn.to_out.1.bias": 0.1 * torch.randn(C, generator=gen)}


def seeded_layer_models(cfg_name="dataset2", seed=SEED):
    """(ResNet layer model, CondUnet) with the parameters the reference's LayerDiffusion gets for torch.manual_seed(seed):
    the layer model is constructed first (layerdiffusion.py:35-40)."""
    from calodiffusion_amd.resnet import ResNet
    cfg = load_config(cfg_name)
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    layer = ResNet(dim_in=cfg["SHAPE_FINAL"][2] + 1, num_layers=5, cond_size=3 if cfg.get("HGCAL", False) else 1)
    unet = CondUnet(**unet_kwargs_from_config(cfg))
    torch.random.set_rng_state(state)
    return layer, unet
