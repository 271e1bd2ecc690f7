"""CPU: narrow U-Net widths -- the width rule, the channel map and its fold restated in narrow_cases.py, checked in float64 on the
CPU oracle's U-Net (which keeps a block's shortcut conv by its presence in the state_dict, so it expresses a 16 -> 32 block that
runs 32 -> 32); the oracle against the new fixtures; and construction of the pion config."""
import numpy as np
import pytest
import torch

from conftest import gold, rel_l2
from helpers import SEED, t, verify_checksums
from oracle import torch_oracle as O
import narrow_cases as N


@pytest.mark.parametrize("cg,k", N.RULE_TABLE)
def test_width_rule(cg, k):
    assert N.widen_factor(*cg) == k


@pytest.mark.parametrize("c,groups", [(8, 8), (16, 8), (24, 8), (48, 8), (16, 1), (32, 8)])
def test_channel_map_keeps_every_group_and_duplicates_inside_it(c, groups):
    k, cpg = N.widen_factor(c, groups), c // groups
    real, prim = N.channel_map(c, groups)
    assert len(real) == c * k and int(prim.sum()) == c
    assert sorted(real[prim].tolist()) == list(range(c))  # one primary per real channel
    for g in range(groups):  # a wide group holds its real group's channels, each k times
        seg = real[g * k * cpg:(g + 1) * k * cpg].tolist()
        assert sorted(seg) == sorted(list(range(g * cpg, (g + 1) * cpg)) * k)
    # GroupNorm statistics are those of the narrow tensor
    x = torch.randn(2, c, 5, dtype=torch.float64)
    a = torch.nn.functional.group_norm(x, groups).index_select(1, real)
    b = torch.nn.functional.group_norm(x.index_select(1, real), groups)
    assert float((a - b).abs().max()) < 1e-12


def _unet_case(cfg, seed):
    spec = O.spec_from_config(cfg)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((2, spec.channels) + tuple(spec.data_shape), generator=gen, dtype=torch.float64)
    cond = torch.randn((2, spec.cond_size), generator=gen, dtype=torch.float64)
    time = torch.rand((2,), generator=gen, dtype=torch.float64)
    cot = torch.randn((2, 1) + tuple(spec.data_shape), generator=gen, dtype=torch.float64)
    return spec, x, cond, time, cot


@pytest.mark.parametrize("name", ["pion", "tiny"])
def test_widened_forward_and_folded_gradients_equal_the_narrow_net_in_float64(name):
    """[16,16,16,32] on 7x10x23 and [16,16,32,64] on 8x8x8, parameters perturbed by 0.05 N(0,1), batch 2: forward and every
    gradient to 1e-12 (measured 1e-15 and 7e-15)"""
    cfg = N.config() if name == "pion" else N.tiny_config()
    sd = N.seeded_unet_sd(cfg, SEED, perturb=0.05, dtype=torch.float64)
    spec, x, cond, time, cot = _unet_case(cfg, 5)
    narrow = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    y = O.cond_unet_forward(narrow, spec, x, cond, time)
    (y * cot).sum().backward()
    wcfg = N.wide_config(cfg)
    assert wcfg["LAYER_SIZE_UNET"] == ([32, 32, 32, 32] if name == "pion" else [32, 32, 32, 64])
    wide = {k: v.clone().requires_grad_(True) for k, v in N.widen_state_dict(sd, cfg).items()}
    assert list(wide) == list(sd)  # a block keeps its shortcut by the config's widths
    if name == "pion":  # 522 753 parameters run as 1 239 713
        assert (sum(v.numel() for v in sd.values()), sum(v.numel() for v in wide.values())) == (N.PION_PARAMS, 1239713)
    yw = O.cond_unet_forward(wide, O.spec_from_config(wcfg), x, cond, time)
    (yw * cot).sum().backward()
    assert rel_l2(yw.detach().numpy(), y.detach().numpy()) < 1e-12
    folded = N.fold_grads({k: v.grad for k, v in wide.items()}, cfg)
    worst = max((rel_l2(folded[k].numpy(), v.grad.numpy()), k) for k, v in narrow.items() if float(v.grad.abs().max()) > 0)
    print(f"[{name}] forward {rel_l2(yw.detach().numpy(), y.detach().numpy()):.1e}, worst folded gradient {worst[0]:.1e} ({worst[1]})")
    assert worst[0] < 1e-12, worst
    for k, v in narrow.items():
        assert folded[k].shape == v.shape, k
    # expand and fold are transposes of each other: <expand(a), b> == <a, fold(b)>
    gen = torch.Generator().manual_seed(9)
    b = {k: torch.randn(v.shape, generator=gen, dtype=torch.float64) for k, v in wide.items()}
    lhs = sum(float((N.widen_state_dict(sd, cfg)[k] * b[k]).sum()) for k in sd)
    rhs = sum(float((sd[k] * N.fold_grads(b, cfg)[k]).sum()) for k in sd)
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)


def test_pion_model_constructs_with_the_reference_weights():
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    g = gold("narrow_pion")
    cfg = N.config()
    state = torch.random.get_rng_state()
    torch.manual_seed(SEED)
    m = CaloDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"])
    torch.random.set_rng_state(state)
    assert m.do_embed and m._data_shape == [N.V]
    assert sum(p.numel() for p in m.model.parameters()) == N.PION_PARAMS
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["sd_keys"]]
    verify_checksums(sd, g)
    gc = m.NN_embed.gc
    assert (gc.num_layers, int(gc.alpha_out), gc.dim_r_out) == N.GRID
    bound, alpha, rin = N.layout(gc)
    assert bound[-1] == N.V and alpha == [1, 10, 10, 10, 1, 10, 1] and rin == [5, 9, 11, 6, 5, 5, 3]
    assert g["xml.relevant"].tolist() == [0, 1, 2, 3, 5, 6, 7] and int(g["xml.total"]) == N.V


def test_pion_config_carries_the_reference_values():
    from calodiffusion_amd.configs import load_config
    cfg = load_config("dataset1_pion")
    assert cfg["LAYER_SIZE_UNET"] == [16, 16, 16, 32] and cfg["DATASET_NUM"] == 0 and cfg["PART_TYPE"] == "pion"
    assert cfg["SHAPE_FINAL"] == [-1, 1, 7, 10, 23] and cfg["SHAPE_ORIG"] == [-1, 533] and cfg["SHOWER_EMBED"] == "orig-NN"


# ---- the oracle against the fixtures (test_oracle_golden.py's bounds: 2e-6 a forward and a loss, 2e-5 a gradient tensor) ------
def _pion_oracle(g, objective, time_embed):
    cfg = N.config(objective, time_embed)
    sd = N.seeded_unet_sd(cfg, SEED)
    Ws = [t(g[f"nn.encs.{i}.weight"]) for i in range(N.GRID[0])]
    Ds = [t(g[f"nn.decs.{i}.weight"]) for i in range(N.GRID[0])]
    lay = (g["lay.bound"].tolist(), g["lay.alpha"].tolist(), g["lay.rin"].tolist())
    return cfg, sd, Ws, Ds, lay


@pytest.mark.parametrize("objective", N.OBJECTIVES)
def test_oracle_reproduces_the_pion_denoise(objective):
    g = gold("narrow_pion")
    cfg, sd, Ws, Ds, lay = _pion_oracle(g, objective, "log")
    with torch.no_grad():
        y = N.oracle_denoise(cfg, sd, Ws, Ds, lay, t(g["x"]), t(g["E"]), t(g["sigma"]), t(g["layers"]))
    err = rel_l2(y.numpy(), g[f"den.{objective}.log.b3"])
    print(f"[{objective}] oracle against the reference: {err:.2e}")
    assert err < 2e-6


def test_oracle_reproduces_the_pion_loss_and_gradients():
    g, gg = gold("narrow_pion"), gold("narrow_pion_grads")
    cfg, sd, Ws, Ds, lay = _pion_oracle(g, "hybrid_weight", "log")
    sd = {k: v.requires_grad_(True) for k, v in sd.items()}
    sigma = (t(g["rnd_normal"]) * 1.2 - 1.2).exp()  # hybrid_weight: P_mean = -1.2, P_std = 1.2 (models/loss.py)
    loss = N.oracle_loss(cfg, sd, Ws, Ds, lay, t(g["data"]), t(g["E"]), t(g["noise"]), sigma, t(g["layers"]), "l2")
    loss.backward()
    want = float(gg["loss.hybrid_weight.l2.loss"])
    assert abs(float(loss.detach()) - want) <= 2e-6 * abs(want)
    for k in gg.files:
        if k.startswith("loss.hybrid_weight.l2.grad."):
            err = rel_l2(sd[k[len("loss.hybrid_weight.l2.grad."):]].grad.numpy(), gg[k])
            assert err < 2e-5, (k, err)


def test_oracle_reproduces_the_narrow_tiny_record():
    g = gold("narrow_tiny")
    cfg = N.tiny_config()
    sd = {k: v.requires_grad_(True) for k, v in N.seeded_unet_sd(cfg, SEED).items()}
    verify_checksums({"model." + k: v.detach() for k, v in sd.items()}, g)
    om = O.OracleModel(cfg, sd)
    with torch.no_grad():
        y = om.denoise(t(g["x"]), t(g["E"]), t(g["sigma"]), t(g["layers"]))
    assert rel_l2(y.numpy(), g["den.b2"]) < 2e-6
    loss = om.hybrid_l2_loss(t(g["data"]), t(g["E"]), t(g["noise"]), t(g["layers"]), rnd_normal=t(g["rnd_normal"]))
    loss.backward()
    want = float(g["loss.loss"])
    assert abs(float(loss.detach()) - want) <= 2e-6 * abs(want)
    for k in g.files:
        if k.startswith("loss.grad."):
            err = rel_l2(om.sd[k[len("loss.grad."):]].grad.numpy(), g[k])
            assert err < 2e-5, (k, err)
