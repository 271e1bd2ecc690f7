"""What the narrow-width fixture (tools/gen_golden_narrow.py), its host tests and its GPU tests share: the synthetic pion
geometry, the configs, the cases, and a restatement of the plan's widening -- the width rule, the channel map, the widened
``state_dict`` and the fold of its gradients -- as index operations on a ``state_dict``.

The map (DESIGN, "Narrow U-Net widths"): a config width C with G GroupNorm groups runs as Cw = C k.  With cpg = C / G, wide channel
j lies in group j // (k cpg) at w = j % (k cpg); it holds real channel g cpg + w % cpg and is copy number w // cpg.  Along an output
axis every copy carries the real channel's values, along an input axis copy 0 carries the real column and the others are zero.  The
fold is the transpose: the sum over the copies of an output axis, the primary column of an input axis."""
import os

import torch

import ds1_model_cases as K1
from ds1_model_cases import eighths, layout, oracle_denoise, oracle_loss, rel_l2  # noqa: F401  (alpha_out is 10 in both geometries)

HERE = os.path.dirname(os.path.abspath(__file__))
XML = os.path.join(HERE, "golden", "binning_ds0_synthetic.xml")
V, GRID = 323, (7, 10, 23)
PION_PARAMS = 522753
OBJECTIVES, TIME_EMBEDS, LOSS_CASES, SIGMAS, TRAJ_STEPS = K1.OBJECTIVES, K1.TIME_EMBEDS, K1.LOSS_CASES, K1.SIGMAS, K1.TRAJ_STEPS
TINY_WIDTHS = [16, 16, 32, 64]   # the record without an embedding, on the 8x8x8 grid of `tiny`
MAP_WIDTHS = [16, 16, 16, 16]    # device map = restated map: no shortcut conv on either side
# the width rule over a table: (C, G) -> k, 0 = refused
RULE_TABLE = (((8, 8), 4), ((16, 8), 2), ((24, 8), 4), ((48, 8), 2), ((32, 8), 1), ((64, 8), 1), ((96, 8), 1), ((20, 8), 0),
              ((136, 8), 0), ((288, 8), 0), ((16, 1), 2), ((12, 4), 0), ((16, 16), 4), ((256, 8), 1))


def config(objective="hybrid_weight", time_embed="log", **over):
    """the pion config over the synthetic binning file"""
    from calodiffusion_amd.configs import load_config
    cfg = dict(load_config("dataset1_pion"))
    cfg.update(BIN_FILE=XML, SHAPE_ORIG=[-1, V], SHAPE_PAD=[-1, 1, V], TRAINING_OBJ=objective, TIME_EMBED=time_embed)
    cfg.update(over)
    return cfg


def tiny_config(widths=None, **over):
    from calodiffusion_amd.configs import load_config
    cfg = dict(load_config("tiny"))
    cfg.update(LAYER_SIZE_UNET=list(widths or TINY_WIDTHS))
    cfg.update(over)
    return cfg


def widen_factor(c, groups):
    """the smallest k of {1, 2, 4} with C % G == 0, C k % 32 == 0, (C k / G) % 4 == 0 and C k <= 256; 0: refused"""
    if c <= 0 or c % groups:
        return 0
    for k in (1, 2, 4):
        if (c * k) % 32 == 0 and ((c * k) // groups) % 4 == 0 and c * k <= 256:
            return k
    return 0


def wide_widths(widths, groups):
    ks = [widen_factor(c, groups) for c in widths]
    assert all(ks), (widths, groups)
    return [c * k for c, k in zip(widths, ks)]


def channel_map(c, groups):
    """(real channel of every wide channel, whether it is the primary copy), both of length C k"""
    k, cpg = widen_factor(c, groups), c // groups
    j = torch.arange(c * k)
    w = j % (k * cpg)
    return (j // (k * cpg)) * cpg + w % cpg, (w // cpg) == 0


def key_axes(cfg):
    """{state_dict key of the U-Net: (output width or None, [input widths] or None, input axis first)} for the keys with a U-Net
    width on an axis; widths as the config states them.  Every other key (and axis) stays as it is."""
    L = list(cfg["LAYER_SIZE_UNET"])
    nres = len(L) - 1
    ax = {}

    def res(pre, cins, cout, mlp=True):
        if mlp:
            ax[pre + ".mlp.1.weight"] = ax[pre + ".mlp.1.bias"] = (cout, None, False)
        ax[pre + ".block1.proj.conv.weight"] = (cout, cins, False)
        ax[pre + ".block2.proj.conv.weight"] = (cout, [cout], False)
        for b in ("block1", "block2"):
            for leaf in ("proj.conv.bias", "norm.weight", "norm.bias"):
                ax[f"{pre}.{b}.{leaf}"] = (cout, None, False)
        if sum(cins) != cout:  # the shortcut is kept or dropped by the config's widths
            ax[pre + ".res_conv.conv.weight"] = (cout, cins, False)
            ax[pre + ".res_conv.conv.bias"] = (cout, None, False)

    def attn(pre, c):
        ax[pre + ".fn.fn.to_qkv.conv.weight"] = (None, [c], False)
        for leaf in ("fn.fn.to_out.0.conv.weight", "fn.fn.to_out.0.conv.bias", "fn.fn.to_out.1.weight", "fn.fn.to_out.1.bias",
                     "fn.norm.weight", "fn.norm.bias"):
            ax[f"{pre}.{leaf}"] = (c, None, False)

    ax["init_conv.conv.weight"] = ax["init_conv.conv.bias"] = (L[0], None, False)
    for i in range(nres):
        ci, co = L[i], L[i + 1]
        res(f"downs.{i}.0", [ci], co)
        res(f"downs.{i}.1", [co], co)
        if i + 1 < nres:
            ax[f"downs.{i}.2.conv.weight"] = (co, [co], False)
            ax[f"downs.{i}.2.conv.bias"] = (co, None, False)
        if cfg.get("BLOCK_ATTN", False):
            attn(f"downs_attn.{i}", co)
    for i in range(nres):
        ci, co = L[nres - 1 - i], L[nres - i]
        res(f"ups.{i}.0", [co, co], ci)  # cat(x, skip): two segments, each with its own map
        res(f"ups.{i}.1", [ci], ci)
        if i + 1 < nres:
            ax[f"ups.{i}.2.convTrans.weight"] = (ci, [ci], True)
            ax[f"ups.{i}.2.convTrans.bias"] = (ci, None, False)
        if cfg.get("BLOCK_ATTN", False):
            attn(f"ups_attn.{i}", ci)
    res("mid_block1", [L[-1]], L[-1])
    res("mid_block2", [L[-1]], L[-1])
    if cfg.get("MID_ATTN", False):
        attn("mid_attn", L[-1])
    res("final_conv.0", [L[1]], L[0], mlp=False)
    ax["final_conv.1.conv.weight"] = (None, [L[0]], False)
    return ax


def _in_map(cins, groups):
    """the concatenated input axis: real column of every wide column, the primary mask, and the wide column of every real one"""
    real, prim, base = [], [], 0
    for c in cins:
        r, p = channel_map(c, groups)
        real.append(r + base)
        prim.append(p)
        base += c
    real, prim = torch.cat(real), torch.cat(prim)
    return real, prim, torch.nonzero(prim).flatten()[torch.argsort(real[prim])]


def widen_state_dict(sd, cfg):
    """the U-Net state_dict the plan runs: every tensor expanded by the map"""
    groups, out = cfg.get("BLOCK_GROUPS", 8), {}
    axes = key_axes(cfg)
    for key, v in sd.items():
        co, cins, in_first = axes.get(key, (None, None, False))
        o_ax, i_ax = (1, 0) if in_first else (0, 1)
        if co is not None:
            v = v.index_select(o_ax, channel_map(co, groups)[0])
        if cins is not None:
            real, prim, _ = _in_map(cins, groups)
            shape = [1] * v.dim()
            shape[i_ax] = -1
            v = v.index_select(i_ax, real) * prim.to(v.dtype).reshape(shape)
        out[key] = v.contiguous()
    return out


def fold_grads(wide, cfg):
    """the transpose of widen_state_dict on a dict of gradients"""
    groups, out = cfg.get("BLOCK_GROUPS", 8), {}
    axes = key_axes(cfg)
    for key, g in wide.items():
        co, cins, in_first = axes.get(key, (None, None, False))
        o_ax, i_ax = (1, 0) if in_first else (0, 1)
        if cins is not None:
            g = g.index_select(i_ax, _in_map(cins, groups)[2])
        if co is not None:
            shape = list(g.shape)
            shape[o_ax] = co
            g = torch.zeros(shape, dtype=g.dtype).index_add_(o_ax, channel_map(co, groups)[0], g)
        out[key] = g.contiguous()
    return out


def wide_config(cfg):
    return dict(cfg, LAYER_SIZE_UNET=wide_widths(cfg["LAYER_SIZE_UNET"], cfg.get("BLOCK_GROUPS", 8)))


def seeded_unet_sd(cfg, seed, perturb=0.0, dtype=torch.float32):
    """state_dict of our parameter holder for cfg's U-Net after manual_seed(seed) (the reference's initialisation), optionally with
    every parameter perturbed by perturb N(0, 1) from a second generator; the global RNG is left as it was"""
    from calodiffusion_amd.unet import CondUnet, unet_kwargs_from_config
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    net = CondUnet(**unet_kwargs_from_config(cfg))
    torch.random.set_rng_state(state)
    gen = torch.Generator().manual_seed(seed + 1)
    return {k: (v.detach() + perturb * torch.randn(v.shape, generator=gen)).to(dtype) for k, v in net.state_dict().items()}


def grid_oracle_loss(cfg, sd, data, E, noise, sigma, layers, dtype=torch.float32):
    """hybrid_weight 'l2' loss of a model without an embedding (calodiffusion.py:154-169, models/loss.py:163-179) in `dtype`"""
    from oracle import torch_oracle as O
    c = lambda v: v.to(dtype)  # noqa: E731
    sd = {k: c(v) for k, v in sd.items()}
    data, noise, sigma = c(data), c(noise), c(sigma).reshape(-1, 1, 1, 1, 1)
    x = data + sigma * noise
    c_skip, c_out, c_in = O.edm_scalings(sigma, 1.0 if "log" in cfg.get("NOISE_SCHED", "linear") else 0.5)
    t_emb = c(O.time_embed(sigma.reshape(-1), cfg["TIME_EMBED"]))
    xin = c(O.add_rz_phi(x * c_in, cfg["DATASET_NUM"], cfg.get("R_Z_INPUT", False), cfg.get("PHI_INPUT", False)))
    out = c_skip * x + c_out * O.cond_unet_forward(sd, O.spec_from_config(cfg), xin, c(torch.cat([E, layers], dim=1)), t_emb)
    weight = 1.0 + 1.0 / sigma ** 2
    return (weight * (out - data) ** 2).sum() / (weight.mean() * data.numel())
