"""What the HGCal in-model fixture (tools/gen_golden_hgcal_model.py), its host tests and its GPU tests share: the config, the
cases, the exact perturbation of geometry "t", and a restatement of the reference's embedded denoiser -- the CPU oracle's U-Net
between the two dense einsum maps of Embeder / Decoder (calodiffusion/utils/HGCal_utils.py:315-349) -- in any dtype."""
import numpy as np
import torch

from ds1_model_cases import LOSS_CASES, OBJECTIVES, OTHER_SAMPLERS, SIGMAS, TIME_EMBEDS, TRAJ_STEPS, eighths, rel_l2  # noqa: F401

LAYERS, CELLS, GRID = 8, 61, (8, 8, 8)
E_GRID = GRID[1] * GRID[2]
STATE = (1, LAYERS, CELLS)
# geometry "m": ragged cell counts, one layer with the centre cell only; rings 0 .. 7 (the tiny config's 8 radial bins)
NCELLS_M = (61, 47, 1, 53, 29, 61, 38, 17)
# geometry "t" (maps only): more than 256 cells a layer, rings up to 30 on 4 x 26 bins
BINS_T, NCELLS_T = (2, 4, 26), (300, 271)
RN = dict(emax=1000.0, emin=1.0, max_deposit=2, logE=True)  # the ReverseNormHGCal record's keywords


def config(objective="hybrid_weight", time_embed="log", **over):
    from calodiffusion_amd.configs import load_config
    cfg = dict(load_config("tiny"))
    cfg.update(SHOWER_EMBED="NN", SHAPE_PAD=[-1, 1, LAYERS, CELLS], TRAINABLE_EMBED=True, BIN_FILE="/nonexistent/geom.pkl",
               TRAINING_OBJ=objective, TIME_EMBED=time_embed)
    cfg.update(over)
    return cfg


def hashed_perturbation(shape):
    """A dense perturbation in [-0.125, 0.125) that every platform forms to the bit: multiples of 1/1024 from an integer hash
    of the element index (geometry "t": the fixture stores the initial maps, which compress; both sides add this)."""
    idx = np.arange(int(np.prod(shape)), dtype=np.uint64)
    k = ((idx * np.uint64(2654435761)) % np.uint64(1 << 32)) >> np.uint64(24)
    return ((k.astype(np.float64) - 128.0) / 1024.0).astype(np.float32).reshape(shape)


def masked(a, mask):
    """the entries of `a` under `mask`, in row-major order: how the fixture stores a map's gradient (it is 0 elsewhere)"""
    return np.asarray(a)[np.asarray(mask, dtype=bool)]


def enc_einsum(mat, x):
    """Embeder.forward: x (B, C, L, N) -> (B, C, L, E)"""
    return torch.einsum("l e n, b c l n -> b c l e", mat, x)


def dec_einsum(mat, z):
    """Decoder.forward: z (B, C, L, E) -> (B, C, L, N)"""
    return torch.einsum("l n e, b c l e -> b c l n", mat, z)


def oracle_denoise(cfg, sd, enc, dec, x, E, sigma, layers, dtype=torch.float32):
    """calodiffusion.py:154-169 with an HGCalConverter inside forward, in `dtype`: sd the U-Net's state_dict, enc (L, E, N) and
    dec (L, N, E) the effective maps (``mat * mask``); x (B, 1, L, N)."""
    from oracle import torch_oracle as O
    spec = O.spec_from_config(cfg)
    c = lambda v: v.to(dtype)  # noqa: E731
    sd = {k: c(v) for k, v in sd.items()}
    x, sigma = c(x), c(sigma).reshape(-1, 1, 1, 1)
    sd_ = 1.0 if "log" in cfg.get("NOISE_SCHED", "linear") else 0.5
    c_skip, c_out, c_in = O.edm_scalings(sigma, sd_)
    t_emb = O.time_embed(sigma.reshape(-1), cfg["TIME_EMBED"])
    B = x.shape[0]
    g = enc_einsum(c(enc), x * c_in).reshape((B, 1) + GRID)
    xin = c(O.add_rz_phi(g, cfg["DATASET_NUM"], cfg.get("R_Z_INPUT", False), cfg.get("PHI_INPUT", False)))
    cond = c(torch.cat([E, layers], dim=1))
    F = O.cond_unet_forward(sd, spec, xin, cond, t_emb)
    pred = dec_einsum(c(dec), F.reshape(B, 1, LAYERS, E_GRID))
    obj = cfg["TRAINING_OBJ"]
    if "noise_pred" in obj:
        return x - sigma * pred
    if "mean_pred" in obj:
        return pred
    return c_skip * x + c_out * pred


def oracle_loss(cfg, sd, enc, dec, data, E, noise, sigma, layers, loss_type, dtype=torch.float32):
    """models/loss.py:163-210 on the cell-space state"""
    data, noise, sigma = data.to(dtype), noise.to(dtype), sigma.to(dtype).reshape(-1, 1, 1, 1)
    out = oracle_denoise(cfg, sd, enc, dec, data + sigma * noise, E, sigma, layers, dtype)
    obj = cfg["TRAINING_OBJ"]
    if "noise_pred" in obj:
        pred, target, weight = (data - (data - sigma * out)) / sigma, noise, torch.ones_like(sigma)
    elif "mean_pred" in obj:
        pred, target, weight = out, data, 1.0 / sigma ** 2
    else:
        pred, target, weight = out, data, 1.0 + 1.0 / sigma ** 2
    if loss_type == "l2":
        return (weight * (pred - target) ** 2).sum() / (weight.mean() * data.numel())
    return {"l1": torch.nn.functional.l1_loss, "mse": torch.nn.functional.mse_loss,
            "huber": torch.nn.functional.smooth_l1_loss}[loss_type](target, pred)
