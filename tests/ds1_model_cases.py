"""What the Dataset-1 model fixture (tools/gen_golden_ds1_model.py), its host tests and its GPU tests share: the synthetic
geometry, the config, the cases, and a restatement of the reference's embedded denoiser -- the CPU oracle's U-Net between two
per-layer ``matmul`` maps -- in any dtype."""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
XML = os.path.join(HERE, "golden", "binning_ds1_synthetic.xml")
V, GRID = 368, (5, 10, 30)
OBJECTIVES = ("hybrid_weight", "noise_pred", "mean_pred")
TIME_EMBEDS = ("log", "sigma")
# (objective, loss type) of the stored losses and gradients
LOSS_CASES = (("hybrid_weight", "l2"), ("hybrid_weight", "huber"), ("noise_pred", "l2"), ("mean_pred", "l2"))
SIGMAS = (40.0, 1.0, 0.03125)
TRAJ_STEPS = 4
# the reference samplers the generator tries on the flat state, beyond DDim and DDPM: (tag, class name, steps, config overrides)
OTHER_SAMPLERS = (("euler", "Euler", 4, {}), ("heun", "Heun", 4, {}), ("dpm2", "DPM2", 4, {}), ("lms", "LMS", 5, {}),
                  ("dpmpp2m", "DPMPP2M", 5, {}), ("dpmpp2s", "DPMPP2S", 4, {}), ("dpm", "DPM", 4, {}))


def config(objective="hybrid_weight", time_embed="log", **over):
    from calodiffusion_amd.configs import load_config
    cfg = dict(load_config("dataset1_photon"))
    cfg.update(BIN_FILE=XML, TRAINING_OBJ=objective, TIME_EMBED=time_embed)
    cfg.update(over)
    return cfg


def layout(gc):
    """(bound, alpha, rin) of a GeomConverter (ours or the reference's)"""
    bound = [int(b) for b in gc.layer_boundaries]
    alpha = [int(a) for a in gc.lay_alphas]
    rin = [len(e) - 1 for e in gc.lay_r_edges]
    return bound, alpha, rin


def enc_matmul(x, Ws, bound, alpha, A):
    """NNConverter.enc as per-layer matmuls: x (B, V) -> (B, 1, L, A, R)"""
    out = []
    for i, W in enumerate(Ws):
        o = x[:, bound[i]:bound[i + 1]].reshape(x.shape[0], alpha[i], -1) @ W.T
        if alpha[i] == 1:
            o = o.expand(-1, A, -1) / A
        out.append(o)
    return torch.stack(out, dim=1).unsqueeze(1)


def dec_matmul(g, Ds, alpha):
    """NNConverter.dec: g (B, 1, L, A, R) -> (B, V)"""
    out = []
    for i, D in enumerate(Ds):
        o = g[:, 0, i] @ D.T
        if alpha[i] == 1:
            o = o.sum(dim=-2, keepdim=True)
        out.append(o.reshape(g.shape[0], -1))
    return torch.cat(out, dim=1)


def oracle_denoise(cfg, sd, Ws, Ds, lay, x, E, sigma, layers, dtype=torch.float32):
    """calodiffusion.py:154-169 with an NN_embed, in `dtype`: sd the U-Net's state_dict, Ws / Ds the matrices."""
    from oracle import torch_oracle as O
    bound, alpha, _ = lay
    spec = O.spec_from_config(cfg)
    c = lambda v: v.to(dtype)  # noqa: E731
    sd = {k: c(v) for k, v in sd.items()}
    x, sigma = c(x), c(sigma).reshape(-1, 1)
    sd_ = 1.0 if "log" in cfg.get("NOISE_SCHED", "linear") else 0.5
    c_skip, c_out, c_in = O.edm_scalings(sigma, sd_)
    t_emb = O.time_embed(sigma.reshape(-1), cfg["TIME_EMBED"])
    g = enc_matmul(x * c_in, [c(w) for w in Ws], bound, alpha, GRID[1])
    xin = c(O.add_rz_phi(g, cfg["DATASET_NUM"], cfg.get("R_Z_INPUT", False), cfg.get("PHI_INPUT", False)))
    cond = c(torch.cat([E, layers], dim=1))
    pred = dec_matmul(O.cond_unet_forward(sd, spec, xin, cond, t_emb), [c(d) for d in Ds], alpha)
    obj = cfg["TRAINING_OBJ"]
    if "noise_pred" in obj:
        return x - sigma * pred
    if "mean_pred" in obj:
        return pred
    return c_skip * x + c_out * pred


def oracle_loss(cfg, sd, Ws, Ds, lay, data, E, noise, sigma, layers, loss_type, dtype=torch.float32):
    """models/loss.py:163-210 on the flat state"""
    data, noise, sigma = data.to(dtype), noise.to(dtype), sigma.to(dtype).reshape(-1, 1)
    out = oracle_denoise(cfg, sd, Ws, Ds, lay, data + sigma * noise, E, sigma, layers, dtype)
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


def eighths(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).to(torch.float32) / 8.0


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


_models = {}


def model(objective="hybrid_weight", time_embed="log", loss_type="l2", fresh=False):
    """The seeded model with the fixture's perturbed NN_embed matrices (one per case, shared by the tests that only read it)."""
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    from conftest import gold
    from helpers import SEED, t
    key = (objective, time_embed, loss_type)
    if fresh or key not in _models:
        cfg = config(objective, time_embed, LOSS_TYPE=loss_type)
        torch.manual_seed(SEED)
        m = CaloDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=loss_type)
        g = gold("ds1_model")
        m.NN_embed.load_state_dict({k[3:]: t(g[k]) for k in g.files if k.startswith("nn.")})
        m.eval()
        if fresh:
            return m
        _models[key] = m
    return _models[key]


def inputs(*names):
    from conftest import gold
    from helpers import t
    g = gold("ds1_model")
    return [t(g[n]).cuda() for n in names]
