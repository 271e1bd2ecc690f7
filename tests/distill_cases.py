"""Consistency distillation (calodiffusion_amd/distill.py): the definition restated on the CPU oracle, and the seeded models
and batches the host and GPU tests share."""
import numpy as np
import torch
import torch.nn.functional as F

from helpers import seeded_model
from oracle import torch_oracle as O

N_GRID = 40  # CONSIS_NSTEPS of every case (the sampler cases' own value)
LOSSES = {"mse": F.mse_loss, "l1": F.l1_loss, "huber": F.smooth_l1_loss}  # the reductions of CD_LOSS_MSE / L1 / HUBER


def frozen_teacher(name="tiny", over=None):
    m = seeded_model(name, dict({"CONSIS_NSTEPS": N_GRID}, **(over or {})))
    return m.requires_grad_(False)


def perturb_(model, seed, rel=0.05):
    """Every parameter tensor of ``model`` moved by ``rel`` of its own RMS (of 1 for a zero tensor) times seeded unit normals."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            rms = float(p.detach().float().pow(2).mean().sqrt()) or 1.0
            p.add_((rel * rms * torch.randn(p.shape, generator=gen)).to(p.device))
    return model


def oracle_of(model, grads=False):
    """The CPU oracle with ``model``'s present weights (private copies; ``grads``: leaves that take gradients)."""
    sd = {k[6:]: v.detach().cpu().clone().requires_grad_(grads) for k, v in model.state_dict().items() if k.startswith("model.")}
    return O.OracleModel(model.config, sd)


def batch(cfg, B, seed):
    """(data, noise, E, layers, index) on the CPU: one pair index per sample, all different while B <= N_GRID - 1."""
    gen = torch.Generator().manual_seed(seed)
    shape = [B] + list(cfg["SHAPE_PAD"][1:])
    data, noise = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    E = torch.rand((B, 3 if cfg.get("HGCAL") else 1), generator=gen)
    layers = torch.randn((B, 1 + cfg["SHAPE_FINAL"][2]), generator=gen) if "layer" in cfg["SHOWERMAP"] else None
    index = torch.randperm(N_GRID - 1, generator=gen)[:B]
    return data, noise, E, layers, index


def ode_formula(x_hi, d_hi, s_hi, s_lo, x_e=None, d_e=None):
    """The Euler x_lo, or with (x_e, D_e) the Heun x_lo, as the issue states them: one torch op per product, difference and
    quotient (fp32 on the CPU)."""
    view = (-1,) + (1,) * (x_hi.dim() - 1)
    s_hi, s_lo = s_hi.reshape(view), s_lo.reshape(view)
    d = (x_hi - d_hi) / s_hi
    if x_e is None:
        return x_hi + (s_lo - s_hi) * d
    d2 = (x_e - d_e) / s_lo
    return x_hi + (s_lo - s_hi) * (0.5 * (d + d2))


def oracle_step(om, x_hi, E, s_hi, layers, target, loss_type):
    """(loss, {name: gradient}, the oracle's output) of loss_type(denoise(x_hi, s_hi) - target) by autograd through the oracle.
    ``target``: a tensor, or a callable that makes one from the oracle's (detached) output."""
    out = om.denoise(x_hi, E, s_hi, layers)
    if callable(target):
        target = target(out.detach())
    loss = LOSSES[loss_type](out, target)
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in om.sd.items()}, out.detach()


def target_away_from(out, seed, floor=1e-2):
    """A random target -- unit normals, drawn without regard to ``out`` -- except where that leaves the residual out - target
    below ``floor`` in magnitude: there the target moves to 2 floor from out (l1's gradient is the residual's sign: an element
    within rounding of zero could flip it).  The residual is then of out's own size, so the denoiser's rounding is not amplified
    through the difference."""
    gen = torch.Generator().manual_seed(seed)
    target = torch.randn(out.shape, generator=gen)
    r = out - target
    return torch.where(r.abs() < floor, out - 2 * floor * torch.where(r < 0, -1.0, 1.0), target)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))
