"""Sampler references that run on the CPU oracle, shared by the host tests, the device tests and tools/diag: an interpreter of the
step programs, the oracle behind a sampler's view of the model, the DPMAdaptive and SDE runs, and the comparison of one golden
sampler case.  (sampler_cases.py stays free of the oracle: the fixture generator imports it.)"""
import copy

import numpy as np
import torch

from conftest import rel_l2
from helpers import seeded_unet
from oracle import torch_oracle as O
from calodiffusion_amd.calodiffusion import CaloDiffusion
from calodiffusion_amd.configs import load_config


def interpret_program(prog, denoise, start, noise):
    """Host-side interpreter of a sampler step program (the semantics of cd_sampler_run, include/calodiff.h) in torch on the
    CPU, with the oracle as the denoiser: checks the program BUILDERS without a GPU."""
    from calodiffusion_amd.engine import SOP_DENOISE, SOP_LINCOMB, SOP_LINDIV, SOP_RANDN, SOP_RECORD
    bufs = [torch.zeros_like(start) for _ in range(prog.n_bufs)]
    bufs[0] = start * np.float32(prog.start_scale)
    n_steps = prog.coefs.shape[0]
    xs, x0s = [None] * n_steps, [None] * n_steps
    it = iter(noise)
    for i in range(n_steps):
        ops = prog.ops if prog.op_begin is None else prog.ops[prog.op_begin[i]:prog.op_begin[i + 1]]
        row = torch.from_numpy(prog.coefs[i])
        for kind, dst, src, col in ops:
            if kind in (SOP_LINCOMB, SOP_LINDIV):
                acc = row[col] * bufs[src[0]]
                for k in range(1, len(src)):
                    acc = acc + row[col + k] * bufs[src[k]]
                bufs[dst] = acc / row[col + len(src)] if kind == SOP_LINDIV else acc
            elif kind == SOP_DENOISE:
                bufs[dst] = denoise(bufs[src[0]], row[col])
            elif kind == SOP_RANDN:
                bufs[dst] = next(it)
            elif kind == SOP_RECORD:
                (xs if dst == 0 else x0s)[i] = bufs[src[0]]
    return bufs[0], xs, x0s


class OracleBackedModel:
    """What a sampler sees of CaloDiffusion -- denoise, nsteps, loss_function -- with the CPU oracle as the denoiser."""

    def __init__(self, cfg):
        self.om = O.OracleModel(cfg, seeded_unet("tiny").state_dict())
        self.host = CaloDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"])
        self.loss_function, self.nsteps = self.host.loss_function, self.host.nsteps

    def denoise(self, x, E=None, sigma=None, layers=None):
        with torch.no_grad():
            return self.om.denoise(x, E, sigma.reshape(-1), layers)


def dpm_adaptive_on_oracle(opts, n, rows=3, seed=41):
    """(inputs, final x, denoise calls, steps) of calodiffusion_amd.sample.DPMAdaptive run on the CPU oracle."""
    from calodiffusion_amd import sample
    cfg = copy.deepcopy(load_config("tiny"))
    cfg["SAMPLER_OPTIONS"] = opts
    gen = torch.Generator().manual_seed(seed)
    start = torch.randn((rows, 1, 8, 8, 8), generator=gen)
    E, layers = torch.rand((rows, 3), generator=gen), torch.randn((rows, 9), generator=gen)
    smp = sample.DPMAdaptive(cfg)
    x, _, _ = smp(OracleBackedModel(cfg), start, E, layers, n)
    return (start, E, layers), x, smp.denoise_calls, smp.steps_taken


SDE_CASES = [("DPMPPSDE", {}), ("DPMPPSDE", {"ETA": 1.0, "S_NOISE": 1.1}), ("DPMPPSDE", {"ETA": 0.6, "R": 0.4}),
             ("DPMPP2MSDE", {}), ("DPMPP2MSDE", {"ETA": 1.0}), ("DPMPP2MSDE", {"ETA": 0.7, "SOLVER": "midpoint", "S_NOISE": 0.9}),
             ("DPMPP3MSDE", {}), ("DPMPP3MSDE", {"ETA": 1.0}), ("DPMPP3MSDE", {"ETA": 0.5, "S_NOISE": 1.2})]


def sde_oracle_run(name, opts, den, start, sig, noise):
    """One SDE case on the CPU restatement (oracle/samplers_oracle.py) with the given unit normals."""
    from oracle import samplers_oracle as SO
    eta, s_noise = opts.get("ETA", 0.0), opts.get("S_NOISE", 1.0)
    if name == "DPMPPSDE":
        return SO.dpmpp_sde(den, start, sig, iter(noise), eta, s_noise, opts.get("R", 0.5))
    if name == "DPMPP2MSDE":
        return SO.dpmpp_2m_sde(den, start, sig, iter(noise), eta, s_noise, opts.get("SOLVER", "heun"))
    return SO.dpmpp_3m_sde(den, start, sig, iter(noise), eta, s_noise)


def check_sampler_case(tag, g, x, xs, x0s, tol):
    """Final tensor (where the reference's is finite) and the stored trajectory slots of one sampler case."""
    want = g[f"{tag}.x"]
    if np.isfinite(want).all():
        assert rel_l2(np.asarray(x), want) < tol, (tag, rel_l2(np.asarray(x), want))
    else:  # Heun / DPM2 divide by t_next = 0 on their last step (see calodiffusion_amd/sample.py): not finite here either
        assert not np.isfinite(np.asarray(x)).all(), tag
    for k in g.files:
        if k.startswith(tag + ".xs") and xs is not None:
            assert rel_l2(np.asarray(xs[int(k.split("xs")[1])]), g[k]) < tol, k
        if k.startswith(tag + ".x0s") and x0s is not None:
            assert rel_l2(np.asarray(x0s[int(k.split("x0s")[1])]), g[k]) < tol, k
