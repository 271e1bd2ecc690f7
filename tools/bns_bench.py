"""Time BespokeNonStationary on Dataset-3 (TIME_EMBED 'sigma'), event-timed, the variants back to back:
  1. ms per sampling step: BNS (DENOISE_PS + LINCOMB, one captured step graph) against DPMPP2M (one denoise per step as well),
     B = 32, N steps;
  2. ms per cd_bns_theta_grad at N = 8 against N x cd_denoise + (N - 1) x input-only cd_denoise_vjp at the same shape."""
import os
import sys
import tempfile

import torch

sys.path.insert(0, ".")
from calodiffusion_amd import sample  # noqa: E402
from calodiffusion_amd.calodiffusion import CaloDiffusion  # noqa: E402
from calodiffusion_amd.configs import load_config  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
N = int(sys.argv[2]) if len(sys.argv) > 2 else 20  # sampling steps
NG = 8  # theta-gradient steps
REPS = 5

cfg = load_config("dataset3")
torch.manual_seed(1234)
m = CaloDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"])
shape = [B] + list(cfg["SHAPE_PAD"][1:])
start = torch.randn(shape).cuda()
E = torch.rand((B, 1)).cuda()
layers = torch.randn((B, 1 + cfg["SHAPE_FINAL"][2])).cuda() if "layer" in cfg["SHOWERMAP"] else None
cond = m.cond_tensor(E, layers)


def timed(fn):
    fn()  # warm-up (graph capture, workspace)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(REPS):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / REPS


tmp = tempfile.mkdtemp()
theta = torch.stack([torch.full((N,), 0.9), torch.full((N,), 0.3)])
torch.save(torch.nn.Parameter(theta), os.path.join(tmp, "bns.pth"))
c = dict(cfg, SAMPLER_OPTIONS={"SAMPLER_PATH": os.path.join(tmp, "bns.pth")})
bns = sample.BespokeNonStationary(c)
dpm = sample.DPMPP2M(dict(cfg))
per = {}
for name, smp in (("BNS", bns), ("DPMPP2M", dpm), ("BNS", bns), ("DPMPP2M", dpm)):
    m.noise_offset = 0
    ms = timed(lambda: smp(m, start, E, layers, N, 0, False))
    per.setdefault(name, []).append(ms / N)
    print(f"B={B} {name}: {ms:.3f} ms per {N}-step trajectory, {ms / N:.3f} ms per step", flush=True)
bns_ms, dpm_ms = min(per["BNS"]), min(per["DPMPP2M"])
print(f"B={B}: BNS / DPMPP2M per step = {bns_ms / dpm_ms:.4f}", flush=True)

eng = m.engine()
th = torch.stack([torch.full((NG,), 0.9), torch.full((NG,), 0.3)]).cuda()
sig = torch.randn((NG, B)).cuda().abs() + 0.1
data = start.abs() + 0.05
gy = torch.randn(shape).cuda()
grad_ms = timed(lambda: eng.bns_theta_grad(data, cond, th, sig))


def parts():
    for i in range(NG):
        eng.denoise(data, sig[i], cond)
    for i in range(NG - 1):
        eng.denoise_vjp(data, sig[i], cond, gy, param_grads=False)


parts_ms = timed(parts)
grad_ms = min(grad_ms, timed(lambda: eng.bns_theta_grad(data, cond, th, sig)))
print(f"B={B} N={NG}: cd_bns_theta_grad {grad_ms:.3f} ms; {NG} x denoise + {NG - 1} x input-only VJP {parts_ms:.3f} ms; "
      f"ratio {grad_ms / parts_ms:.4f}", flush=True)
