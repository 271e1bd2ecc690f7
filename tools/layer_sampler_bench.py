"""Time a step-program sampler on LayerDiffusion's layer stage (cd_layer_sampler_run, Heun) next to DDim (cd_layer_sample) at
batch 64 and 256: both are one launch per trajectory, so the figure of merit is the time per denoise call."""
import sys

import torch

sys.path.insert(0, ".")
from calodiffusion_amd import sample  # noqa: E402
from calodiffusion_amd.configs import load_config  # noqa: E402
from calodiffusion_amd.engine import SOP_DENOISE  # noqa: E402
from calodiffusion_amd.layerdiffusion import LayerDiffusion  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 50  # sampler steps
REPS = 5

cfg = load_config("dataset2")
cfg["LAYER_STEPS"] = N
torch.manual_seed(1234)
m = LayerDiffusion(cfg, n_steps=400, loss_type="l2")


def denoise_calls(smp):
    if isinstance(smp, sample.DDim):
        return N
    prog = smp.build(m, N, 0).finalize()
    per = [o[0] for o in prog.ops].count(SOP_DENOISE)
    return per * (prog.coefs.shape[0] if prog.op_begin is None else 1)


def time_ms(E, start):
    m.sample_layers(E, start=start, sample_offset=0)  # warm-up
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(REPS):
        m.sample_layers(E, start=start, sample_offset=0)
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / REPS


for B in (64, 256):
    E, start = torch.rand((B, 1)).cuda() + 0.5, torch.randn((B, 46)).cuda()
    per = {}
    for name in ("DDim", "Heun"):
        m.layer_sampler = sample.DDim(cfg) if name == "DDim" else sample.Heun(cfg)
        ms, calls = time_ms(E, start), denoise_calls(m.layer_sampler)
        per[name] = ms * 1e3 / calls
        print(f"B={B} {name}: {ms:.3f} ms per {N}-step trajectory, {calls} denoise calls, {per[name]:.1f} us per denoise", flush=True)
    print(f"B={B}: Heun / DDim per denoise = {per['Heun'] / per['DDim']:.3f}", flush=True)
