"""Time cd_preprocess (calodiffusion_amd.preprocess), event-timed: 4096 Dataset-2 showers ('layer-logit-norm') and 1024 Dataset-3
showers ('logit-norm'), and a device-to-device copy of the same bytes for scale.  Prints ms per call (best of the rounds),
the implied TB/s over read + write bytes of the voxel tensor, and the share of the copy's rate.

    python tools/preprocess_bench.py [reps]"""
import ctypes as C
import sys

import torch

sys.path.insert(0, ".")
from calodiffusion_amd import engine  # noqa: E402
from calodiffusion_amd.configs import load_config  # noqa: E402
from calodiffusion_amd.postprocess import DATASET_PARAMS  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
ROUNDS = 3
lib = engine.load_library()
engine.require_gpu()


def timed(fn):
    fn()  # warm-up
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(ROUNDS):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(REPS):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        best = min(best, ev[0].elapsed_time(ev[1]) / REPS)
    return best


for name, B, p_zero in (("dataset2", 4096, 0.65), ("dataset3", 1024, 0.88)):
    cfg = load_config(name)
    D, H, W = cfg["SHAPE_PAD"][2:]
    N = D * H * W
    gen = torch.Generator(device="cuda").manual_seed(7)
    raw = torch.rand((B, N), generator=gen, device="cuda") * 50.0 + 0.02
    raw[torch.rand((B, N), generator=gen, device="cuda") < p_zero] = 0.0
    e = 10.0 ** (3.0 + 3.0 * torch.rand((B,), generator=gen, device="cuda"))
    raw *= (0.8 * e / raw.sum(dim=1))[:, None]
    out = torch.empty((B, 1, D, H, W), device="cuda")
    layerE = torch.empty((B, D + 1), device="cuda") if "layer" in cfg["SHOWERMAP"] else None
    e_out, status = torch.empty((B, 1), device="cuda"), torch.zeros((1,), dtype=torch.int32, device="cuda")
    c = DATASET_PARAMS[cfg["DATASET_NUM"]]
    consts = (C.c_float * 6)(c["logit_mean"], c["logit_std"], c["totalE_mean"], c["totalE_std"], c["layers_mean"], c["layers_std"])
    dims = (C.c_int32 * 3)(D, H, W)

    def call():
        engine._check(lib.cd_preprocess(raw.data_ptr(), e.data_ptr(), out.data_ptr(), engine._ptr(layerE), e_out.data_ptr(),
                                        status.data_ptr(), B, dims, consts, float(cfg["MAXDEP"]), float(cfg["EMIN"]),
                                        float(cfg["EMAX"]), int(cfg["logE"]), 0.001, engine._stream()))

    ms = timed(call)
    assert int(status.item()) == 0 and bool(torch.isfinite(out).all())
    ms_copy = timed(lambda: out.view(B, N).copy_(raw))
    tb = 2 * 4 * B * N / 1e12
    print(f"{name}: B={B} ({4 * B * N / 1e6:.1f} MB in, as much out): cd_preprocess {ms:.4f} ms = {tb / ms * 1e3:.2f} TB/s over "
          f"read + write; copy of the same bytes {ms_copy:.4f} ms = {tb / ms_copy * 1e3:.2f} TB/s; share of the copy's rate "
          f"{ms_copy / ms:.2f}", flush=True)
