#!/usr/bin/env python3
"""What the widening of narrow U-Net widths costs: the Dataset-1 pion config ([16, 16, 16, 32], run as [32, 32, 32, 32]) against
the same U-Net given directly as [32, 32, 32, 32] -- a plan without widening that does the same activation work.

    python tools/narrow_bench.py [--bin-file tests/golden/binning_ds0_synthetic.xml --denoise-batch 128 --train-batch 32
                                  --iters 30 --rounds 5]
Times cd_denoise, cd_train_step and a forced weight sync (cd_plan_set_weights: what follows every optimizer step) with device
events, the two plans interleaved round by round; reports the median round of each and the difference: nothing for denoise (the
same launches), the gradient fold for a training step, the widening stage for a weight sync.  One JSON line on stdout, with the
shader clock before and after where the box reports it."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from calodiffusion_amd.calodiffusion import CaloDiffusion  # noqa: E402
from calodiffusion_amd.configs import load_config  # noqa: E402


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def sclk_mhz():
    try:
        return int(torch.cuda.clock_rate())
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bin-file", default=os.path.join(ROOT, "tests", "golden", "binning_ds0_synthetic.xml"))
    ap.add_argument("--voxels", type=int, default=323, help="voxels of the binning file (533 for the CaloChallenge pion file)")
    ap.add_argument("--denoise-batch", type=int, default=128)
    ap.add_argument("--train-batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    base = dict(load_config("dataset1_pion"))
    base.update(BIN_FILE=a.bin_file, SHAPE_ORIG=[-1, a.voxels], SHAPE_PAD=[-1, 1, a.voxels])
    calls = {}
    gen = torch.Generator().manual_seed(0)
    for tag, widths in (("narrow", [16, 16, 16, 32]), ("wide", [32, 32, 32, 32])):
        cfg = dict(base, LAYER_SIZE_UNET=widths)
        torch.manual_seed(1234)
        m = CaloDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"])
        eng = m.engine()
        eng.safe_denoise = False  # cd_denoise itself (no stream synchronisation for the range flag)
        for kind, B in (("denoise", a.denoise_batch), ("train", a.train_batch)):
            x = torch.randn((B, a.voxels), generator=gen).cuda()
            n = torch.randn((B, a.voxels), generator=gen).cuda()
            sigma = torch.exp(torch.randn((B,), generator=gen) * 1.2 - 1.2).cuda()
            cond = m.cond_tensor(torch.rand((B, 1), generator=gen).cuda(), torch.randn((B, 8), generator=gen).cuda())
            if kind == "denoise":
                calls[(tag, kind)] = lambda eng=eng, x=x, sigma=sigma, cond=cond: eng.denoise(x, sigma, cond)
            else:
                calls[(tag, kind)] = lambda eng=eng, x=x, n=n, sigma=sigma, cond=cond: eng.train_step(x, n, sigma, cond, "l2")
        calls[(tag, "sync")] = lambda eng=eng: eng.sync_weights(force=True)
    clk0 = sclk_mhz()
    for fn in calls.values():  # kernels, autotune, workspaces
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, fn in calls.items():
            ms[k].append(timed(fn, a.iters))
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {"denoise_batch": a.denoise_batch, "train_batch": a.train_batch, "iters": a.iters, "rounds": a.rounds,
           "sclk_mhz_before": clk0, "sclk_mhz_after": sclk_mhz(), "device": torch.cuda.get_device_name(0)}
    for kind in ("denoise", "train", "sync"):
        nar, wid = med[("narrow", kind)], med[("wide", kind)]
        out[kind] = {"narrow_ms": round(nar, 4), "wide_ms": round(wid, 4), "difference_ms": round(nar - wid, 4),
                     "narrow_rounds_ms": [round(v, 4) for v in ms[("narrow", kind)]],
                     "wide_rounds_ms": [round(v, 4) for v in ms[("wide", kind)]]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
