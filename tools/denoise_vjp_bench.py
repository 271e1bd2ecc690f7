#!/usr/bin/env python3
"""Event-timed cd_denoise, cd_denoise_vjp (with and without the parameter gradients) and cd_train_step on one config.

    python tools/denoise_vjp_bench.py [--config dataset2 --batches 32,64 --iters 20 --train-batch 32]
    python tools/denoise_vjp_bench.py --only vjp0 --batches 64 --iters 5     # input-only calls alone (for a kernel trace)
One JSON line per measurement on stdout.  The init-conv input-gradient kernel's own time comes from a kernel trace of this tool
(rocprofv3 --kernel-trace --stats: init_dgrad_kernel)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from calodiffusion_amd.calodiffusion import CaloDiffusion  # noqa: E402
from calodiffusion_amd.configs import load_config  # noqa: E402


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="dataset2")
    ap.add_argument("--batches", default="32,64")
    ap.add_argument("--train-batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default=None, choices=["denoise", "vjp", "vjp0", "train"])
    a = ap.parse_args()
    cfg = load_config(a.config)
    torch.manual_seed(1234)
    m = CaloDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"])
    eng = m.engine()
    eng.safe_denoise = False  # cd_denoise itself (no stream synchronisation for the range flag)
    gen = torch.Generator().manual_seed(0)
    kinds = [a.only] if a.only else ["denoise", "vjp", "vjp0", "train"]
    for B in (int(b) for b in a.batches.split(",")):
        shape = [B] + list(cfg["SHAPE_PAD"][1:])
        x = torch.randn(shape, generator=gen).cuda()
        gy = torch.randn(shape, generator=gen).cuda()
        sigma = torch.exp(torch.randn((B,), generator=gen) * 1.2 - 1.2).cuda()
        E = torch.rand((B, 1), generator=gen).cuda()
        layers = torch.randn((B, 1 + cfg["SHAPE_FINAL"][2]), generator=gen).cuda() if "layer" in cfg["SHOWERMAP"] else None
        cond = m.cond_tensor(E, layers)
        calls = {
            "denoise": lambda: eng.denoise(x, sigma, cond),
            "vjp": lambda: eng.denoise_vjp(x, sigma, cond, gy, param_grads=True),
            "vjp0": lambda: eng.denoise_vjp(x, sigma, cond, gy, param_grads=False),
            "train": lambda: eng.train_step(x, gy, sigma, cond, "l2"),
        }
        for k in kinds:
            if k == "train" and B != a.train_batch:
                continue
            ms = timed(calls[k], a.iters)
            print(json.dumps({"config": a.config, "batch": B, "call": {"denoise": "cd_denoise", "vjp": "cd_denoise_vjp(grads)",
                                                                      "vjp0": "cd_denoise_vjp(NULL)", "train": "cd_train_step"}[k],
                              "ms": round(ms, 4)}), flush=True)
    eng.check_status()


if __name__ == "__main__":
    main()
