#!/usr/bin/env python3
"""Event-timed gradient calls of LayerDiffusion's layer model (dataset 2): cd_layer_denoise, cd_layer_denoise_vjp with and without
the parameter gradients, cd_layer_train_step and cd_layer_loss at batch 64 and 256.

    python tools/layer_vjp_bench.py [--batches 64,256 --iters 50 --rounds 2]
    python tools/layer_vjp_bench.py --only train      # one call alone (an A/B library through CALODIFF_LIB, or a kernel trace)
The calls are timed in alternation, `rounds` times over, and the best round of each is kept; one JSON line per call and batch,
then the three ratios DESIGN.md section 5 quotes."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from calodiffusion_amd.configs import load_config  # noqa: E402
from calodiffusion_amd.layerdiffusion import LayerDiffusion  # noqa: E402

NAMES = {"denoise": "cd_layer_denoise", "vjp": "cd_layer_denoise_vjp(grads)", "vjp0": "cd_layer_denoise_vjp(NULL)",
         "train": "cd_layer_train_step", "loss": "cd_layer_loss"}


def timed(fn, iters, warmup=5):
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--only", default=None, choices=sorted(NAMES))
    a = ap.parse_args(argv)
    cfg = load_config("dataset2")
    torch.manual_seed(1234)
    m = LayerDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type="l2")
    m.set_layer_state(True)
    eng = m.engine()
    gen = torch.Generator().manual_seed(0)
    kinds = [a.only] if a.only else list(NAMES)
    out = {}
    for B in (int(b) for b in a.batches.split(",")):
        x = torch.randn((B, eng.dim), generator=gen).cuda()
        gy = torch.randn((B, eng.dim), generator=gen).cuda()
        sigma = torch.exp(torch.randn((B,), generator=gen) * 1.2 - 1.2).cuda()
        E = torch.rand((B, 1), generator=gen).cuda()
        calls = {
            "denoise": lambda: eng.denoise(x, sigma, E),
            "vjp": lambda: eng.denoise_vjp(x, sigma, E, gy, param_grads=True),
            "vjp0": lambda: eng.denoise_vjp(x, sigma, E, gy, param_grads=False),
            "train": lambda: eng.train_step(x, gy, sigma, E, "l2"),
            "loss": lambda: eng.loss(x, gy, sigma, E, "l2"),
        }
        best = {}
        for _ in range(a.rounds):
            for k in kinds:
                ms = timed(calls[k], a.iters)
                best[k] = min(ms, best.get(k, ms))
        for k in kinds:
            out[(k, B)] = best[k]
            print(json.dumps({"batch": B, "call": NAMES[k], "ms": round(best[k], 4)}), flush=True)
        if not a.only:
            print(json.dumps({"batch": B, "vjp(grads) / train_step": round(best["vjp"] / best["train"], 3),
                              "vjp(NULL) / vjp(grads)": round(best["vjp0"] / best["vjp"], 3),
                              "loss / train_step": round(best["loss"] / best["train"], 3)}), flush=True)
    return out


if __name__ == "__main__":
    main()
