#!/usr/bin/env python3
"""Time of one consistency-distillation step (ConsistencyDistillation.step: teacher and target denoise calls, the ODE step,
cd_train_step_target, FusedAdam, the EMA) on Dataset-2 for both solvers, beside what it is made of on the same box:

    python tools/distill_bench.py [--batch 32 --repeats 10 --timeout 300 --out profiles/distill_bench.json]

  parts    the ordinary training step (zero_grad -> compute_loss -> backward -> FusedAdam.step, bench.py --mode train's loop) and
           one denoise call at that batch
  euler    step() with CONSIS_SOLVER 'euler':  expectation = training step + 2 denoise calls (teacher, target)
  heun     step() with CONSIS_SOLVER 'heun':   expectation = training step + 3 denoise calls (teacher twice, target)

The expectation is a yardstick, not a gate: a step above 1.15 x of it (the box-to-box spread of profiles/README.md) points at the
new kernels or at a hidden synchronisation.  Every case runs in a process of its own under --timeout (a case that fails or runs
out of time ends the run: nothing more is started on the GPU); each has one warm-up step and --repeats timed ones between two
synchronisations, the shader clock and socket power sampled meanwhile (tools/clock_trace.py's sampler: `gpu_state`).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def timed(fn, repeats, smp, phase):
    import torch
    fn()  # warm-up: workspaces, the kernel choices of the process
    torch.cuda.synchronize()
    smp.phase = phase
    t0 = time.perf_counter()
    for _ in range(repeats):
        fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    smp.phase = "idle"
    return round(1e3 * dt / repeats, 3)


def child(a):
    import torch
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    from calodiffusion_amd.configs import load_config
    from calodiffusion_amd.distill import ConsistencyDistillation
    from calodiffusion_amd.optim import FusedAdam
    from clock_trace import Sampler, phase_summary
    cfg = dict(load_config("dataset2"), CONSIS_NSTEPS=100, CONSIS_SOLVER=a.child if a.child != "parts" else "heun")
    torch.manual_seed(1234)
    model = CaloDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"])
    B = a.batch
    g = torch.Generator().manual_seed(4321)
    shape = [B] + list(cfg["SHAPE_PAD"][1:])
    data, noise = torch.randn(shape, generator=g).cuda(), torch.randn(shape, generator=g).cuda()
    E, layers = torch.rand((B, 1), generator=g).cuda(), torch.randn((B, 1 + cfg["SHAPE_FINAL"][2]), generator=g).cuda()
    rnd = torch.randn((B,), generator=g).cuda()
    smp = Sampler(0.010)
    smp.phase = "idle"
    smp.th.start()
    out = {"case": a.child, "batch": B, "repeats": a.repeats, "device": model.engine().device_name}
    if a.child == "parts":
        opt = FusedAdam(model.parameters(), lr=float(cfg["LR"]))

        def train():
            opt.zero_grad()
            model.compute_loss(data, E, noise=noise, layers=layers, rnd_normal=rnd).backward()
            opt.step()
        sigma = (rnd * 1.2 - 1.2).exp()

        def denoise():
            with torch.no_grad():
                model.denoise(data, E=E, sigma=sigma, layers=layers)
        out["train_step_ms"] = timed(train, a.repeats, smp, "train")
        out["denoise_ms"] = timed(denoise, a.repeats, smp, "denoise")
        out["gpu_state"] = {k: phase_summary(smp, k, drop_head=0.1) for k in ("train", "denoise")}
    else:
        d = ConsistencyDistillation(model.requires_grad_(False))
        opt = FusedAdam(d.student.parameters(), lr=float(cfg["LR"]))
        index = torch.randint(0, d.n_grid - 1, (B,), generator=g)
        losses = []
        out["step_ms"] = timed(lambda: losses.append(d.step(opt, data, E, layers, noise=noise, index=index)), a.repeats, smp, "step")
        out["first_loss"], out["last_loss"] = float(losses[0]), float(losses[-1])
        out["range_fallbacks"] = sum(m.engine().range_fallbacks for m in (d.teacher, d.student, d.target))
        out["gpu_state"] = phase_summary(smp, "step", drop_head=0.1)
    smp.stop = True
    smp.th.join()
    out["clock_source"] = smp.source
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds for each case's process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distill_bench.json"))
    ap.add_argument("--child", default=None, choices=("parts", "euler", "heun"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    result = {}
    for case in ("parts", "euler", "heun"):  # (this process never touches the GPU: every case is a fresh child)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", case, "--batch", str(a.batch), "--repeats", str(a.repeats)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"distill_bench: case {case} ended with status {r.returncode}; nothing more is started")
        result[case] = json.loads(lines[-1][7:])
        print(case, json.dumps(result[case]), flush=True)
    parts = result["parts"]
    for case, calls in (("euler", 2), ("heun", 3)):
        expect = parts["train_step_ms"] + calls * parts["denoise_ms"]
        result[case]["expected_ms"] = round(expect, 3)
        result[case]["ratio_to_expected"] = round(result[case]["step_ms"] / expect, 3)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1)
    print(json.dumps({k: {kk: v.get(kk) for kk in ("step_ms", "expected_ms", "ratio_to_expected", "train_step_ms", "denoise_ms")
                          if kk in v} for k, v in result.items()}))


if __name__ == "__main__":
    main()
