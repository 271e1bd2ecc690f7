"""Times one training epoch of the classifier test (70 % of 2 x 20 000 rows, d = 226, 2024 hidden units, 2 hidden layers, dropout
0.2, batch 256: 110 steps) on the device, twice: cd_classifier_train_epoch, and the reference's loop restated with torch-ROCm
modules in fp32 (hgcal_metrics.py:68-84) on the same card.  Prints one JSON line with both.  Not a test; bench.py does not call it.

    python tools/classifier_bench.py [--epochs 3] [--time-limit 120]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from calodiffusion_amd import classifier as CL  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=3, help="timed epochs per path (after one warm-up epoch)")
    ap.add_argument("--time-limit", type=float, default=120.0, help="seconds per path; an epoch that starts later is not run")
    ap.add_argument("--rows", type=int, default=40_000)
    ap.add_argument("--dim", type=int, default=226)
    args = ap.parse_args()
    torch.backends.cuda.matmul.allow_tf32 = False
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal((args.rows, args.dim)).astype(np.float32)).cuda()
    y = torch.from_numpy((rng.random(args.rows) < 0.5).astype(np.float32)).cuda()
    n_train, batch = int(args.rows * 0.7), 256
    steps = -(-n_train // batch)

    def timed(epoch_fn):
        epoch_fn(0)  # warm-up
        torch.cuda.synchronize()
        times, begin = [], time.perf_counter()
        for e in range(args.epochs):
            if time.perf_counter() - begin > args.time_limit:
                break
            t0 = time.perf_counter()
            epoch_fn(e + 1)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return times

    # the library
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        model = CL.DNN(2, 2024, args.dim, 0.2).cuda()
    desc, params = model.desc(), model.device_params()
    n = CL.num_params(desc)
    grads, m, v = (torch.zeros((n,), device="cuda") for _ in range(3))
    ws = CL._workspace(desc, batch, x.device)

    def device_epoch(e):
        perm = torch.from_numpy(np.random.default_rng(e).permutation(n_train).astype(np.int32)).cuda()
        return CL.train_epoch(desc, params, x, y, perm, batch, 0, e * steps, grads, m, v, 1e-4, workspace=ws)

    dev = timed(device_epoch)

    # torch-ROCm, fp32: the reference's loop
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        ref = CL.DNN(2, 2024, args.dim, 0.2).cuda()
    layers, optim, crit = ref.layers, torch.optim.Adam(ref.parameters(), lr=1e-4), torch.nn.BCEWithLogitsLoss()

    def torch_epoch(e):
        ref.train()
        perm = torch.from_numpy(np.random.default_rng(e).permutation(n_train)).cuda()
        for lo in range(0, n_train, batch):
            idx = perm[lo:lo + batch]
            loss = crit(layers(x[idx]), y[idx].unsqueeze(1))
            optim.zero_grad()
            loss.backward()
            optim.step()

    tor = timed(torch_epoch)
    flop = 6.0 * batch * (args.dim * 2024 + 2 * 2024 * 2024) * steps  # forward + two backward products per layer
    out = {"steps_per_epoch": steps, "device_epoch_s": dev, "torch_rocm_fp32_epoch_s": tor,
           "device_ms_per_step": 1e3 * min(dev) / steps if dev else None, "torch_ms_per_step": 1e3 * min(tor) / steps if tor else None,
           "device_tflops": flop / min(dev) / 1e12 if dev else None}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
