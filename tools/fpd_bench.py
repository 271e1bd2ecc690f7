#!/usr/bin/env python3
"""Times of the Frechet physics distance on the GPU, at the sizes an evaluation runs:

    python tools/fpd_bench.py [--seconds 1.0 --host-pairs 1 --out fpd_bench.json]

A seeded float64 feature matrix of 100 000 rows and D = 226 columns (Datasets 2 and 3: 1 + 45 + 4 x 45) with columns of different
scales and offsets, generated on the device.

kernel: one cd_fpd_moments call for the 40 sets of one batch size (2 x 20 bootstrap batches), at 20 000 and at 50 000 rows a set,
indices drawn with replacement -- calls into preallocated outputs and workspace, enqueued back to back between two device events
for about --seconds, after a warm-up; nothing is allocated or synchronised inside the window.  Two FLOP counts: `issued`, what the
fp64 matrix instructions execute (120 tile pairs of the 240 padded columns: 512 FLOP per row and pair), and `useful`,
n d (d + 1) per set (the symmetric half of np.cov's Gram matrix).  The shares are of the vendor's published peak FP64 matrix rate
of an MI355X, 78.6 TFLOP/s (AMD Instinct MI355X data sheet); nobody has measured that peak here.  The first and the last set
are compared with the NumPy restatement of tests/fpd_cases.py before anything is timed.

end to end: wall-clock time of evaluate.fpd() at its defaults (400 moments, 200 distances, the fit) on two host arrays of 100 000
rows, next to the NumPy restatement of the same call on the host cores.  The restatement's 400 covariances take minutes, so it is
timed on --host-pairs pairs per batch size and scaled to the 20 of the call.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FP64_MATRIX_PEAK = 78.6e12  # FLOP/s, AMD Instinct MI355X data sheet
ROWS, D, SETS = 100000, 226, 40


def device_features(rows, d, seed, shape_seed=17):
    """Columns of scales over three decades and offsets up to 50 (from shape_seed), standard-normal rows (from seed)."""
    g = torch.Generator(device="cuda").manual_seed(shape_seed)
    scale = 10.0 ** (3.0 * torch.rand((d,), generator=g, device="cuda", dtype=torch.float64) - 2.0)
    offset = 100.0 * torch.rand((d,), generator=g, device="cuda", dtype=torch.float64) - 50.0
    g.manual_seed(1000 + seed)
    return torch.randn((rows, d), generator=g, device="cuda", dtype=torch.float64) * scale + offset


def time_calls(call, seconds):
    def window(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / n

    window(2)  # warm-up
    n = max(5, int(seconds / window(5)))
    return n, window(n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--host-pairs", type=int, default=1)
    ap.add_argument("--out", default="fpd_bench.json")
    a = ap.parse_args()
    import fpd_cases as F
    from calodiffusion_amd import evaluate as E
    result = {"device": torch.cuda.get_device_name(0), "fp64_matrix_peak_flops": FP64_MATRIX_PEAK, "rows": ROWS, "d": D, "sets": SETS,
              "host_threads": int(os.environ.get("OMP_NUM_THREADS", 0)) or len(os.sched_getaffinity(0))}
    x = device_features(ROWS, D, 17)
    centre = x.mean(dim=0)
    x_host, centre_host = x.cpu().numpy(), centre.cpu().numpy()
    tiles = (D + 1 + 15) // 16
    pairs = tiles * (tiles + 1) // 2
    for n in (20000, 50000):
        g = torch.Generator(device="cuda").manual_seed(n)
        idx = torch.randint(0, ROWS, (SETS, n), generator=g, device="cuda", dtype=torch.int32)
        mean = torch.empty((SETS, D), dtype=torch.float64, device="cuda")
        cov = torch.empty((SETS, D, D), dtype=torch.float64, device="cuda")
        status = torch.zeros((1,), dtype=torch.int32, device="cuda")
        nbytes = E.moments_workspace_bytes(D, SETS, n)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
        call = lambda: E.launch_moments(x, centre, idx, [n] * SETS, mean, cov, status, ws)  # noqa: E731
        call()
        assert int(status.item()) == 0
        lists = idx[[0, SETS - 1]].cpu().numpy()
        F.assert_moments_within_bounds(mean[[0, SETS - 1]].cpu().numpy(), cov[[0, SETS - 1]].cpu().numpy(), x_host, centre_host, lists)
        calls, sec = time_calls(call, a.seconds)
        issued, useful = SETS * n * pairs * 512, SETS * n * D * (D + 1)
        r = {"rows_per_set": n, "calls": calls, "ms_per_call": round(sec * 1e3, 4), "workspace_MB": round(nbytes / 1e6, 1),
             "issued_TFLOP_per_s": round(issued / sec / 1e12, 2), "issued_share_of_peak": round(issued / sec / FP64_MATRIX_PEAK, 3),
             "useful_TFLOP_per_s": round(useful / sec / 1e12, 2), "useful_share_of_peak": round(useful / sec / FP64_MATRIX_PEAK, 3)}
        result[f"moments_{n}"] = r
        print(n, json.dumps(r), flush=True)
        del idx, mean, cov, ws
    # end to end at the defaults
    real, gen = x_host, device_features(ROWS, D, 18).cpu().numpy()
    del x
    torch.cuda.empty_cache()
    E.fpd(real[:2000], gen[:2000], min_samples=200, max_samples=500, num_batches=2, num_points=3)  # warm
    t0 = time.perf_counter()
    value, err = E.fpd(real, gen)
    t_dev = time.perf_counter() - t0
    t0 = time.perf_counter()
    E.fpd(torch.from_numpy(real).cuda(), torch.from_numpy(gen).cuda())
    t_dev_resident = time.perf_counter() - t0
    sizes = E.fpd_batch_sizes()
    lists = [l[:a.host_pairs] for l in E.fpd_index_lists(ROWS, ROWS, sizes, 20, 42)]
    t0 = time.perf_counter()
    m = np.abs(real).max(axis=0)
    m[m == 0] = 1.0
    X, Y = real / m, gen / m
    t_norm = time.perf_counter() - t0
    t_mom = t_dist = 0.0
    for l in lists:
        for k in range(l.shape[0]):
            t0 = time.perf_counter()
            ra, rb = X[l[k, 0]], Y[l[k, 1]]
            mom = ra.mean(axis=0), np.cov(ra, rowvar=False), rb.mean(axis=0), np.cov(rb, rowvar=False)
            t1 = time.perf_counter()
            F.restate_frechet(*mom)
            t_mom, t_dist = t_mom + t1 - t0, t_dist + time.perf_counter() - t1
    scale = 20 / a.host_pairs
    result["fpd_defaults"] = {"value": value, "error": err, "device_s_from_host_arrays": round(t_dev, 3),
                              "device_s_from_device_tensors": round(t_dev_resident, 3),
                              "restatement_s": round(t_norm + scale * (t_mom + t_dist), 1), "restatement_moments_s": round(scale * t_mom, 1),
                              "restatement_distances_s": round(scale * t_dist, 2), "restatement_scaled_from_pairs_per_size": a.host_pairs}
    print(json.dumps(result["fpd_defaults"]), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
