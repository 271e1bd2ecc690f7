#!/usr/bin/env python3
"""Times of the kernel physics distance and the separation powers on the GPU, at the size an evaluation runs:

    python tools/kpd_bench.py [--out kpd_bench.json]

Two seeded float64 feature matrices of 100 000 rows and D = 226 columns (tools/fpd_bench.py's generator).  Every figure is the
median of 10 calls after 2 warm-ups, each call between two device events:

kpd: evaluate.kpd() at its defaults (10 batches of 5000 + 5000 rows) from device tensors and from host arrays.
sums: the one cd_kpd_sums call inside it (the Gram kernel and the kernel that adds its partials), into preallocated outputs and
workspace.  Two FLOP counts: `issued`, what the fp64 matrix instructions execute (the 64 x 64 blocks of the upper triangle over
228 padded columns), and `useful`, the upper triangle of the 10 000 x 10 000 Gram matrix over 226 columns.  The shares are of the
vendor's published peak FP64 matrix rate of an MI355X, 78.6 TFLOP/s (AMD Instinct MI355X data sheet); nobody has measured that
peak here.  The first batch is compared with NumPy before anything is timed.
separation: evaluate.separation_powers() from device tensors, and the two cd_column_histograms calls inside it.
host: one batch of the restatement's arithmetic in NumPy on the host cores (three 5000 x 5000 kernel matrices; np.sum in place of
tests/kpd_cases.py's math.fsum, which would take longer still).
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fpd_bench import FP64_MATRIX_PEAK, device_features  # noqa: E402

ROWS, D, BATCHES, M, BLOCK = 100000, 226, 10, 5000, 64


def median_ms(call, repeats=10, warm=2):
    times = []
    for k in range(warm + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        if k >= warm:
            times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(min(times)), float(max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="kpd_bench.json")
    a = ap.parse_args()
    from calodiffusion_amd import evaluate as E
    result = {"device": torch.cuda.get_device_name(0), "fp64_matrix_peak_flops": FP64_MATRIX_PEAK, "rows": ROWS, "d": D, "batches": BATCHES,
              "batch_size": M, "host_threads": int(os.environ.get("OMP_NUM_THREADS", 0)) or len(os.sched_getaffinity(0))}
    real, gen = device_features(ROWS, D, 17), device_features(ROWS, D, 18)
    real_host, gen_host = real.cpu().numpy(), gen.cpu().numpy()

    # the raw call, on the matrix kpd() builds
    X, Y = E._normalise(real, gen)
    Z = torch.cat([X, Y])
    lists = E.kpd_index_lists(ROWS, ROWS, BATCHES, M, 42)
    lists[:, 1] += ROWS
    idx = torch.from_numpy(lists.reshape(2 * BATCHES, M).astype(np.int32)).cuda()
    sums = torch.empty((BATCHES, 3), dtype=torch.float64, device="cuda")
    status = torch.zeros((1,), dtype=torch.int32, device="cuda")
    nbytes = E.kpd_workspace_bytes(2 * BATCHES, M)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    call = lambda: E.launch_kpd_sums(Z, idx, [M] * (2 * BATCHES), 1.0 / D, 4, sums, status, ws)  # noqa: E731
    call()
    assert int(status.item()) == 0
    Zh = Z.cpu().numpy()
    t0 = time.perf_counter()
    A, Bm = Zh[lists[0, 0]], Zh[lists[0, 1]]
    host = []
    for p, q, off in ((A, A, True), (Bm, Bm, True), (A, Bm, False)):
        k = (p @ q.T * (1.0 / D) + 1.0) ** 2
        k *= k
        host.append(k.sum() - np.trace(k) if off else k.sum())
    t_host = time.perf_counter() - t0
    got = sums[0].cpu().numpy()
    assert np.all(np.abs(got - host) <= 1e-11 * np.abs(host)), (got, host)
    ms, lo, hi = median_ms(call)
    nb = -(-2 * M // BLOCK)
    issued = BATCHES * (nb * (nb + 1) // 2) * BLOCK * BLOCK * ((D + 3) // 4 * 4) * 2
    useful = BATCHES * (2 * M) * (2 * M + 1) // 2 * D * 2
    result["sums"] = {"ms_per_call": round(ms, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3), "workspace_MB": round(nbytes / 1e6, 2),
                      "issued_TFLOP_per_s": round(issued / ms / 1e9, 2), "issued_share_of_peak": round(issued / (ms * 1e-3) / FP64_MATRIX_PEAK, 3),
                      "useful_TFLOP_per_s": round(useful / ms / 1e9, 2), "useful_share_of_peak": round(useful / (ms * 1e-3) / FP64_MATRIX_PEAK, 3)}
    print(json.dumps(result["sums"]), flush=True)
    result["host_one_batch_numpy_s"] = round(t_host, 2)
    del X, Y, Z, ws

    out = {}
    ms_dev, _, _ = median_ms(lambda: out.__setitem__("v", E.kpd(real, gen)))
    ms_host, _, _ = median_ms(lambda: E.kpd(real_host, gen_host))
    result["kpd_defaults"] = {"value": out["v"][0], "error": out["v"][1], "ms_from_device_tensors": round(ms_dev, 2),
                              "ms_from_host_arrays": round(ms_host, 2), "sums_share_of_device_call": round(ms / ms_dev, 3)}
    print(json.dumps(result["kpd_defaults"]), flush=True)

    # separation powers
    lo_, hi_ = real.amin(dim=0).cpu().numpy(), real.amax(dim=0).cpu().numpy()
    edges = torch.from_numpy(np.stack([np.linspace(lo_[j], hi_[j], 50) for j in range(D)])).cuda()
    both = torch.cat([real, gen])
    counts = torch.empty((2, D, 49), dtype=torch.int32, device="cuda")
    ws = torch.empty((E.histogram_workspace_bytes(ROWS, D, 50),), dtype=torch.uint8, device="cuda")

    def histograms():
        E.launch_column_histograms(both, 0, ROWS, edges, counts[0], ws)
        E.launch_column_histograms(both, ROWS, ROWS, edges, counts[1], ws)

    ms_hist, _, _ = median_ms(histograms)
    assert int(counts[0].sum().item()) == ROWS * D
    ms_sep, _, _ = median_ms(lambda: out.__setitem__("s", E.separation_powers(real, gen)))
    t0 = time.perf_counter()
    np.histogram(real_host[:, 0], bins=edges[0].cpu().numpy())
    np.histogram(gen_host[:, 0], bins=edges[0].cpu().numpy())
    t_np = (time.perf_counter() - t0) * D
    result["separation"] = {"total": float(np.sum(out["s"])), "ms_two_histogram_calls": round(ms_hist, 3),
                            "histogram_GB_per_s": round(2 * ROWS * D * 8 / ms_hist / 1e6, 1), "ms_separation_powers": round(ms_sep, 2),
                            "numpy_histograms_s_scaled_from_one_column": round(t_np, 2)}
    print(json.dumps(result["separation"]), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
