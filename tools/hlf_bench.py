#!/usr/bin/env python3
"""Times of the shower observables on the GPU, at the sizes an evaluation runs:

    python tools/hlf_bench.py [--seconds 1.0 --host-showers 16384 --out hlf_bench.json]

  dataset2   45 layers x 16 alpha x 9 r  (V = 6480)    B = 100 000   2.6 GB of showers
  dataset3   45 layers x 50 alpha x 18 r (V = 40500)   B = 16 384    2.65 GB of showers
  photon     the Dataset-1-shaped synthetic file (V = 368: layers of 8, 160, 190, 5 and 5 voxels)   B = 1 000 000   1.47 GB
The binning files are generated from the configs' grids with the XML writer of tools/gen_golden_hlf.py (regular cylinders; radial
bin widths 4.65 and 2.325 mm).  Showers are seeded: about 30 % occupancy over six decades, generated on the device.

kernel: one cd_hlf_compute launch on showers that are already on the device -- launches into preallocated outputs, enqueued back
to back between two device events for about --seconds, after a warm-up; nothing is allocated or synchronised inside the window.
Bytes are what the algorithm needs, B V 4 of showers plus the records (B R 68); the share is of the 6.29 TB/s streaming read of
an MI355X.  The eta / phi tables (16 bytes a voxel, shared by all showers) are
served from cache and not counted.  The first, the middle and the last 64 shower rows are compared with the NumPy restatement of
tests/hlf_cases.py before anything is timed.

host (context, not the kernel): wall-clock time, from a float32 HOST array of --host-showers showers, of the restatement (NumPy
float64 on the host cores) and of HighLevelFeatures.CalculateFeatures (upload in chunks, launch, records back, the host
dictionaries), scaled per 100 000 showers.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

STREAM_READ = 6.29e12  # bytes/s
CASES = {"dataset2": ("dataset2", 4.65, 100000), "dataset3": ("dataset3", 2.325, 16384)}


def device_showers(B, V, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.empty((B, V), dtype=torch.float32, device="cuda")
    rows = max(1, (1 << 26) // V)
    for lo in range(0, B, rows):  # in slices: the temporaries stay small beside 2.6 GB of showers
        n = min(rows, B - lo)
        u = torch.rand((n, V), generator=g, device="cuda")
        keep = torch.rand((n, V), generator=g, device="cuda") < 0.3
        x[lo:lo + n] = torch.where(keep, 10.0 ** (6.0 * u - 3.0), torch.zeros((), device="cuda"))
    return x


def time_kernel(hlf, x, seconds):
    """ms of one cd_hlf_compute launch: n launches into preallocated outputs, enqueued back to back between two device events with
    no synchronisation and no allocation in between; n from a short calibration so that the window is about `seconds`."""
    out, hits = hlf._launch(x, 0.0)

    def window(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            hlf._launch(x, 0.0, out, hits)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / n

    window(3)  # warm-up
    n = max(10, int(seconds / window(10)))
    return n, window(n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--host-showers", type=int, default=16384)
    ap.add_argument("--out", default="hlf_bench.json")
    ap.add_argument("--cases", default="dataset2,dataset3,photon")
    a = ap.parse_args()
    import hlf_cases as H
    from gen_golden_hlf import write_regular_binning
    from calodiffusion_amd.configs import load_config
    from calodiffusion_amd.hlf import HighLevelFeatures
    result = {"device": torch.cuda.get_device_name(0), "stream_read_bytes_per_s": STREAM_READ}
    with tempfile.TemporaryDirectory() as tmp:
        for case in a.cases.split(","):
            if case == "photon":  # small ragged layers: tests/golden/binning_ds1_synthetic.xml, 1.47 GB (beyond the 256 MB cache)
                B, L = 1000000, 5
                hlf = HighLevelFeatures("photon", filename=os.path.join(ROOT, "tests", "golden", "binning_ds1_synthetic.xml"))
            else:
                cfg_name, r_width, B = CASES[case]
                L, A, R = load_config(cfg_name)["SHAPE_FINAL"][2:]
                path = os.path.join(tmp, f"binning_{case}.xml")
                write_regular_binning(path, L, A, R, r_width)
                hlf = HighLevelFeatures("electron", filename=path)
            V = hlf.total_voxels
            hlf._device_handle()
            x = device_showers(B, V, 17)
            geo = H.Geometry(hlf.bin_edges, np.concatenate(hlf.eta_all_layers), np.concatenate(hlf.phi_all_layers),
                             hlf.relevantLayers, hlf.layers_with_centres)
            rec, hits = hlf._launch(x, 0.0)
            for rows in (slice(0, 64), slice(B // 2 - 32, B // 2 + 32), slice(B - 64, B)):  # first, middle and last trip of the grid's loop
                H.assert_within_fp64_bounds(rec[rows].cpu().numpy(), hits[rows].cpu().numpy(), *H.restate(x[rows].cpu().numpy(), geo), geo)
            del rec, hits
            calls, sec = time_kernel(hlf, x, a.seconds)
            nbytes = B * V * 4 + B * len(hlf.relevantLayers) * 68
            r = {"V": V, "B": B, "layers": L, "calls": calls, "ms_per_call": round(sec * 1e3, 4), "bytes_per_call": nbytes,
                 "TB_per_s": round(nbytes / sec / 1e12, 3), "share_of_stream_read": round(nbytes / sec / STREAM_READ, 3)}
            # host context: the same showers from a host array
            n = min(a.host_showers, B)
            host = x[:n].cpu().numpy()
            del x
            torch.cuda.empty_cache()
            t0 = time.perf_counter()
            H.restate(host, geo)
            t_np = time.perf_counter() - t0
            hlf.CalculateFeatures(host)  # warm
            t0 = time.perf_counter()
            hlf.CalculateFeatures(host)
            t_cls = time.perf_counter() - t0
            r["host"] = {"showers": n, "restatement_s_per_100k": round(t_np * 1e5 / n, 3),
                         "class_from_host_array_s_per_100k": round(t_cls * 1e5 / n, 3)}
            result[case] = r
            print(case, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
