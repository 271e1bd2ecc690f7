#!/usr/bin/env python3
"""Times of the shower statistics on the GPU beside the shower observables (section 8e), on the SAME bytes,
in one run on one card:

    python tools/shower_stats_bench.py [--seconds 1.0 --out shower_stats_bench.json]

  dataset2   45 layers x 16 alpha x 9 r  (V = 6480)    B = 16 384   0.42 GB of showers
  dataset3   45 layers x 50 alpha x 18 r (V = 40500)   B = 4 096    0.66 GB of showers     (both beyond the 256 MB cache)
Showers are seeded as in tools/hlf_bench.py (about 30 % occupancy over six decades, generated on the device); the binning files
of cd_hlf_compute come from the XML writer of tools/gen_golden_hlf.py, the tables of cd_shower_stats_compute from
ShowerStatistics.for_grid.

Per case, after the first, middle and last 64 showers have been compared with the NumPy restatement of
tests/shower_stats_cases.py: cd_shower_stats_compute with both profiles, the same without profiles (moment sums alone: the
difference is what the profile walk costs), cd_hlf_compute, cd_threshold_conserve on a copy (rows of R cells), and torch.sum over
the same showers (this run's own streaming read, as PyTorch's reduction does it).  Each is
launched into preallocated outputs back to back between two device events for about --seconds, after a warm-up; the two
reductions are timed alternately, twice, so that a drift of the clocks shows as a spread.  Bytes are what the algorithm needs --
B V 4 of showers plus the records it writes (stats: B L 56 + B (A + R) 8; hlf: B L 68; cut: B V 8, read and written) -- and the
share is of the 6.29 TB/s streaming read of an MI355X; the geometry tables are served from cache and not counted.  The
device's clocks as the run saw them (torch.cuda.clock_rate, if the build has it) are noted in the result.
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

STREAM_READ = 6.29e12  # bytes/s
CASES = {"dataset2": ("dataset2", 4.65, 16384), "dataset3": ("dataset3", 2.325, 4096)}


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / n


def calls_for(fn, seconds):
    window(fn, 3)  # warm-up
    return max(10, int(seconds / window(fn, 10)))


def clocks():
    try:
        return {"sclk_mhz": torch.cuda.clock_rate()}
    except Exception as err:  # (needs amdsmi in the torch build)
        return {"sclk_mhz": None, "why": type(err).__name__}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default="shower_stats_bench.json")
    ap.add_argument("--cases", default="dataset2,dataset3")
    a = ap.parse_args()
    import shower_stats_cases as S
    from gen_golden_hlf import write_regular_binning
    from hlf_bench import device_showers
    from calodiffusion_amd import engine
    from calodiffusion_amd.configs import load_config
    from calodiffusion_amd.hlf import HighLevelFeatures
    from calodiffusion_amd.shower_stats import ShowerStatistics
    from calodiffusion_amd.utils import threshold_conserveE
    result = {"device": torch.cuda.get_device_name(0), "stream_read_bytes_per_s": STREAM_READ, "clocks_before": clocks()}
    with tempfile.TemporaryDirectory() as tmp:
        for case in a.cases.split(","):
            cfg_name, r_width, B = CASES[case]
            L, A, R = load_config(cfg_name)["SHAPE_FINAL"][2:]
            path = os.path.join(tmp, f"binning_{case}.xml")
            write_regular_binning(path, L, A, R, r_width)
            hlf = HighLevelFeatures("electron", filename=path)
            geo = ShowerStatistics.for_grid((L, A, R))
            V = geo.voxels
            x = device_showers(B, V, 17)
            tab = S.Tables.of(geo)
            out = geo._launch(x, 1e-3, 1e-6)
            for rows in (slice(0, 64), slice(B // 2 - 32, B // 2 + 32), slice(B - 64, B)):
                S.assert_raw_within_fp64_bounds(tuple(o[rows].cpu().numpy() for o in out), x[rows].cpu().numpy(), tab)
            bare = geo._launch(x, 1e-3, 1e-6, profiles=False)
            h_out, h_hits = hlf._launch(x, 0.0)
            cut = x.clone().reshape(-1, R)
            threshold_conserveE(cut, 1e-3)  # (through the public wrapper once; timed below without its per-call device check)
            lib, stream, total = engine.load_library(), engine._stream(), torch.empty((), dtype=torch.float32, device="cuda")
            runs = {"stats": lambda: geo._launch(x, 1e-3, 1e-6, out=out),
                    "stats_no_profiles": lambda: geo._launch(x, 1e-3, 1e-6, profiles=False, out=bare),
                    "hlf": lambda: hlf._launch(x, 0.0, h_out, h_hits),
                    "cut": lambda: engine._check(lib.cd_threshold_conserve(cut.data_ptr(), None, cut.shape[0], R, 1e-3, stream)),
                    "torch_sum": lambda: torch.sum(x, dim=(0, 1), out=total)}  # this run's streaming read of the same bytes, as PyTorch does it
            nbytes = {"stats": B * V * 4 + B * L * 56 + B * (A + R) * 8, "stats_no_profiles": B * V * 4 + B * L * 56,
                      "hlf": B * V * 4 + B * L * 68, "cut": B * V * 8, "torch_sum": B * V * 4}
            n = {k: calls_for(fn, a.seconds) for k, fn in runs.items()}
            times = {k: [] for k in runs}
            for _ in range(2):  # alternately
                for k, fn in runs.items():
                    times[k].append(window(fn, n[k]))
            r = {"V": V, "B": B, "layers": L}
            for k in runs:
                sec = min(times[k])
                r[k] = {"calls": n[k], "ms_per_call": [round(t * 1e3, 4) for t in times[k]], "bytes_per_call": nbytes[k],
                        "TB_per_s": round(nbytes[k] / sec / 1e12, 3), "share_of_stream_read": round(nbytes[k] / sec / STREAM_READ, 3)}
            r["stats_over_hlf_time"] = round(min(times["stats"]) / min(times["hlf"]), 3)
            r["stats_share_of_torch_sum_rate"] = round(r["stats"]["TB_per_s"] / r["torch_sum"]["TB_per_s"], 3)
            result[case] = r
            print(case, json.dumps(r), flush=True)
            del x, cut, out, bare, h_out, h_hits
            torch.cuda.empty_cache()
    result["clocks_after"] = clocks()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
