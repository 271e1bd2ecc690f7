#!/usr/bin/env python3
"""Times of the HGCal forward pre-processing (cd_preprocess_hgcal) at HGCal's shape: 28 layers, 12 x 21 bins,
1988 cells, --batch showers (default 1280: 285 MB of cells, beyond the 256 MB Infinity Cache).

    python tools/preprocess_hgcal_bench.py [--batch 1280 --seconds 1.0 --out preprocess_hgcal_bench.json]     (GPU)
    python tools/preprocess_hgcal_bench.py --reference-host [--batch 256]                                     (build host, no GPU)

  fused      one cd_preprocess_hgcal launch from the raw cells
  unfused    the device composition: cd_geom_apply of the scaled cells into a temporary, then the enc == NULL form
             (the cells are pre-scaled outside the loop: the composition is timed WITHOUT its x shower_scale pass)
  copy       a float4 copy_ of the input bytes, for scale
The map is synthetic (one or two non-zeros per cell, seeded: tools/geom_bench.py's).  Outputs of the two forms are compared
bitwise before anything is timed.  Each timing is a loop of back-to-back calls for --seconds between two device events, after a
warm-up; the shader clock is sampled meanwhile (tools/clock_trace.py's sampler).  bytes/s counts the cells read and the three
outputs written.  --reference-host times the reference's numpy path (Embeder on the CPU, preprocess_hgcal_shower, the gen map)
where the reference is mounted: wall-clock context only.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

L, A, R, N = 28, 12, 21, 1988
EMAX, EMIN, SCALE, DNUM = [100, 2.01, 1.572], [50, 1.99, 1.57], 200.0, 111


def inputs(B, seed=3):
    rng = np.random.default_rng(seed)
    raw = (rng.random((B, L, N), dtype=np.float32) * (rng.random((B, L, N), dtype=np.float32) > 0.66)).astype(np.float32)
    gen_info = np.stack([rng.uniform(lo, hi, B) for lo, hi in zip(EMIN, EMAX)], axis=1).astype(np.float32)
    raw *= (0.6 * gen_info[:, 0] / SCALE / raw.reshape(B, -1).sum(1))[:, None, None]
    return raw, gen_info


def reference_host(B):
    from oracle import gen_golden  # noqa: F401  (puts the reference on sys.path)
    from calodiffusion.utils import HGCal_utils as ref_hg
    from geom_bench import synthetic_maps
    enc, _ = synthetic_maps(L, A * R, N)
    emb = ref_hg.Embeder(A, R, torch.from_numpy(enc), None)
    raw, gen_info = inputs(B)
    t0 = time.perf_counter()
    shower = raw.astype(np.float32) * SCALE
    with torch.no_grad():
        grid = emb(torch.Tensor(shower)).numpy()
    data, layerE = ref_hg.preprocess_hgcal_shower(grid, gen_info[:, 0], None, "layer-logit-norm", dataset_num=DNUM, max_deposit=1.0)
    gen = (gen_info - np.array(EMIN)) / (np.array(EMAX) - np.array(EMIN))
    out = data.astype(np.float32), gen.astype(np.float32), layerE.astype(np.float32)
    dt = time.perf_counter() - t0
    print(json.dumps({"reference_host_seconds": round(dt, 3), "showers": B, "ms_per_shower": round(dt / B * 1e3, 3),
                      "threads": torch.get_num_threads(), "finite": bool(np.isfinite(out[0]).all())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1280)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default="preprocess_hgcal_bench.json")
    ap.add_argument("--reference-host", action="store_true")
    a = ap.parse_args()
    if a.reference_host:
        return reference_host(min(a.batch, 256) if a.batch == 1280 else a.batch)
    from calodiffusion_amd import engine, hgcal
    from calodiffusion_amd.postprocess import DATASET_PARAMS
    from clock_trace import Sampler, phase_summary
    from geom_bench import synthetic_maps
    B = a.batch
    lib = engine.load_library()
    engine.require_gpu()
    enc_mat, dec_mat = synthetic_maps(L, A * R, N)
    conv = hgcal.HGCalConverter.from_matrices([L, A, R], enc_mat, dec_mat)
    handle = conv.embeder.packed().handle
    raw_np, gen_np = inputs(B)
    raw, gen_info = torch.from_numpy(raw_np).cuda(), torch.from_numpy(gen_np).cuda()
    scaled = raw * SCALE
    c = DATASET_PARAMS[DNUM]
    consts = (C.c_double * 6)(c["logit_mean"], c["logit_std"], c["totalE_mean"], c["totalE_std"], c["layers_mean"], c["layers_std"])
    emin, emax = (C.c_double * 3)(*EMIN), (C.c_double * 3)(*EMAX)
    E = A * R
    outs = [(torch.empty((B, L * E), device="cuda"), torch.empty((B, L + 1), device="cuda"), torch.empty((B, 3), device="cuda"))
            for _ in range(2)]
    tmp, status = torch.empty((B, L, E), device="cuda"), torch.zeros((1,), dtype=torch.int32, device="cuda")
    copy_dst = torch.empty_like(raw)

    def pre(map_handle, x, cells, o):
        engine._check(lib.cd_preprocess_hgcal(map_handle, x.data_ptr(), cells, gen_info.data_ptr(), 3, o[0].data_ptr(), o[1].data_ptr(),
                                              o[2].data_ptr(), status.data_ptr(), B, L, cells, E, consts, 0.0, 1.0, 1.0, emin, emax,
                                              SCALE, engine._stream()))

    def unfused():
        engine._check(lib.cd_geom_apply(handle, scaled.data_ptr(), tmp.data_ptr(), B, 1.0, 0.0, 0, engine._stream()))
        pre(None, tmp, E, outs[1])

    forms = {"fused": lambda: pre(handle, raw, N, outs[0]), "unfused": unfused, "copy": lambda: copy_dst.copy_(raw)}
    forms["fused"]()
    forms["unfused"]()
    torch.cuda.synchronize()
    check = {"bitwise_equal": all(bool(torch.equal(x, y)) for x, y in zip(*outs)), "status": int(status.item()),
             "finite": bool(torch.isfinite(outs[0][0]).all())}
    print(json.dumps(check), flush=True)
    assert check["bitwise_equal"] and check["status"] == 0 and check["finite"]
    in_bytes = raw.numel() * 4
    moved = {"fused": in_bytes + sum(t.numel() * 4 for t in outs[0]),
             "unfused": in_bytes + 3 * tmp.numel() * 4 + sum(t.numel() * 4 for t in outs[0]), "copy": 2 * in_bytes}
    smp = Sampler(5e-3)
    smp.th.start()
    result = {"shape": {"L": L, "E": E, "N": N, "B": B}, "input_MB": round(in_bytes / 1e6, 1), "check": check,
              "enc_nnz": int((enc_mat != 0).sum())}
    for name, fn in forms.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        smp.phase = name
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n, t0 = 0, time.perf_counter()
        e0.record()
        while time.perf_counter() - t0 < a.seconds:
            for _ in range(10):
                fn()
            n += 10
            torch.cuda.synchronize()
        e1.record()
        torch.cuda.synchronize()
        smp.phase = "idle"
        us = e0.elapsed_time(e1) * 1e3 / n
        result[name] = dict(calls=n, us_per_call=round(us, 2), min_bytes_moved=moved[name],
                            TB_per_s=round(moved[name] / us / 1e6, 3), **phase_summary(smp, name))
        print(name, json.dumps(result[name]), flush=True)
    smp.stop = True
    smp.th.join()
    result["clock_source"] = smp.source
    result["fused_over_unfused"] = round(result["fused"]["us_per_call"] / result["unfused"]["us_per_call"], 3)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
