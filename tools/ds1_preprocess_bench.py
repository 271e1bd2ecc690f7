"""Time cd_preprocess_ds1 and cd_reverse_norm_ds1 (calodiffusion_amd.preprocess / postprocess) at the Dataset-1 photon shape of
tests/golden/binning_ds1_synthetic.xml (368 voxels, 5 layers, grid 5 x 10 x 30), flat 'layer-logit-norm' and grid 'logit-norm',
at B = 128 and B = 8192.  Event-timed, ms per call (best of the rounds), with a device-to-device copy of the voxel bytes for scale.

    python tools/ds1_preprocess_bench.py [--reps 20]          (GPU)
    python tools/ds1_preprocess_bench.py --reference-host     (where the reference is mounted, no GPU)

--reference-host times the reference's numpy functions (preprocess_shower and ReverseNormCaloChall, which read the binning file
and build a GeomConverter on every call) on the same shapes, on the host cores: wall-clock context only."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
XML = os.path.join(REPO, "tests", "golden", "binning_ds1_synthetic.xml")
V, GRID = 368, (5, 10, 30)
EMIN, EMAX, MAXDEP, ECUT = 0.256, 4194.304, 3.1, 0.0000001
BATCHES = (128, 8192)
FORMS = (("flat layer-logit-norm", True, "layer-logit-norm"), ("grid logit-norm", False, "logit-norm"))


def inputs(B, orig, smap):
    """(raw (B, V) GeV, e (B, 1) GeV, normalised voxels, e01 (B, 1), layerE or None): seeded, about half the voxels zero"""
    rng = np.random.default_rng(7)
    e = (EMIN * (EMAX / EMIN) ** rng.random((B, 1))).astype(np.float32)
    raw = rng.random((B, V)) + 0.01
    raw[rng.random((B, V)) < 0.5] = 0.0
    raw[:, ::37] = 1.0   # every layer keeps a deposit
    raw = (raw * (0.8 * e / raw.sum(axis=1, keepdims=True))).astype(np.float32)
    vox = rng.normal(0.0, 1.0, (B, V) if orig else (B, 1) + GRID).astype(np.float32)
    lE = rng.normal(0.0, 1.0, (B, GRID[0] + 1)).astype(np.float32) if "layer" in smap else None
    return raw, e, vox, rng.random((B, 1)).astype(np.float32), lE


def reference_host():
    from oracle import gen_golden  # noqa: F401  (puts the reference on sys.path)
    from calodiffusion.utils import utils as ref
    for name, orig, smap in FORMS:
        for B in BATCHES:
            raw, e, vox, e01, lE = inputs(B, orig, smap)
            with contextlib.redirect_stdout(io.StringIO()):
                t0 = time.perf_counter()
                ref.preprocess_shower(raw.copy(), e.copy(), None, XML, smap, dataset_num=1, orig_shape=orig, ecut=ECUT, max_deposit=MAXDEP)
                t1 = time.perf_counter()
                ref.ReverseNormCaloChall(vox.copy(), e01.copy(), emax=EMAX, emin=EMIN, binning_file=XML, max_deposit=MAXDEP, logE=True,
                                         layerE=None if lE is None else lE.copy(), showerMap=smap, dataset_num=1, orig_shape=orig,
                                         ecut=ECUT)
                t2 = time.perf_counter()
            print(json.dumps({"form": name, "B": B, "reference_host_forward_ms": round((t1 - t0) * 1e3, 3),
                              "reference_host_reverse_ms": round((t2 - t1) * 1e3, 3)}), flush=True)


def device(reps):
    import ctypes as C
    import torch
    from calodiffusion_amd import engine, geom1, xml_handler
    from calodiffusion_amd.postprocess import DATASET1_PARAMS
    lib = engine.load_library()
    engine.require_gpu()
    gc = geom1.GeomConverter(xml_handler.XMLHandler("photon", XML))
    rm = gc.radial_map()
    conv_w, unconv_w = gc._fixed_weights()

    def timed(fn):
        fn()  # warm-up
        torch.cuda.synchronize()
        best = float("inf")
        for _ in range(3):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(reps):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            best = min(best, ev[0].elapsed_time(ev[1]) / reps)
        return best

    for name, orig, smap in FORMS:
        c = DATASET1_PARAMS[11 if orig else 1]
        consts = (C.c_double * 6)(c["logit_mean"], c["logit_std"], c["totalE_mean"], c["totalE_std"], c["layers_mean"], c["layers_std"])
        for B in BATCHES:
            raw, e, vox, e01, lE = (None if a is None else torch.from_numpy(a).cuda() for a in inputs(B, orig, smap))
            en = (EMIN * (EMAX / EMIN) ** e01).reshape(-1).contiguous()
            out = torch.empty((B, V) if orig else (B, 1) + GRID, device="cuda")
            layerE = torch.empty((B, GRID[0] + 1), device="cuda") if lE is not None else None
            e_out, status = torch.empty((B, 1), device="cuda"), torch.zeros((1,), dtype=torch.int32, device="cuda")
            back = torch.empty((B, V), device="cuda")

            def forward():
                engine._check(lib.cd_preprocess_ds1(rm.handle, None if orig else conv_w.data_ptr(), raw.data_ptr(), e.data_ptr(),
                                                    out.data_ptr(), engine._ptr(layerE), e_out.data_ptr(), status.data_ptr(), B,
                                                    consts, MAXDEP, EMIN, EMAX, 1, 1.0, engine._stream()))

            def reverse():
                engine._check(lib.cd_reverse_norm_ds1(rm.handle, None if orig else unconv_w.data_ptr(), vox.data_ptr(), en.data_ptr(),
                                                      engine._ptr(lE), back.data_ptr(), B, consts, MAXDEP, ECUT, engine._stream()))

            ms_f = timed(forward)
            assert int(status.item()) == 0 and bool(torch.isfinite(out).all())
            ms_r = timed(reverse)
            assert bool(torch.isfinite(back).all())
            ms_copy = timed(lambda: back.copy_(raw))
            print(json.dumps({"form": name, "B": B, "forward_ms": round(ms_f, 4), "reverse_ms": round(ms_r, 4),
                              "copy_of_the_flat_showers_ms": round(ms_copy, 4)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--reference-host", action="store_true")
    a = ap.parse_args()
    reference_host() if a.reference_host else device(a.reps)
