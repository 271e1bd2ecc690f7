"""Generate tests/golden/preprocess.npz from the reference's own ``utils.preprocess_shower`` and the incident-energy map of
``DataLoaderCaloChall`` (calodiffusion/utils/utils.py:290-312, 315-436) on seeded synthetic raw showers.

TEST INFRASTRUCTURE, like oracle/gen_golden.py: runs only where the reference is mounted, and imports it through that
script's stub-import preamble (by importing the script).  Only data is written: raw inputs and the reference's outputs.

    python tools/gen_preprocess_golden.py [--out FILE]      # default tests/golden/preprocess.npz

Inputs, per tag (8 showers each), in MeV as the CaloChallenge files store them (the loader's shower_scale 0.001 makes GeV):
    d2  45 x 16 x 9,  'layer-logit-norm', ~65 % exact zeros      d3  45 x 50 x 18, 'logit-norm', ~88 % exact zeros
  - a gamma-like longitudinal profile and an exponential radial fall-off per shower, log-normal voxel fluctuations;
  - shower 0 has two empty layers (3 and 40);
  - incident energies log-uniform over [1, 1000] GeV, deposited fraction in [0.6, 0.95] (below max_deposit = 2);
  - every non-zero voxel is at least 0.02 MeV, above the 15.1 keV read-out threshold (ECUT), so the round trip through
    ReverseNorm keeps the zero pattern.
Outputs: {tag}.data (B, D*H*W), {tag}.layerE (d2), {tag}.E for logE=True, and d2.E_lin for logE=False (the voxel and layer
outputs do not depend on logE).

Conditioning.  The GPU test holds every (shower, layer) element of layerE to a RELATIVE bar (3e-5).  A normalised layer energy
that happens to land next to zero, (logit - layers_mean) / layers_std ~ 0, carries the reference's own fp32 rounding (its
sums, its float32 log) as an arbitrarily large relative error; such an element would test the reference's rounding, not the
code.  The generator therefore evaluates the same formulas in float64 (from the float32 quotients shower / (max_deposit e)
the reference sums) and takes the first seed, counting up from the base seed, for which the reference's own output is within
1e-5 of the float64 value on every (shower, layer) row of layerE and of the voxel tensor.  The criterion involves the
reference and exact arithmetic only, never the device code.  The script also prints the reference's own round trip
(ReverseNormCaloChall(preprocess_shower(raw)) against raw), the figure the GPU round-trip bar is derived from.
"""
from __future__ import annotations

import argparse
import contextlib
import io
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402  (stubs the absent modules and puts the reference on sys.path)
import numpy as np  # noqa: E402
from calodiffusion.utils import utils as ref_utils  # noqa: E402  (the REFERENCE's module: its path comes first)

from calodiffusion_amd.postprocess import DATASET_PARAMS  # noqa: E402

BASE_SEED = G.SEED + 90
SHOWER_SCALE = 0.001          # DataLoaderCaloChall's default (utils.py:276)
EMIN, EMAX, MAXDEP, ECUT = 1.0, 1000.0, 2, 0.0000151
CASES = (("d2", (45, 16, 9), 2, "layer-logit-norm", 0.65), ("d3", (45, 50, 18), 3, "logit-norm", 0.88))
B = 8
WELL_CONDITIONED = 1e-5


def synth_showers(rng, dims, p_zero):
    """(showers (B, D*H*W) float32 MeV, incident_energies (B, 1) float32 MeV)."""
    D, H, W = dims
    e = (10.0 ** (3.0 + 3.0 * rng.random((B, 1)))).astype(np.float32)
    z = np.arange(D, dtype=np.float64)[None, :, None, None] + 0.5
    r = np.arange(W, dtype=np.float64)[None, None, None, :]
    a = rng.uniform(2.0, 5.0, (B, 1, 1, 1))
    b = rng.uniform(0.25, 0.6, (B, 1, 1, 1))
    r0 = rng.uniform(0.8, 2.5, (B, 1, 1, 1))
    prof = z ** a * np.exp(-b * z) * np.exp(-r / r0)
    v = prof * np.exp(rng.normal(0.0, 1.0, (B, D, H, W)))
    v[rng.random((B, D, H, W)) < p_zero] = 0.0
    v[0, 3] = 0.0
    v[0, 40] = 0.0
    frac = rng.uniform(0.6, 0.95, (B, 1, 1, 1))
    v *= frac * e.astype(np.float64).reshape(B, 1, 1, 1) / v.sum(axis=(1, 2, 3), keepdims=True)
    v[(v > 0) & (v < 0.02)] = 0.02
    return v.reshape(B, -1).astype(np.float32), e


def reference_outputs(showers, energies, dims, dnum, smap):
    """What DataLoaderCaloChall computes after reading the file (utils.py:290-312)."""
    e = energies.astype(np.float32) * SHOWER_SCALE
    shower = showers.astype(np.float32) * SHOWER_SCALE
    e = np.reshape(e, (-1, 1))
    with contextlib.redirect_stdout(io.StringIO()):
        data, layerE = ref_utils.preprocess_shower(shower.copy(), e.copy(), (-1, 1) + tuple(dims), "", smap, dataset_num=dnum,
                                                   orig_shape=False, ecut=ECUT, max_deposit=MAXDEP)
    E_log = np.log10(e / EMIN) / np.log10(EMAX / EMIN)
    E_lin = (e - EMIN) / (EMAX - EMIN)
    f32 = lambda a: None if a is None else np.ascontiguousarray(np.ma.filled(a, 0.0), dtype=np.float32)  # noqa: E731
    return f32(data), f32(layerE), f32(E_log), f32(E_lin)


def float64_outputs(showers, energies, dims, dnum, smap):
    """The same map in float64, from the float32 quotients the reference forms (constants rounded to float32 as numpy does)."""
    c = {k: np.float64(np.float32(v)) for k, v in DATASET_PARAMS[dnum].items()}
    alpha, one_m = np.float64(np.float32(1e-6)), np.float64(np.float32(1 - 2e-6))
    e = np.reshape(energies.astype(np.float32) * np.float32(SHOWER_SCALE), (-1, 1))
    x = ((showers.astype(np.float32) * np.float32(SHOWER_SCALE)) / (np.float32(MAXDEP) * e)).astype(np.float64)
    logit = lambda t: np.log((alpha + one_m * t) / (1.0 - (alpha + one_m * t)))  # noqa: E731
    layerE = None
    if "layer" in smap:
        layers = x.reshape(B, dims[0], -1).sum(-1)
        total = layers.sum(-1, keepdims=True)
        layerE = np.concatenate([(total - c["totalE_mean"]) / c["totalE_std"],
                                 (logit(layers / total) - c["layers_mean"]) / c["layers_std"]], axis=1)
    return (logit(x) - c["logit_mean"]) / c["logit_std"], layerE


def worst_row(got, want, rows):
    num = np.linalg.norm((got - want).reshape(rows + (-1,)), axis=-1)
    den = np.linalg.norm(want.reshape(rows + (-1,)), axis=-1)
    return float((num / np.maximum(den, 1e-30)).max())


def make_case(tag, dims, dnum, smap, p_zero):
    for seed in range(BASE_SEED, BASE_SEED + 64):
        rng = np.random.default_rng([seed, dnum])
        showers, energies = synth_showers(rng, dims, p_zero)
        data, layerE, E_log, E_lin = reference_outputs(showers, energies, dims, dnum, smap)
        d64, l64 = float64_outputs(showers, energies, dims, dnum, smap)
        w_vox = worst_row(data.astype(np.float64), d64, (B, dims[0]))
        w_lay = worst_row(layerE.astype(np.float64), l64, (B, dims[0] + 1)) if layerE is not None else 0.0
        print(f"{tag} seed {seed}: reference vs float64, worst row: voxels {w_vox:.2e}, layerE {w_lay:.2e}")
        if max(w_vox, w_lay) < WELL_CONDITIONED:
            break
    else:
        raise RuntimeError("no well-conditioned seed")
    zeros = float((showers == 0).mean())
    dep = showers.astype(np.float64).sum(1) / energies[:, 0]
    assert zeros >= 0.6 and (dep < MAXDEP).all() and (showers >= 0).all()
    assert (showers.reshape((B,) + dims)[0, [3, 40]] == 0).all()
    print(f"{tag}: {zeros:.3f} zeros, deposited fraction {dep.min():.3f}..{dep.max():.3f}, "
          f"E {energies.min():.0f}..{energies.max():.0f} MeV")
    # the reference's own round trip, in the loader's units (GeV)
    with contextlib.redirect_stdout(io.StringIO()):
        back, _ = ref_utils.ReverseNormCaloChall(data.reshape((B, 1) + dims).copy(), E_log.copy(), emax=EMAX, emin=EMIN,
                                                 max_deposit=MAXDEP, logE=True, layerE=None if layerE is None else layerE.copy(),
                                                 showerMap=smap, dataset_num=dnum, orig_shape=False, ecut=ECUT)
    raw = showers * np.float32(SHOWER_SCALE)
    back = np.asarray(back, dtype=np.float64).reshape(B, -1)
    rt = float(np.linalg.norm(back - raw) / np.linalg.norm(raw))
    print(f"{tag}: reference round trip rel L2 {rt:.3e}, zero pattern agrees on {((back == 0) == (raw == 0)).mean():.6f}")
    out = {f"{tag}.showers": showers, f"{tag}.incident_energies": energies, f"{tag}.data": data, f"{tag}.E": E_log}
    if layerE is not None:
        out[f"{tag}.layerE"] = layerE
        out[f"{tag}.E_lin"] = E_lin
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(G.GOLD, "preprocess.npz"))
    args = ap.parse_args()
    out = {}
    for case in CASES:
        out.update(make_case(*case))
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}  ({os.path.getsize(args.out) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
