"""Generate tests/golden/shower_stats.npz from the reference's own plot classes (calodiffusion/utils/plots.py) and
``utils.apply_mask_conserveE`` on seeded showers.

TEST INFRASTRUCTURE, like oracle/gen_golden.py: runs only where the reference is mounted, on the CPU, and imports it through that
script's stub-import preamble (by importing the script; it stubs mplhep and h5py).  Only data is written.

    MPLBACKEND=Agg python tools/gen_golden_shower_stats.py [--out-dir DIR]      # default tests/golden

Nothing is drawn: ``Plot._plot`` and ``Plot._hist`` are replaced by recorders that keep the dictionary of arrays (and the
``binning=``) each class hands over and return ``MagicMock`` axes, ``save_names`` returns no names, and ``HGCal_utils.load_geom``
returns the synthetic geometry built here.

Geometries: the grids (5, 16, 9), (3, 50, 18) and (2, 3, 5) as SHAPE_FINAL (-1, 1, L, A, R), and an HGCal geometry of 3 layers
with 37, 30 and 21 real cells (max_ncell 37; the maps are 40 wide, as a geometry file's are wider than max_ncell) and 5, 4 and 3
rings.  Cells beyond a layer's count are ordinary cells at ring 0 and x = y = 0, and are lit like any other.

Showers: two samples of 8 per geometry ("Geant4", "CaloDiffusion"), float32, about 30 % of the cells non-zero, those 10^u with u
uniform in [-3, 3).  Shower 0 is all zero; shower 1 has one cell per layer; layer 1 of shower 3 is exactly zero; layer 0 of
shower 4 holds a single cell of 1e-7 of the shower (a non-zero layer below the 1e-6 rule); shower 2 holds, for each of 1e-3, 1e-6
and EMIN, the float32 threshold and its two float32 neighbours.
Margins asserted here, so that the reference itself is unambiguous and no case has to be left out of a comparison: apart from the
planted values no cell is within relative 1e-3 of 1e-3, 1e-6 or EMIN; no non-zero layer sum is within a factor 2 of 1e-6 of its
shower; every row of the cut keeps at least a quarter of its energy, all of it, or none.

Stored per geometry (prefix "<tag>."): ``shape`` (the plot shape), ``showers.<sample>``, ``energies.<sample>``; for every class
``<Class>.<call>.<sample>`` (the array of that sample in the class's call number <call> of _plot / _hist) and
``<Class>.<call>.binning`` where one was passed; ``cut.in`` (the CaloDiffusion sample with negative cells planted), ``cut.out``
(= apply_mask_conserveE(cut.in, cut.in < EMIN)), ``cut.mask`` and ``cut.masked`` (the same with a seeded mask); for HGCal the
geometry arrays ``geom.*``.
"""
from __future__ import annotations

import argparse
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = {"g5x16x9": (5, 16, 9), "g3x50x18": (3, 50, 18), "g2x3x5": (2, 3, 5)}
HGCAL_NCELLS, HGCAL_NRINGS, HGCAL_WIDTH = (37, 30, 21), (5, 4, 3), 40
N_SHOWERS = 8
EMIN = 0.05
SAMPLES = ("Geant4", "CaloDiffusion")
THRESHOLDS = (1e-3, 1e-6, EMIN)
GRID_CLASSES = ("ELayer", "SparsityLayer", "AverageShowerWidth", "AverageER", "AverageEPhi", "HistEtot", "HistERatio", "HistNhits",
                "HistMaxE", "HistMaxELayer", "HistVoxelE")
HGCAL_CLASSES = ("ELayer", "SparsityLayer", "HistEtot", "HistERatio", "HistNhits", "HistMaxE", "HistMaxELayer", "HistVoxelE",
                 "RadialEnergyHGCal", "RCenterHGCal", "PhiCenterHGCal")


def synthetic_hgcal(rng):
    L = len(HGCAL_NCELLS)
    geom = types.SimpleNamespace(nlayers=L, ncells=np.array(HGCAL_NCELLS), nrings=np.array(HGCAL_NRINGS),
                                 xmap=np.zeros((L, HGCAL_WIDTH)), ymap=np.zeros((L, HGCAL_WIDTH)), ring_map=np.zeros((L, HGCAL_WIDTH)))
    for l, (n, rings) in enumerate(zip(HGCAL_NCELLS, HGCAL_NRINGS)):
        ring = rng.integers(0, rings, n)
        ring[:rings] = np.arange(rings)  # every ring is used
        rad = (ring + rng.uniform(0.1, 0.9, n)) * 1.2
        ang = rng.uniform(0.0, 2.0 * np.pi, n)
        geom.xmap[l, :n], geom.ymap[l, :n], geom.ring_map[l, :n] = rad * np.sin(ang), rad * np.cos(ang), ring
    return geom


def loaded(geom):
    """What HGCal_utils.load_geom adds to the unpickled object."""
    out = types.SimpleNamespace(**vars(geom))
    out.theta_map = np.arctan2(out.xmap, out.ymap) % (2.0 * np.pi)
    out.max_ncell = int(round(np.amax(out.ncells)))
    return out


def near(x, thr):
    return (x != 0) & (np.abs(x.astype(np.float64) / thr - 1.0) < 1e-3)


def seeded_showers(rng, L, n):
    """(N_SHOWERS, L, n) float32 with the special showers of the module docstring."""
    x = np.where(rng.random((N_SHOWERS, L, n)) < 0.3, 10.0 ** rng.uniform(-3.0, 3.0, (N_SHOWERS, L, n)), 0.0).astype(np.float32)
    for thr in THRESHOLDS:
        x[near(x, thr)] *= np.float32(1.01)
    x[0] = 0.0
    x[1] = 0.0
    for l in range(L):
        x[1, l, rng.integers(n)] = np.float32(10.0 ** rng.uniform(-1.0, 2.0))
    x[3, 1] = 0.0
    x[4, 0] = 0.0
    x[4, 0, rng.integers(n)] = np.float32(1e-7 * x[4].astype(np.float64).sum())
    planted = np.zeros(x.shape, dtype=bool)
    cells = rng.choice(L * n, 9, replace=False)
    k = 0
    for thr in THRESHOLDS:
        t = np.float32(thr)
        for v in (np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(1))):
            x[2].reshape(-1)[cells[k]] = v
            planted[2].reshape(-1)[cells[k]] = True
            k += 1
    for thr in THRESHOLDS:
        assert not (near(x, thr) & ~planted).any(), thr
    layer = x.astype(np.float64).sum(-1)
    total = layer.sum(-1, keepdims=True)
    ratio = layer[layer > 0] / np.broadcast_to(1e-6 * total, layer.shape)[layer > 0]
    assert not ((ratio > 0.5) & (ratio < 2.0)).any()
    assert (layer[4, 0] > 0) and layer[4, 0] < 0.5e-6 * total[4, 0]
    return x


def cut_margin(x, mask):
    """Rows (last axis) that keep some but less than a quarter of their energy."""
    c = np.maximum(x.astype(np.float64), 0.0)
    T, K = c.sum(-1), np.where(mask, 0.0, c).sum(-1)
    return (K > 0) & (K < T) & (K < 0.25 * T)


def cut_cases(rng, x, apply_mask_conserveE):
    """cut.* of one geometry from the CaloDiffusion sample x in its plot shape."""
    x = x.copy()
    neg = (rng.random(x.shape) < 0.05)
    x[neg] = -(10.0 ** rng.uniform(-3.0, -1.0, x.shape)).astype(np.float32)[neg]
    bad = cut_margin(x, x < EMIN)
    x[bad[..., None] & (x < EMIN)] = 0.0  # such a row loses nothing
    assert not cut_margin(x, x < EMIN).any()
    mask = rng.random(x.shape) < 0.5
    mask[cut_margin(x, mask)] = False
    mask.reshape(-1, x.shape[-1])[0] = True  # one row with nothing kept
    assert not cut_margin(x, mask).any()
    out = apply_mask_conserveE(x.copy(), x < EMIN)
    masked = apply_mask_conserveE(x.copy(), mask)
    assert out.dtype == np.float32 and masked.dtype == np.float32
    return {"cut.in": x, "cut.out": out, "cut.mask": mask, "cut.masked": masked, "cut.emin": np.float64(EMIN)}


def run_classes(plots, names, config, data, energies, records):
    flags = types.SimpleNamespace(plot_extensions=["png"], plot_reshape=False, cms=False, plot_folder="", generated="", plot_label="")
    out = {}
    for name in names:
        del records[:]
        getattr(plots, name)(flags, config)(dict(data), energies)
        for call, (feed, binning) in enumerate(records):
            for sample in SAMPLES:
                out[f"{name}.{call}.{sample}"] = np.array(feed[sample])
            if binning is not None:
                out[f"{name}.{call}.binning"] = np.asarray(binning, dtype=np.float64)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    from oracle import gen_golden as G  # noqa: F401  (stubs the absent modules and puts the reference on sys.path)
    from calodiffusion.utils import plots, utils as ref_utils
    import calodiffusion.utils.HGCal_utils as ref_hgcal
    assert "reference" in plots.__file__ and "reference" in ref_utils.__file__

    records = []

    def record(self, feed_dict, *a, binning=None, **kw):
        records.append(({k: np.array(v) for k, v in feed_dict.items()}, binning))
        return MagicMock(), MagicMock()

    plots.Plot._plot = record
    plots.Plot._hist = record
    plots.Plot.save_names = lambda self, plot_name: []
    plots.Plot.save_fig = lambda self, name, fig, ax0: None

    data = {}
    for i, (tag, (L, A, R)) in enumerate(GRIDS.items()):
        rng = np.random.default_rng(G.SEED + 300 + i)
        shape = (-1, 1, L, A, R)
        showers = {s: seeded_showers(rng, L, A * R).reshape(shape) for s in SAMPLES}
        energies = (10.0 ** rng.uniform(0.0, 3.0, (N_SHOWERS, 1))).astype(np.float32)
        config = {"SHAPE_FINAL": list(shape), "CHECKPOINT_NAME": "x"}
        out = run_classes(plots, GRID_CLASSES, config, showers, energies, records)
        out.update(cut_cases(rng, showers["CaloDiffusion"], ref_utils.apply_mask_conserveE))
        out.update({"shape": np.array(shape), "energies": energies, **{f"showers.{s}": v for s, v in showers.items()}})
        data.update({f"{tag}.{k}": v for k, v in out.items()})
        print(f"{tag}: {len(out)} arrays")

    rng = np.random.default_rng(G.SEED + 310)
    geom = synthetic_hgcal(rng)
    ref_hgcal.load_geom = lambda filename: loaded(geom)
    L, n = len(HGCAL_NCELLS), max(HGCAL_NCELLS)
    showers = {s: seeded_showers(rng, L, n) for s in SAMPLES}  # (N, L, cells), as the HGCal classes index them
    energies = (10.0 ** rng.uniform(0.0, 3.0, (N_SHOWERS, 1))).astype(np.float32)
    config = {"SHAPE_FINAL": [-1, 1, L, 4, 4], "SHAPE_PAD": [-1, 1, L, n], "HGCAL": True, "BIN_FILE": "synthetic", "CHECKPOINT_NAME": "x"}
    out = run_classes(plots, HGCAL_CLASSES, config, showers, energies, records)
    out.update(cut_cases(rng, showers["CaloDiffusion"], ref_utils.apply_mask_conserveE))
    out.update({"shape": np.array((-1, L, n)), "energies": energies, **{f"showers.{s}": v for s, v in showers.items()}})
    out.update({f"geom.{k}": np.asarray(getattr(geom, k)) for k in ("ncells", "nrings", "xmap", "ymap", "ring_map")})
    data.update({f"hgcal.{k}": v for k, v in out.items()})
    print(f"hgcal: {len(out)} arrays")

    path = os.path.join(args.out_dir, "shower_stats.npz")
    np.savez_compressed(path, **data)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
