"""Generate tests/golden/hlf.npz from the reference's own ``HighLevelFeatures`` (calodiffusion/utils/HighLevelFeatures.py) and
``XMLHandler`` on seeded showers, and the two regular-grid binning files it reads them with (data: the CaloChallenge XML format).

TEST INFRASTRUCTURE, like oracle/gen_golden.py: runs only where the reference is mounted, on the CPU, and imports it through that
script's stub-import preamble (by importing the script).  Only data is written.

    MPLBACKEND=Agg python tools/gen_golden_hlf.py [--out-dir DIR]      # default tests/golden

(The reference class imports matplotlib at module level; Agg needs no display.)

Geometries:
  small   binning_reg_small.xml (written here)   electron, 5 layers x 16 alpha x 9 r, V = 720
  wide    binning_reg_wide.xml (written here)    electron, 3 layers x 50 alpha x 18 r, 900 voxels a layer (Dataset 3's), V = 2700
  photon  binning_ds1_synthetic.xml              photon, V = 368, offsets 0, 8, 168, 358, 363
  pion    binning_ds0_synthetic.xml              pion, V = 323; the ids 12-14 of its layers 5-7 exercise the reference's quirk: a
                                                 layer has centres when its INDEX is among the ids of the alpha-binned layers,
                                                 so layer 6 (id 13, 10 alpha bins) has none
Showers, 8 per geometry, float32: about 30 % of the voxels non-zero, those 10^u with u uniform in [-3, 3); shower 0 is all zero;
shower 1 has one non-zero voxel in every layer with more than one alpha bin and nothing else.

Stored per geometry (prefix "<tag>."): the showers and incident energies; the reference's attributes (bin_edges, relevantLayers,
layersBinnedInAlpha, num_alpha, num_voxel, r_edges concatenated with r_edges_n their lengths, eta / phi of all layers
concatenated in layer order, float64); and its features -- E_tot, E_layers (8, R) in relevantLayers order (float32), centre_layers
(the keys of EC_etas) and EC_etas / EC_phis / width_etas / width_phis (8, K) in that order (float64).

``FDP.pre_process`` (train/evaluate.py:26-47) is not run: evaluate.py imports jetnet, which is not installed here.  The test of
``feature_matrix`` writes that formula out over the reference's values stored here.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REGULAR = {  # tag: (file, layers, alpha bins, radial bins, radial bin width in mm)
    "small": ("binning_reg_small.xml", 5, 16, 9, 4.65),
    "wide": ("binning_reg_wide.xml", 3, 50, 18, 2.325),
}
IRREGULAR = {"photon": ("binning_ds1_synthetic.xml", "photon"), "pion": ("binning_ds0_synthetic.xml", "pion")}
N_SHOWERS = 8


def write_regular_binning(path, layers, n_alpha, n_r, r_width, particle="electron", pid=11):
    """A CaloChallenge binning file of a regular cylinder: `layers` layers of n_alpha x n_r voxels, radial edges k * r_width."""
    edges = ",".join(repr(float(k * r_width)) for k in range(n_r + 1))
    lines = ['<?xml version="1.0" encoding="UTF-8"?>', "<Bins>", f'  <Bin pid="{pid}" etaMin="0" etaMax="130" name="{particle}">']
    lines += [f'    <Layer id="{l}" r_edges="{edges}" n_bin_alpha="{n_alpha}"/>' for l in range(layers)]
    lines += ["  </Bin>", "</Bins>", ""]
    with open(path, "w") as fh:
        fh.write("\n".join(lines))


def seeded_showers(rng, hlf):
    V = hlf.bin_edges[-1]
    x = np.where(rng.random((N_SHOWERS, V)) < 0.3, 10.0 ** rng.uniform(-3.0, 3.0, (N_SHOWERS, V)), 0.0).astype(np.float32)
    x[0] = 0.0
    x[1] = 0.0
    binned = [l for l, n in zip(hlf.relevantLayers, hlf.num_alpha) if n > 1]
    for l in binned:
        x[1, rng.integers(hlf.bin_edges[l], hlf.bin_edges[l + 1])] = np.float32(10.0 ** rng.uniform(-1.0, 2.0))
    return x


def one_geometry(tag, path, particle, seed, RefHLF):
    hlf = RefHLF(particle, filename=path)
    rng = np.random.default_rng(seed)
    x = seeded_showers(rng, hlf)
    energies = (10.0 ** rng.uniform(0.0, 3.0, (N_SHOWERS, 1))).astype(np.float32)
    hlf.CalculateFeatures(x)
    keys = list(hlf.EC_etas)
    assert list(hlf.E_layers) == list(hlf.relevantLayers) and keys == list(hlf.EC_phis) == list(hlf.width_etas) == list(hlf.width_phis)
    out = {
        "showers": x, "energies": energies,
        "bin_edges": np.array(hlf.bin_edges, dtype=np.int64), "relevantLayers": np.array(hlf.relevantLayers, dtype=np.int64),
        "layersBinnedInAlpha": np.array(hlf.layersBinnedInAlpha, dtype=np.int64), "num_alpha": np.array(hlf.num_alpha, dtype=np.int64),
        "num_voxel": np.array(hlf.num_voxel, dtype=np.int64),
        "r_edges": np.concatenate([np.asarray(r, dtype=np.float64) for r in hlf.r_edges]),
        "r_edges_n": np.array([len(r) for r in hlf.r_edges], dtype=np.int64),
        "eta": np.concatenate(hlf.eta_all_layers).astype(np.float64), "phi": np.concatenate(hlf.phi_all_layers).astype(np.float64),
        "E_tot": hlf.E_tot, "E_layers": np.stack([hlf.E_layers[l] for l in hlf.relevantLayers], axis=1),
        "centre_layers": np.array(keys, dtype=np.int64),
    }
    for name in ("EC_etas", "EC_phis", "width_etas", "width_phis"):
        d = getattr(hlf, name)
        out[name] = np.stack([d[l] for l in keys], axis=1)
        assert out[name].dtype == np.float64
    assert out["E_tot"].dtype == np.float32 and out["E_layers"].dtype == np.float32
    assert [len(e) for e in hlf.eta_all_layers] == list(np.diff(hlf.bin_edges))
    print(f"{tag}: V {hlf.bin_edges[-1]}, layers with voxels {hlf.relevantLayers}, with centres {keys}")
    return {f"{tag}.{k}": v for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    from oracle import gen_golden as G  # noqa: F401  (stubs the absent modules and puts the reference on sys.path)
    from calodiffusion.utils.HighLevelFeatures import HighLevelFeatures as RefHLF
    assert RefHLF.__module__ == "calodiffusion.utils.HighLevelFeatures" and "reference" in sys.modules[RefHLF.__module__].__file__

    data = {}
    for i, (tag, (name, layers, n_alpha, n_r, width)) in enumerate(REGULAR.items()):
        path = os.path.join(args.out_dir, name)
        write_regular_binning(path, layers, n_alpha, n_r, width)
        print(f"wrote {path}")
        data.update(one_geometry(tag, path, "electron", G.SEED + 90 + i, RefHLF))
    for i, (tag, (name, particle)) in enumerate(IRREGULAR.items()):
        data.update(one_geometry(tag, os.path.join(REPO, "tests", "golden", name), particle, G.SEED + 95 + i, RefHLF))  # committed files
    path = os.path.join(args.out_dir, "hlf.npz")
    np.savez_compressed(path, **data)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
