"""What the Dataset-0/1 pre-processing fixture (tools/gen_golden_ds1_preprocess.py), its host tests and its GPU tests share: the
two synthetic geometries, the cases and their configs."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
XML = {"ph": os.path.join(HERE, "golden", "binning_ds1_synthetic.xml"), "pi": os.path.join(HERE, "golden", "binning_ds1_synthetic2.xml")}
# tag -> (dataset_num, orig_shape, showerMap)
CASES = {"ph.flat.layer": (1, True, "layer-logit-norm"), "ph.flat.plain": (1, True, "logit-norm"),
         "ph.grid.plain": (1, False, "logit-norm"), "pi.flat.layer": (0, True, "layer-logit-norm")}
TAGS = tuple(CASES)
# (V, (L, A, R), layer offsets) of the two geometries
SHAPES = {"ph": (368, (5, 10, 30), [0, 8, 168, 358, 363, 368]), "pi": (97, (3, 4, 17), [0, 5, 73, 97])}
B = 8
SCALE = np.float32(0.001)  # DataLoaderCaloChall's shower_scale: the fixture's MeV -> the loader's GeV
_geom = {}


def config(tag, **over):
    """The shipped Dataset-1 photon config (the reference's pion config has the same constants) over the case's geometry."""
    from calodiffusion_amd.configs import load_config
    dnum, orig, smap = CASES[tag]
    V, grid, _ = SHAPES[tag[:2]]
    cfg = dict(load_config("dataset1_photon"))
    cfg.update(BIN_FILE=XML[tag[:2]], DATASET_NUM=dnum, SHOWERMAP=smap, SHOWER_EMBED="orig-NN" if orig else "NN",
               PART_TYPE="photon" if dnum == 1 else "pion", SHAPE_ORIG=[-1, V], SHAPE_PAD=[-1, 1, V], SHAPE_FINAL=[-1, 1, *grid])
    cfg.update(over)
    return cfg


def geometry(tag):
    """The geom1.GeomConverter of a case's binning file (one per file: its device handle is reused)."""
    from calodiffusion_amd import geom1, xml_handler
    key = tag[:2]
    if key not in _geom:
        _geom[key] = geom1.GeomConverter(xml_handler.XMLHandler("photon" if key == "ph" else "pion", XML[key]))
    return _geom[key]


def segments(tag):
    """Row boundaries of the case's voxel tensor: the ragged layers (flat) or L equal layers (grid)."""
    V, (L, A, R), bound = SHAPES[tag[:2]]
    return bound if CASES[tag][1] else [i * A * R for i in range(L + 1)]


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def worst_row(got, want, seg):
    """The largest rel L2 over the (shower, segment) rows."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    worst = 0.0
    for lo, hi in zip(seg, seg[1:]):
        num, den = np.linalg.norm(got[:, lo:hi] - want[:, lo:hi], axis=1), np.linalg.norm(want[:, lo:hi], axis=1)
        worst = max(worst, float((num / np.maximum(den, 1e-30)).max()))
    return worst
