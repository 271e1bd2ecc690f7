"""Shared by the HGCal forward pre-processing tests: the cases of tests/golden/preprocess_hgcal.npz
(tools/gen_preprocess_hgcal_golden.py), the config a test builds for one, and the converter rebuilt from the stored geometry."""
import functools
import types

import numpy as np

from conftest import gold

SCALE = 200.0
# (geometry, set, map key): 'l' = 'layer-logit-norm', 'n' = 'logit-norm'
CASES = [("g", 111, "l"), ("g", 111, "n"), ("g", 101, "l"), ("g", 101, "n"), ("h", 111, "l"), ("h", 101, "l")]
MAPS = {"l": "layer-logit-norm", "n": "logit-norm"}
BATCH = {"g": 8, "h": 4}


def bins(tag):
    return [int(b) for b in gold("preprocess_hgcal")[f"{tag}.bins"]]


def config(tag, dnum, m):
    """The values of the reference's config_HGCal.json on top of the shipped hgcal config, on the fixture's grid."""
    from calodiffusion_amd.configs import load_config
    shape = [-1, 1] + bins(tag)
    return dict(load_config("hgcal"), EMAX=[100, 2.01, 1.572], EMIN=[50, 1.99, 1.57], MAXDEP=1.0, logE=False, ECUT=0.001,
                SHOWERSCALE=200, SHOWERMAP=MAPS[m], DATASET_NUM=dnum, SHAPE_PAD=shape, SHAPE_FINAL=shape)


def geometry(tag):
    g = gold("preprocess_hgcal")
    ncells = g[f"{tag}.ncells"]
    return types.SimpleNamespace(ncells=ncells, ring_map=g[f"{tag}.ring_map"], theta_map=g[f"{tag}.theta_map"],
                                 nlayers=len(ncells), max_ncell=int(round(np.amax(ncells))))


@functools.lru_cache(maxsize=None)
def converter(tag, dnum):
    """What the loader builds: HGCalConverter over the geometry, init(norm=True, dataset_num) (HGCal_utils.py:136-142)."""
    from calodiffusion_amd.hgcal import HGCalConverter
    return HGCalConverter.from_geometry(geometry(tag), bins(tag), norm=True, dataset_num=dnum)


def embedded(g, tag, dnum):
    """The reference's embedded grid; for "h" set 101 (not stored) the stored set-111 grid through set 101's affine, as torch
    forms it: float32 subtraction, then float32 division."""
    key = f"{tag}.{dnum}.emb"
    if key in g.files:
        return g[key]
    from calodiffusion_amd.postprocess import HGCAL_EMBED_PARAMS
    mean, std = HGCAL_EMBED_PARAMS[dnum]
    return ((g[f"{tag}.111.emb"] - np.float32(mean)) / np.float32(std)).astype(np.float32)
