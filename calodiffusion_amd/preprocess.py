"""Forward pre-processing of raw showers into training tensors: ``utils.preprocess_shower`` and the incident-energy map of
``DataLoaderCaloChall`` of the reference (calodiffusion/utils/utils.py:290-312, 315-436) for the regular-grid datasets, on the
device (``cd_preprocess``).  The inverse of ``postprocess.ReverseNorm``, for the same configurations.

Supported: ``dataset_num`` 2 / 3, ``showerMap`` 'layer-logit-norm' / 'logit-norm' (the shipped Dataset-2 / Dataset-3 configs),
regular grid (``orig_shape=False``).  Dataset-0/1 (geometry conversion from the binning XML), ``orig_shape``, the quantile /
log / sqrt / scaled maps and HGCal's ``preprocess_hgcal_shower`` are not provided.  Reading the HDF5 file stays the caller's.

A shower without energy (incident energy <= 0, or no deposit at all) is where the reference's masked arrays hand back
unspecified fill values; here such a row raises ``ValueError`` and nothing is returned.  An empty LAYER of a shower that has
energy elsewhere is ordinary data."""
import ctypes as C

import numpy as np
import torch

from . import engine
from .postprocess import DATASET_PARAMS

SHOWER_MAPS = ("layer-logit-norm", "logit-norm")


def _refuse_uncovered(who, showerMap, dataset_num, orig_shape):
    if orig_shape:
        raise NotImplementedError("%s: orig_shape=True (the irregular Dataset-0/1 binning) is not provided" % who)
    if dataset_num in (0, 1):
        raise NotImplementedError("%s: dataset_num %r needs the geometry conversion from the binning XML (GeomConverter), which "
                                  "is not provided; only the regular-grid datasets 2 and 3 are" % (who, dataset_num))
    if dataset_num not in (2, 3):
        raise NotImplementedError("%s: no pre-processing for dataset_num %r (regular-grid datasets 2 and 3 only; HGCal's "
                                  "preprocess_hgcal_shower is not provided)" % (who, dataset_num))
    if showerMap not in SHOWER_MAPS:
        missing = [k for k in ("quantile", "scaled", "sqrt", "log") if k in showerMap.replace("logit", "")]
        what = "the %s map" % missing[0] if missing else "this map"
        raise NotImplementedError("%s: showerMap '%s' is not provided (%s is missing; %s only)"
                                  % (who, showerMap, what, " / ".join(SHOWER_MAPS)))


def _device_f32(a, name):
    """numpy array or tensor (host or device) -> contiguous fp32 device tensor; the values are not touched."""
    if isinstance(a, torch.Tensor):
        return a.detach().to(device="cuda", dtype=torch.float32).contiguous()
    a = np.asarray(a)
    if a.dtype == object:
        raise TypeError("%s must be a numeric array" % name)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _run(shower, e, dims, showerMap, dataset_num, max_deposit, emin, emax, logE, shower_scale):
    """(data (B,1,D,H,W), layerE (B,D+1) or None, E (B,1)): device tensors, one cd_preprocess call and one flag read."""
    D, H, W = (int(d) for d in dims)
    v = _device_f32(shower, "shower")
    if v.dim() < 2 or v.numel() != v.shape[0] * D * H * W:
        raise ValueError("preprocess: showers of %s do not hold %d x %d x %d voxels each" % (tuple(v.shape), D, H, W))
    B = v.shape[0]
    if B == 0:
        raise ValueError("preprocess: no showers")
    en = _device_f32(e, "e").reshape(-1)
    if en.numel() != B:
        raise ValueError("preprocess: %d incident energies for %d showers" % (en.numel(), B))
    c = DATASET_PARAMS[dataset_num]
    out = torch.empty((B, 1, D, H, W), dtype=torch.float32, device="cuda")
    layerE = torch.empty((B, D + 1), dtype=torch.float32, device="cuda") if "layer" in showerMap else None
    e_out = torch.empty((B, 1), dtype=torch.float32, device="cuda")
    status = torch.empty((1,), dtype=torch.int32, device="cuda")
    lib = engine.load_library()
    consts = (C.c_float * 6)(c["logit_mean"], c["logit_std"], c["totalE_mean"], c["totalE_std"], c["layers_mean"], c["layers_std"])
    engine._check(lib.cd_preprocess(v.data_ptr(), en.data_ptr(), out.data_ptr(), engine._ptr(layerE), e_out.data_ptr(),
                                    status.data_ptr(), B, (C.c_int32 * 3)(D, H, W), consts, float(max_deposit), float(emin),
                                    float(emax), int(bool(logE)), float(shower_scale), engine._stream()))
    bad = int(status.item())
    if bad:
        raise ValueError("preprocess: shower %d (the last such row of this call) has no energy -- incident energy <= 0 or no "
                         "deposit at all; the reference's masked arrays return unspecified fill values there.  Drop such rows "
                         "before the call" % (bad - 1))
    return out, layerE, e_out


def preprocess_shower(shower, e, shape, binning_file="", showerMap="log-norm", dataset_num=2, orig_shape=False, ecut=0,
                      max_deposit=2):
    """``utils.preprocess_shower`` (utils.py:315-436), same arguments and return values: (shower (B, D*H*W) float32 ndarray,
    layerE (B, 1+D) float32 ndarray or None).  ``shower`` and ``e`` are already in the loader's units (the reference's loader
    multiplies by shower_scale before this call); ``shape`` is the config's SHAPE_PAD, (-1, 1, D, H, W).  ``ecut`` only
    matters to the quantile maps, which are not provided."""
    _refuse_uncovered("preprocess_shower", showerMap, dataset_num, orig_shape)
    dims = tuple(shape)[-3:]
    # the incident-energy map is not part of this function: emin / emax only have to be valid
    out, layerE, _ = _run(shower, e, dims, showerMap, dataset_num, max_deposit, 1.0, 2.0, False, 1.0)
    return out.reshape(out.shape[0], -1).cpu().numpy(), None if layerE is None else layerE.cpu().numpy()


class Preprocess:
    """Raw CaloChallenge showers -> one loader batch on the device.

    Built from the config keys ``generate()`` needs as well: SHAPE_PAD (or SHAPE_FINAL), EMAX, EMIN, logE, MAXDEP, SHOWERMAP,
    DATASET_NUM.  ``shower_scale`` is ``DataLoaderCaloChall``'s (utils.py:276, 290-291): 0.001 turns the files' MeV into GeV;
    pass 1.0 for arrays that are already scaled.  Called with ``showers`` (B, D*H*W) (any shape with that many voxels per
    row) and ``incident_energies`` (B,) or (B, 1), numpy arrays or tensors; returns device tensors ``(E, layers, data)`` in
    the order of a loader batch: E (B, 1), layers (B, 1+D) (None for a map without layer energies), data (B, 1, D, H, W) --
    ready for ``compute_loss(data, E, noise, layers)``."""

    def __init__(self, config, shower_scale=0.001):
        if config.get("HGCAL", False):
            raise NotImplementedError("Preprocess: HGCal's preprocess_hgcal_shower (its embedding needs the geometry file) is "
                                      "not provided")
        missing = [k for k in ("EMAX", "EMIN", "logE", "MAXDEP", "SHOWERMAP") if k not in config]
        shape = config.get("SHAPE_PAD", config.get("SHAPE_FINAL"))
        if shape is None:
            missing.append("SHAPE_PAD")
        if missing:
            raise ValueError("Preprocess: the config lacks %s" % ", ".join(missing))
        self.dataset_num = config.get("DATASET_NUM", 2)
        self.showerMap = config["SHOWERMAP"]
        _refuse_uncovered("Preprocess", self.showerMap, self.dataset_num, False)
        self.dims = tuple(int(d) for d in shape[-3:])
        self.emax, self.emin, self.logE = float(config["EMAX"]), float(config["EMIN"]), bool(config["logE"])
        self.max_deposit = float(config["MAXDEP"])
        self.shower_scale = float(shower_scale)

    def __call__(self, showers, incident_energies):
        data, layers, E = _run(showers, incident_energies, self.dims, self.showerMap, self.dataset_num, self.max_deposit,
                               self.emin, self.emax, self.logE, self.shower_scale)
        return E, layers, data
