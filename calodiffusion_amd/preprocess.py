"""Forward pre-processing of raw showers into training tensors: ``utils.preprocess_shower`` and the incident-energy map of
``DataLoaderCaloChall`` of the reference (calodiffusion/utils/utils.py:290-312, 315-436) for the regular-grid datasets, on the
device (``cd_preprocess``).  The inverse of ``postprocess.ReverseNorm``, for the same configurations.

Supported: ``dataset_num`` 2 / 3, ``showerMap`` 'layer-logit-norm' / 'logit-norm' (the shipped Dataset-2 / Dataset-3 configs),
regular grid (``orig_shape=False``).  The quantile / log / sqrt / scaled maps are not provided.  Reading the HDF5 file stays
the caller's.

Dataset 0 / 1 (the irregular CaloChallenge binning) have their own pair, ``preprocess_shower(..., binning_file, dataset_num=0|1)``
and ``PreprocessDS1`` (on ``cd_preprocess_ds1`` over a ``geom1.GeomConverter``): the flat form (``orig_shape=True``, SHOWER_EMBED
'orig...': both maps, layer energies over the ragged layer segments) and the grid form (``orig_shape=False``: ``convert`` inside
the launch, 'logit-norm' only -- the reference's own function fails on a 'layer' map there).

HGCal has its own pair, ``preprocess_hgcal_shower`` and ``PreprocessHGCal`` (``DataLoaderHGCal``, utils/HGCal_utils.py:20-164,
on ``cd_preprocess_hgcal``): raw cells through the geometry map of an ``hgcal.HGCalConverter`` to a loader batch in one launch.

A shower without energy (incident energy <= 0, or no deposit at all) is where the reference's masked arrays hand back
unspecified fill values; here such a row raises ``ValueError`` and nothing is returned.  An empty LAYER of a shower that has
energy elsewhere is ordinary data."""
import ctypes as C

import numpy as np
import torch

from .abi import _check, _ptr, _stream, _upload, load_library
from .postprocess import (DATASET1_PARAMS, DATASET_PARAMS, SHOWER_MAPS, ds1_geometry, refuse_uncovered_ds1,  # noqa: F401
                          refuse_uncovered_map)


def _refuse_uncovered(who, showerMap, dataset_num, orig_shape):
    if dataset_num in (0, 1):
        raise NotImplementedError("%s: dataset_num %r needs the irregular geometry of the binning XML: pass binning_file to "
                                  "preprocess_shower, or use PreprocessDS1(config, geometry); without one only the regular-grid "
                                  "datasets 2 and 3 are provided" % (who, dataset_num))
    if orig_shape:
        raise NotImplementedError("%s: orig_shape=True is the irregular Dataset-0/1 binning; dataset_num %r is not provided in it"
                                  % (who, dataset_num))
    if dataset_num not in (2, 3):
        raise NotImplementedError("%s: no pre-processing for dataset_num %r (regular-grid datasets 2 and 3 only; HGCal's "
                                  "preprocess_hgcal_shower is not provided)" % (who, dataset_num))
    refuse_uncovered_map(who, showerMap)


_device_f32 = lambda a, name: _upload(a, torch.float32, name)  # noqa: E731  (numpy array or tensor, host or device)


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
    lib = load_library()
    consts = (C.c_float * 6)(c["logit_mean"], c["logit_std"], c["totalE_mean"], c["totalE_std"], c["layers_mean"], c["layers_std"])
    _check(lib.cd_preprocess(v.data_ptr(), en.data_ptr(), out.data_ptr(), _ptr(layerE), e_out.data_ptr(),
                             status.data_ptr(), B, (C.c_int32 * 3)(D, H, W), consts, float(max_deposit), float(emin),
                             float(emax), int(bool(logE)), float(shower_scale), _stream()))
    bad = int(status.item())
    if bad:
        raise ValueError("preprocess: shower %d (the last such row of this call) has no energy -- incident energy <= 0 or no "
                         "deposit at all; the reference's masked arrays return unspecified fill values there.  Drop such rows "
                         "before the call" % (bad - 1))
    return out, layerE, e_out


def _run_ds1(shower, e, gc, grid_form, showerMap, dataset_num, max_deposit, emin, emax, logE, shower_scale):
    """(data (B, V) or (B,1,L,A,R), layerE (B,1+L) or None, E (B,1)): device tensors, one cd_preprocess_ds1 call and one flag
    read.  ``gc``: the geom1.GeomConverter; ``grid_form``: convert inside the launch."""
    rm = gc.radial_map()
    v = _device_f32(shower, "shower")
    if v.dim() < 2 or v.numel() != v.shape[0] * rm.V:
        raise ValueError("preprocess: showers of %s do not hold the geometry's %d voxels each" % (tuple(v.shape), rm.V))
    B = v.shape[0]
    if B == 0:
        raise ValueError("preprocess: no showers")
    en = _device_f32(e, "e").reshape(-1)
    if en.numel() != B:
        raise ValueError("preprocess: %d incident energies for %d showers" % (en.numel(), B))
    c = DATASET1_PARAMS[dataset_num + (0 if grid_form else 10)]
    out = torch.empty((B, 1, rm.L, rm.A, rm.R) if grid_form else (B, rm.V), dtype=torch.float32, device="cuda")
    layerE = torch.empty((B, rm.L + 1), dtype=torch.float32, device="cuda") if "layer" in showerMap else None
    e_out = torch.empty((B, 1), dtype=torch.float32, device="cuda")
    status = torch.empty((1,), dtype=torch.int32, device="cuda")
    w = gc._fixed_weights()[0] if grid_form else None
    consts = (C.c_double * 6)(c["logit_mean"], c["logit_std"], c["totalE_mean"], c["totalE_std"], c["layers_mean"], c["layers_std"])
    _check(load_library().cd_preprocess_ds1(rm.handle, _ptr(w), v.data_ptr(), en.data_ptr(), out.data_ptr(),
                                            _ptr(layerE), e_out.data_ptr(), status.data_ptr(), B, consts,
                                            float(max_deposit), float(emin), float(emax), int(bool(logE)),
                                            float(shower_scale), _stream()))
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
    matters to the quantile maps, which are not provided.

    ``dataset_num`` 0 / 1 with a ``binning_file``: the geometry is read from it (pions / photons); returns (B, V) with
    ``orig_shape=True`` and (B, L*A*R) -- the converted grid -- without, and layerE (B, 1 + L)."""
    if dataset_num in (0, 1) and binning_file:
        refuse_uncovered_ds1("preprocess_shower", showerMap, orig_shape)
        gc = ds1_geometry("preprocess_shower", dataset_num, binning_file)
        # the incident-energy map is not part of this function: emin / emax only have to be valid
        out, layerE, _ = _run_ds1(shower, e, gc, not orig_shape, showerMap, dataset_num, max_deposit, 1.0, 2.0, False, 1.0)
        return out.reshape(out.shape[0], -1).cpu().numpy(), None if layerE is None else layerE.cpu().numpy()
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
            raise NotImplementedError("Preprocess: an HGCal config needs preprocess_hgcal_shower and the geometry map: use "
                                      "PreprocessHGCal(config, geometry)")
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


class PreprocessDS1:
    """Raw CaloChallenge Dataset-0/1 showers -> one loader batch on the device: what ``DataLoaderCaloChall`` (utils.py:260-312)
    does after reading the file, in one ``cd_preprocess_ds1`` call.  The peer of ``PreprocessHGCal``.

    Built from the config keys EMAX, EMIN, logE, MAXDEP, SHOWERMAP, DATASET_NUM (0 pions, 1 photons), SHAPE_ORIG, SHAPE_FINAL and
    SHOWER_EMBED: with 'orig' in it (the shipped configs) the flat form, ``data`` (B, V), the state of a model with an
    ``NN_embed``; otherwise the grid form, ``data`` (B, 1, L, A, R), ``GeomConverter.convert`` inside the launch.  ``geometry`` is
    a ``geom1.GeomConverter``, a ``geom1.NNConverter`` (its ``.gc`` gives the layout; the fixed area-weighted matrices convert,
    as in the reference's loader) or None: built from BIN_FILE.  Called with ``showers`` (B, V) and ``incident_energies`` (B,) or
    (B, 1), numpy arrays or tensors; returns device tensors ``(E (B, 1), layers (B, 1+L) or None, data)`` -- ready for
    ``compute_loss(data, E, noise, layers)``."""

    def __init__(self, config, geometry=None, shower_scale=0.001):
        missing = [k for k in ("EMAX", "EMIN", "logE", "MAXDEP", "SHOWERMAP", "DATASET_NUM") if k not in config]
        if missing:
            raise ValueError("PreprocessDS1: the config lacks %s" % ", ".join(missing))
        self.dataset_num, self.showerMap = config["DATASET_NUM"], config["SHOWERMAP"]
        if self.dataset_num not in (0, 1):
            raise NotImplementedError("PreprocessDS1: dataset_num %r is not an irregular CaloChallenge set (0 pions, 1 photons); "
                                      "use Preprocess or PreprocessHGCal" % (self.dataset_num,))
        self.grid_form = "orig" not in config.get("SHOWER_EMBED", "")
        refuse_uncovered_ds1("PreprocessDS1", self.showerMap, not self.grid_form)
        if geometry is None and not config.get("BIN_FILE"):
            raise ValueError("PreprocessDS1: the config lacks BIN_FILE and no geometry was given")
        self.geometry = gc = ds1_geometry("PreprocessDS1", self.dataset_num, config.get("BIN_FILE", ""), geometry)
        bound, _, _ = gc.descriptor()
        if "SHAPE_ORIG" in config and int(config["SHAPE_ORIG"][-1]) != bound[-1]:
            raise ValueError("PreprocessDS1: the geometry has %d voxels, SHAPE_ORIG says %d" % (bound[-1], config["SHAPE_ORIG"][-1]))
        have = (int(gc.num_layers), int(gc.alpha_out), int(gc.dim_r_out))
        if "SHAPE_FINAL" in config and tuple(int(d) for d in config["SHAPE_FINAL"][-3:]) != have:
            raise ValueError("PreprocessDS1: the geometry maps onto (layers, alpha_out, dim_r_out) = %s, SHAPE_FINAL says %s"
                             % (have, tuple(config["SHAPE_FINAL"][-3:])))
        self.emax, self.emin, self.logE = float(config["EMAX"]), float(config["EMIN"]), bool(config["logE"])
        self.max_deposit = float(config["MAXDEP"])
        self.shower_scale = float(shower_scale)

    def __call__(self, showers, incident_energies):
        data, layers, E = _run_ds1(showers, incident_energies, self.geometry, self.grid_form, self.showerMap, self.dataset_num,
                                   self.max_deposit, self.emin, self.emax, self.logE, self.shower_scale)
        return E, layers, data


# ---- HGCal ---------------------------------------------------------------------------------------------------------------------
HGCAL_SETS = (100, 101, 111, 120, 121)
# the on-chip limits of cd_preprocess_hgcal's fused form (include/calodiff.h)
FUSED_GRID_BYTES, FUSED_MAX_CELLS, FUSED_MAX_LAYERS = 48 * 1024, 2048, 512


def _refuse_uncovered_hgcal(who, showerMap, dataset_num, orig_shape):
    if orig_shape:
        raise NotImplementedError("%s: orig_shape=True is not provided" % who)
    if dataset_num not in HGCAL_SETS:
        raise NotImplementedError("%s: no HGCal constants for dataset_num %r (the HGCal sets are %s)"
                                  % (who, dataset_num, ", ".join(str(n) for n in HGCAL_SETS)))
    refuse_uncovered_map(who, showerMap)


def _run_hgcal(showers, gen_info, bins, showerMap, dataset_num, max_deposit, emin, emax, conv=None, max_cells=None,
               shower_scale=1.0, fused=True):
    """(data (B,1,L,A,R), layerE (B,1+L) or None, E (B,k)): device tensors, one cd_preprocess_hgcal call and one flag read.
    ``conv`` None: ``showers`` are already on the grid.  Otherwise raw cells (B, L, >= max_cells); a grid beyond the fused
    form's on-chip limit (or ``fused=False``) runs the composition, ``conv.enc`` then the grid form: the same bits."""
    L, A, R = (int(d) for d in bins)
    v = _device_f32(showers, "showers")
    B = v.shape[0] if v.dim() else 0
    if B == 0:
        raise ValueError("preprocess_hgcal: no showers")
    g = _device_f32(gen_info, "gen_info")
    if g.dim() == 1:
        g = g.reshape(-1, 1)
    k = len(emin)
    if g.dim() != 2 or tuple(g.shape) != (B, k):
        raise ValueError("preprocess_hgcal: gen_info of %s for %d showers and %d EMIN / EMAX columns" % (tuple(g.shape), B, k))
    lib = load_library()
    handle, cells, stride, mean, std = None, A * R, A * R, 0.0, 1.0
    if conv is None:
        if v.numel() != B * L * A * R:
            raise ValueError("preprocess_hgcal: showers of %s do not hold %d x %d x %d grid values each" % (tuple(v.shape), L, A, R))
    else:
        pm = conv.embeder.packed()
        n = pm.cols if max_cells is None else int(max_cells)
        if v.dim() != 3 or v.shape[1] != L or v.shape[2] < n or n != pm.cols or (pm.layers, pm.rows) != (L, A * R):
            raise ValueError("preprocess_hgcal: showers of %s are not (batch, %d layers, >= %d cells) for a geometry map of "
                             "(%d, %d, %d)" % (tuple(v.shape), L, n, pm.layers, pm.rows, pm.cols))
        std, mean = conv._affine()
        if fused and 4 * L * A * R <= FUSED_GRID_BYTES and n <= FUSED_MAX_CELLS and L <= FUSED_MAX_LAYERS:
            handle, cells, stride = pm.handle, n, int(v.shape[2])
        else:
            v = conv.enc(v[:, :, :n] * float(shower_scale)).contiguous()
    c = DATASET_PARAMS[dataset_num]
    out = torch.empty((B, 1, L, A, R), dtype=torch.float32, device="cuda")
    layerE = torch.empty((B, L + 1), dtype=torch.float32, device="cuda") if "layer" in showerMap else None
    e_out = torch.empty((B, k), dtype=torch.float32, device="cuda")
    status = torch.empty((1,), dtype=torch.int32, device="cuda")
    consts = (C.c_double * 6)(c["logit_mean"], c["logit_std"], c["totalE_mean"], c["totalE_std"], c["layers_mean"], c["layers_std"])
    _check(lib.cd_preprocess_hgcal(handle, v.data_ptr(), stride, g.data_ptr(), k, out.data_ptr(), _ptr(layerE),
                                   e_out.data_ptr(), status.data_ptr(), B, L, cells, A * R, consts, float(mean), float(std),
                                   float(max_deposit), (C.c_double * k)(*emin), (C.c_double * k)(*emax),
                                   float(shower_scale), _stream()))
    bad = int(status.item())
    if bad:
        raise ValueError("preprocess_hgcal: shower %d (the last such row of this call) has an incident energy <= 0, NaN or inf; "
                         "the reference's masked arrays return unspecified fill values there.  Drop such rows before the call"
                         % (bad - 1))
    return out, layerE, e_out


def preprocess_hgcal_shower(shower, e, shape, showerMap="log-norm", dataset_num=2, orig_shape=False, ecut=0, max_deposit=2):
    """``preprocess_hgcal_shower`` (utils/HGCal_utils.py:20-86), same arguments and return values: (shower float32 ndarray shaped
    like the input, layerE (B, 1+L) float32 ndarray or None).  ``shower`` is the EMBEDDED shower (..., L, alpha, r) in the
    loader's units and ``e`` the incident energies (B,); ``shape`` and ``ecut`` are not used by the reference either.  A layer
    without deposit and a shower without any are defined results (the masked logit); only ``e`` <= 0, NaN or inf raises."""
    _refuse_uncovered_hgcal("preprocess_hgcal_shower", showerMap, dataset_num, orig_shape)
    dims = tuple(shower.shape)
    if len(dims) < 4:
        raise ValueError("preprocess_hgcal_shower: the embedded shower is (batch, ..., layers, alpha, r); got %s" % (dims,))
    # the condition map is not part of this function: emin / emax only have to be valid
    out, layerE, _ = _run_hgcal(shower, _device_f32(e, "e").reshape(-1, 1), dims[-3:], showerMap, dataset_num, max_deposit,
                                [0.0], [1.0])
    return out.reshape(dims).cpu().numpy(), None if layerE is None else layerE.cpu().numpy()


class PreprocessHGCal:
    """Raw HGCal cell energies -> one loader batch on the device: what ``DataLoaderHGCal(embed=True)`` (utils/HGCal_utils.py:89-164)
    does after reading the file, in one ``cd_preprocess_hgcal`` call.

    Built from the config keys that loader is called with: SHAPE_PAD / SHAPE_FINAL, EMAX and EMIN (lists, one entry per
    ``gen_info`` column, or scalars), MAXDEP, SHOWERMAP, DATASET_NUM, SHOWERSCALE (200.0 when absent; the ``shower_scale``
    argument overrides it) and MAX_CELLS (the geometry's when absent).  ``geometry`` is an ``hgcal.HGCalConverter``; its
    ``norm`` / ``embed_mean`` / ``embed_std`` are used as they are, so the loader's ``init(norm=True, dataset_num)`` is the
    caller's, as for ``generate(geometry=)``.  Called with ``showers`` (B, L, >= max_cells) and ``gen_info`` (B,) / (B, k), numpy
    arrays or tensors; returns device tensors ``(E (B, k), layers (B, 1+L) or None, data (B, 1, L, A, R))`` -- ready for
    ``compute_loss(data, E, noise, layers)``."""

    def __init__(self, config, geometry, shower_scale=None):
        from .hgcal import HGCalConverter
        if not isinstance(geometry, HGCalConverter):
            raise TypeError("PreprocessHGCal: geometry must be an hgcal.HGCalConverter, not %s" % type(geometry).__name__)
        missing = [k for k in ("EMAX", "EMIN", "MAXDEP", "SHOWERMAP", "DATASET_NUM") if k not in config]
        shape = config.get("SHAPE_PAD", config.get("SHAPE_FINAL"))
        if shape is None:
            missing.append("SHAPE_PAD")
        if missing:
            raise ValueError("PreprocessHGCal: the config lacks %s" % ", ".join(missing))
        self.dataset_num, self.showerMap = config["DATASET_NUM"], config["SHOWERMAP"]
        _refuse_uncovered_hgcal("PreprocessHGCal", self.showerMap, self.dataset_num, False)
        self.bins = tuple(int(d) for d in shape[-3:])
        if self.bins != (geometry.num_layers, geometry.num_alpha_bins, geometry.num_r_bins):
            raise ValueError("PreprocessHGCal: the config's grid %s is not the geometry's %s"
                             % (self.bins, (geometry.num_layers, geometry.num_alpha_bins, geometry.num_r_bins)))
        self.emin = [float(x) for x in np.atleast_1d(config["EMIN"])]
        self.emax = [float(x) for x in np.atleast_1d(config["EMAX"])]
        if len(self.emin) != len(self.emax):
            raise ValueError("PreprocessHGCal: EMIN and EMAX differ in length")
        self.max_deposit = float(config["MAXDEP"])
        self.shower_scale = float(config.get("SHOWERSCALE", 200.0) if shower_scale is None else shower_scale)
        self.max_cells = None if config.get("MAX_CELLS") is None else int(config["MAX_CELLS"])
        self.geometry = geometry
        self.fused = True

    def __call__(self, showers, gen_info):
        data, layers, E = _run_hgcal(showers, gen_info, self.bins, self.showerMap, self.dataset_num, self.max_deposit, self.emin,
                                     self.emax, conv=self.geometry, max_cells=self.max_cells, shower_scale=self.shower_scale,
                                     fused=self.fused)
        return E, layers, data
