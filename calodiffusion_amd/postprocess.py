"""Inverse pre-processing of generated showers: ``utils.ReverseNorm`` of the reference (calodiffusion/utils/utils.py:253-257,
446-573) for the regular-grid datasets, on the device (``cd_reverse_norm``).

Supported: ``dataset_num`` 2 / 3, ``showerMap`` 'layer-logit-norm' / 'logit-norm' (the shipped Dataset-2 / Dataset-3 configs), and
the HGCal variant ``ReverseNormHGCal`` (utils/HGCal_utils.py:167-292) as two device stages around its geometry decode.  With an
``hgcal.HGCalConverter`` as ``NN_embed`` the decode runs on the device between them (``cd_geom_apply`` / ``cd_geom_decode_sparse``)
and only the final showers are copied to the host; any other ``NN_embed`` is called through the reference's ``dec_batches`` on the
host.

Dataset 0 / 1 (the irregular CaloChallenge binning) run on ``cd_reverse_norm_ds1`` over a ``geom1.GeomConverter``, built from
``binning_file`` or passed as ``geometry=``: the flat form (``orig_shape=True``, the shipped 'orig' configs) with both maps, and
the grid form (``orig_shape=False``: ``unconvert`` inside the launch) with 'logit-norm' -- the reference's own
``preprocess_shower`` fails on a 'layer' map after the conversion, so there is nothing to invert.  There, where float32 exp
overflows (a normalised voxel beyond ~ 88.7 after un-normalising) reverse_logit is its limit 1 instead of the reference's
inf / inf.  Quantile, log, sqrt and scaled maps are not provided."""
import ctypes as C

import numpy as np
import torch

from .abi import _check, _ptr, _stream, load_library

# normalisation constants of the reference (calodiffusion/utils/consts.py:82-116): data, not code
DATASET_PARAMS = {
    2: dict(logit_mean=-12.8564, logit_std=1.9123, totalE_mean=0.3926, totalE_std=0.05546, layers_mean=-6.35551, layers_std=3.90699),
    3: dict(logit_mean=-13.4753, logit_std=1.1070, totalE_mean=0.0, totalE_std=1.0, layers_mean=0.0, layers_std=1.0),
}


# HGCal sets (consts.py:118-181)
DATASET_PARAMS.update({
    100: dict(logit_mean=-13.7371, logit_std=0.68639, totalE_mean=0.0055, totalE_std=0.00018, layers_mean=-4.4450, layers_std=2.37667),
    101: dict(logit_mean=-18.3170, logit_std=1.03153, totalE_mean=0.5538, totalE_std=0.01767, layers_mean=-4.5836, layers_std=2.98382),
    111: dict(logit_mean=-17.3442, logit_std=3.26085, totalE_mean=1.1076, totalE_std=0.03535, layers_mean=-4.5836, layers_std=2.98382),
    120: dict(logit_mean=-18.1561, logit_std=1.56255, totalE_mean=0.5389, totalE_std=0.30325, layers_mean=-6.7899, layers_std=5.64943),
    121: dict(logit_mean=-17.8664, logit_std=2.34207, totalE_mean=1.0270, totalE_std=0.09394, layers_mean=-11.6495, layers_std=7.31088),
})
# (embed_mean, embed_std) of the sets that have them (consts.py:136-137, 150-151, 163-164, 177-178): HGCalConverter's `norm`
HGCAL_EMBED_PARAMS = {101: (0.0835, 3.1083), 111: (0.0, 1.0), 120: (0.0, 1.0), 121: (0.0, 1.0)}
# Dataset 0 / 1 (consts.py:4-80): pions and photons on the converted grid, and + 10 in their original flat shape.  A dict of its
# own: membership in DATASET_PARAMS is what the regular-grid and HGCal functions accept.
DATASET1_PARAMS = {
    0: dict(logit_mean=-12.4783, logit_std=2.21267, totalE_mean=0.0, totalE_std=1.0, layers_mean=0.0, layers_std=1.0),
    10: dict(logit_mean=-11.7610, logit_std=2.84317, totalE_mean=0.2359, totalE_std=0.08255, layers_mean=-4.9742, layers_std=4.89629),
    1: dict(logit_mean=-12.1444, logit_std=2.45056, totalE_mean=0.0, totalE_std=1.0, layers_mean=0.0, layers_std=1.0),
    11: dict(logit_mean=-9.9807, logit_std=3.14168, totalE_mean=0.3123, totalE_std=0.02872, layers_mean=-4.9023, layers_std=5.17364),
}
SHOWER_MAPS = ("layer-logit-norm", "logit-norm")


def refuse_uncovered_map(who, showerMap):
    """Every pre-processing entry point provides SHOWER_MAPS only: name the missing map."""
    if showerMap not in SHOWER_MAPS:
        missing = [k for k in ("quantile", "scaled", "sqrt", "log") if k in showerMap.replace("logit", "")]
        what = "the %s map" % missing[0] if missing else "this map"
        raise NotImplementedError("%s: showerMap '%s' is not provided (%s is missing; %s only)"
                                  % (who, showerMap, what, " / ".join(SHOWER_MAPS)))


def refuse_uncovered_ds1(who, showerMap, orig_shape):
    """The Dataset-0/1 forms neither direction provides, by name."""
    refuse_uncovered_map(who, showerMap)
    if "layer" in showerMap and not orig_shape:
        raise NotImplementedError("%s: a 'layer' map on the converted grid (orig_shape=False) is not provided: the reference's own "
                                  "preprocess_shower fails there (np.sum over axes (3, 4) of the 4-D tensor convert returns), so "
                                  "there are no semantics to follow.  Use the flat form (orig_shape=True, SHOWER_EMBED 'orig...') "
                                  "or 'logit-norm'" % who)


def ds1_geometry(who, dataset_num, binning_file="", geometry=None):
    """The ``geom1.GeomConverter`` of a Dataset-0/1 call: ``geometry`` (a GeomConverter, or an NNConverter, whose ``.gc`` is
    used), else built from the binning file as the reference builds it (utils.py:326-332, 469-472)."""
    from .geom1 import GeomConverter, NNConverter
    if isinstance(geometry, NNConverter):
        return geometry.gc
    if isinstance(geometry, GeomConverter):
        return geometry
    if geometry is not None:
        raise TypeError("%s: geometry must be a geom1.GeomConverter or geom1.NNConverter, not %s" % (who, type(geometry).__name__))
    from .xml_handler import XMLHandler
    return GeomConverter(XMLHandler("photon" if dataset_num == 1 else "pion", binning_file))


def _reverse_ds1(v, energy, layerE, gc, grid_form, c, max_deposit, ecut):
    """(B, V) device tensor: one cd_reverse_norm_ds1 call."""
    rm = gc.radial_map()
    B = v.shape[0]
    per = rm.L * rm.A * rm.R if grid_form else rm.V
    if v.numel() != B * per:
        raise ValueError("ReverseNorm: voxels of %s do not hold %d values each (%s)"
                         % (tuple(v.shape), per, "the (L, alpha, r) grid" if grid_form else "the flat shower"))
    if layerE is not None and tuple(layerE.shape) != (B, rm.L + 1):
        raise ValueError("ReverseNorm: layerE must have shape (batch, 1 + layers) = (%d, %d), got %s" % (B, rm.L + 1, tuple(layerE.shape)))
    if energy.numel() != B:
        raise ValueError("ReverseNorm: %d incident energies for %d showers" % (energy.numel(), B))
    out = torch.empty((B, rm.V), dtype=torch.float32, device="cuda")
    w = gc._fixed_weights()[1] if grid_form else None
    consts = (C.c_double * 6)(c["logit_mean"], c["logit_std"], c["totalE_mean"], c["totalE_std"], c["layers_mean"], c["layers_std"])
    _check(load_library().cd_reverse_norm_ds1(rm.handle, _ptr(w), v.data_ptr(), energy.data_ptr(),
                                              _ptr(layerE), out.data_ptr(), B, consts, float(max_deposit),
                                              float(ecut), _stream()))
    return out


def ReverseNorm(voxels, e, hgcal=False, **kwargs):
    """Same call as the reference's ``utils.ReverseNorm``: returns (data float32 ndarray, energy)."""
    if hgcal:
        return ReverseNormHGCal(voxels, e, **kwargs)
    return ReverseNormCaloChall(voxels, e, **kwargs)


def _staged(v, energy, layerE, dims, c, max_deposit, alpha, layer_eps, stage):
    lib = load_library()
    B = v.shape[0]
    out = torch.empty((B, int(np.prod(dims))), dtype=torch.float32, device="cuda")
    consts = (C.c_float * 6)(c["logit_mean"], c["logit_std"], c["totalE_mean"], c["totalE_std"], c["layers_mean"], c["layers_std"])
    _check(lib.cd_reverse_norm_staged(v.data_ptr(), energy.data_ptr() if energy is not None else None,
                                      layerE.data_ptr() if layerE is not None else None, out.data_ptr(), B,
                                      (C.c_int32 * 3)(*dims), consts, float(max_deposit), 0.0, float(alpha), float(layer_eps),
                                      int(stage), _stream()))
    return out


def ReverseNormHGCal(voxels, e, shape=None, emax=9999.0, emin=0.0001, max_deposit=2, logE=True, layerE=None, showerMap="log",
                     dataset_num=2, orig_shape=False, ecut=0.0, embed=False, NN_embed=None, binning_file="", config=None,
                     sparse_decoding=False, sparse_per_batch=False):
    """``utils.ReverseNormHGCal`` (calodiffusion/utils/HGCal_utils.py:167-292), same arguments and return values.  The incident
    energy is LINEAR in e here (``emin + (emax - emin) e``, :195-199, whatever ``logE`` says), reverse_logit uses alpha 1e-8, the
    energy cut is disabled in the reference (``if ecut > 0 and False``).  ``embed``: ``NN_embed`` decodes between the two device
    stages -- an ``hgcal.HGCalConverter`` on the device (``sparse_decoding`` / ``sparse_per_batch`` included), any other object
    through its ``dec_batches`` on the host (the reference builds an ``HGCalConverter`` from ``binning_file`` when none is given:
    that needs its geometry pickle, so here the converter must be passed in)."""
    if dataset_num not in DATASET_PARAMS:
        raise NotImplementedError("ReverseNormHGCal: no constants for dataset_num %r" % (dataset_num,))
    if "logit" not in showerMap or "norm" not in showerMap or "quantile" in showerMap:
        raise NotImplementedError("ReverseNormHGCal: showerMap '%s' is not provided ([layer-]logit-norm only)" % showerMap)
    c = DATASET_PARAMS[dataset_num]
    e = np.asarray(e, dtype=np.float32)
    gen_out = np.array(emin) + (np.array(emax) - np.array(emin)) * e
    energy = gen_out[:, 0]
    v = torch.as_tensor(voxels, dtype=torch.float32).cuda().contiguous()
    B = v.shape[0]
    data = _staged(v, None, None, (int(np.prod(v.shape[1:])), 1, 1), c, max_deposit, 1e-8, 1e-8, 1).reshape(v.shape)
    if embed:
        if NN_embed is None:
            raise NotImplementedError("ReverseNormHGCal(embed=True) needs the geometry converter (NN_embed): building one takes the "
                                      "geometry file of the HGCalShowers package, which does not ship with the reference")
        from .hgcal import HGCalConverter
        if isinstance(NN_embed, HGCalConverter):
            data = NN_embed.dec(data, sparse_decoding=sparse_decoding, sparse_per_batch=sparse_per_batch)
        else:
            dec = NN_embed.dec_batches(data.cpu().numpy(), sparse_decoding=sparse_decoding, sparse_per_batch=sparse_per_batch)
            data = torch.as_tensor(np.asarray(dec, dtype=np.float32)).cuda().contiguous()
    layer_mode = "layer" in showerMap
    le = None
    if layer_mode:
        assert layerE is not None
        le = torch.as_tensor(np.asarray(layerE, dtype=np.float32)).cuda().contiguous()
        data = data.squeeze()
        if data.dim() != 3 or le.shape != (B, data.shape[1] + 1):
            raise ValueError("ReverseNormHGCal: the layer renormalisation works on decoded showers (batch, layers, cells) with "
                             "layerE (batch, 1 + layers); got %s and %s" % (tuple(data.shape), tuple(le.shape)))
        dims = (data.shape[1], 1, data.shape[2])
    else:
        dims = (1, 1, int(np.prod(data.shape[1:])))
    en = torch.as_tensor(np.ascontiguousarray(energy.reshape(B), dtype=np.float32)).cuda()
    out = _staged(data.contiguous(), en, le, dims, c, max_deposit, 1e-8, 1e-8, 2)
    return out.reshape(data.shape).cpu().numpy(), gen_out


def ReverseNormCaloChall(voxels, e, emax=9999.0, emin=0.0001, config=None, shape=None, binning_file="", max_deposit=2, logE=True,
                         layerE=None, showerMap="log", dataset_num=2, orig_shape=False, ecut=0.0, geometry=None, **kwargs):
    """``utils.ReverseNormCaloChall`` (utils.py:446-573), same arguments and return values: (data (B, voxels) float32 ndarray,
    energy).  Dataset 0 / 1 take the geometry from ``binning_file`` or from ``geometry=`` (a ``geom1.GeomConverter`` or
    ``NNConverter``); ``voxels`` is then (B, V) with ``orig_shape=True`` and (B, [1,] L, A, R) without."""
    if dataset_num in (0, 1):
        if not binning_file and geometry is None:
            raise NotImplementedError("ReverseNorm: dataset_num %r needs the irregular geometry: pass binning_file= (the "
                                      "CaloChallenge binning XML) or geometry= (a geom1.GeomConverter)" % (dataset_num,))
        refuse_uncovered_ds1("ReverseNorm", showerMap, orig_shape)
        gc = ds1_geometry("ReverseNorm", dataset_num, binning_file, geometry)
        e = np.asarray(e, dtype=np.float32)
        energy = emin * (emax / emin) ** e if logE else emin + (emax - emin) * e   # utils.py:480-483, host numpy like the reference
        layer_mode = "layer" in showerMap
        if layer_mode and layerE is None:
            raise AssertionError("layerE is required for a 'layer' shower map")
        v = torch.as_tensor(voxels, dtype=torch.float32).cuda().contiguous()
        en = torch.as_tensor(np.ascontiguousarray(energy.reshape(-1), dtype=np.float32)).cuda()
        le = torch.as_tensor(np.asarray(layerE, dtype=np.float32)).cuda().contiguous() if layer_mode else None
        out = _reverse_ds1(v, en, le, gc, not orig_shape, DATASET1_PARAMS[dataset_num + (10 if orig_shape else 0)], max_deposit, ecut)
        return out.cpu().numpy(), energy
    if dataset_num not in DATASET_PARAMS or orig_shape:
        raise NotImplementedError("ReverseNorm: only the regular-grid datasets 2 and 3 are provided (and Dataset 0 / 1 with a "
                                  "binning file or geometry)")
    if showerMap not in ("layer-logit-norm", "logit-norm"):
        raise NotImplementedError("ReverseNorm: showerMap '%s' is not provided" % showerMap)
    c = DATASET_PARAMS[dataset_num]
    e = np.asarray(e, dtype=np.float32)
    energy = emin * (emax / emin) ** e if logE else emin + (emax - emin) * e   # utils.py:480-483, host numpy like the reference
    layer_mode = "layer" in showerMap
    if layer_mode and layerE is None:
        raise AssertionError("layerE is required for a 'layer' shower map")
    v = torch.as_tensor(voxels, dtype=torch.float32).cuda().contiguous()
    B, D, H, W = v.shape[0], v.shape[-3], v.shape[-2], v.shape[-1]
    en = torch.as_tensor(np.ascontiguousarray(energy.reshape(B), dtype=np.float32)).cuda()
    le = torch.as_tensor(np.asarray(layerE, dtype=np.float32)).cuda().contiguous() if layer_mode else None
    if le is not None and tuple(le.shape) != (B, D + 1):
        raise ValueError("ReverseNorm: layerE must have shape (batch, 1 + layers)")
    out = torch.empty((B, D * H * W), dtype=torch.float32, device="cuda")
    lib = load_library()
    dims = (C.c_int32 * 3)(D, H, W)
    consts = (C.c_float * 6)(c["logit_mean"], c["logit_std"], c["totalE_mean"], c["totalE_std"], c["layers_mean"], c["layers_std"])
    _check(lib.cd_reverse_norm(v.data_ptr(), en.data_ptr(), le.data_ptr() if le is not None else None, out.data_ptr(), B,
                               dims, consts, float(max_deposit), float(ecut), _stream()))
    return out.cpu().numpy(), energy
