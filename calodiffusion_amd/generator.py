"""Generator files: one self-contained blob per model, from which the C ABI generates showers without Python.

``export_generator(model, sample_steps)`` writes everything ``Diffusion.generate`` / ``LayerDiffusion.generate`` need for one
regular-grid model -- the U-Net's descriptor, coordinate profiles and weights, LayerDiffusion's layer model, each stage's compiled
sampler exactly as the Python path hands it to the library, and the inverse pre-processing record -- in the format DESIGN.md
("Generator file") documents.  It runs on the CPU.  ``cd_generator_create`` / ``cd_generator_run`` (include/calodiff.h) turn the
file into "incident energies in, physical showers out"; ``Generator`` is the thin ctypes wrapper over them, and
tools/cd_generate_example.c the same from C.

Scope: DATASET_NUM 2 / 3 (format version 1) and HGCal (format version 2, whose ``GEOM`` section carries the geometry maps by
their sparse entries: the decoder of a pre-embedded model's ``geometry=`` converter, or both maps of a model with the converter
inside) and Dataset 0 / 1 (format version 3, whose ``RADL`` section carries the irregular layout as ``cd_radial_create`` takes it and
the matrices in ``cd_radial_enc`` / ``cd_radial_dec`` layout: encoder and decoder of a model with SHOWER_EMBED 'orig-NN', or the
un-conversion matrices of the ``geometry=`` converter of a model on the converted grid) with a ``[layer-]logit-norm`` map, any
width the plan takes, any sampler that compiles to a CdStep table or to a step
program that does not depend on the batch.  Everything else is refused at export, by name.
"""
from __future__ import annotations

import ctypes as C
import os
import struct
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import engine
from .abi import LIB_PATH, CdGeneratorRun, Handle, WorkspaceCache, _check, _dev32, _nbytes, _ptr, _stream, load_library, require_gpu

MAGIC = b"CDGENBLB"
FORMAT_VERSION = 1       # regular-grid files: written as they always were, byte for byte
FORMAT_VERSION_GEOM = 2  # HGCal files: a GEOM section, energy columns, per-column EMAX / EMIN in RNRM
FORMAT_VERSION_RADIAL = 3  # Dataset-0/1 files: a RADL section, the float64 constants of cd_reverse_norm_ds1 in RNRM
STAGED_ALPHA = STAGED_LAYER_EPS = 1e-8  # ReverseNormHGCal's reverse_logit alpha and layer threshold (postprocess.py)
HEADER_BYTES, SECTION_ENTRY_BYTES, ALIGN = 64, 24, 64
WEIGHT_RECORD_BYTES, WEIGHT_NAME_BYTES = 112, 96
TAG_META, TAG_UNET, TAG_LAYER, TAG_UNET_SAMPLER, TAG_LAYER_SAMPLER, TAG_REVNORM = b"META", b"UNET", b"LAYR", b"USMP", b"LSMP", b"RNRM"
TAG_GEOM = b"GEOM"
TAG_RADIAL = b"RADL"


def fnv1a64(data: bytes) -> int:
    """64-bit FNV-1a, the file's checksum: the library's loop (cd_generator_checksum, host code) when it is built, else the same
    loop in Python (a few seconds for a 10 MB file)."""
    data = bytes(data)
    if os.path.exists(LIB_PATH):
        out = C.c_uint64()
        _check(load_library().cd_generator_checksum(data, len(data), C.byref(out)))
        return int(out.value)
    return fnv1a64_py(data)


def fnv1a64_py(data: bytes) -> int:
    h = 0xCBF29CE484222325
    for b in bytes(data):
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def _pad(b: bytes, align: int) -> bytes:
    return b + b"\0" * (-len(b) % align)


class _Capture:
    """Stands where the model stands in a sampler call and records what the sampler hands to the engine: the CdStep table
    (``ddim_sample``) or the step program (``sampler_run``), with ``use_graph``.  Everything else is the model's own (schedule
    tables, loss function, config), so the compiled sampler is the one the Python path would run."""

    def __init__(self, model):
        self._model = model
        self.table = self.program = None
        self.use_graph = True

    def __getattr__(self, name):
        return getattr(self._model, name)

    def engine(self):
        return self

    def cond_tensor(self, E, layers):
        return None

    def step_noise_stream(self, start):
        return 0, 0

    def denoise(self, *a, **k):
        raise NotImplementedError("export_generator: this sampler calls the model back from the host: it has no table or program")

    def ddim_sample(self, start, cond, steps, use_graph=True, **kw):
        self.table = np.ascontiguousarray(steps, dtype=np.float32)
        self.use_graph = bool(use_graph)
        return start, None, None

    def sampler_run(self, start, cond, program, use_graph=True, **kw):
        self.program = program
        self.use_graph = bool(use_graph)
        return start, None, None


def compile_sampler(model, sampler, num_steps: int, sample_offset: int, state_shape) -> dict:
    """What ``sampler(model, start, ...)`` passes to the library for these steps: {'table': (n, 4) fp32} or {'program': Program},
    with 'use_graph' and 'noise_tensors_drawn'."""
    from . import sample
    name = type(sampler).__name__
    if isinstance(sampler, sample.DPMAdaptive):
        raise NotImplementedError(f"export_generator: {name} decides every step on the host (a loop around denoise): it has no device "
                                  "table or program to export")
    if isinstance(sampler, sample.BespokeNonStationary):
        raise NotImplementedError(f"export_generator: {name}'s step program carries a sigma column per sample: it depends on the "
                                  "batch and cannot be compiled once")
    cap = _Capture(model)
    sampler(cap, torch.zeros((1,) + tuple(state_shape)), None, None, num_steps, sample_offset, False)
    out = dict(use_graph=cap.use_graph, noise_tensors_drawn=int(sampler.noise_tensors_drawn))
    if cap.program is not None:
        out["program"] = cap.program
    elif cap.table is not None:
        out["table"] = cap.table
    else:
        raise NotImplementedError(f"export_generator: {name} handed the library neither a step table nor a program")
    return out


def _sampler_section(c: dict) -> bytes:
    if "table" in c:
        t = c["table"]
        head = struct.pack("<8if", 0, t.shape[0], 0, 0, 0, 0, c["noise_tensors_drawn"], int(c["use_graph"]), 1.0)
        return _pad(head, 64) + t.astype("<f4").tobytes()
    p = c["program"]
    coefs = np.ascontiguousarray(p.coefs, dtype="<f4")
    n_steps, n_coef = coefs.shape
    ops = engine._pack_ops(p).astype("<i4")
    head = struct.pack("<8if", 1, n_steps, len(p.ops), n_coef, p.n_bufs, int(p.op_begin is not None), c["noise_tensors_drawn"],
                       int(c["use_graph"]), float(p.start_scale))
    body = ops.tobytes()
    if p.op_begin is not None:
        assert len(p.op_begin) == n_steps + 1
        body += np.asarray(p.op_begin, dtype="<i4").tobytes()
    return _pad(head, 64) + body + coefs.tobytes()


def _net_section(desc, state_dict, coords=()) -> bytes:
    """UNET / LAYR: header, descriptor, coordinate profiles, the weight records, then the fp32 tensors (64-byte aligned)."""
    desc = bytes(desc)
    coords = [np.ascontiguousarray(a, dtype="<f4") for a in coords]
    n_coord = [len(a) for a in coords] + [0] * (3 - len(coords))
    items = [(k, v.detach().to("cpu", torch.float32).contiguous().numpy()) for k, v in state_dict.items()]
    front = struct.pack("<8I", len(desc), len(items), *n_coord, 0, 0, 0) + _pad(desc, 8) + b"".join(a.tobytes() for a in coords)
    off = len(front) + WEIGHT_RECORD_BYTES * len(items)
    off += -off % 64
    records, data = b"", b""
    for name, arr in items:
        raw = name.encode()
        if len(raw) >= WEIGHT_NAME_BYTES:
            raise ValueError(f"export_generator: tensor name {name!r} is longer than {WEIGHT_NAME_BYTES - 1} bytes")
        records += raw.ljust(WEIGHT_NAME_BYTES, b"\0") + struct.pack("<QQ", arr.size, off + len(data))
        data += _pad(arr.astype("<f4").tobytes(), 64)
    return _pad(front + records, 64) + data


def _geom_map_record(m, layers: int) -> bytes:
    """One map of the GEOM section: {rows, cols, nnz, is_mask}, then row_ptr, col_idx, val, each piece 64-byte aligned.  The
    pattern is the one ``m.packed()`` has: the non-zeros of a frozen map, the mask of a trainable one."""
    from .hgcal import map_entries
    row_ptr, col_idx, val = map_entries(m.mat, m.mask if m.trainable else None)
    rows, cols = (int(v) for v in m.mat.shape[1:])
    assert row_ptr.shape == (layers * rows + 1,)
    return (_pad(struct.pack("<4i", rows, cols, len(col_idx), int(m.trainable)), 64) + _pad(row_ptr.astype("<i4").tobytes(), 64) +
            _pad(col_idx.astype("<i4").tobytes(), 64) + _pad(val.astype("<f4").tobytes(), 64))


def _geom_section(conv, form: int) -> bytes:
    """GEOM: {form, L, A, R, N, n_maps, embed_mean, embed_std} and the decoder (form 0), or the encoder then the decoder (form 1)."""
    L, A, R = conv.num_layers, conv.num_alpha_bins, conv.num_r_bins
    N = int(conv.decoder.mat.shape[1])
    std, mean = conv._affine()
    maps = [conv.decoder] if form == 0 else [conv.embeder, conv.decoder]
    head = struct.pack("<6i2f", form, L, A, R, N, len(maps), float(mean), float(std))
    return _pad(head, 64) + b"".join(_geom_map_record(m, L) for m in maps)


def _hgcal_form(model, geometry):
    """None for a regular-grid model; else (form, converter) of an HGCal model, or the refusal by name."""
    from .hgcal import HGCalConverter
    from .postprocess import DATASET_PARAMS
    cfg = model.config
    if not (cfg.get("HGCAL", False) or getattr(model, "hgcal", False)):
        if geometry is not None:
            raise ValueError("export_generator: geometry= is for HGCal models (a pre-embedded one's converter); this model has none")
        return None
    if getattr(model, "do_embed", False):
        if not isinstance(model.NN_embed, HGCalConverter):
            raise NotImplementedError("export_generator: an HGCal model with an in-model embedding (do_embed) that is not an "
                                      "hgcal.HGCalConverter is not provided")
        if geometry is not None:
            raise ValueError("export_generator: this HGCal model has its converter inside (do_embed): the file takes model.NN_embed, "
                             "geometry= must not be given")
        form, conv = 1, model.NN_embed
    else:
        if geometry is None:
            raise NotImplementedError("export_generator: a pre-embedded HGCal model needs its geometry maps in the file: pass "
                                      "geometry=<hgcal.HGCalConverter>, what generate(geometry=) takes")
        if not isinstance(geometry, HGCalConverter):
            raise TypeError("export_generator(geometry=) takes an hgcal.HGCalConverter")
        if geometry.trainable:
            raise NotImplementedError("export_generator: the geometry= converter of a pre-embedded HGCal model must be frozen "
                                      "(trainable=False): the sampled decode's view holds values, not a trainable map's mask")
        form, conv = 0, geometry
    if cfg.get("DATASET_NUM") not in DATASET_PARAMS:
        raise NotImplementedError(f"export_generator: no HGCal constants for DATASET_NUM {cfg.get('DATASET_NUM')!r} "
                                  "(postprocess.DATASET_PARAMS)")
    grid = tuple(int(v) for v in cfg["SHAPE_FINAL"][2:])
    if (conv.num_layers, conv.num_alpha_bins, conv.num_r_bins) != grid:
        raise ValueError(f"export_generator: the converter maps onto (layers, alpha, r) = "
                         f"{(conv.num_layers, conv.num_alpha_bins, conv.num_r_bins)}, SHAPE_FINAL gives the U-Net the grid {grid}")
    return form, conv


class _Radial(NamedTuple):
    """What a Dataset-0/1 file carries of its geometry (``_radial_form``)."""
    form: int    # 0 on the converted grid, 1 in-model
    gc: object   # the geom1.GeomConverter: the layout
    mats: list   # form 1: [encoder, decoder]; form 0: [un-conversion], each the flat fp32 concatenation over the layers


def _radial_section(gc, form: int, mats) -> bytes:
    """RADL: {form, L, alpha_out, r_out, V, n_mats, wtotal}, then bound[L + 1], alpha[L], rin[L] (int32) and the matrices (fp32, each
    the concatenation cd_radial_enc / cd_radial_dec take), every piece 64-byte aligned."""
    bound, alpha, rin = gc.descriptor()
    L, A, R = int(gc.num_layers), int(gc.alpha_out), int(gc.dim_r_out)
    wtotal = R * sum(rin)
    mats = [np.ascontiguousarray(m, dtype="<f4").reshape(-1) for m in mats]
    assert len(mats) == form + 1 and all(m.size == wtotal for m in mats)
    head = struct.pack("<7i", form, L, A, R, bound[-1], len(mats), wtotal)
    ints = b"".join(_pad(np.asarray(v, dtype="<i4").tobytes(), 64) for v in (bound, alpha, rin))
    return _pad(head, 64) + ints + b"".join(_pad(m.tobytes(), 64) for m in mats)


def _radial_form(model, geometry):
    """The ``_Radial`` record of a Dataset-0/1 model, or the refusal by name.  Form 1: SHOWER_EMBED 'orig-NN', the
    converter inside the model -- its trained encoder and decoder go into the file.  Form 0: a model on the converted grid with the
    ``geometry=`` converter ``generate(geometry=)`` takes -- its fixed un-conversion matrices (``GeomConverter.pinv_mats``)."""
    from .geom1 import GeomConverter, NNConverter
    from .postprocess import refuse_uncovered_ds1
    cfg = model.config
    dnum, embed = cfg.get("DATASET_NUM"), cfg.get("SHOWER_EMBED", "")
    if getattr(model, "do_embed", False):
        if not isinstance(model.NN_embed, NNConverter) or "orig" not in embed:
            raise NotImplementedError(f"export_generator: a Dataset-{dnum} model with an in-model embedding (do_embed) other than a "
                                      "geom1.NNConverter over the flat shower (SHOWER_EMBED 'orig-NN') is not provided")
        if geometry is not None:
            raise ValueError(f"export_generator: this Dataset-{dnum} model has its converter inside (do_embed, SHOWER_EMBED 'orig-NN'): "
                             "the file takes model.NN_embed, geometry= must not be given")
        pad, final = cfg.get("SHAPE_PAD") or cfg["SHAPE_FINAL"], [int(v) for v in cfg["SHAPE_FINAL"]]
        if len(pad) < 3 or int(pad[2]) != final[2]:
            raise NotImplementedError(f"export_generator: Dataset {dnum} with SHAPE_PAD {list(pad)} is not provided: a generator file "
                                      f"serves CaloDiffusion and LayerDiffusion of one config, and the two-stage model exists for "
                                      f"SHAPE_PAD = SHAPE_FINAL = {final} only (with 'orig-NN' the state is SHAPE_ORIG either way)")
        conv = model.NN_embed
        mats = [torch.cat([lay.weight.detach().reshape(-1) for lay in part]).to("cpu", torch.float32).numpy() for part in (conv.encs, conv.decs)]
        form, gc = 1, conv.gc
    else:
        if "orig" in embed:
            raise NotImplementedError(f"export_generator: a Dataset-{dnum} model on the flat shower without an in-model converter "
                                      f"(SHOWER_EMBED {embed!r}) is not provided")
        if geometry is None:
            raise NotImplementedError(f"export_generator: Dataset {dnum} on the converted grid needs its irregular geometry in the "
                                      "file: pass geometry=<geom1.GeomConverter or NNConverter>, what generate(geometry=) takes")
        if not isinstance(geometry, (GeomConverter, NNConverter)):
            raise TypeError("export_generator(geometry=) on a Dataset-0/1 config takes a geom1.GeomConverter or NNConverter")
        refuse_uncovered_ds1("export_generator", cfg.get("SHOWERMAP", ""), False)  # a 'layer' map on the grid: no layerE there
        form, gc = 0, geometry.gc if isinstance(geometry, NNConverter) else geometry
        mats = [torch.cat([m.reshape(-1) for m in gc.pinv_mats]).to("cpu", torch.float32).numpy()]
    grid = tuple(int(v) for v in cfg["SHAPE_FINAL"][2:])
    have = (int(gc.num_layers), int(gc.alpha_out), int(gc.dim_r_out))
    if have != grid:
        raise ValueError(f"export_generator: the converter maps onto (layers, alpha_out, dim_r_out) = {have}, SHAPE_FINAL gives the "
                         f"U-Net the grid {grid}")
    return _Radial(form, gc, mats)


def _refuse_out_of_scope(model, debug, geometry=None):
    """Raises for what a generator file does not hold, by name; returns (``_hgcal_form``'s (form, converter) or None,
    ``_radial_form``'s record or None): at most one of the two is set."""
    cfg = model.config
    if debug:
        raise NotImplementedError("export_generator: a debug trajectory request is not part of a generator file (cd_generator_run "
                                  "returns showers only)")
    hgcal = cfg.get("HGCAL", False) or getattr(model, "hgcal", False)
    radial = _radial_form(model, geometry) if not hgcal and cfg.get("DATASET_NUM", 2) in (0, 1) else None
    geom = _hgcal_form(model, geometry) if radial is None else None
    if geom is None and radial is None:  # a regular grid (the two forms above have their own checks)
        if cfg.get("DATASET_NUM", 2) not in (2, 3):
            raise NotImplementedError(f"export_generator: Dataset {cfg.get('DATASET_NUM')} is not provided (DATASET_NUM 0 to 3 and HGCal)")
        if getattr(model, "do_embed", False) or getattr(model, "NN_embed", None) is not None:
            raise NotImplementedError("export_generator: a model with an in-model geometry embedding (do_embed) is not provided: its "
                                      "maps would have to be in the file")
    if cfg.get("SHOWERMAP") not in ("layer-logit-norm", "logit-norm"):
        raise NotImplementedError(f"export_generator: SHOWERMAP {cfg.get('SHOWERMAP')!r} is not provided ([layer-]logit-norm only)")
    missing = [k for k in ("EMAX", "EMIN", "logE", "MAXDEP", "ECUT") if k not in cfg]
    if missing:
        raise ValueError(f"export_generator: the config lacks {missing}: the inverse pre-processing record needs them")
    return geom, radial


def export_generator(model, sample_steps: int, sample_offset: int = 0, path: Optional[str] = None, debug: bool = False,
                     geometry=None) -> bytes:
    """The generator file of ``model`` (a ``CaloDiffusion`` or ``LayerDiffusion`` as constructed from its config) for
    ``model.generate(loader, sample_steps, sample_offset=sample_offset)``; also written to ``path`` when given.  ``geometry``: the
    ``hgcal.HGCalConverter`` of a pre-embedded HGCal model, what ``generate(geometry=)`` takes (frozen); an HGCal model with the
    converter inside writes ``model.NN_embed`` and takes none.  Dataset 0 / 1: a model with SHOWER_EMBED 'orig-NN' writes
    ``model.NN_embed`` and takes none; a model on the converted grid takes the ``geom1.GeomConverter`` / ``NNConverter`` of
    ``generate(geometry=)``.  Runs without a GPU and without the library."""
    from .layerdiffusion import LayerDiffusion
    from .postprocess import DATASET1_PARAMS, DATASET_PARAMS
    geom, radial = _refuse_out_of_scope(model, debug, geometry)
    cfg = model.config
    sample_steps, sample_offset = int(sample_steps), int(sample_offset or 0)
    two_stage = isinstance(model, LayerDiffusion)
    if two_stage:
        model._layer_dim()  # the ValueError that names SHAPE_PAD[2] + 1 != SHAPE_FINAL[2] + 1
    unet = model.base_model if two_stage else model.model
    opts = dict(unet._engine_opts)
    coords = opts.pop("coords")
    data_shape = [int(v) for v in model._data_shape]
    D, H, W = (int(v) for v in cfg["SHAPE_FINAL"][2:])
    if geom is not None and geom[0] == 1:
        cells = int(geom[1].decoder.mat.shape[1])
        if data_shape != [1, D, cells]:
            raise NotImplementedError(f"export_generator: the sampler state {data_shape} is not the (1, L, N) cell-space shower")
    elif radial is not None and radial.form == 1:
        if data_shape != [int(radial.gc.layer_boundaries[-1])]:
            raise NotImplementedError(f"export_generator: the sampler state {data_shape} is not the (V,) flat shower of the converter")
    elif data_shape != [1, D, H, W]:
        raise NotImplementedError(f"export_generator: the sampler state {data_shape} is not the (1, D, H, W) grid")
    layer_map = "layer" in cfg["SHOWERMAP"]

    sections = []
    if two_stage:
        # the Python path compiles the layer sampler first (LayerDiffusion.sample)
        lay = compile_sampler(model, model.layer_sampler, int(model.layer_steps), sample_offset, (D + 1,))
        sections += [(TAG_LAYER, _net_section(engine.layer_mlp_desc(model.layer_model, **model.layer_model._engine_opts),
                                              model.layer_model.state_dict())),
                     (TAG_LAYER_SAMPLER, _sampler_section(lay))]
    net = compile_sampler(model, model.sampler_algorithm, sample_steps, sample_offset, data_shape)
    r, z, phi = coords
    sections += [(TAG_UNET, _net_section(engine.unet_desc(unet, **opts), unet.state_dict(), (r, z, phi))),
                 (TAG_UNET_SAMPLER, _sampler_section(net))]

    if radial is not None:  # ReverseNormCaloChall's choice: the '+ 10' constants in the original flat shape (utils.py:474-477)
        c = DATASET1_PARAMS[cfg["DATASET_NUM"] + (10 if radial.form == 1 else 0)]
    else:
        c = DATASET_PARAMS[cfg["DATASET_NUM"]]
    if geom is None:
        rev = struct.pack("<6i8f2d", D, H, W, int(layer_map), int(bool(cfg["logE"])), int(cfg["DATASET_NUM"]),
                          c["logit_mean"], c["logit_std"], c["totalE_mean"], c["totalE_std"], c["layers_mean"], c["layers_std"],
                          float(cfg["MAXDEP"]), float(cfg["ECUT"]), float(cfg["EMAX"]), float(cfg["EMIN"]))
    if radial is not None:  # cd_reverse_norm_ds1 takes the constants as float64
        rev = _pad(rev, 80) + struct.pack("<6d", *(float(c[k]) for k in ("logit_mean", "logit_std", "totalE_mean", "totalE_std", "layers_mean", "layers_std")))
    energy_cols = 1
    if geom is not None:
        # ReverseNormHGCal: np.array(emin) + (np.array(emax) - np.array(emin)) * e over the (B, cols) conditioning values
        energy_cols = int(unet.cond_size) - (D + 1 if layer_map else 0)
        if not 1 <= energy_cols <= 8:
            raise NotImplementedError(f"export_generator: {energy_cols} incident-energy columns (1 to 8 are provided)")
        emax = np.broadcast_to(np.atleast_1d(np.asarray(cfg["EMAX"], dtype=np.float64)), (energy_cols,))
        emin = np.broadcast_to(np.atleast_1d(np.asarray(cfg["EMIN"], dtype=np.float64)), (energy_cols,))
        rev = struct.pack("<6i8f2d", D, H, W, int(layer_map), int(bool(cfg["logE"])), int(cfg["DATASET_NUM"]),
                          c["logit_mean"], c["logit_std"], c["totalE_mean"], c["totalE_std"], c["layers_mean"], c["layers_std"],
                          float(cfg["MAXDEP"]), float(cfg["ECUT"]), float(emax[0]), float(emin[0]))
        rev = _pad(rev, 80) + struct.pack("<2i2f", energy_cols, 0, STAGED_ALPHA, STAGED_LAYER_EPS)
        rev += emax.astype("<f8").tobytes() + emin.astype("<f8").tobytes()
    name = str(cfg.get("CHECKPOINT_NAME", "")).encode()[:63]
    shape4 = data_shape + [0] * (4 - len(data_shape))
    meta = struct.pack("<12iQ2i", len(data_shape), *shape4, unet.cond_size, energy_cols, int(two_stage), int(layer_map), sample_steps,
                       int(model.layer_steps) if two_stage else 0, sample_offset, int(model.noise_seed), D + 1 if layer_map else 0, 0)
    meta += name.ljust(64, b"\0")
    sections = [(TAG_META, meta), (TAG_REVNORM, _pad(rev, 16 if geom is not None else 128 if radial is not None else 80))] + sections
    if geom is not None:
        sections.append((TAG_GEOM, _geom_section(geom[1], geom[0])))
    if radial is not None:
        sections.append((TAG_RADIAL, _radial_section(radial.gc, radial.form, radial.mats)))
    version = FORMAT_VERSION_GEOM if geom is not None else FORMAT_VERSION_RADIAL if radial is not None else FORMAT_VERSION

    # header, section table, 64-byte aligned sections; the checksum covers everything behind the header
    off = HEADER_BYTES + SECTION_ENTRY_BYTES * len(sections)
    off += -off % ALIGN
    table, payload = b"", b""
    for tag, body in sections:
        table += struct.pack("<4sIQQ", tag, 0, off + len(payload), len(body))
        payload += _pad(body, ALIGN)
    rest = _pad(table, ALIGN) + payload
    total = HEADER_BYTES + len(rest)
    blob = _pad(MAGIC + struct.pack("<IIQQ", version, len(sections), total, fnv1a64(rest)), HEADER_BYTES) + rest
    if path is not None:
        with open(path, "wb") as fh:
            fh.write(blob)
    return blob


class Generator(Handle):
    """``cd_generator_*`` for Python users: ``Generator(blob)`` (bytes or a path), ``.info``, ``.run(E, ...)``.  Needs the GPU."""

    INFO_KEYS = ("voxels", "layers", "energy_columns", "has_layer_stage", "takes_layers", "sample_steps", "layer_steps", "format_version")

    def __init__(self, blob):
        if not isinstance(blob, (bytes, bytearray, memoryview)):
            with open(blob, "rb") as fh:
                blob = fh.read()
        blob = bytes(blob)
        self.lib = load_library()
        require_gpu()
        super().__init__(self.lib.cd_generator_destroy)
        _check(self.lib.cd_generator_create(blob, len(blob), C.byref(self.handle), _stream()))
        info = (C.c_int32 * 8)()
        _check(self.lib.cd_generator_info(self.handle, info))
        self.info = dict(zip(self.INFO_KEYS, (int(v) for v in info)))
        geo = (C.c_int32 * 8)()
        _check(self.lib.cd_generator_geometry(self.handle, geo))
        # 'geometry': None (a regular grid), 'hgcal' or 'radial' (Dataset 0 / 1); 'form': 0 converted at the end of the run, 1 the
        # converter inside the model; 'state_shape': the sampler's per-sample state
        self.geometry = dict(geometry=(None, "hgcal", "radial")[geo[0]], form=int(geo[1]), state_shape=tuple(int(v) for v in geo[3:3 + geo[2]]))
        self._ws = WorkspaceCache()

    def workspace_bytes(self, batch: int) -> int:
        return _nbytes(self.lib.cd_generator_workspace_bytes, self.handle, int(batch))

    def workspace(self, batch: int) -> torch.Tensor:
        """One workspace kept: the last batch size asked for."""
        return self._ws.get("run", (int(batch),), "cuda", lambda: self.workspace_bytes(batch))

    def run(self, E, layers=None, seed: int = 1234, offset: int = 0, shard=None, normalised: bool = True, workspace=None,
            sparse_decoding: bool = False, sparse_per_batch: bool = False, decode_seed: int = 1234, decode_offset: int = 0):
        """(showers (B, voxels), layers_out (B, 1 + D) or None, next_offset): one cd_generator_run_ex call.  ``E`` (B, energy
        columns) device tensor ((B,) for one column) of conditioning values (``normalised``) or physical energies; ``shard`` =
        (first_row, global_batch).  An HGCal file (format version 2, and no other) returns a fourth value, the next decode offset:
        ``sparse_decoding`` / ``sparse_per_batch`` are ``generate()``'s, drawn from the decoder's own stream at (``decode_seed``,
        ``decode_offset``) -- ``Decoder.noise_seed`` / ``noise_offset`` -- and chained over batches like ``offset``."""
        cols = self.info["energy_columns"]
        E = _dev32(E, "E")
        if E.numel() % cols or (E.dim() > 1 and E.shape[-1] != cols):
            raise ValueError(f"E must have shape (batch, {cols}), not {tuple(E.shape)}")
        E = E.reshape(-1, cols)
        B = E.shape[0]
        if layers is not None:
            layers = _dev32(layers, "layers")
            if tuple(layers.shape) != (B, self.info["layers"] + 1):
                raise ValueError(f"layers must have shape ({B}, {self.info['layers'] + 1}), not {tuple(layers.shape)}")
        first, gb = (0, B) if shard is None else (int(shard[0]), int(shard[1]))
        ws = self.workspace(B) if workspace is None else workspace
        showers = torch.empty((B, self.info["voxels"]), dtype=torch.float32, device=E.device)
        lout = torch.empty((B, self.info["layers"] + 1), dtype=torch.float32, device=E.device) if self.info["takes_layers"] else None
        nxt, dnxt = C.c_uint64(0), C.c_uint64(0)
        args = CdGeneratorRun(
            struct_size=C.sizeof(CdGeneratorRun), batch=B, energy=E.data_ptr(), energy_is_normalised=int(bool(normalised)),
            sparse_mode=(2 if sparse_per_batch else 1) if sparse_decoding else 0, layers=_ptr(layers), seed=int(seed),
            offset=int(offset), first_row=first, global_batch=gb, showers=showers.data_ptr(), layers_out=_ptr(lout),
            next_offset=C.pointer(nxt), decode_seed=int(decode_seed), decode_offset=int(decode_offset),
            next_decode_offset=C.pointer(dnxt), workspace=ws.data_ptr(), workspace_bytes=ws.numel(), stream=_stream())
        _check(self.lib.cd_generator_run_ex(self.handle, C.byref(args)))
        if self.info["format_version"] == FORMAT_VERSION_GEOM:
            return showers, lout, int(nxt.value), int(dnxt.value)
        return showers, lout, int(nxt.value)
