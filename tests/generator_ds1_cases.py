"""What the host and GPU tests of Dataset-0/1 generator files (format version 3) and of two-stage in-model HGCal files share: the
models, a reader of the format written from DESIGN.md section 8d alone, and the corruptions a reader must reject."""
import math
import struct

import numpy as np
import torch

import ds1_model_cases as K1
import layer_inmodel_cases as L
import narrow_cases as KN

STEPS = 3
GRID_OVER = dict(SHOWER_EMBED="", SHAPE_PAD=[-1, 1] + list(K1.GRID), SHOWERMAP="logit-norm")
# cd_radial_create's limits (include/calodiff.h)
MAX_LAYERS, MAX_WEIGHT_FLOATS, MAX_ROW_FLOATS = 64, 8192, 6144


def photon_given(**over):
    """form 1, single stage: CaloDiffusion over the photon config (SHAPE_PAD = SHAPE_FINAL); layers from the caller"""
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    return L.model("ph", cls=CaloDiffusion, **over)


def two_stage(rec, **over):
    """form 1, two stages: LayerDiffusion of a record of layer_inmodel_cases ('ph', 'pi': version 3; 'hg': version 2)"""
    return L.model(rec, **over)


def on_the_grid(**over):
    """form 0: a photon model on the converted grid, 'logit-norm', and the GeomConverter generate(geometry=) takes"""
    from calodiffusion_amd import geom1, xml_handler
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    from helpers import SEED
    cfg = K1.config(**dict(GRID_OVER, **over))
    torch.manual_seed(SEED)
    m = CaloDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"])
    m.eval()
    return m, geom1.GeomConverter(xml_handler.XMLHandler("photon", K1.XML))


def energies(n, seed, emax=4194.304, emin=0.256):
    """n conditioning values e in [0, 1) on which this host's numpy float32 power -- what the Python path scales by -- is the
    correctly rounded one, which cd_generator_run forms on the device (test_gpu_generator.py has the reasons)"""
    rng = np.random.default_rng(seed)
    keep = []
    while len(keep) < n:
        e = rng.random(4 * n, dtype=np.float32)
        host = (emax / emin) ** e
        exact = np.array([math.pow(float(np.float32(emax / emin)), float(v)) for v in e]).astype(np.float32)
        keep += [v for v, ok in zip(e, host == exact) if ok]
    return torch.tensor(np.array(keep[:n], dtype=np.float32)).reshape(n, 1)


# ---------------------------------------------------------------------- a reader of format version 3, from DESIGN.md alone
def pad64(n):
    return n + (-n % 64)


def walk(blob):
    """({tag: (offset, size)}, version, checksum)"""
    assert blob[:8] == b"CDGENBLB"
    version, n_sec, total, checksum = struct.unpack_from("<IIQQ", blob, 8)
    assert total == len(blob) and blob[32:64] == b"\0" * 32
    sections = {}
    for i in range(n_sec):
        tag, _, off, size = struct.unpack_from("<4sIQQ", blob, 64 + 24 * i)
        assert off % 64 == 0 and off >= 64 + 24 * n_sec and off + size <= total
        sections[tag] = (off, size)
    return sections, version, checksum


def radial(blob, sec):
    """the RADL section: header fields, the three layout arrays and the matrices, each with its file offset"""
    off, size = sec
    form, layers, alpha_out, r_out, voxels, n_mats, wtotal = struct.unpack_from("<7i", blob, off)
    out = dict(form=form, grid=(layers, alpha_out, r_out), voxels=voxels, n_mats=n_mats, wtotal=wtotal, at=off)
    pos = off + 64
    for name, count in (("bound", layers + 1), ("alpha", layers), ("rin", layers)):
        out[name], out[name + "_at"] = np.frombuffer(blob, "<i4", count, pos), pos
        pos += pad64(4 * count)
    out["mats"], out["mats_at"] = [], []
    for _ in range(n_mats):
        out["mats"].append(np.frombuffer(blob, "<f4", wtotal, pos))
        out["mats_at"].append(pos)
        pos += pad64(4 * wtotal)
    assert pos <= off + pad64(size)
    return out


def revnorm(blob, sec):
    off, size = sec
    assert size == 128
    D, H, W, layer_map, logE, dnum = struct.unpack_from("<6i", blob, off)
    c32 = struct.unpack_from("<6f", blob, off + 24)
    maxdep, ecut = struct.unpack_from("<2f", blob, off + 48)
    emax, emin = struct.unpack_from("<2d", blob, off + 56)
    c64 = struct.unpack_from("<6d", blob, off + 80)
    return dict(grid=(D, H, W), layer_map=layer_map, logE=logE, dataset_num=dnum, consts32=c32, consts64=c64, maxdep=maxdep, ecut=ecut,
                emax=emax, emin=emin)


def meta(blob, sec):
    off, _ = sec
    v = struct.unpack_from("<12iQ2i", blob, off)
    return dict(state=tuple(v[1:1 + v[0]]), ndim=v[0], shape4=v[1:5], cond_size=v[5], energy_cols=v[6], two_stage=v[7], takes_layers=v[8],
                sample_steps=v[9], layer_steps=v[10], sample_offset=v[11], seed=v[12], layer_dim=v[13])


def reseal(blob):
    """the same bytes under a fresh checksum: what is left for the reader to reject is the structure"""
    from calodiffusion_amd import generator as G
    return blob[:24] + struct.pack("<Q", G.fnv1a64(blob[64:])) + blob[32:]


def _put(blob, at, fmt, *values):
    raw = struct.pack(fmt, *values)
    return blob[:at] + raw + blob[at + len(raw):]


def corruptions(blob):
    """(label, bytes) of every bad version-3 file the reader must reject"""
    secs, version, _ = walk(blob)
    assert version == 3
    r = radial(blob, secs[b"RADL"])
    layers, A, R = r["grid"]
    cuts = set()
    for off, size in secs.values():
        cuts |= {off - 1, off, off + 1, off + size - 1, off + size, off + size + 1}
    for at in [r["at"], r["bound_at"], r["alpha_at"], r["rin_at"]] + r["mats_at"]:  # and inside RADL: around every array
        cuts |= {at - 1, at, at + 1}
    cuts.add(r["mats_at"][-1] + 4 * r["wtotal"] - 1)
    for cut in sorted(cuts):
        if 0 < cut < len(blob):
            yield f"truncated at {cut}", blob[:cut]
    # truncated, but with a header that agrees with the new length and a fresh checksum: the counts must catch it
    g_off, g_size = secs[b"RADL"]
    index = {tag: i for i, tag in enumerate(secs)}
    entry = 64 + 24 * index[b"RADL"]
    assert g_off + pad64(g_size) >= len(blob) - 63  # RADL is the last section
    for name, at in [("bound", r["bound_at"]), ("alpha", r["alpha_at"]), ("rin", r["rin_at"])] + [(f"matrix {k}", a) for k, a in enumerate(r["mats_at"])]:
        cut = at + 4
        short = _put(_put(blob[:cut], 16, "<Q", cut), entry + 16, "<Q", cut - g_off)
        yield f"RADL ends inside {name} (resealed)", reseal(short)
    # the section table: offsets and lengths flipped
    for tag, i in index.items():
        off, size = secs[tag]
        e = 64 + 24 * i
        name = tag.decode()
        yield f"{name}: offset past the file", reseal(_put(blob, e + 8, "<Q", len(blob)))
        yield f"{name}: offset 2^63", reseal(_put(blob, e + 8, "<Q", 1 << 63))
        yield f"{name}: offset not aligned", reseal(_put(blob, e + 8, "<Q", off + 4))
        yield f"{name}: offset inside the table", reseal(_put(blob, e + 8, "<Q", 64))
        yield f"{name}: length past the file", reseal(_put(blob, e + 16, "<Q", len(blob) - off + 1))
        yield f"{name}: length 2^64 - 1", reseal(_put(blob, e + 16, "<Q", (1 << 64) - 1))
        yield f"{name}: length 0", reseal(_put(blob, e + 16, "<Q", 0))
    yield "RADL appears twice", reseal(_put(blob, 64 + 24 * index[b"USMP"], "<4s", b"RADL"))
    # the layout: every rule of cd_radial_create
    b, a, n = r["bound"], r["alpha"], r["rin"]
    yield "bound[0] not 0", reseal(_put(blob, r["bound_at"], "<i", 1))
    yield "bound not monotone", reseal(_put(blob, r["bound_at"] + 4 * 2, "<i", int(b[1])))
    yield "bound decreasing", reseal(_put(blob, r["bound_at"] + 4 * 2, "<i", int(b[1]) - 1))
    yield "bound negative", reseal(_put(blob, r["bound_at"] + 4 * 1, "<i", -5))
    yield "alpha outside {1, A}", reseal(_put(blob, r["alpha_at"] + 4 * 1, "<i", 2 if A != 2 else 3))
    yield "alpha 0", reseal(_put(blob, r["alpha_at"], "<i", 0))
    yield "alpha swapped (span mismatch)", reseal(_put(blob, r["alpha_at"], "<i", A if int(a[0]) == 1 else 1))
    yield "span mismatch: rin one more", reseal(_put(blob, r["rin_at"] + 4 * 1, "<i", int(n[1]) + 1))
    yield "rin 0", reseal(_put(blob, r["rin_at"], "<i", 0))
    yield "rin negative", reseal(_put(blob, r["rin_at"], "<i", -int(n[0])))
    yield "voxel count not bound[L]", reseal(_put(blob, g_off + 16, "<i", r["voxels"] + 1))
    yield "wtotal one less", reseal(_put(blob, g_off + 24, "<i", r["wtotal"] - 1))
    yield "wtotal one more", reseal(_put(blob, g_off + 24, "<i", r["wtotal"] + 1))
    yield "matrix entry NaN", reseal(_put(blob, r["mats_at"][0] + 4 * 7, "<f", float("nan")))
    yield "last matrix entry inf", reseal(_put(blob, r["mats_at"][-1] + 4 * (r["wtotal"] - 1), "<f", float("inf")))
    # each limit exceeded by one
    yield "layers 65", reseal(_put(blob, g_off + 4, "<i", MAX_LAYERS + 1))
    yield "layers 0", reseal(_put(blob, g_off + 4, "<i", 0))
    yield "layers 2^31 - 1", reseal(_put(blob, g_off + 4, "<i", 2 ** 31 - 1))
    yield "wtotal 8193", reseal(_put(blob, g_off + 24, "<i", MAX_WEIGHT_FLOATS + 1))
    yield "wtotal 2^31 - 1", reseal(_put(blob, g_off + 24, "<i", 2 ** 31 - 1))
    yield "voxels 6145", reseal(_put(blob, g_off + 16, "<i", MAX_ROW_FLOATS + 1))
    yield "grid row 6145", reseal(_put(blob, g_off + 8, "<2i", 1, MAX_ROW_FLOATS // layers + 1))
    yield "alpha_out 2^31 - 1", reseal(_put(blob, g_off + 8, "<i", 2 ** 31 - 1))
    yield "r_out 0", reseal(_put(blob, g_off + 12, "<i", 0))
    yield "grid disagrees with RNRM", reseal(_put(blob, g_off + 12, "<i", R - 1))
    yield "unknown form", reseal(_put(blob, g_off, "<i", 2))
    yield "form negative", reseal(_put(blob, g_off, "<i", -1))
    yield "form disagrees with the matrix count", reseal(_put(blob, g_off, "<i", 1 - r["form"]))
    yield "matrix count 3", reseal(_put(blob, g_off + 20, "<i", 3))
    # RNRM and META against it
    r_off, m_off = secs[b"RNRM"][0], secs[b"META"][0]
    yield "constant NaN", reseal(_put(blob, r_off + 80, "<d", float("nan")))
    yield "logit_std 0", reseal(_put(blob, r_off + 88, "<d", 0.0))
    yield "ECUT negative", reseal(_put(blob, r_off + 52, "<f", -1.0))
    yield "MAXDEP 0", reseal(_put(blob, r_off + 48, "<f", 0.0))
    yield "EMIN 0 with logE", reseal(_put(blob, r_off + 64, "<d", 0.0))
    yield "RNRM cut to the version-1 record", reseal(_put(blob, 64 + 24 * index[b"RNRM"] + 16, "<Q", 80))
    yield "state dimensions of the other form", reseal(_put(blob, m_off, "<i", 4 if r["form"] == 1 else 1))
    yield "state size one more", reseal(_put(blob, m_off + 4, "<i", struct.unpack_from("<i", blob, m_off + 4)[0] + 1))
    yield "two energy columns", reseal(_put(blob, m_off + 24, "<i", 2))
    if r["form"] == 0:
        yield "layer map on the converted grid", reseal(_put(_put(blob, r_off + 12, "<i", 1), m_off + 32, "<i", 1))
    # versions against sections
    yield "version 3 without RADL", _put(blob, 12, "<I", len(secs) - 1)
    yield "version 1 with RADL", _put(blob, 8, "<I", 1)
    yield "version 2 with RADL", _put(blob, 8, "<I", 2)
    yield "RADL renamed GEOM", reseal(_put(blob, entry, "<4s", b"GEOM"))
    yield "future version", _put(blob, 8, "<I", 4)
