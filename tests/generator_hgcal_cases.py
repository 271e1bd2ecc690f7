"""What the host and GPU tests of HGCal generator files (format version 2) share: the models -- the tiny pre-embedded config and
the in-model config of hgcal_model_cases over geometry "m" (tests/golden/hgcal_model.npz), with per-column EMAX / EMIN that differ
-- a reader of the format written from DESIGN.md section 8d alone, and the corruptions a reader must reject."""
import struct

import numpy as np
import torch

from conftest import gold
import hgcal_model_cases as K

EMAX, EMIN = [100, 2.01, 1.572], [50, 1.99, 1.57]
RN = dict(EMAX=EMAX, EMIN=EMIN, logE=True, MAXDEP=2, ECUT=0.0)
BINS = [-1, 1] + list(K.GRID)
NORM = (0.0835, 3.1083)  # (embed_mean, embed_std) of HGCal set 101: a norm that is not the identity
SEED = 1234


def converter(trainable=False, norm=False):
    """geometry "m": frozen, init()'s own maps; trainable, the fixture's perturbed maps over init()'s masks, with
    zeros among the masked entries"""
    from calodiffusion_amd import hgcal
    g = gold("hgcal_model")
    if trainable:
        mats = []
        for mat, mask in ((g["nn.embeder.mat"], g["init.enc_mask"]), (g["nn.decoder.mat"], g["init.dec_mask"])):
            mat = mat.copy()
            mat.reshape(-1)[np.flatnonzero(mask)[::5]] = 0.0  # every fifth masked entry: a pattern that keeps zeros
            mats.append(mat)
        conv = hgcal.HGCalConverter.from_matrices(BINS, mats[0], mats[1], g["init.enc_mask"], g["init.dec_mask"], trainable=True)
    else:
        conv = hgcal.HGCalConverter.from_matrices(BINS, g["init.enc_mat"], g["init.dec_mat"])
    if norm:
        conv.norm, (conv.embed_mean, conv.embed_std) = True, NORM
    return conv


def pre_embedded(two_stage, **over):
    """the tiny config (SHOWER_EMBED 'NN-pre-embed', three energy columns, 'layer-logit-norm')"""
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    from calodiffusion_amd.configs import load_config
    from calodiffusion_amd.layerdiffusion import LayerDiffusion
    cfg = dict(load_config("tiny"), **RN)
    cfg.update(over)
    torch.manual_seed(SEED)
    return (LayerDiffusion if two_stage else CaloDiffusion)(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"])


def in_model(trainable, **over):
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    cfg = K.config(TRAINABLE_EMBED=trainable, NN_EMBED=converter(trainable), **RN)
    cfg.update(over)
    torch.manual_seed(SEED)
    m = CaloDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"])
    m.eval()
    return m


# ---------------------------------------------------------------------- a reader of format version 2, from DESIGN.md alone
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


def geom(blob, sec):
    """(header dict, [map dict]) of a GEOM section; every map with the file offsets of its three arrays"""
    off, size = sec
    form, L, A, R, N, n_maps, mean, std = struct.unpack_from("<6i2f", blob, off)
    head = dict(form=form, bins=(L, A, R), cells=N, n_maps=n_maps, embed_mean=mean, embed_std=std)
    pos, maps = off + 64, []
    for _ in range(n_maps):
        rows, cols, nnz, is_mask = struct.unpack_from("<4i", blob, pos)
        m = dict(rows=rows, cols=cols, nnz=nnz, is_mask=is_mask, at=pos)
        pos += 64
        for name, count, dt in (("row_ptr", L * rows + 1, "<i4"), ("col_idx", nnz, "<i4"), ("val", nnz, "<f4")):
            assert pos % 64 == 0
            m[name], m[name + "_at"] = np.frombuffer(blob, dt, count, pos), pos
            pos += pad64(4 * count)
        maps.append(m)
    assert pos <= off + pad64(size)
    return head, maps


def dense(m, layers):
    """(values, pattern), both (layers, rows, cols), of one map record"""
    val = np.zeros((layers * m["rows"], m["cols"]), dtype=np.float32)
    pat = np.zeros(val.shape, dtype=bool)
    lines = np.repeat(np.arange(layers * m["rows"]), np.diff(m["row_ptr"]))
    assert not pat[lines, m["col_idx"]].any() or len(set(zip(lines.tolist(), m["col_idx"].tolist()))) == m["nnz"]
    val[lines, m["col_idx"]] = m["val"]
    pat[lines, m["col_idx"]] = True
    shape = (layers, m["rows"], m["cols"])
    return val.reshape(shape), pat.reshape(shape)


def reseal(blob):
    """the same bytes under a fresh checksum: what is left for the reader to reject is the structure"""
    from calodiffusion_amd import generator as G
    return blob[:24] + struct.pack("<Q", G.fnv1a64(blob[64:])) + blob[32:]


def _put(blob, at, fmt, *values):
    raw = struct.pack(fmt, *values)
    return blob[:at] + raw + blob[at + len(raw):]


def corruptions(blob):
    """(label, bytes) of every bad version-2 file the reader must reject"""
    secs, version, _ = walk(blob)
    assert version == 2
    head, maps = geom(blob, secs[b"GEOM"])
    cuts = set()
    for off, size in secs.values():
        cuts |= {off - 1, off, off + 1, off + size - 1, off + size, off + size + 1}
    for m in maps:  # and inside GEOM: around every array of every map
        for name in ("at", "row_ptr_at", "col_idx_at", "val_at"):
            cuts |= {m[name] - 1, m[name], m[name] + 1}
        cuts.add(m["val_at"] + 4 * m["nnz"] - 1)
    for cut in sorted(cuts):
        if 0 < cut < len(blob):
            yield f"truncated at {cut}", blob[:cut]
    # truncated, but with a header that agrees with the new length and a fresh checksum: the counts must catch it
    g_off, g_size = secs[b"GEOM"]
    index = {tag: i for i, tag in enumerate(secs)}
    entry = 64 + 24 * index[b"GEOM"]
    assert g_off + pad64(g_size) >= len(blob) - 63  # GEOM is the last section
    for m in maps:
        for name in ("row_ptr_at", "col_idx_at", "val_at"):
            cut = m[name] + 4
            short = _put(_put(blob[:cut], 16, "<Q", cut), entry + 16, "<Q", cut - g_off)
            yield f"GEOM ends inside {name} (resealed)", reseal(short)
    d = maps[-1]
    L = head["bins"][0]
    counts = np.diff(d["row_ptr"])
    full = int(np.flatnonzero(counts[1:] >= 2)[0]) + 1  # a line with two entries or more, not the first
    p = int(d["row_ptr"][full])
    yield "row_ptr[0] not 0", reseal(_put(blob, d["row_ptr_at"], "<i", 1))
    yield "row_ptr not monotone", reseal(_put(blob, d["row_ptr_at"] + 4 * full, "<i", int(d["row_ptr"][full + 1]) + 1))
    yield "row_ptr negative", reseal(_put(blob, d["row_ptr_at"] + 4 * (full + 1), "<i", -1))
    yield "row_ptr ends past nnz", reseal(_put(blob, d["row_ptr_at"] + 4 * (L * d["rows"]), "<i", d["nnz"] + 1))
    yield "column == cols", reseal(_put(blob, d["col_idx_at"] + 4 * p, "<i", d["cols"]))
    yield "column negative", reseal(_put(blob, d["col_idx_at"] + 4 * p, "<i", -1))
    yield "row not sorted", reseal(_put(blob, d["col_idx_at"] + 4 * p, "<2i", int(d["col_idx"][p + 1]), int(d["col_idx"][p])))
    yield "column twice in a row", reseal(_put(blob, d["col_idx_at"] + 4 * p, "<i", int(d["col_idx"][p + 1])))
    yield "nnz one less", reseal(_put(blob, d["at"] + 8, "<i", d["nnz"] - 1))
    yield "nnz one more", reseal(_put(blob, d["at"] + 8, "<i", d["nnz"] + 1))
    yield "nnz negative", reseal(_put(blob, d["at"] + 8, "<i", -1))
    yield "nnz 2^31 - 1", reseal(_put(blob, d["at"] + 8, "<i", 2 ** 31 - 1))
    yield "value NaN", reseal(_put(blob, d["val_at"] + 4 * p, "<f", float("nan")))
    yield "value inf", reseal(_put(blob, d["val_at"], "<f", float("inf")))
    yield "map rows disagree with the cell count", reseal(_put(blob, d["at"], "<i", d["rows"] + 1))
    yield "map rows 2^31 - 1", reseal(_put(blob, d["at"], "<2i", 2 ** 31 - 1, 2 ** 31 - 1))
    yield "cells disagree with the maps", reseal(_put(blob, g_off + 16, "<i", head["cells"] + 1))
    yield "bins disagree with the grid", reseal(_put(blob, g_off + 4, "<i", L + 1))
    yield "unknown form", reseal(_put(blob, g_off, "<i", 2))
    yield "form disagrees with the map count", reseal(_put(blob, g_off, "<i", 1 - head["form"]))
    yield "embed_std 0", reseal(_put(blob, g_off + 28, "<f", 0.0))
    r_off = secs[b"RNRM"][0]
    yield "energy columns 9", reseal(_put(blob, r_off + 80, "<i", 9))
    yield "energy columns disagree with META", reseal(_put(blob, r_off + 80, "<i", 2))
    yield "EMAX below EMIN in column 2", reseal(_put(blob, r_off + 96 + 8 * 2, "<d", 1.0))
    # version 2 without GEOM (it is the last entry of the table: one section fewer), version 1 with GEOM
    yield "version 2 without GEOM", _put(blob, 12, "<I", len(secs) - 1)
    yield "version 1 with GEOM", _put(blob, 8, "<I", 1)
    yield "future version", _put(blob, 8, "<I", 3)
