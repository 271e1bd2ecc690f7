"""CPU: the generator file (calodiffusion_amd/generator.py, format: DESIGN.md "Generator file").  The exporter runs without a GPU;
a pure-Python walk of its sections finds every weight, the compiled samplers equal what the Python path hands the library, the
checksum verifies; the stand-alone reader (tools/generator_blob_check.cpp over csrc/generator_blob.h, the code cd_generator_create
runs) accepts the file and rejects every corruption with exit 1 and a message, never a signal; the export refusals, by name."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from calodiffusion_amd import generator as G
from calodiffusion_amd import sample, schedule
from calodiffusion_amd.engine import CdLayerMlpDesc, CdSamplerOp, CdUnetDesc, _pack_ops

STEPS = 3


def _cfg(name, **over):
    from calodiffusion_amd.configs import load_config
    cfg = dict(load_config(name))
    cfg.update(over)
    return cfg


def _build(cls, cfg):
    torch.manual_seed(1234)
    return cls(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"])


@pytest.fixture(scope="module")
def ds2():
    from calodiffusion_amd.layerdiffusion import LayerDiffusion
    m = _build(LayerDiffusion, _cfg("dataset2", LAYER_STEPS=12))
    return m, G.export_generator(m, STEPS)


@pytest.fixture(scope="module")
def ds3():
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    m = _build(CaloDiffusion, _cfg("dataset3"))
    return m, G.export_generator(m, 2)


# ---------------------------------------------------------------------- a reader of the format in Python, from DESIGN.md alone
def walk(blob):
    assert blob[:8] == G.MAGIC
    version, n_sec, total, checksum = struct.unpack_from("<IIQQ", blob, 8)
    assert version == G.FORMAT_VERSION and total == len(blob)
    assert blob[32:64] == b"\0" * 32
    sections = {}
    for i in range(n_sec):
        tag, _, off, size = struct.unpack_from("<4sIQQ", blob, 64 + 24 * i)
        assert off % 64 == 0 and off >= 64 + 24 * n_sec and off + size <= total
        sections[tag] = (off, size)
    return sections, checksum


def net(blob, sec):
    off, size = sec
    desc_bytes, n_w, n_r, n_z, n_phi = struct.unpack_from("<5I", blob, off)
    pos = off + 32
    desc = blob[pos:pos + desc_bytes]
    pos += desc_bytes + (-desc_bytes % 8)
    coords = []
    for n in (n_r, n_z, n_phi):
        coords.append(np.frombuffer(blob, "<f4", n, pos))
        pos += 4 * n
    weights = {}
    for i in range(n_w):
        rec = blob[pos + 112 * i: pos + 112 * (i + 1)]
        name = rec[:96].split(b"\0", 1)[0].decode()
        numel, data_off = struct.unpack("<QQ", rec[96:])
        assert data_off % 64 == 0 and data_off + 4 * numel <= size
        weights[name] = np.frombuffer(blob, "<f4", numel, off + data_off)
    return desc, coords, weights


def sampler(blob, sec):
    off, _ = sec
    kind, n_steps, n_ops, n_coef, n_bufs, has_begin, drawn, use_graph, scale = struct.unpack_from("<8if", blob, off)
    out = dict(kind=kind, n_steps=n_steps, n_bufs=n_bufs, drawn=drawn, use_graph=use_graph, start_scale=scale)
    pos = off + 64
    if kind == 0:
        out["table"] = np.frombuffer(blob, "<f4", 4 * n_steps, pos).reshape(n_steps, 4)
        return out
    out["ops"] = np.frombuffer(blob, "<i4", 10 * n_ops, pos).reshape(n_ops, 10)
    pos += 40 * n_ops
    out["op_begin"] = None
    if has_begin:
        out["op_begin"] = np.frombuffer(blob, "<i4", n_steps + 1, pos)
        pos += 4 * (n_steps + 1)
    out["coefs"] = np.frombuffer(blob, "<f4", n_steps * n_coef, pos).reshape(n_steps, n_coef)
    return out


def _same_weights(found, state_dict):
    assert set(found) == set(state_dict)
    for k, v in state_dict.items():
        assert np.array_equal(found[k], v.detach().cpu().numpy().reshape(-1)), k


def test_dataset2_layerdiffusion_file(ds2):
    m, blob = ds2
    secs, checksum = walk(blob)
    assert list(secs) == [b"META", b"RNRM", b"LAYR", b"LSMP", b"UNET", b"USMP"]
    assert G.fnv1a64(blob[64:]) == checksum
    desc, coords, weights = net(blob, secs[b"UNET"])
    _same_weights(weights, m.base_model.state_dict())
    d = CdUnetDesc.from_buffer_copy(desc)
    assert d.struct_size == len(desc) and tuple(d.grid) == (45, 16, 9) and d.cond_size == 47 and list(d.layer_sizes)[:4] == [32, 32, 64, 32]
    for have, want in zip(coords, m.base_model._engine_opts["coords"]):
        assert np.array_equal(have, want)
    ldesc, _, lweights = net(blob, secs[b"LAYR"])
    _same_weights(lweights, m.layer_model.state_dict())
    assert list(lweights) == list(m.layer_model.state_dict())  # state_dict order: cd_layer_sample takes them by position
    ld = CdLayerMlpDesc.from_buffer_copy(ldesc)
    assert (ld.dim_in, ld.cond_size, ld.n_res) == (46, 1, 4)
    us, ls = sampler(blob, secs[b"USMP"]), sampler(blob, secs[b"LSMP"])
    assert us["kind"] == 0 and np.array_equal(us["table"], schedule.ddim_step_table(STEPS, 0.0, 0)) and us["drawn"] == 0
    assert ls["kind"] == 0 and np.array_equal(ls["table"], schedule.ddim_step_table(12, 0.0, 0))
    off = secs[b"META"][0]
    assert struct.unpack_from("<12iQ2i", blob, off) == (4, 1, 45, 16, 9, 47, 1, 1, 1, STEPS, 12, 0, 1234, 46, 0)
    assert blob[off + 64: off + 128].rstrip(b"\0") == b"dataset2"
    rev = struct.unpack_from("<6i8f2d", blob, secs[b"RNRM"][0])
    assert rev[:6] == (45, 16, 9, 1, 1, 2) and rev[14:] == (1000.0, 1.0)
    assert rev[6:14] == tuple(np.float32([-12.8564, 1.9123, 0.3926, 0.05546, -6.35551, 3.90699, 2, 0.0000151]).tolist())


def test_dataset3_calodiffusion_file(ds3):
    m, blob = ds3
    secs, checksum = walk(blob)
    assert list(secs) == [b"META", b"RNRM", b"UNET", b"USMP"]
    assert G.fnv1a64(blob[64:]) == checksum
    _, _, weights = net(blob, secs[b"UNET"])
    _same_weights(weights, m.model.state_dict())
    us = sampler(blob, secs[b"USMP"])
    assert np.array_equal(us["table"], schedule.ddim_step_table(2, 0.0, 0))
    meta = struct.unpack_from("<12iQ2i", blob, secs[b"META"][0])
    assert meta[:9] == (4, 1, 45, 50, 18, 1, 1, 0, 0) and meta[13] == 0


@pytest.mark.parametrize("name,opts,steps,offset", [("DPMPP2M", {}, 5, 0), ("Heun", {}, 4, 1), ("DPMPPSDE", {"ETA": 1.0}, 3, 0),
                                                    ("DPM", {}, 4, 0), ("DDPM", {}, 4, 2)])
def test_compiled_sampler_is_what_the_python_path_builds(name, opts, steps, offset):
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    m = _build(CaloDiffusion, _cfg("dataset3", SAMPLER=name, SAMPLER_OPTIONS=opts, LAYER_SIZE_UNET=[16, 16, 16, 16]))
    blob = G.export_generator(m, steps, sample_offset=offset)
    us = sampler(blob, walk(blob)[0][b"USMP"])
    if name == "DDPM":
        want = schedule.ddim_step_table(steps, 1.0, offset)
        assert us["kind"] == 0 and np.array_equal(us["table"], want) and us["drawn"] == want.shape[0]
        return
    prog = getattr(sample, name)(m.config).build(m, steps, offset).finalize()
    assert us["kind"] == 1 and us["n_bufs"] == prog.n_bufs and us["start_scale"] == np.float32(prog.start_scale)
    assert np.array_equal(us["coefs"], prog.coefs, equal_nan=True) and us["drawn"] == prog.n_randn
    assert np.array_equal(us["ops"], _pack_ops(prog)) and us["ops"].shape[1] * 4 == struct.calcsize("<10i") == 40
    assert (us["op_begin"] is None) == (prog.op_begin is None)
    if prog.op_begin is not None:
        assert list(us["op_begin"]) == list(prog.op_begin)
    assert CdSamplerOp.kind.offset == 0 and CdSamplerOp.col.offset == 36


def test_checksum_loops_agree():
    data = bytes(range(256)) * 3 + b"generator"
    assert G.fnv1a64(data) == G.fnv1a64_py(data)
    assert G.fnv1a64_py(b"") == 0xCBF29CE484222325 and G.fnv1a64_py(b"a") == 0xAF63DC4C8601EC8C


# ---------------------------------------------------------------------- the stand-alone reader
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("blobcheck") / "generator_blob_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "calodiffusion_amd", "csrc"),
                        os.path.join(ROOT, "tools", "generator_blob_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _check(checker, tmp_path, blob, name="g.cdgen"):
    path = tmp_path / name
    path.write_bytes(blob)
    return subprocess.run([checker, str(path)], capture_output=True, text=True)


def _reseal(blob):
    """the same bytes under a fresh checksum: what is left for the reader to reject is the structure"""
    return blob[:24] + struct.pack("<Q", G.fnv1a64(blob[64:])) + blob[32:]


def corruptions(blob):
    """(label, bytes) of every bad file the reader must reject"""
    secs, _ = walk(blob)
    for tag, (off, size) in secs.items():
        for edge in (off, off + size):
            for cut in (edge - 1, edge, edge + 1):
                if 0 < cut < len(blob):
                    yield f"truncated at {tag.decode()} {cut}", blob[:cut]
    index = {tag: i for i, tag in enumerate(secs)}
    entry = 64 + 24 * index[b"UNET"]
    yield "section offset past the end", _reseal(blob[:entry + 8] + struct.pack("<Q", len(blob) + 64) + blob[entry + 16:])
    yield "section size past the end", _reseal(blob[:entry + 16] + struct.pack("<Q", len(blob)) + blob[entry + 24:])
    yield "section offset + size wraps", _reseal(blob[:entry + 8] + struct.pack("<QQ", 2 ** 64 - 64, 128) + blob[entry + 24:])
    u = secs[b"USMP"][0]
    yield "step count overflows its section", _reseal(blob[:u + 4] + struct.pack("<i", 1 << 20) + blob[u + 8:])
    w = secs[b"UNET"][0]
    yield "weight count overflows its section", _reseal(blob[:w + 4] + struct.pack("<I", 65536) + blob[w + 8:])
    desc_bytes, _, n_r, n_z, n_phi = struct.unpack_from("<5I", blob, w)
    rec = w + 32 + desc_bytes + (-desc_bytes % 8) + 4 * (n_r + n_z + n_phi)
    yield "weight numel wraps", _reseal(blob[:rec + 96] + struct.pack("<Q", 2 ** 62 + 1) + blob[rec + 104:])
    yield "weight offset past its section", _reseal(blob[:rec + 104] + struct.pack("<Q", secs[b"UNET"][1]) + blob[rec + 112:])
    flip = len(blob) // 2
    yield "flipped payload byte", blob[:flip] + bytes([blob[flip] ^ 0x10]) + blob[flip + 1:]
    yield "wrong magic", b"CDGENBLX" + blob[8:]
    yield "future version", blob[:8] + struct.pack("<I", G.FORMAT_VERSION + 1) + blob[12:]
    yield "empty", b""
    yield "header only", blob[:64]


def test_reader_accepts_the_files(checker, tmp_path, ds2, ds3):
    for _, blob in (ds2, ds3):
        r = _check(checker, tmp_path, blob)
        assert r.returncode == 0, r.stderr
        assert "UNET" in r.stdout and "format version 1" in r.stdout
    assert "layer model: 40 tensors" in _check(checker, tmp_path, ds2[1]).stdout


def test_reader_rejects_every_corruption(checker, tmp_path, ds2):
    labels = []
    for label, bad in corruptions(ds2[1]):
        r = _check(checker, tmp_path, bad)
        assert r.returncode == 1, (label, r.returncode, r.stderr)  # a signal would be a negative status
        assert r.stderr.strip(), label
        labels.append(label)
    assert len(labels) >= 30 + 12 and sum(lab.startswith("truncated") for lab in labels) >= 30
    assert "checksum" in _check(checker, tmp_path, next(b for lab, b in corruptions(ds2[1]) if lab == "flipped payload byte")).stderr
    assert "overflow" in _check(checker, tmp_path, next(b for lab, b in corruptions(ds2[1]) if lab.startswith("step count"))).stderr


# ---------------------------------------------------------------------- refusals
def test_export_refusals_by_name(ds2):
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    import ds1_model_cases
    with pytest.raises(NotImplementedError, match="HGCal"):
        G.export_generator(_build(CaloDiffusion, _cfg("tiny")), 3)
    with pytest.raises(NotImplementedError, match="Dataset 1"):
        G.export_generator(_build(CaloDiffusion, ds1_model_cases.config()), 3)
    small = dict(LAYER_SIZE_UNET=[16, 16, 16, 16])
    m = _build(CaloDiffusion, _cfg("dataset3", **small))
    m.do_embed = True
    with pytest.raises(NotImplementedError, match="do_embed"):
        G.export_generator(m, 3)
    with pytest.raises(NotImplementedError, match="DPMAdaptive"):
        G.export_generator(_build(CaloDiffusion, _cfg("dataset3", SAMPLER="DPMAdaptive", **small)), 3)
    with pytest.raises(NotImplementedError, match="BespokeNonStationary"):
        G.export_generator(_build(CaloDiffusion, _cfg("dataset3", SAMPLER="BespokeNonStationary", **small)), 3)
    with pytest.raises(NotImplementedError, match="debug"):
        G.export_generator(ds2[0], STEPS, debug=True)
    with pytest.raises(NotImplementedError, match="SHOWERMAP"):
        G.export_generator(_build(CaloDiffusion, _cfg("dataset3", SHOWERMAP="log-norm", **small)), 3)
