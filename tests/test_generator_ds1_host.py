"""CPU: Dataset-0/1 generator files (format version 3; calodiffusion_amd/generator.py) and the two-stage
in-model HGCal file (version 2, form 1, with LAYR / LSMP).  The exporter runs without a GPU; the reader is the host code
cd_generator_create parses with (csrc/generator_blob.h), built into tools/generator_blob_check.cpp."""
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
import ds1_model_cases as K1
import generator_ds1_cases as H
import layer_inmodel_cases as L
import narrow_cases as KN

from calodiffusion_amd import generator as G

STEPS = H.STEPS
# sha256 of export_generator(LayerDiffusion(dataset2, LAYER_STEPS=12) built under torch.manual_seed(1234), 3), 11662720 bytes: the
# pin of tests/test_generator_hgcal_host.py (the exporter before format version 2), asserted again next to format version 3
DATASET2_TWO_STAGE_SHA256 = "e5c1bf4e87c3b083ddc129d5baa1cbca08edf94b55d6f3ffa23f40fd4ee5afe0"


@pytest.fixture(scope="module")
def photon():
    m = H.photon_given()
    return m, G.export_generator(m, STEPS)


@pytest.fixture(scope="module")
def photon2():
    m = H.two_stage("ph")
    return m, G.export_generator(m, STEPS)


@pytest.fixture(scope="module")
def pion2():
    m = H.two_stage("pi")
    return m, G.export_generator(m, STEPS)


@pytest.fixture(scope="module")
def grid():
    m, gc = H.on_the_grid()
    return m, gc, G.export_generator(m, STEPS, geometry=gc)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("blobcheck") / "generator_blob_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "calodiffusion_amd", "csrc"),
                        os.path.join(ROOT, "tools", "generator_blob_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _check(checker, tmp_path, blob):
    path = tmp_path / "g.cdgen"
    path.write_bytes(blob)
    return subprocess.run([checker, str(path)], capture_output=True, text=True)


def _matrices(conv):
    return [torch.cat([lay.weight.detach().reshape(-1) for lay in part]).numpy() for part in (conv.encs, conv.decs)]


def _layout_is(r, gc):
    bound, alpha, rin = gc.descriptor()
    assert r["grid"] == (gc.num_layers, int(gc.alpha_out), gc.dim_r_out) and r["voxels"] == bound[-1]
    assert r["bound"].tolist() == bound and r["alpha"].tolist() == alpha and r["rin"].tolist() == rin
    assert r["wtotal"] == gc.dim_r_out * sum(rin)


@pytest.mark.parametrize("which", ["photon", "photon2", "pion2"])
def test_form_1_file_holds_the_layout_the_matrices_and_the_constants(which, request):
    from calodiffusion_amd.postprocess import DATASET1_PARAMS
    m, blob = request.getfixturevalue(which)
    two_stage, cases = which.endswith("2"), (KN if which == "pion2" else K1)
    secs, version, checksum = H.walk(blob)
    assert version == G.FORMAT_VERSION_RADIAL == 3
    assert list(secs) == [b"META", b"RNRM"] + ([b"LAYR", b"LSMP"] if two_stage else []) + [b"UNET", b"USMP", b"RADL"]
    assert checksum == G.fnv1a64_py(blob[64:])
    r = H.radial(blob, secs[b"RADL"])
    assert r["form"] == 1 and r["n_mats"] == 2
    _layout_is(r, m.NN_embed.gc)
    for got, want in zip(r["mats"], _matrices(m.NN_embed)):  # bit for bit, in cd_radial_enc / cd_radial_dec layout
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    rn = H.revnorm(blob, secs[b"RNRM"])
    c = DATASET1_PARAMS[m.config["DATASET_NUM"] + 10]  # the flat form's constants
    assert rn["consts64"] == tuple(c[k] for k in ("logit_mean", "logit_std", "totalE_mean", "totalE_std", "layers_mean", "layers_std"))
    assert rn["grid"] == cases.GRID and rn["layer_map"] == 1 and rn["logE"] == 1 and rn["dataset_num"] == m.config["DATASET_NUM"]
    assert rn["maxdep"] == np.float32(m.config["MAXDEP"]) and rn["ecut"] == np.float32(m.config["ECUT"])
    assert (rn["emax"], rn["emin"]) == (m.config["EMAX"], m.config["EMIN"])
    mt = H.meta(blob, secs[b"META"])
    assert mt["state"] == (cases.V,) and mt["shape4"] == (cases.V, 0, 0, 0)  # the 1-D state
    assert mt["cond_size"] == 2 + cases.GRID[0] and mt["energy_cols"] == 1 and mt["two_stage"] == int(two_stage) and mt["takes_layers"] == 1
    assert mt["layer_dim"] == cases.GRID[0] + 1 and mt["layer_steps"] == (L.LAYER_STEPS if two_stage else 0)


def test_the_pion_file_keeps_the_configs_narrow_widths(pion2):
    """[16, 16, 16, 32] as the checkpoint has them: the plan widens inside cd_generator_create"""
    m, blob = pion2
    secs, _, _ = H.walk(blob)
    off, _ = secs[b"UNET"]
    desc_bytes, n_weights = struct.unpack_from("<2I", blob, off)
    sd = m.base_model.state_dict()
    assert n_weights == len(sd) and tuple(sd["init_conv.conv.weight"].shape)[0] == 16
    pos = off + 32 + desc_bytes + (-desc_bytes % 8) + 4 * (KN.GRID[2] + KN.GRID[0] + KN.GRID[1])
    seen = {}
    for i in range(n_weights):
        rec = blob[pos + 112 * i:pos + 112 * (i + 1)]
        seen[rec[:96].split(b"\0")[0].decode()] = struct.unpack_from("<Q", rec, 96)[0]
    assert seen == {k: v.numel() for k, v in sd.items()}


def test_form_0_file_holds_the_unconversion_matrices(grid):
    from calodiffusion_amd.postprocess import DATASET1_PARAMS
    m, gc, blob = grid
    secs, version, checksum = H.walk(blob)
    assert version == 3 and list(secs) == [b"META", b"RNRM", b"UNET", b"USMP", b"RADL"] and checksum == G.fnv1a64_py(blob[64:])
    r = H.radial(blob, secs[b"RADL"])
    assert r["form"] == 0 and r["n_mats"] == 1
    _layout_is(r, gc)
    want = torch.cat([p.reshape(-1) for p in gc.pinv_mats]).to(torch.float32).numpy()
    assert np.array_equal(r["mats"][0].view(np.uint32), want.view(np.uint32))
    rn = H.revnorm(blob, secs[b"RNRM"])
    c = DATASET1_PARAMS[1]  # the converted grid's constants
    assert rn["consts64"] == tuple(c[k] for k in ("logit_mean", "logit_std", "totalE_mean", "totalE_std", "layers_mean", "layers_std"))
    assert rn["layer_map"] == 0
    mt = H.meta(blob, secs[b"META"])
    assert mt["state"] == (1,) + K1.GRID and mt["cond_size"] == 1 and mt["takes_layers"] == 0 and mt["layer_dim"] == 0
    # an NNConverter as geometry= is its GeomConverter, as for generate(geometry=): the same bytes
    from calodiffusion_amd import geom1
    assert G.export_generator(m, STEPS, geometry=geom1.NNConverter(geomconverter=gc)) == blob


def test_two_stage_in_model_hgcal_is_a_version_2_form_1_file():
    m = H.two_stage("hg")
    blob = G.export_generator(m, STEPS)
    secs, version, checksum = H.walk(blob)
    assert version == G.FORMAT_VERSION_GEOM == 2 and checksum == G.fnv1a64_py(blob[64:])
    assert list(secs) == [b"META", b"RNRM", b"LAYR", b"LSMP", b"UNET", b"USMP", b"GEOM"]
    form, layers, _, _, cells, n_maps = struct.unpack_from("<6i", blob, secs[b"GEOM"][0])
    assert (form, layers, cells, n_maps) == (1, L.LAYERS["hg"], L.STATE["hg"][2], 2)
    mt = H.meta(blob, secs[b"META"])
    assert mt["state"] == L.STATE["hg"] and mt["two_stage"] == 1 and mt["energy_cols"] == 3 and mt["layer_steps"] == L.LAYER_STEPS
    assert mt["cond_size"] == 3 + L.LAYERS["hg"] + 1


def test_reader_accepts_the_new_files(checker, tmp_path, photon2, pion2, grid):
    r = _check(checker, tmp_path, photon2[1])
    assert r.returncode == 0, r.stderr
    assert "format version 3" in r.stdout and "radial geometry: form 1 (in-model), grid (5, 10, 30), 368 voxels, 1590 matrix floats x 2" in r.stdout
    assert "1 x 8 10 x 16 10 x 19 1 x 5 1 x 5" in r.stdout and "layer model:" in r.stdout
    r = _check(checker, tmp_path, pion2[1])
    assert r.returncode == 0 and "grid (7, 10, 23), 323 voxels" in r.stdout, r.stderr
    r = _check(checker, tmp_path, grid[2])
    assert r.returncode == 0 and "form 0 (on the converted grid)" in r.stdout and "x 1\n" in r.stdout and "layer model" not in r.stdout, r.stderr
    r = _check(checker, tmp_path, G.export_generator(H.two_stage("hg"), STEPS))
    assert r.returncode == 0 and "format version 2" in r.stdout and "geometry: form 1 (in-model)" in r.stdout and "layer model:" in r.stdout, r.stderr


@pytest.mark.parametrize("which", ["photon2", "grid"])
def test_reader_rejects_every_corruption(checker, tmp_path, which, request):
    blob = request.getfixturevalue(which)[-1]
    said = {}
    for label, bad in H.corruptions(blob):
        r = _check(checker, tmp_path, bad)
        assert r.returncode == 1, (label, r.returncode, r.stderr)  # a signal would be a negative status
        assert r.stderr.strip(), label
        said[label] = r.stderr
    assert sum(lab.startswith("truncated") for lab in said) >= 30 and len(said) >= 30 + 80  # (five sections at the least)
    for label, word in (("bound not monotone", "strictly increasing"), ("alpha outside {1, A}", "1 or alpha_out"),
                        ("span mismatch: rin one more", "alpha * rin"), ("matrix entry NaN", "not finite"), ("layers 65", "layers"),
                        ("wtotal 8193", "8192"), ("voxels 6145", "6144"), ("grid row 6145", "6144"), ("bound[0] not 0", "bound[0]"),
                        ("version 3 without RADL", "must have a RADL"), ("version 1 with RADL", "RADL section in a format version 1"),
                        ("RADL renamed GEOM", "GEOM section in a format version 3"), ("future version", "format version 4"),
                        ("RADL appears twice", "appears twice"), ("constant NaN", "not finite")):
        assert word in said[label], (label, said[label])
    if which == "grid":
        assert "layer" in said["layer map on the converted grid"]


def test_export_refusals_by_name(photon, grid):
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    m, _ = photon
    _, gc, _ = grid
    with pytest.raises(ValueError, match=r"converter inside.*geometry= must not be given"):
        G.export_generator(m, STEPS, geometry=gc)
    with pytest.raises(NotImplementedError, match=r"'layer' map on the converted grid"):
        G.export_generator(H.on_the_grid(SHOWERMAP="layer-logit-norm")[0], STEPS, geometry=gc)
    with pytest.raises(NotImplementedError, match=r"Dataset 1.*geometry="):
        G.export_generator(H.on_the_grid()[0], STEPS)
    with pytest.raises(TypeError, match="GeomConverter or NNConverter"):
        G.export_generator(H.on_the_grid()[0], STEPS, geometry=object())
    for cases in (K1, KN):  # the shipped SHAPE_PAD: on a two-stage export, and in the config of a one-stage one
        two = L.model("ph" if cases is K1 else "pi")
        two.shape_pad = [-1, 1, cases.V]
        with pytest.raises(ValueError, match=r"SHAPE_PAD\[2\] \+ 1 != SHAPE_FINAL\[2\] \+ 1.*SHAPE_PAD = SHAPE_FINAL"):
            G.export_generator(two, STEPS)
        one = L.model("ph" if cases is K1 else "pi", cls=CaloDiffusion, SHAPE_PAD=[-1, 1, cases.V])
        with pytest.raises(NotImplementedError, match=rf"Dataset {one.config['DATASET_NUM']} with SHAPE_PAD \[-1, 1, {cases.V}\].*SHAPE_PAD = SHAPE_FINAL"):
            G.export_generator(one, STEPS)
    with pytest.raises(NotImplementedError, match="DPMAdaptive"):
        G.export_generator(H.photon_given(SAMPLER="DPMAdaptive"), STEPS)
    with pytest.raises(NotImplementedError, match="BespokeNonStationary"):
        G.export_generator(H.photon_given(SAMPLER="BespokeNonStationary", TIME_EMBED="sigma"), STEPS)
    with pytest.raises(NotImplementedError, match="debug"):
        G.export_generator(m, STEPS, debug=True)
    with pytest.raises(NotImplementedError, match="SHOWERMAP"):
        G.export_generator(H.photon_given(SHOWERMAP="log-norm"), STEPS)
    with pytest.raises(ValueError, match=r"\(5, 10, 30\).*\(7, 10, 23\)"):
        G.export_generator(H.on_the_grid(DATASET_NUM=0, SHAPE_FINAL=[-1, 1, 7, 10, 23], SHAPE_PAD=[-1, 1, 7, 10, 23])[0], STEPS, geometry=gc)
    assert isinstance(m, CaloDiffusion)


def test_a_program_sampler_compiles_on_the_flat_state():
    m = H.photon_given(SAMPLER="DPMPP2M")
    blob = G.export_generator(m, 5)
    secs, _, _ = H.walk(blob)
    kind, n_steps, n_ops = struct.unpack_from("<3i", blob, secs[b"USMP"][0])
    program = m.sampler_algorithm.build(m, 5, 0).finalize()
    assert (kind, n_steps, n_ops) == (1, program.coefs.shape[0], len(program.ops))


def test_regular_grid_files_are_the_previous_bytes():
    from calodiffusion_amd.configs import load_config
    from calodiffusion_amd.layerdiffusion import LayerDiffusion
    cfg = dict(load_config("dataset2"), LAYER_STEPS=12)
    torch.manual_seed(1234)
    blob = G.export_generator(LayerDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"]), 3)
    assert struct.unpack_from("<I", blob, 8)[0] == G.FORMAT_VERSION == 1
    assert hashlib.sha256(blob).hexdigest() == DATASET2_TWO_STAGE_SHA256
