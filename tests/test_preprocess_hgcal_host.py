"""CPU: the HGCal forward pre-processing (cd_preprocess_hgcal / preprocess.PreprocessHGCal / preprocess_hgcal_shower) as far as
it can be checked without a GPU -- the C ABI's three descriptions agree on the entry point, bad arguments and uncovered
configurations are refused before anything touches the device, and tests/golden/preprocess_hgcal.npz holds the cases and is
what tools/gen_preprocess_hgcal_golden.py writes from the reference."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLD, ROOT, gold
from calodiffusion_amd import engine
from preprocess_hgcal_cases import BATCH, CASES, bins, config, embedded, geometry


def _prototype(name):
    txt = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "calodiff.h")).read(), flags=re.S)
    m = re.search(r"^\s*int\s+%s\s*\((.*?)\)\s*;" % name, txt, flags=re.S | re.M)
    assert m, "%s is not declared in include/calodiff.h" % name
    return [a.strip() for a in m.group(1).split(",")]


def _call(lib, **over):
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    a = dict(enc=None, showers=p, row_stride=4, gen_info=p, gen_cols=1, out=p, layerE=p, e_out=p, status=p, batch=1, layers=2,
             cells=4, grid=4, consts=(C.c_double * 6)(0, 1, 0, 1, 0, 1), embed_mean=0.0, embed_std=1.0, max_deposit=1.0,
             emin=(C.c_double * 1)(0.0), emax=(C.c_double * 1)(1.0), shower_scale=200.0, stream=None)
    a.update(over)
    return lib.cd_preprocess_hgcal(*a.values())


def test_cd_preprocess_hgcal_is_declared_bound_and_exported():
    decl = _prototype("cd_preprocess_hgcal")
    assert "cd_preprocess_hgcal" in engine._SIGNATURES
    res, argtypes = engine._SIGNATURES["cd_preprocess_hgcal"]
    assert res is C.c_int and len(decl) == len(argtypes), (decl, argtypes)
    scalars = {"int": C.c_int, "float": C.c_float, "int64_t": C.c_int64}
    for d, a in zip(decl, argtypes):
        if "*" in d or "[" in d:
            assert a is C.c_void_p or hasattr(a, "contents"), (d, a)
        else:
            assert a is scalars[d.split()[0]], (d, a)
    names = [re.sub(r"\[\d*\]", "", d).split()[-1].lstrip("*") for d in decl]
    assert names == ["enc", "showers", "row_stride", "gen_info", "gen_cols", "out", "layerE", "e_out", "status", "batch", "layers",
                     "cells", "grid", "consts", "embed_mean", "embed_std", "max_deposit", "emin", "emax", "shower_scale", "stream"]
    lib = engine.load_library()  # binds every symbol of the table: AttributeError if the library does not export it
    assert lib.cd_preprocess_hgcal.argtypes == argtypes


@pytest.mark.parametrize("over,needle", [
    (dict(showers=None), b"bad argument"),
    (dict(status=None), b"bad argument"),
    (dict(emin=None), b"bad argument"),
    (dict(batch=0), b"bad argument"),
    (dict(layers=0), b"layers"),
    (dict(layers=5000), b"layers"),
    (dict(gen_cols=9), b"gen_info"),
    (dict(emax=(C.c_double * 1)(0.0)), b"emax > emin"),
    (dict(max_deposit=0.0), b"max_deposit"),
    (dict(cells=3), b"cells = row_stride = grid"),   # no map: the showers are on the grid
    (dict(row_stride=5), b"cells = row_stride = grid"),
])
def test_bad_arguments_are_refused_before_any_launch(over, needle):
    lib = engine.load_library()
    assert _call(lib, **over) == -1
    assert needle in lib.cd_last_error()


def test_the_alias_sits_beside_reverse_norm_hgcal():
    from calodiffusion.utils import HGCal_utils as alias
    from calodiffusion_amd import preprocess
    assert alias.preprocess_hgcal_shower is preprocess.preprocess_hgcal_shower
    assert alias.PreprocessHGCal is preprocess.PreprocessHGCal
    assert callable(alias.ReverseNormHGCal)


@pytest.mark.parametrize("kwargs,needle", [
    (dict(showerMap="log-norm", dataset_num=111), "log map"),
    (dict(showerMap="logit-scaled", dataset_num=111), "scaled"),
    (dict(showerMap="layer-logit-norm-quantile", dataset_num=101), "quantile"),
    (dict(showerMap="layer-logit-norm", dataset_num=111, orig_shape=True), "orig_shape"),
    (dict(showerMap="layer-logit-norm", dataset_num=2), "dataset_num 2"),
])
def test_uncovered_configurations_are_refused_by_name(kwargs, needle, monkeypatch):
    from calodiffusion_amd import preprocess
    monkeypatch.setattr(preprocess, "_run_hgcal", lambda *a, **k: pytest.fail("the device path was reached"))
    monkeypatch.setattr(preprocess, "_device_f32", lambda *a, **k: pytest.fail("the device path was reached"))
    emb, e = np.ones((2, 3, 4, 5), dtype=np.float32), np.full((2,), 60.0, dtype=np.float32)
    with pytest.raises(NotImplementedError, match=needle):
        preprocess.preprocess_hgcal_shower(emb, e, None, **kwargs)
    if not kwargs.get("orig_shape"):
        from calodiffusion_amd.hgcal import HGCalConverter
        conv = HGCalConverter.from_matrices([3, 4, 5], np.zeros((3, 20, 7), dtype=np.float32), np.zeros((3, 7, 20), dtype=np.float32))
        cfg = dict(config("g", 111, "l"), SHOWERMAP=kwargs["showerMap"], DATASET_NUM=kwargs["dataset_num"])
        with pytest.raises(NotImplementedError, match=needle):
            preprocess.PreprocessHGCal(cfg, conv)


def test_the_class_reads_its_config_and_wants_a_converter():
    from calodiffusion_amd.hgcal import HGCalConverter
    from calodiffusion_amd.preprocess import PreprocessHGCal
    conv = HGCalConverter.from_matrices([3, 4, 5], np.zeros((3, 20, 7), dtype=np.float32), np.zeros((3, 7, 20), dtype=np.float32))
    cfg = config("g", 111, "l")
    p = PreprocessHGCal(cfg, conv)
    assert p.bins == (3, 4, 5) and p.shower_scale == 200.0 and p.emin == [50.0, 1.99, 1.57] and p.max_cells is None
    assert PreprocessHGCal({k: v for k, v in cfg.items() if k != "SHOWERSCALE"}, conv).shower_scale == 200.0
    assert PreprocessHGCal(cfg, conv, shower_scale=1.0).shower_scale == 1.0
    assert PreprocessHGCal(dict(cfg, EMAX=100.0, EMIN=50.0, MAX_CELLS=7), conv).emax == [100.0]
    with pytest.raises(TypeError, match="HGCalConverter"):
        PreprocessHGCal(cfg, object())
    with pytest.raises(ValueError, match="MAXDEP"):
        PreprocessHGCal({k: v for k, v in cfg.items() if k != "MAXDEP"}, conv)
    with pytest.raises(ValueError, match="grid"):
        PreprocessHGCal(config("h", 111, "l"), conv)


def test_fixture_holds_the_cases_the_issue_asks_for():
    from calodiffusion_amd.hgcal import init_map
    g = gold("preprocess_hgcal")
    assert os.path.getsize(os.path.join(GOLD, "preprocess_hgcal.npz")) < 512 * 1024
    assert bins("g") == [3, 4, 5] and bins("h") == [28, 12, 21]
    assert [int(n) for n in g["g.ncells"]] == [37, 29, 1]
    h_cells = g["h.ncells"]
    assert int(h_cells.max()) == 301 and len(set(h_cells.tolist())) > 10 and g["h.ring_map"].max() == 20 and g["h.ring_map"].min() == 0
    for tag in ("g", "h"):
        B, (L, A, R) = BATCH[tag], bins(tag)
        raw, gen_info, n = g[f"{tag}.raw"], g[f"{tag}.gen_info"], geometry(tag).max_ncell
        assert raw.dtype == np.float32 and raw.shape[:2] == (B, L) and (raw >= 0).all() and (raw[:, :, :n] == 0).mean() >= 0.6
        assert raw.shape[2] == (41 if tag == "g" else 301)
        for l in range(L):
            assert not raw[:, l, int(h_cells[l] if tag == "h" else g["g.ncells"][l]):].any()
        assert gen_info.shape == (B, 3) and g[f"{tag}.E"].shape == (B, 3)
        for k, (lo, hi) in enumerate(zip([50, 1.99, 1.57], [100, 2.01, 1.572])):
            assert (gen_info[:, k] >= lo).all() and (gen_info[:, k] <= hi).all()
        assert (g[f"{tag}.E"] >= 0).all() and (g[f"{tag}.E"] <= 1).all()
        # the stored geometry gives the map the reference embedded with: its grid is the product with the scaled cells
        enc = np.stack([init_map(A, R, geometry(tag), l)[0].numpy() for l in range(L)]).astype(np.float64)
        emb = np.einsum("len,bln->ble", enc, raw[:, :, :n].astype(np.float64) * 200.0).reshape(B, L, A, R)
        assert np.allclose(g[f"{tag}.111.emb"], emb, rtol=1e-5, atol=1e-9)
    assert ((g["h.raw"].sum(-1) == 0).sum(1) >= 2).any()
    assert not g["g.raw"][5].any() and g["g.raw"][[0, 1, 2, 3, 4, 6, 7]].reshape(7, -1).any(1).all()   # the zero share
    for tag, dnum, m in CASES:
        B, (L, A, R) = BATCH[tag], bins(tag)
        key = f"{tag}.{dnum}.{m}"
        assert g[key + ".data"].shape == (B, L, A, R) and g[key + ".data"].dtype == np.float32 and np.isfinite(g[key + ".data"]).all()
        assert ((key + ".layerE") in g.files) == (m == "l")
        if m == "l":
            assert g[key + ".layerE"].shape == (B, L + 1) and np.isfinite(g[key + ".layerE"]).all()
        emb = embedded(g, tag, dnum)
        assert bool((emb < 0).any()) == (dnum == 101)
        if dnum == 101:
            assert 0.5 < (emb < 0).mean() < 1.0
            assert len(np.unique(g[key + ".data"][emb < 0])) == 1   # the masked logit: one value, 0 before the normalisation


def _reference_root():
    txt = open(os.path.join(ROOT, "oracle", "gen_golden.py")).read()
    return re.search(r'^REF = "(.*)"$', txt, flags=re.M).group(1)


@pytest.mark.skipif(not os.path.isdir(os.path.join(_reference_root(), "calodiffusion")),
                    reason="the reference is not mounted here (it is on the build box only)")
def test_fixture_is_what_the_generator_writes(tmp_path):
    out = tmp_path / "preprocess_hgcal.npz"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_preprocess_hgcal_golden.py"), "--out", str(out)],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    new, old = np.load(out), gold("preprocess_hgcal")
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape, k
        assert new[k].tobytes() == old[k].tobytes(), k
