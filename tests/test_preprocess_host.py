"""CPU: the forward pre-processing (cd_preprocess / calodiffusion_amd.preprocess) as far as it can be checked without a GPU --
the C ABI's three descriptions agree on the new entry point, the uncovered configurations are refused by name before anything
touches the device, and tests/golden/preprocess.npz is what tools/gen_preprocess_golden.py writes from the reference."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLD, ROOT, gold
from calodiffusion_amd import engine


def _prototype(name):
    txt = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "calodiff.h")).read(), flags=re.S)
    m = re.search(r"^\s*int\s+%s\s*\((.*?)\)\s*;" % name, txt, flags=re.S | re.M)
    assert m, "%s is not declared in include/calodiff.h" % name
    return [a.strip() for a in m.group(1).split(",")]


def test_cd_preprocess_is_declared_bound_and_exported():
    decl = _prototype("cd_preprocess")
    assert "cd_preprocess" in engine._SIGNATURES
    res, argtypes = engine._SIGNATURES["cd_preprocess"]
    assert res is C.c_int and len(decl) == len(argtypes), (decl, argtypes)
    scalars = {"int": C.c_int, "float": C.c_float}
    for d, a in zip(decl, argtypes):
        if "*" in d or "[" in d:
            assert a is C.c_void_p or hasattr(a, "contents"), (d, a)
        else:
            assert a is scalars[d.split()[0]], (d, a)
    # the argument style of cd_reverse_norm: dims, the six constants, max_deposit, then the energy map, nullable layerE, stream
    names = [re.sub(r"\[\d*\]", "", d).split()[-1].lstrip("*") for d in decl]
    assert names == ["showers", "energy", "out", "layerE", "e_out", "status", "batch", "dims", "consts", "max_deposit", "emin",
                     "emax", "logE", "shower_scale", "stream"]
    lib = engine.load_library()  # binds every symbol of the table: AttributeError if the library does not export it
    assert lib.cd_preprocess.argtypes == argtypes
    # bad arguments are refused before any launch (no GPU is touched)
    assert lib.cd_preprocess(None, None, None, None, None, None, 1, (C.c_int32 * 3)(1, 1, 1), (C.c_float * 6)(), 2.0, 1.0, 1000.0,
                             1, 1.0, None) == -1
    assert b"bad argument" in lib.cd_last_error()


def test_the_alias_sits_beside_reverse_norm():
    from calodiffusion.utils import utils as alias
    from calodiffusion_amd import preprocess
    assert alias.preprocess_shower is preprocess.preprocess_shower and alias.Preprocess is preprocess.Preprocess
    assert callable(alias.ReverseNorm)


@pytest.mark.parametrize("kwargs,needle", [
    (dict(showerMap="layer-logit-norm", dataset_num=1), "dataset_num 1"),
    (dict(showerMap="layer-logit-norm", dataset_num=0), "dataset_num 0"),
    (dict(showerMap="logit-norm", dataset_num=2, orig_shape=True), "orig_shape"),
    (dict(showerMap="logit-norm-quantile", dataset_num=2), "quantile"),
    (dict(showerMap="log-norm", dataset_num=2), "log map"),
    (dict(showerMap="sqrt", dataset_num=3), "sqrt"),
    (dict(showerMap="logit-scaled", dataset_num=3), "scaled"),
    (dict(showerMap="logit-norm", dataset_num=111), "dataset_num 111"),
])
def test_preprocess_shower_refuses_uncovered_configurations_by_name(kwargs, needle, monkeypatch):
    from calodiffusion_amd import preprocess
    monkeypatch.setattr(preprocess, "_run", lambda *a, **k: pytest.fail("the device path was reached"))
    raw, e = np.ones((2, 6480), dtype=np.float32), np.ones((2, 1), dtype=np.float32)
    with pytest.raises(NotImplementedError, match=needle):
        preprocess.preprocess_shower(raw, e, (-1, 1, 45, 16, 9), "", **kwargs)


def test_preprocess_class_refuses_uncovered_configs_by_name():
    from calodiffusion_amd.configs import load_config
    from calodiffusion_amd.preprocess import Preprocess
    cfg = load_config("dataset2")
    p = Preprocess(cfg)
    assert p.dims == (45, 16, 9) and p.showerMap == "layer-logit-norm" and p.shower_scale == 0.001 and p.logE is True
    assert Preprocess(load_config("dataset3")).dims == (45, 50, 18)
    with pytest.raises(NotImplementedError, match="quantile"):
        Preprocess(dict(cfg, SHOWERMAP="layer-logit-norm-quantile"))
    with pytest.raises(NotImplementedError, match="dataset_num 1"):
        Preprocess(dict(cfg, DATASET_NUM=1))
    with pytest.raises(NotImplementedError, match="preprocess_hgcal_shower"):
        Preprocess(load_config("hgcal"))
    with pytest.raises(ValueError, match="MAXDEP"):
        Preprocess({k: v for k, v in cfg.items() if k != "MAXDEP"})


def test_fixture_holds_the_inputs_the_issue_asks_for():
    g = gold("preprocess")
    assert sorted(g.files) == sorted(["d2.showers", "d2.incident_energies", "d2.data", "d2.layerE", "d2.E", "d2.E_lin",
                                      "d3.showers", "d3.incident_energies", "d3.data", "d3.E"])
    assert os.path.getsize(os.path.join(GOLD, "preprocess.npz")) < 512 * 1024
    for tag, dims in (("d2", (45, 16, 9)), ("d3", (45, 50, 18))):
        raw, e = g[f"{tag}.showers"], g[f"{tag}.incident_energies"]
        assert raw.shape == (8, int(np.prod(dims))) and raw.dtype == np.float32 and e.shape == (8, 1)
        assert (raw >= 0).all() and (raw == 0).mean() >= 0.6
        per_layer = raw.reshape((8,) + dims).sum(axis=(2, 3))
        assert ((per_layer == 0).sum(axis=1) >= 2).any() and (raw.sum(axis=1) > 0).all()
        assert e.min() >= 1e3 and e.max() <= 1e6 and e.max() / e.min() > 50        # MeV, spread over decades
        assert (raw.astype(np.float64).sum(axis=1) / e[:, 0] < 2).all()             # deposited fraction below max_deposit
        assert raw[raw > 0].min() * 1e-3 > 0.0000151                                 # above ECUT (GeV)
        assert np.isfinite(g[f"{tag}.data"]).all() and g[f"{tag}.data"].shape == raw.shape


def _reference_root():
    txt = open(os.path.join(ROOT, "oracle", "gen_golden.py")).read()
    return re.search(r'^REF = "(.*)"$', txt, flags=re.M).group(1)


@pytest.mark.skipif(not os.path.isdir(os.path.join(_reference_root(), "calodiffusion")),
                    reason="the reference is not mounted here (it is on the build box only)")
def test_fixture_is_what_the_generator_writes(tmp_path):
    out = tmp_path / "preprocess.npz"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_preprocess_golden.py"), "--out", str(out)],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    new, old = np.load(out), gold("preprocess")
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape, k
        assert new[k].tobytes() == old[k].tobytes(), k
