"""CPU: the host half of calodiffusion_amd.shower_stats -- the geometry tables, the derivations named after the reference's plot
classes (fed with the float64 restatement of the device's raw sums), the binnings, and the refusals -- against the fixture taken
from the reference's own classes (tests/golden/shower_stats.npz).  Bounds: shower_stats_cases."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import shower_stats_cases as S
from conftest import ROOT
from calodiffusion_amd import engine, shower_stats
from calodiffusion_amd.shower_stats import ShowerStatistics, ShowerStats


def geometry(tag):
    return ShowerStatistics.for_hgcal(S.hgcal_geom()) if tag == "hgcal" else ShowerStatistics.for_grid((-1, 1) + S.GRIDS[tag])


def restated_stats(tag, sample):
    geo = geometry(tag)
    tab = S.Tables.of(geo)
    return ShowerStats(*S.restate(S.fixture(tag)[f"showers.{sample}"], tab), tab.n), tab


@pytest.mark.parametrize("tag", S.TAGS)
def test_derivations_reproduce_every_recorded_reference_array(tag):
    geant, tab = restated_stats(tag, "Geant4")
    S.check_against_reference(tag, "Geant4", geant, tab)
    S.check_against_reference(tag, "CaloDiffusion", restated_stats(tag, "CaloDiffusion")[0], tab, geant=geant)


@pytest.mark.parametrize("tag", S.TAGS)
def test_voxel_sample_and_binnings_equal_the_recorded_ones(tag):
    f = S.fixture(tag)
    ref, gen = f["showers.Geant4"], f["showers.CaloDiffusion"]
    assert np.array_equal(shower_stats.voxel_sample(ref), f["HistVoxelE.0.Geant4"])
    assert np.array_equal(shower_stats.voxel_sample(gen, 3), gen[:3].reshape(-1))
    S.check_binnings(tag, shower_stats.binnings(restated_stats(tag, "Geant4")[0], restated_stats(tag, "CaloDiffusion")[0], ref, gen))


def test_grid_tables_match_hand_written_ones():
    """(L, A, R) = (2, 3, 5): cell i of a layer is (alpha i // 5, r i % 5)."""
    third = 2.0 * math.pi / 3.0
    want_r_bin = [0, 1, 2, 3, 4] * 3
    want_a_bin = [0] * 5 + [1] * 5 + [2] * 5
    want_angle = [-third] * 5 + [0.0] * 5 + [third] * 5
    quirk = [0.5] * 3 + [1.5] * 3 + [2.5] * 3 + [3.5] * 3 + [4.5] * 3  # (A, R) read as (R, A): plots.py:507-510
    radial = [0.5, 1.5, 2.5, 3.5, 4.5] * 3
    for projection, want_r in (("reference", quirk), ("radial", radial)):
        r_bin, a_bin, r_coord, angle = shower_stats.grid_tables((-1, 1, 2, 3, 5), projection)
        for got, want, dtype in ((r_bin, want_r_bin, np.int32), (a_bin, want_a_bin, np.int32), (r_coord, want_r, np.float64)):
            assert got.dtype == dtype and got.shape == (2, 15) and np.array_equal(got, [want, want]), projection
        np.testing.assert_allclose(angle, [want_angle, want_angle], rtol=0, atol=4 * 2.0 ** -53 * math.pi)
    geo = ShowerStatistics.for_grid((2, 3, 5))
    assert (geo.n_layers, geo.n_cells, geo.n_rbins, geo.n_abins) == (2, 15, 5, 3)
    with pytest.raises(ValueError, match="r_projection must be 'reference' or 'radial'"):
        ShowerStatistics.for_grid((2, 3, 5), "geometric")


def test_hgcal_tables_come_from_the_geometry_maps():
    g = S.hgcal_geom()
    geo = ShowerStatistics.for_hgcal(g)
    assert (geo.n_layers, geo.n_cells, geo.n_rbins, geo.n_abins, geo.a_bin) == (3, 37, 5, 0, None)
    assert np.array_equal(geo.r_bin, g.ring_map[:, :37].astype(np.int32))
    assert np.array_equal(geo.r_coord, (g.xmap[:, :37] ** 2 + g.ymap[:, :37] ** 2) ** 0.5) and np.array_equal(geo.angle, g.theta_map[:, :37])
    with pytest.raises(ValueError, match="a_profile was not computed"):
        restated_stats("hgcal", "Geant4")[0].energy_phi()


def test_limits_and_shapes_are_refused_by_name():
    ok = dict(r_bin=np.zeros((2, 4), np.int32), n_rbins=1, a_bin=None, n_abins=0, r_coord=np.zeros((2, 4)), angle=np.zeros((2, 4)))
    ShowerStatistics(**ok)
    for change, message in ((dict(r_bin=np.zeros((2, 4097), np.int32), r_coord=np.zeros((2, 4097)), angle=np.zeros((2, 4097))), "4097 cells a layer"),
                            (dict(r_bin=np.zeros((513, 1), np.int32), r_coord=np.zeros((513, 1)), angle=np.zeros((513, 1))), "513 layers"),
                            (dict(n_rbins=257), "257 radial bins"), (dict(n_rbins=0), "0 radial bins"),
                            (dict(a_bin=np.zeros((2, 4), np.int32), n_abins=257), "257 angular bins"),
                            (dict(n_abins=3), "3 angular bins without an a_bin table"),
                            (dict(r_bin=np.full((2, 4), 1, np.int32)), r"r_bin holds indices outside \[-1, 1\)"),
                            (dict(r_bin=np.full((2, 4), -2, np.int32)), r"r_bin holds indices outside \[-1, 1\)"),
                            (dict(a_bin=np.full((2, 4), 2, np.int32), n_abins=2), r"a_bin holds indices outside \[-1, 2\)"),
                            (dict(r_coord=np.full((2, 4), np.inf)), "r_coord and angle must be finite"),
                            (dict(angle=np.full((2, 4), np.nan)), "r_coord and angle must be finite"),
                            (dict(angle=np.zeros((2, 5))), "must share one")):
        with pytest.raises(ValueError, match=message):
            ShowerStatistics(**{**ok, **change})
    geo = ShowerStatistics.for_grid((2, 3, 5))
    launched = []
    geo._launch = lambda *a, **k: launched.append(a)
    for bad in (np.zeros((4, 29), np.float32), np.zeros((30,), np.float32), np.zeros((4, 2, 16), np.float32)):
        with pytest.raises(ValueError, match="expected showers of 2 x 15 = 30 elements"):
            geo.compute(bad)
    with pytest.raises(ValueError, match="chunk must be positive"):
        geo.compute(np.zeros((4, 30), np.float32), chunk=0)
    assert not launched
    with pytest.raises(ValueError, match="7 energies for 8 showers"):
        restated_stats("g2x3x5", "Geant4")[0].e_ratio(np.ones(7))


def _desc(L=2, n=4, n_rbins=1, n_abins=0, r_bin=None, a_bin=None, r_coord=None, angle=None, struct_size=None, null=()):
    keep = {"r_bin": (C.c_int32 * (L * n))(*(r_bin or [0] * (L * n))), "a_bin": (C.c_int32 * (L * n))(*a_bin) if a_bin is not None else None,
            "r_coord": (C.c_double * (L * n))(*(r_coord or [0.0] * (L * n))), "angle": (C.c_double * (L * n))(*(angle or [0.0] * (L * n)))}
    for name in null:
        keep[name] = None
    d = engine.CdShowerStatsDesc(C.sizeof(engine.CdShowerStatsDesc) if struct_size is None else struct_size, L, n, n_rbins, n_abins,
                                 keep["r_bin"], keep["a_bin"], keep["r_coord"], keep["angle"])
    return d, keep


@pytest.mark.parametrize("kwargs, message", [
    (dict(struct_size=48), "CdShowerStatsDesc.struct_size is 48"),
    (dict(L=0), "n_layers must be in [1, 512], got 0"),
    (dict(L=1, n=4097), "n_cells must be in [1, 4096], got 4097"),
    (dict(n_rbins=257), "n_rbins must be in [1, 256], got 257"),
    (dict(n_abins=257, a_bin=[0] * 8), "n_abins must be in [0, 256], got 257"),
    (dict(null=("r_bin",)), "the r_bin table is null"),
    (dict(null=("r_coord",)), "the r_coord table is null"),
    (dict(null=("angle",)), "the angle table is null"),
    (dict(n_abins=2), "an a_bin table goes with n_abins > 0"),
    (dict(a_bin=[0] * 8), "an a_bin table goes with n_abins > 0"),
    (dict(r_bin=[0, 0, 0, 1, 0, 0, 0, 0]), "r_bin[3] = 1 is outside [-1, 1)"),
    (dict(n_abins=2, a_bin=[0, 1, -2, 0, 0, 0, 0, 0]), "a_bin[2] = -2 is outside [-1, 2)"),
    (dict(r_coord=[0.0] * 7 + [float("inf")]), "r_coord[7] is not finite"),
    (dict(angle=[float("nan")] + [0.0] * 7), "angle[0] is not finite"),
])
def test_library_refuses_a_bad_descriptor_before_touching_the_device(kwargs, message):
    lib = engine.load_library()
    d, keep = _desc(**kwargs)
    handle = C.c_void_p()
    assert lib.cd_shower_stats_create(C.byref(d), C.byref(handle), None) == -1
    assert message in lib.cd_last_error().decode(), lib.cd_last_error()
    assert not handle.value


def test_library_refuses_bad_cut_arguments():
    lib = engine.load_library()
    for args, message in (((None, None, 1, 4, 0.0, None), "x must not be null"), ((1 << 12, None, -1, 4, 0.0, None), "rows must not be negative"),
                          ((1 << 12, None, 1, 0, 0.0, None), "row_len must be in [1, 4096], got 0"),
                          ((1 << 12, None, 1, 4097, 0.0, None), "row_len must be in [1, 4096], got 4097")):
        assert lib.cd_threshold_conserve(*args) == -1
        assert message in lib.cd_last_error().decode()


def test_descriptor_matches_the_header_and_the_stub(tmp_path):
    """CdShowerStatsDesc holds pointers, which test_abi's struct parser does not read: compare its three descriptions here, and
    its layout as the C compiler sees it."""
    import subprocess
    txt = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "calodiff.h")).read(), flags=re.S)
    body = re.search(r"struct CdShowerStatsDesc \{(.*?)\};", txt, flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls == ["uint32_t struct_size", "int32_t n_layers", "int32_t n_cells", "int32_t n_rbins", "int32_t n_abins", "const int32_t* r_bin",
                     "const int32_t* a_bin", "const double* r_coord", "const double* angle"]
    assert [n for n, _ in engine.CdShowerStatsDesc._fields_] == [d.split()[-1] for d in decls] and C.sizeof(engine.CdShowerStatsDesc) == 56
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("cd_shower_stats_create", "cd_shower_stats_destroy", "cd_shower_stats_compute", "cd_threshold_conserve"):
        assert name in engine._SIGNATURES and re.search(rf"\b{name}\s*\(", txt) and name in md
    lines = ['#include <stddef.h>', '#include "calodiff.h"',
             f'_Static_assert(sizeof(CdShowerStatsDesc) == {C.sizeof(engine.CdShowerStatsDesc)}, "CdShowerStatsDesc");']
    lines += [f'_Static_assert(offsetof(CdShowerStatsDesc, {name}) == {getattr(engine.CdShowerStatsDesc, name).offset}, "{name}");'
              for name, _ in engine.CdShowerStatsDesc._fields_]
    src = tmp_path / "stats_abi.c"
    src.write_text("\n".join(lines + ["int main(void) { return 0; }", ""]))
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "stats_abi.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_generate_refuses_a_cut_of_normalised_showers():
    from helpers import seeded_model
    with pytest.raises(ValueError, match="cuts physical showers"):
        seeded_model("tiny").generate([], 2, reverse_norm=False, emin=1e-3)


def test_generate_refuses_a_cut_of_anything_but_a_regular_grid_or_hgcal_cells():
    """Before sampling for the Dataset-0/1 device form (irregular SHAPE_ORIG voxels); when it returns for a reverse_norm callable
    whose showers are not layers x alpha x r elements each.  Neither reaches the device."""
    import inspect
    import torch
    import ds1_model_cases as K
    from helpers import SEED, seeded_model
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    from calodiffusion_amd.layerdiffusion import LayerDiffusion
    cfg = K.config()
    state = torch.random.get_rng_state()
    torch.manual_seed(SEED)
    ds1 = CaloDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"])
    torch.random.set_rng_state(state)
    sampled = []
    ds1.sample = lambda *a, **k: sampled.append(a)
    with pytest.raises(ValueError, match="not provided for Dataset 0 / 1"):
        ds1.generate([(torch.zeros((2, 1)), torch.zeros((2, 6)), None)], 2, geometry=ds1.NN_embed, emin=0.1)
    assert not sampled
    grid = seeded_model("dataset2")  # 45 x 16 x 9 = 6480 elements a shower, rows of 9
    for bad in (np.ones((15, 368), np.float32), np.ones((9, 100), np.float32), np.ones((6480,), np.float32)):
        with pytest.raises(ValueError, match=r"are not the regular grid of SHAPE_FINAL \(6480 elements a shower, rows of 9\)"):
            grid._energy_cut(bad, 0.1)
    assert "emin" in inspect.signature(LayerDiffusion.generate).parameters and "emin" in inspect.signature(CaloDiffusion.generate).parameters
