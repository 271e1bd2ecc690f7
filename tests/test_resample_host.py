"""CPU-only: every case of resample_cases.py has the property it exists for, by the launchers' own arithmetic (mirrored there), and the
fp64 reference of test_gpu_resample.py agrees with itself and with the golden vectors of the reference."""
import numpy as np
import pytest
import torch

import resample_cases as R
from conftest import gold, rel_l2
from oracle import torch_oracle as O


def _names(table):
    return [c.name for c in table]


def test_case_names_are_unique_and_the_groups_name_cases():
    every = _names(R.CONVT_CASES + R.TILED_CASES + R.FLAT_CASES + R.CONV_BWD_CASES + R.CONVT_BWD_CASES)
    assert len(set(every)) == len(every)
    assert set(R.CONVT_NO_WHOLE_TILE) | set(R.CONVT_CT) | set(R.CHILD_FWD_T) | set(R.CONVT_SEAMED_BOTH) <= set(_names(R.CONVT_CASES))
    assert set(R.CHILD_FWD_S) <= set(_names(R.TILED_CASES + R.FLAT_CASES))
    assert set(R.CONV_BWD_SEAMED) | set(R.CONV_BWD_NZ) | set(R.CHILD_BWD) <= set(_names(R.CONV_BWD_CASES))
    assert set(R.CONV_BWD_SEAMED) | set(R.CONV_BWD_NZ) == set(_names(R.CONV_BWD_CASES))
    assert set(R.CONVT_BWD_TILED) | set(R.CONVT_BWD_FLAT) == set(_names(R.CONVT_BWD_CASES))
    assert set(R.CHILD_BWD_T) <= set(_names(R.CONVT_BWD_CASES))


# ---- transposed conv ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CONVT_NO_WHOLE_TILE)
def test_transposed_conv_cases_have_no_tile_that_covers_the_grid(name):
    c = R.by_name(R.CONVT_CASES, name)
    dout = R.convt_out(c.din, c.kz, c.sz, c.out_pad)
    az, bh = R.convt_class_extents(dout, c.sz)
    tiles = R.convt_all_tiles(c.c, c.din, dout, c.sz, c.batch)
    assert tiles, "the launcher would refuse the shape"
    assert R.convt_tile_lds(az, bh, c.din[2], c.c) > R.CONVT_LDS_LIMIT
    assert not R.convt_has_whole_tile(c.c, c.din, dout, c.sz)
    cand = R.convt_candidates(c.c, c.din, dout, c.sz, c.batch)
    assert 1 <= len(cand) <= 14 and len(set(cand)) == len(cand)
    for tz, th in cand:   # a seam in z or in phi in whatever the timer picks
        assert tz < az or th < bh
        assert R.convt_tile_lds(tz, th, c.din[2], c.c) <= R.CONVT_LDS_LIMIT


def test_transposed_conv_case_properties():
    cases = {c.name: c for c in R.CONVT_CASES}
    for name, ct in R.CONVT_CT.items():
        assert R.convt_ct(cases[name].c) == ct
    assert {R.convt_ct(c.c) for c in R.CONVT_CASES} == {1, 2, 3, 4}
    c = cases["t32_6x12x9_ds3l1"]
    assert R.convt_out(c.din, c.kz, c.sz, c.out_pad) == (11, 25, 19)
    assert cases["t96_5x7x6_nocz"].sz == 1
    # 128 channels with kz = 4, 64 channels on a wide grid: every tile that fits is seamed in z AND in phi
    assert "t128_9x9x9_k4" in R.CONVT_SEAMED_BOTH and cases["t128_9x9x9_k4"].kz == 4
    for name in R.CONVT_SEAMED_BOTH:
        c = cases[name]
        dout = R.convt_out(c.din, c.kz, c.sz, c.out_pad)
        az, bh = R.convt_class_extents(dout, c.sz)
        tiles = R.convt_all_tiles(c.c, c.din, dout, c.sz, c.batch)
        assert tiles and all(tz < az and th < bh for tz, th, _ in tiles), name
    # the batch case: more workgroups than the 256 CUs, on the tile taken without timing too
    c = cases["t32_4x8x5_b40"]
    dout = R.convt_out(c.din, c.kz, c.sz, c.out_pad)
    az, bh = R.convt_class_extents(dout, c.sz)
    for tz, th in R.convt_candidates(c.c, c.din, dout, c.sz, c.batch)[:1]:
        assert c.batch * (-(-az // tz)) * (-(-bh // th)) > 256
    # all four output paddings' parities of phi and r occur in the forward table
    assert {cc.out_pad[1:] for cc in R.CONVT_CASES} == {(0, 0), (1, 1), (0, 1), (1, 0)}


def test_transposed_conv_enumeration_on_a_shape_worked_by_hand():
    """32 channels, input 10 x 8 x 9, stride 2: Az = 10, Bh = 8, 36-float records of 144 B, 9 voxels per row: a tile of
    (TZ + 2)(TH + 2) rows holds ((TZ + 2)(TH + 2) 9 + 1) 144 B <= 143 360 B, i.e. (TZ + 2)(TH + 2) <= 110."""
    dout = R.convt_out((10, 8, 9), 3, 2, (0, 0, 0))
    assert dout == (19, 16, 18) and R.convt_class_extents(dout, 2) == (10, 8)
    tiles = {(tz, th) for tz, th, _ in R.convt_all_tiles(32, (10, 8, 9), dout, 2)}
    assert all((tz + 2) * (th + 2) <= 110 for tz, th in tiles)
    assert (10, 8) not in tiles and (10, 7) in tiles              # 12 x 10 = 120 rows; 12 x 9 = 108
    assert (9, 8) in tiles and (5, 8) not in tiles                # 11 x 10 = 110 fits; TZ = 5..9 all give two z tiles: the largest is kept
    assert (10, 4) not in tiles and (10, 6) not in tiles          # TH = 4..7 all give two phi tiles: only TH = 7 is kept


# ---- strided conv -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.TILED_CASES, ids=_names(R.TILED_CASES))
def test_halo_tiled_cases_are_declined_by_the_flat_kernel_and_have_no_whole_grid_tile(case):
    for batch in (case.batch, case.batch + 1):
        for prec in R.PRECISIONS:
            assert not R.flat_accepts(case.din, R.K344, case.stride, case.cout, batch, prec), prec
    for prec, vb in R.TILED_VOX_BYTES.items():
        assert R.tiled_whole_grid_lds(case.din, R.K344, case.stride, vb) > 150 * R.KIB, prec
        tiles = R.tiled_tiles(case.din, R.K344, case.stride, vb)
        dout = R.conv_out(case.din, R.K344, case.stride)
        assert tiles and all(tz < dout[0] or th < dout[1] for tz, th in tiles), prec
        if case.din[1] == 50:   # Dataset-3's level-0 width: not even one output plane spans phi
            assert all(th < dout[1] for tz, th in tiles), prec


def test_halo_tiled_table_covers_the_channel_splits():
    pairs = {(c.cin, c.cout) for c in R.TILED_CASES}
    assert pairs == set(R.CHANNEL_PAIRS)
    assert {R.flat_ct_max(co) for _, co in pairs} == {1, 2, 3}
    assert R.flat_ct_max(128) == 2 and (128 // 32) % R.flat_ct_max(128) == 0    # CTtot > 3 -> CT = 2, two channel groups
    assert {c.stride[0] for c in R.TILED_CASES} == {1, 2}
    assert {c.din for c in R.TILED_CASES} == {(5, 22, 18), (7, 50, 18)}
    for din in ((5, 22, 18), (7, 50, 18)):
        assert {(c.cin, c.cout) for c in R.TILED_CASES if c.din == din and c.stride == (2, 2, 2)} == set(R.CHANNEL_PAIRS)


@pytest.mark.parametrize("case", R.FLAT_CASES, ids=_names(R.FLAT_CASES))
def test_flat_cases_are_accepted_and_every_forced_tiling_is_taken(case):
    assert set(case.tilings) == set(R.FLAT_VOX_BYTES)
    dout = R.conv_out(case.din, R.K344, case.stride)
    ovox = int(np.prod(dout))
    for prec, tilings in case.tilings.items():
        assert R.flat_candidates(case.din, R.K344, case.stride, case.cout, case.batch, prec), prec
        assert R.flat_accepts(case.din, R.K344, case.stride, case.cout, case.batch, prec), prec
        for nt, vt in tilings:
            assert vt > 0   # (a negative vt would run the warp-specialised kernel on the wrong weight image)
            assert R.flat_override_valid(nt, vt, case.din, R.K344, case.stride, case.cout, prec), (prec, nt, vt)
        units = [R.flat_units(nt, case.din, R.K344, case.stride) for nt, _ in tilings]
        assert len(set(tilings)) == len(tilings) >= 4
        # from one row tile per unit down to the fewest units a tiling the override takes can have
        reachable = [R.flat_units(nt, case.din, R.K344, case.stride) for nt in range(1, 65) for vt in range(1, 9)
                     if R.flat_override_valid(nt, vt, case.din, R.K344, case.stride, case.cout, prec)]
        assert max(units) == max(reachable) == (ovox + 31) // 32 >= 5 and min(units) == min(reachable) <= 3, (prec, units)
        assert len(set(units)) >= 3, (prec, units)
        assert all(32 * (nt - 1) < ovox for nt, _ in tilings)   # no tiling has a wave without rows in every unit
        # a unit boundary inside an output plane, not only between planes (the 8 x 4 output plane of 9 x 16 x 9 is one row tile)
        assert (dout[1] * dout[2]) % 32 == 0 or any((32 * nt) % (dout[1] * dout[2]) for nt, _ in tilings)
    assert min(R.flat_units(nt, case.din, R.K344, case.stride) for nt, _ in case.tilings["f16x2"]) <= 2
    # the f32 arithmetic has no strided flat kernel: the case runs on the halo-tiled f32 kernel there
    assert not R.flat_accepts(case.din, R.K344, case.stride, case.cout, case.batch, "f32")
    assert R.tiled_tiles(case.din, R.K344, case.stride, R.TILED_VOX_BYTES["f32"])


def test_flat_table_covers_the_geometries_and_channel_tiles():
    assert {R.flat_geo(R.K344, c.stride) for c in R.FLAT_CASES} == {1, 2}
    assert {R.flat_ct_max(c.cout) for c in R.FLAT_CASES} == {1, 2, 3}
    assert {c.din for c in R.FLAT_CASES} == {(9, 16, 9), (9, 25, 9), (6, 25, 9)}
    assert any(c.din[1] % 2 for c in R.FLAT_CASES)
    planes = [int(np.prod(R.conv_out(c.din, R.K344, c.stride)[1:])) for c in R.FLAT_CASES]
    assert sum(p % 32 != 0 for p in planes) >= 2


# ---- backward -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CONV_BWD_CASES, ids=_names(R.CONV_BWD_CASES))
def test_conv_backward_cases(case):
    dout = R.conv_out(case.din, R.K344, case.stride)
    if case.name in R.CONV_BWD_NZ:
        assert R.wgrad_strided_nz(case.din, 3, case.stride[0]) == R.CONV_BWD_NZ[case.name]
    if case.name in R.CONV_BWD_SEAMED:
        # dx: the transposed kernel reads dy (cout channels on the conv's output grid) and has no tile over the whole grid
        assert case.din[1] % 2 == 0
        assert not R.convt_has_whole_tile(case.cout, dout, case.din, case.stride[0])
        assert R.convt_all_tiles(case.cout, dout, case.din, case.stride[0], case.batch)


def test_conv_backward_table():
    assert sorted(R.CONV_BWD_NZ.values()) == [1, 2, 4]
    assert {c.stride[0] for c in R.CONV_BWD_CASES if c.name in R.CONV_BWD_SEAMED} == {1, 2}
    scales = {c.dy_scale for c in R.CONV_BWD_CASES if c.din == (5, 22, 18) and c.stride == (2, 2, 2)}
    assert scales == {1.0, 3e-7, 2e4}
    # the rung arithmetic on the first grid, by hand: coarse 5 x 4 x 2, RP = 32, rows of (8 + 3)(5 + 2) = 77 records
    assert R.wgrad_strided_lds(4, (9, 8, 5), 3, 2) == (33 + 9 * 77) * 144
    assert R.wgrad_strided_lds(2, (9, 16, 9), 3, 2) == (65 + 5 * 209) * 144 <= 160 * R.KIB < R.wgrad_strided_lds(4, (9, 16, 9), 3, 2)
    assert R.wgrad_strided_lds(1, (5, 25, 9), 3, 2) == (49 + 3 * 308) * 144 <= 160 * R.KIB < R.wgrad_strided_lds(2, (5, 25, 9), 3, 2)
    # the declined case of test_conv_weight_gradient_ladder_rungs (test_gpu_backward.py)
    assert R.wgrad_strided_nz((3, 18, 17), 3, 2) == 0 and R.wgrad_strided_lds(1, (3, 18, 17), 3, 2) == 184032


@pytest.mark.parametrize("case", R.CONVT_BWD_CASES, ids=_names(R.CONVT_BWD_CASES))
def test_conv_transpose_backward_cases(case):
    assert case.batch >= 2
    din, k, stride = R.convt_bwd_dx_geom(case)
    assert R.conv_out(din, k, stride) == case.din          # the input gradient's conv lands on the up conv's input grid
    assert R.flat_geo(k, stride) == (3 if case.kz == 4 else (1 if case.sz == 2 else 2))
    if case.name == R.CONVT_BWD_WGRAD_KD4:                 # dw: on the strided fp16 kernel, kd = 4
        assert case.kz == 4 and R.wgrad_strided_nz(din, 4, case.sz) > 0
    if case.name in R.CONVT_BWD_TILED:
        for prec in R.PRECISIONS:
            assert not R.flat_accepts(din, k, stride, case.c, case.batch, prec), prec
        for prec, vb in R.TILED_VOX_BYTES.items():
            assert R.tiled_whole_grid_lds(din, k, stride, vb) > 150 * R.KIB, prec
            assert R.tiled_tiles(din, k, stride, vb), prec
    else:
        for prec in R.FLAT_VOX_BYTES:
            cand = R.flat_candidates(din, k, stride, case.c, case.batch, prec)
            assert cand and all(R.flat_units(nt, din, k, stride) > 1 for nt, _, _ in cand), prec


def test_conv_transpose_backward_table():
    k3 = [c for c in R.CONVT_BWD_CASES if c.kz == 3 and c.sz == 2 and c.name in R.CONVT_BWD_TILED]
    assert {c.out_pad for c in k3} == {(0, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1)} and len({c.din for c in k3}) == 1
    assert {c.kz for c in R.CONVT_BWD_CASES} == {3, 4} and {c.sz for c in R.CONVT_BWD_CASES} == {1, 2}
    assert any(c.kz == 4 and c.out_pad[1] for c in R.CONVT_BWD_CASES)    # fold_phi before the 64-tap conv


# ---- the reference ------------------------------------------------------------------------------------------------
def _fp32_rounding(taps_times_cin):
    """fp32 accumulation of n products against fp64: relative L2 of order sqrt(n) eps at worst for stock kernels; 4x headroom"""
    return 4 * np.sqrt(taps_times_cin) * 2.0 ** -24


def test_fp64_reference_equals_the_fp32_reference_to_fp32_rounding():
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 32, 5, 6, 7, generator=gen)
    w, b = torch.randn(64, 32, 3, 4, 4, generator=gen) * 0.05, torch.randn(64, generator=gen)
    for stride in ((2, 2, 2), (1, 2, 2)):
        y32 = O.cyl_conv3d(x, w, b, stride=stride, padding=(1, 1, 1))
        y64 = O.cyl_conv3d(x.double(), w.double(), b.double(), stride=stride, padding=(1, 1, 1))
        assert y64.dtype == torch.float64 and y64.shape == y32.shape
        assert rel_l2(y32.numpy(), y64.numpy()) < _fp32_rounding(48 * 32)
    for kz, sz, op in ((3, 2, (0, 1, 1)), (4, 2, (0, 0, 1)), (3, 1, (0, 1, 0))):
        wt = torch.randn(32, 32, kz, 4, 4, generator=gen) * 0.05
        y32 = O.cyl_conv_transpose3d(x, wt, b[:32], (sz, 2, 2), op)
        y64 = O.cyl_conv_transpose3d(x.double(), wt.double(), b[:32].double(), (sz, 2, 2), op)
        assert y64.dtype == torch.float64 and tuple(y64.shape[2:]) == R.convt_out((5, 6, 7), kz, sz, op)
        assert rel_l2(y32.numpy(), y64.numpy()) < _fp32_rounding(kz * 16 * 32)


def test_fp64_reference_equals_the_golden_resampling_outputs():
    g = gold("primitives_conv")
    tags = sorted({k.split(".")[0] for k in g.files if k.startswith(("down", "up"))})
    assert {"down_d2", "down_odd", "down_noz"} <= set(tags) and sum(t.startswith("up") for t in tags) == 6
    for tag in tags:
        x, w, b = (torch.from_numpy(np.asarray(g[f"{tag}.{k}"])).double() for k in "xwb")
        zs = 2 if int(g[f"{tag}.cz"]) else 1
        if tag.startswith("down"):
            y = O.cyl_conv3d(x, w, b, stride=(zs, 2, 2), padding=(1, 1, 1))
        else:
            e = g[f"{tag}.extra"]
            y = O.cyl_conv_transpose3d(x, w, b, (zs, 2, 2), (0, int(e[1]), int(e[2])))
        want = g[f"{tag}.y"]
        assert tuple(y.shape) == want.shape, tag
        assert rel_l2(y.numpy(), want) < _fp32_rounding(int(np.prod(w.shape[2:])) * x.shape[1]), tag


def test_per_sample_comparison_is_not_diluted_and_locates_the_error():
    want = np.random.default_rng(0).standard_normal((40, 3, 4, 5, 6))
    got = want.copy()
    got[17, 2, 3, 1, 4] += 1.0
    errs = R.per_sample_rel_l2(got, want)
    assert errs[17] > 0.05 and np.count_nonzero(errs) == 1
    assert rel_l2(got, want) < errs[17] / 5          # what a whole-batch norm would have reported
    err, where = R.worst_sample(got, want)
    assert err == errs[17] and "sample 17 of 40" in where and "(3, 1, 4, 2)" in where
    got[3, 0, 0, 0, 0] = np.nan
    err, where = R.worst_sample(got, want)
    assert err == np.inf and "sample 3 of 40" in where and "(0, 0, 0, 0)" in where
