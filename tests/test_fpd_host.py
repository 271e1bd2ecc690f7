"""CPU: the host steps of calodiffusion_amd.evaluate.fpd -- batch sizes, the draws, the Frechet distance of two Gaussians, the
constrained extrapolation -- against the restatement of fpd_cases.py (and SciPy where it is installed), the FDP class's
construction and import paths, and every refusal of cd_fpd_moments (they come before anything touches the device)."""
import ctypes as C

import numpy as np
import pytest

import fpd_cases as F
import hlf_cases as H
from calodiffusion_amd import engine, evaluate as E


def test_batch_sizes():
    want = (1 / np.linspace(1 / 20000, 1 / 50000, 10)).astype("int32")
    got = E.fpd_batch_sizes()
    assert got.dtype == np.int32 and np.array_equal(got, want) and got[0] == 20000 and len(got) == 10
    assert 49999 <= got[-1] <= 50000
    assert np.array_equal(E.fpd_batch_sizes(200, 500, 3), (1 / np.linspace(1 / 200, 1 / 500, 3)).astype("int32"))
    assert list(E.fpd_batch_sizes(200, 500, 3))[:2] == [200, 285]
    with pytest.raises(ValueError, match="min_samples <= max_samples"):
        E.fpd_batch_sizes(500, 200, 3)


def test_index_lists_are_the_global_stream():
    sizes = E.fpd_batch_sizes(200, 500, 3)
    got = list(E.fpd_index_lists(3000, 2500, sizes, num_batches=4, seed=42))
    state = np.random.get_state()
    try:
        np.random.seed(42)
        for b, lists in zip(sizes, got):
            assert lists.shape == (4, 2, b)
            for k in range(4):
                assert np.array_equal(lists[k, 0], np.random.choice(3000, size=b))
                assert np.array_equal(lists[k, 1], np.random.choice(2500, size=b))
    finally:
        np.random.set_state(state)
    again = list(E.fpd_index_lists(3000, 2500, sizes, num_batches=4, seed=42))
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    with pytest.raises(ValueError, match="no rows"):
        next(E.fpd_index_lists(0, 5, sizes))


def test_frechet_distance_of_commuting_covariances():
    rng = np.random.default_rng(3)
    d = 40
    a, b = rng.uniform(0.1, 4.0, d), rng.uniform(0.1, 4.0, d)
    b[5] = 0.0  # a rank-deficient covariance
    mu1, mu2 = rng.normal(size=d), rng.normal(size=d)
    want = np.sum((mu1 - mu2) ** 2) + np.sum((np.sqrt(a) - np.sqrt(b)) ** 2)
    scale = np.sum((mu1 - mu2) ** 2) + a.sum() + b.sum()
    got = E.frechet_distance(mu1, np.diag(a), mu2, np.diag(b))
    assert abs(got - want) <= 8 * d * 2.0 ** -53 * scale
    assert abs(E.frechet_distance(mu2, np.diag(b), mu1, np.diag(a)) - want) <= 8 * d * 2.0 ** -53 * scale
    assert abs(E.frechet_distance(mu1, np.diag(a), mu1, np.diag(a))) <= 8 * d * 2.0 ** -53 * 2 * a.sum()
    assert abs(got - F.restate_frechet(mu1, np.diag(a), mu2, np.diag(b))) <= 8 * d * 2.0 ** -53 * scale


def test_frechet_distance_of_general_covariances():
    x, y = F.feature_like(400, 12, 1), F.feature_like(300, 12, 2, shift=0.5)
    m1, s1, m2, s2 = x.mean(0), np.cov(x, rowvar=False), y.mean(0), np.cov(y, rowvar=False)
    v12, v21 = E.frechet_distance(m1, s1, m2, s2), E.frechet_distance(m2, s2, m1, s1)
    scale = np.sum((m1 - m2) ** 2) + np.trace(s1) + np.trace(s2)
    # The two orders go through different eigen-decompositions.  An eigenvalue of R S2 R carries an absolute error of about
    # d 2^-53 |S|^2, and the root of one near 0 turns that into sqrt(d 2^-53) |S|: d of them, d sqrt(d 2^-53) x scale at worst.
    bound = 12 * np.sqrt(12 * 2.0 ** -53) * scale
    assert v12 > 0 and abs(v12 - v21) <= bound
    assert abs(E.frechet_distance(m1, s1, m1, s1)) <= bound
    low = x[:8]  # 8 rows of 12 features: rank 7
    assert np.isfinite(E.frechet_distance(low.mean(0), np.cov(low, rowvar=False), m2, s2))
    with pytest.raises(ValueError, match="do not belong together"):
        E.frechet_distance(m1, s1, m2[:5], s2[:5, :5])


def test_fit_extrapolation():
    sizes = np.array([200, 285, 500])  # M = 3, the smallest case
    a, err = E.fit_extrapolation(sizes, 0.25 + 7.0 / sizes)
    assert abs(a - 0.25) <= 1e-13 and err <= 1e-13
    # a negative unconstrained intercept: clipped to 0, the slope refitted through the origin
    y = -0.01 + 30.0 / sizes
    x = 1.0 / sizes
    a, err = E.fit_extrapolation(sizes, y)
    assert a == 0.0
    slope = (x @ y) / (x @ x)
    rss = np.sum((y - slope * x) ** 2)
    assert abs(err - np.sqrt(rss / 1 * np.linalg.inv(np.stack([np.ones(3), x], 1).T @ np.stack([np.ones(3), x], 1))[0, 0])) <= 1e-12
    assert E.fit_extrapolation(sizes, y) == pytest.approx(F.restate_fit(sizes, y), rel=1e-12, abs=1e-15)
    # a negative slope: b = 0, a = the mean
    a, _ = E.fit_extrapolation(sizes, 0.5 - 9.0 / sizes)
    assert abs(a - np.mean(0.5 - 9.0 / sizes)) <= 1e-15
    noisy = 0.1 + 20.0 / E.fpd_batch_sizes() + np.random.default_rng(0).normal(0, 1e-4, 10)
    assert E.fit_extrapolation(E.fpd_batch_sizes(), noisy) == pytest.approx(F.restate_fit(E.fpd_batch_sizes(), noisy), rel=1e-9)
    with pytest.raises(ValueError, match="at least 3 points"):
        E.fit_extrapolation([200, 500], [1.0, 2.0])


def test_against_scipy():
    linalg, optimize = pytest.importorskip("scipy.linalg"), pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(0)
    d = 226
    A, B = rng.normal(size=(1000, d)), rng.normal(size=(1000, d)) * 1.1
    m1, s1, m2, s2 = A.mean(0), np.cov(A, rowvar=False), B.mean(0), np.cov(B, rowvar=False)
    want = np.sum((m1 - m2) ** 2) + np.trace(s1) + np.trace(s2) - 2 * np.trace(linalg.sqrtm(s1 @ s2).real)
    got = E.frechet_distance(m1, s1, m2, s2)
    print("frechet_distance - sqrtm form:", got - want, "of", want)
    assert abs(got - want) <= F.SQRTM_ATOL
    sizes, y = F.fit_fixture()
    popt, pcov = optimize.curve_fit(lambda n, a, b: a + b / n, sizes.astype(np.float64), y, bounds=([0, 0], [np.inf, np.inf]))
    a, err = E.fit_extrapolation(sizes, y)
    print("fit - curve_fit, relative:", a / popt[0] - 1, err / np.sqrt(pcov[0, 0]) - 1)
    assert abs(a - popt[0]) <= F.CURVE_FIT_RTOL * abs(popt[0]) and abs(err - np.sqrt(pcov[0, 0])) <= F.CURVE_FIT_RTOL * err


def test_restatement_normalises_with_a_zero_column():
    """The zero column stays (no division by 0) in the restatement the device test compares with; the library's own normalisation
    is on the device (test_gpu_fpd.py)."""
    x, y = F.feature_like(300, 4, 1), F.feature_like(300, 4, 2)
    x[:, 2] = 0.0
    sizes = E.fpd_batch_sizes(50, 100, 3)
    lists = list(E.fpd_index_lists(300, 300, sizes, 2, 1))
    value, err = F.restate_fpd(x, y, lists, sizes)
    assert np.isfinite(value) and np.isfinite(err) and value > 0


def test_constructor_and_import_paths(tmp_path):
    from calodiffusion.train.evaluate import FDP, FDPCalculationError
    import calodiffusion.train  # noqa: F401
    assert FDP is E.FDP and FDPCalculationError is E.FDPCalculationError and issubclass(FDPCalculationError, Exception)
    fdp = FDP(H.binning("small"), "electron", min_samples=200, max_samples=500)
    assert fdp.hlf is not fdp.reference_hlf and fdp.hlf.particle == "electron" and fdp.fpd_kwargs == {"min_samples": 200, "max_samples": 500}
    assert fdp.hlf.total_voxels == fdp.reference_hlf.total_voxels > 0


# ---- refusals: CD_EINVAL with a message, before anything touches the device ------------------------------------------------

def _call(lib, **kw):
    """cd_fpd_moments with plausible arguments (the pointers are never followed: every case is refused first)."""
    a = dict(x=0x1000, rows=100, d=20, centre=0x2000, idx=0x3000, idx_stride=64, counts=[64, 32], sets=2, mean=0x4000, cov=0x5000,
             status=0x6000, workspace=0x7000, workspace_bytes=None, stream=None)
    a.update(kw)
    counts = (C.c_int32 * max(len(a["counts"]), 1))(*a["counts"]) if a["counts"] is not None else None
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = lib.cd_fpd_workspace_bytes(20, 2, 64)
    return lib.cd_fpd_moments(a["x"], a["rows"], a["d"], a["centre"], a["idx"], a["idx_stride"], counts, a["sets"], a["mean"], a["cov"],
                              a["status"], a["workspace"], a["workspace_bytes"], a["stream"])


@pytest.mark.parametrize("change, message", [
    (dict(x=None), "must not be null"), (dict(centre=None), "must not be null"), (dict(idx=None), "must not be null"),
    (dict(counts=None), "must not be null"), (dict(mean=None), "must not be null"), (dict(cov=None), "must not be null"),
    (dict(status=None), "must not be null"), (dict(workspace=None), "must not be null"),
    (dict(d=0), r"d must be in \[1, 256\], got 0"), (dict(d=257), r"d must be in \[1, 256\], got 257"),
    (dict(rows=0), "rows must be positive"), (dict(sets=0), "sets must be at least 1"),
    (dict(counts=[64, 1]), r"counts\[1\] = 1, a covariance needs at least 2 rows"),
    (dict(idx_stride=63), "idx_stride 63 is less than the largest count 64"),
    (dict(idx_stride=2 ** 30), "sets \\* idx_stride must be below"),
    (dict(workspace=0x7004), "8-byte aligned"),
    (dict(workspace_bytes=1000), "workspace of 1000 bytes, needs"),
])
def test_refusals(change, message):
    import re
    lib = engine.load_library()
    assert _call(lib, **change) == -1
    assert re.search(message, lib.cd_last_error().decode()), lib.cd_last_error()


def test_workspace_bytes():
    lib = engine.load_library()
    assert lib.cd_fpd_workspace_bytes(226, 40, 50000) == 40 * 25 * (120 * 2048 + 256)  # 15 tiles of 16 columns: 120 tile pairs
    assert lib.cd_fpd_workspace_bytes(1, 1, 2) == 2048 + 256
    assert lib.cd_fpd_workspace_bytes(256, 1, 2049) == 2 * (153 * 2048 + 256)
    for bad in ((0, 1, 2), (257, 1, 2), (20, 0, 2), (20, 1, 1)):
        assert lib.cd_fpd_workspace_bytes(*bad) == 0 and b"cd_fpd_workspace_bytes: needs" in lib.cd_last_error()
    with pytest.raises(ValueError, match="cd_fpd_workspace_bytes: needs"):
        E.moments_workspace_bytes(300, 1, 2)
