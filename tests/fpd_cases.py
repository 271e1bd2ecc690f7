"""Shared by test_fpd_host.py and test_gpu_fpd.py: a plain NumPy float64 restatement of every step of calodiffusion_amd.evaluate.fpd
(taking the SAME index lists as the library draws), the seeded inputs, and the bounds.

Bounds of the device moments (cd_fpd_moments) against the restatement.  With y_k = x[idx_k] - centre, S_i = sum_k y_ki,
G_ij = sum_k y_ki y_kj, a_i = sum_k |y_ki| and A_ij = sum_k |y_ki y_kj|, two float64 sums of the same n terms in different orders
differ by at most n 2^-52 times the sum of the absolute terms:
    |dG_ij| <= n 2^-52 A_ij,      |dS_i| <= n 2^-52 a_i,      mean: |dS_i| / n.
Carried through cov_ij = (G_ij - S_i S_j / n) / (n - 1), plus the formula's own four roundings (product, quotient, difference,
quotient: 4 2^-53 of |G_ij| + |S_i S_j| / n):
    |dcov_ij| <= [n 2^-52 (A_ij + (a_i |S_j| + |S_i| a_j) / n) + 4 2^-53 (|G_ij| + |S_i S_j| / n)] / (n - 1).
On integer data G and S are exact in any order and only the last term remains.

Tolerances that cannot be derived are MEASURED and written here beside ten times their value:
  * frechet_distance against scipy.linalg.sqrtm on the seeded D = 226 pair: 6.8e-13 absolute on a value of 31 (host CPU)
  * fit_extrapolation against scipy.optimize.curve_fit(bounds=([0, 0], [inf, inf])) on fit_fixture(): 9.4e-9 relative in the value
    and 1.0e-8 in its error.  curve_fit iterates from (1, 1) and stops at its own tolerance, so the difference is curve_fit's; the
    closed form agrees with numpy.linalg.lstsq to 1e-12 (test_fit_extrapolation)
  * fpd() on the device against the restatement at the test's sizes: see FPD_END_TO_END_MEASURED
"""
import numpy as np

SQRTM_MEASURED, SQRTM_ATOL = 6.8e-13, 6.8e-12
CURVE_FIT_MEASURED, CURVE_FIT_RTOL = 1.0e-8, 1.0e-7
# |device fpd - restatement|, value and error, at (min 200, max 500, num_batches 4, num_points 3), D = 20, 3000 rows, values 0.007 to
# 0.36 (normalised and not, shift 0 and 0.5), and FDP.__call__ on 26 features: the largest of the eight differences measured on an
# MI355X (the value's own largest: 5.6e-15); the tolerance is ten times it
FPD_END_TO_END_MEASURED, FPD_END_TO_END_ATOL = 2.8e-14, 2.8e-13
# the same with one column zero in both sets (singular covariances: roots of rounding-sized eigenvalues), value about 0.02
FPD_ZERO_COLUMN_MEASURED, FPD_ZERO_COLUMN_ATOL = 1.35e-9, 1.35e-8


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------

def integer_matrix(rows, d, seed):
    """Integer-valued float64 in [-3, 3]: every product and sum of the Gram matrix is exact."""
    return np.random.default_rng(seed).integers(-3, 4, size=(rows, d)).astype(np.float64)


def feature_like(rows, d, seed, shift=0.0, offset=5.0):
    """Columns of scales over three decades, correlated through a random mixing, each away from 0 by up to `offset` of its own
    spreads (as log-energies and centres of energy are); `shift` moves column 0.
    The offset is moderate by default because of the MEAN's bound: mean_i = centre_i + S_i / n ends in a rounding of size
    2^-53 |mean_i| that the bound n 2^-52 a_i / n of the sums does not contain, so the data keep |mean_i| below a_i (from n = 3 on;
    for n = 2 both sides perform the same operations).  Large offsets: `mean_roundings` of assert_moments_within_bounds."""
    rng = np.random.default_rng(seed)
    mix = rng.normal(size=(d, d)) / np.sqrt(d) + np.eye(d)
    x = (rng.normal(size=(rows, d)) @ mix + rng.uniform(-offset, offset, d)) * 10.0 ** rng.uniform(-2.0, 1.0, d)
    x[:, 0] += shift
    return x


def fit_fixture():
    """Ten means as fpd() fits them: 0.28 + 300 / N at the default batch sizes with noise of 2e-3."""
    sizes = (1 / np.linspace(1 / 20000, 1 / 50000, 10)).astype("int32")
    return sizes, 0.28 + 300.0 / sizes + np.random.default_rng(1).normal(0.0, 2e-3, 10)


def draws(rows, counts, seed):
    """Index lists drawn with replacement."""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, rows, size=n).astype(np.int32) for n in counts]


# ---- the moments -----------------------------------------------------------------------------------------------------------

def restate_sums(x, centre, l):
    """S, G and their absolute counterparts a, A of one index list."""
    y = x[np.asarray(l)] - centre
    return y.sum(axis=0), y.T @ y, np.abs(y).sum(axis=0), np.abs(y).T @ np.abs(y)


def restate_moments(x, centre, l):
    """mean and cov in the kernel's one-pass form, in float64."""
    n = len(l)
    S, G, _, _ = restate_sums(x, centre, l)
    return centre + S / n, (G - np.outer(S, S) / n) / (n - 1)


def moment_bounds(x, centre, l, exact_sums=False):
    """(bound of the mean, bound of the cov) as derived in the module docstring."""
    n = len(l)
    S, G, a, A = restate_sums(x, centre, l)
    formula = 4 * 2.0 ** -53 * (np.abs(G) + np.abs(np.outer(S, S)) / n)
    if exact_sums:
        return np.zeros_like(S), formula / (n - 1)
    order = n * 2.0 ** -52 * (A + (np.outer(a, np.abs(S)) + np.outer(np.abs(S), a)) / n)
    return n * 2.0 ** -52 * a / n, (order + formula) / (n - 1)


def assert_moments_within_bounds(mean, cov, x, centre, lists, want=None, exact_sums=False, mean_roundings=False):
    """Device moments of every list against the restatement (or `want(l)` -> (mean, cov)); returns the worst share of the bound.
    mean_roundings: add the two roundings that end mean_i = centre_i + S_i / n, 2 x 2^-53 |mean_i|, to the mean's bound (for data
    far from 0, where they exceed the bound of the sums)."""
    worst = 0.0
    for s, l in enumerate(lists):
        m_want, c_want = restate_moments(x, centre, l) if want is None else want(l)
        m_bound, c_bound = moment_bounds(x, centre, l, exact_sums)
        if mean_roundings:
            m_bound = m_bound + 2 * 2.0 ** -53 * np.abs(m_want)
        m_err, c_err = np.abs(mean[s] - m_want), np.abs(cov[s] - c_want)
        if exact_sums:
            assert np.array_equal(mean[s], m_want), (s, float(m_err.max()))
        assert np.all(m_err <= m_bound), (s, "mean", float(m_err.max()), float(m_bound.max()))
        assert np.all(c_err <= c_bound), (s, "cov", float(c_err.max()), float(c_bound.max()), np.argwhere(c_err > c_bound)[:8].tolist())
        assert np.array_equal(cov[s], cov[s].T), (s, "cov is not bitwise symmetric")
        worst = max(worst, float(np.max(c_err / np.maximum(c_bound, 1e-300))))
    return worst


# ---- the distance, the fit and the whole metric ----------------------------------------------------------------------------

def restate_frechet(mu1, s1, mu2, s2):
    w, v = np.linalg.eigh(s1)
    root = v @ np.diag(np.sqrt(np.clip(w, 0.0, None))) @ v.T
    m = root @ s2 @ root
    lam = np.linalg.eigvalsh(0.5 * (m + m.T))
    return float(np.sum((mu1 - mu2) ** 2) + np.trace(s1) + np.trace(s2) - 2.0 * np.sum(np.sqrt(np.clip(lam, 0.0, None))))


def restate_fit(sizes, values):
    """a + b / N with a, b >= 0 by least squares: the candidates written out, the best feasible one taken."""
    x, y = 1.0 / np.asarray(sizes, dtype=np.float64), np.asarray(values, dtype=np.float64)
    A = np.stack([np.ones_like(x), x], axis=1)
    rss = lambda p: float(np.sum((y - A @ p) ** 2))  # noqa: E731
    free = np.linalg.lstsq(A, y, rcond=None)[0]
    if free[0] >= 0.0 and free[1] >= 0.0:
        best = free
    else:
        cands = [np.array([0.0, max(float(x @ y / (x @ x)), 0.0)]), np.array([max(float(y.mean()), 0.0), 0.0]), np.zeros(2)]
        best = min(cands, key=rss)
    cov = rss(best) / (len(x) - 2) * np.linalg.inv(A.T @ A)
    return float(best[0]), float(np.sqrt(cov[0, 0]))


def restate_fpd(real, gen, index_lists, sizes, normalise=True):
    """fpd() on the host from the same draws: index_lists[p][k, 0] / [k, 1] are the rows of pair k of size p."""
    X, Y = np.array(real, dtype=np.float64), np.array(gen, dtype=np.float64)
    if normalise:
        m = np.abs(X).max(axis=0)
        m[m == 0] = 1.0
        X, Y = X / m, Y / m
    values = []
    for lists in index_lists:
        vals = []
        for k in range(lists.shape[0]):
            a, b = X[lists[k, 0]], Y[lists[k, 1]]
            vals.append(restate_frechet(a.mean(axis=0), np.cov(a, rowvar=False), b.mean(axis=0), np.cov(b, rowvar=False)))
        values.append(np.mean(vals))
    return restate_fit(sizes, values)
