"""Shared by test_kpd_host.py and test_gpu_kpd.py: a plain NumPy float64 restatement of calodiffusion_amd.evaluate.kpd and
separation_powers (taking the SAME index lists as the library draws), and the bounds.  The seeded inputs are fpd_cases.py's.

Bound of a device kernel sum (cd_kpd_sums) against the restatement, u = 2^-53.  Write b_ij = sum_k |x_ik| |y_jk| and
a_ij = gamma b_ij + 1 >= |gamma x_i.y_j + 1|.
  * the dot product g_ij of d terms: two float64 sums of the same d terms in different orders (the device: the matrix
    instruction, four columns a step; the restatement: BLAS) differ by at most d 2^-52 b_ij, as in fpd_cases.py;
  * one multiply-add by gamma and 1: a fused one on the device (one rounding), a product and a sum in the restatement (two):
    3 u a_ij;
  * so the base of the power differs by at most e_ij a_ij with e_ij = 2 d u gamma b_ij / a_ij + 3 u <= (2 d + 3) u;
  * degree - 1 multiplies on either side, each one rounding relative to the running product, itself at most a_ij^degree:
    2 (degree - 1) u a_ij^degree; and the base's error enters `degree` times: degree (2 d + 3) u a_ij^degree (first order; the
    second-order terms are below u times that and are covered by the factor 1 + 2^-20 on the whole bound);
  * the sum over the region: every term passes through at most DEPTH additions on the device -- 15 in its lane (16 elements of a
    64 x 64 block), 6 in the wave's butterfly, 3 over the block's four waves, then ceil(blocks / 256) - 1 in the thread that adds
    the partials t, t + 256, ... and 8 in the final tree -- DEPTH u times the sum of the absolute terms, which the weighted sum of
    a_ij^degree bounds.  The restatement adds with math.fsum, correctly rounded: one u of the same sum.  A weight of 2 is exact.
Together, with T_ij = a_ij^degree and the region's weights w_ij (1 per counted ordered pair):
    |d sum| <= (1 + 2^-20) u [degree (2 d + 3) + 2 (degree - 1) + DEPTH + 1] sum_ij w_ij T_ij.
(The bound uses (2 d + 3) for every element; the sharper e_ij would only lower it.)

mmd = xx / (m (m - 1)) + yy / (n (n - 1)) - 2 (xy / (m n)): the sums' bounds divided likewise, plus the formula's own roundings,
one per operation (three quotients, a product with 2 that is exact, two additions) relative to at most the sum of the absolute
terms: 6 u (|xx| / (m (m - 1)) + |yy| / (n (n - 1)) + 2 |xy| / (m n)), on either side alike -- it enters only where the sums differ,
but is kept as slack of a few u.  Median and percentiles are order statistics and their linear interpolations: they move by no
more than the largest change of any mmd_i, plus 4 u max |mmd_i| for the interpolation's own arithmetic; the error, half the
difference of two percentiles, likewise.
"""
import math

import numpy as np

U = 2.0 ** -53
BLOCK = 64  # CD_KPD_BLOCK


# ---- the kernel sums -------------------------------------------------------------------------------------------------------

def _power(base, degree):
    k = base
    for _ in range(degree - 1):
        k = k * base
    return k


def _off_diagonal_sum(k):
    """math.fsum over the entries at different positions."""
    return math.fsum(k[~np.eye(k.shape[0], dtype=bool)].tolist())


def restate_sums(x, lx, ly, gamma, degree):
    """{sum XX off the diagonal of positions, sum YY likewise, sum XY} of one batch, each correctly rounded."""
    X, Y = x[np.asarray(lx)], x[np.asarray(ly)]
    xx, yy, xy = (_power(a @ b.T * gamma + 1.0, degree) for a, b in ((X, X), (Y, Y), (X, Y)))
    return np.array([_off_diagonal_sum(xx), _off_diagonal_sum(yy), math.fsum(xy.ravel().tolist())])


def brute_force_sums(x, lx, ly, gamma, degree):
    """The same by a double loop over positions, for small cases."""
    def k(a, b):
        return (float(np.dot(a, b)) * gamma + 1.0) ** degree
    xx = sum(k(x[lx[i]], x[lx[j]]) for i in range(len(lx)) for j in range(len(lx)) if i != j)
    yy = sum(k(x[ly[i]], x[ly[j]]) for i in range(len(ly)) for j in range(len(ly)) if i != j)
    xy = sum(k(x[lx[i]], x[ly[j]]) for i in range(len(lx)) for j in range(len(ly)))
    return np.array([xx, yy, xy])


def device_depth(m, n):
    """Additions a term passes through on the device, at most (module docstring)."""
    nb = -(-(m + n) // BLOCK)
    blocks = nb * (nb + 1) // 2
    return 15 + 6 + 3 + (-(-blocks // 256) - 1) + 8


def sum_bounds(x, lx, ly, gamma, degree):
    """The bound of each of the three sums (module docstring)."""
    X, Y = np.abs(x[np.asarray(lx)]), np.abs(x[np.asarray(ly)])
    d = x.shape[1]
    per_term = degree * (2 * d + 3) + 2 * (degree - 1) + device_depth(len(lx), len(ly)) + 1
    out = []
    for a, b, off in ((X, X, True), (Y, Y, True), (X, Y, False)):
        T = _power(a @ b.T * abs(gamma) + 1.0, degree)
        total = float(T.sum() - np.trace(T)) if off else float(T.sum())
        out.append((1 + 2.0 ** -20) * U * per_term * total * (1 + 2.0 ** -20))  # the second factor: T.sum() is itself rounded
    return np.array(out)


def restate_mmd(sums, m, n):
    xx, yy, xy = (float(v) for v in sums)
    return xx / (m * (m - 1)) + yy / (n * (n - 1)) - 2.0 * (xy / (m * n))


def mmd_bound(sums, bounds, m, n):
    scale = abs(sums[0]) / (m * (m - 1)) + abs(sums[1]) / (n * (n - 1)) + 2 * abs(sums[2]) / (m * n)
    return float(bounds[0] / (m * (m - 1)) + bounds[1] / (n * (n - 1)) + 2 * bounds[2] / (m * n) + 6 * U * scale)


def _normalised(real, gen, normalise):
    X, Y = np.array(real, dtype=np.float64), np.array(gen, dtype=np.float64)
    if normalise:
        m = np.abs(X).max(axis=0)
        m[m == 0] = 1.0
        X, Y = X / m, Y / m
    return X, Y


def restate_kpd(real, gen, lists, normalise=True, degree=4, with_bound=False):
    """kpd() on the host from the same draws: lists[i, 0] / [i, 1] are the rows of batch i.  -> (value, error), and with
    `with_bound` the bound of either against a device result (module docstring)."""
    X, Y = _normalised(real, gen, normalise)
    Z, gamma = np.concatenate([X, Y]), 1.0 / X.shape[1]
    mmds, bounds = [], []
    for i in range(lists.shape[0]):
        lx, ly = lists[i, 0], lists[i, 1] + len(X)
        sums = restate_sums(Z, lx, ly, gamma, degree)
        mmds.append(restate_mmd(sums, len(lx), len(ly)))
        if with_bound:
            bounds.append(mmd_bound(sums, sum_bounds(Z, lx, ly, gamma, degree), len(lx), len(ly)))
    value = float(np.median(mmds))
    error = float((np.percentile(mmds, 83.725) - np.percentile(mmds, 16.275)) / 2)
    if with_bound:
        return value, error, max(bounds) + 4 * U * max(abs(v) for v in mmds)
    return value, error


# ---- histograms and separation powers ---------------------------------------------------------------------------------------

def restate_edges(real, bins=50):
    return np.stack([np.linspace(real[:, j].min(), real[:, j].max(), bins) for j in range(real.shape[1])])


def restate_histograms(values, edges):
    """np.histogram per column on the given edges: (d, nedges - 1) int64."""
    return np.stack([np.histogram(values[:, j], bins=edges[j])[0] for j in range(values.shape[1])]).astype(np.int64)


def restate_separation(real_counts, gen_counts):
    """The reference's formula column by column (utils._separation_power on p = counts / counts.sum())."""
    out = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for c1, c2 in zip(np.asarray(real_counts, dtype=np.float64), np.asarray(gen_counts, dtype=np.float64)):
            p, q = c1 / c1.sum(), c2 / c2.sum()
            out.append(0.5 * float(np.sum((p - q) ** 2 / (p + q + 1e-16))))
    return np.array(out)


def restate_separation_powers(real, gen, bins=50):
    """separation_powers() on the host; a column whose real values are all equal is nan (the reference's density divides by a
    bin width of 0)."""
    real, gen = np.asarray(real, dtype=np.float64), np.asarray(gen, dtype=np.float64)
    edges = restate_edges(real, bins)
    sep = restate_separation(restate_histograms(real, edges), restate_histograms(gen, edges))
    sep[edges[:, 0] == edges[:, -1]] = np.nan
    return sep


def reference_arithmetic(real_col, gen_col, bins=50):
    """One column exactly as the reference computes it: density=True histograms, then utils._separation_power."""
    edges = np.linspace(real_col.min(), real_col.max(), bins)
    with np.errstate(invalid="ignore", divide="ignore"):
        h1, h2 = np.histogram(real_col, bins=edges, density=True)[0], np.histogram(gen_col, bins=edges, density=True)[0]
        p, q = h1 * np.diff(edges), h2 * np.diff(edges)
        return 0.5 * float(np.sum((p - q) ** 2 / (p + q + 1e-16)))
