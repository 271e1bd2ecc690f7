"""The reference's evaluation metric (calodiffusion/train/evaluate.py:21-79): ``FDP``, the Frechet physics distance between generated
and Geant4 showers in the space of the CaloChallenge observables -- the objective of the reference's Optuna search and the figure
its validation quotes.  The reference hands ``HighLevelFeatures``' arrays to ``jetnet.evaluation.fpd``; this package does not
depend on jetnet, so ``fpd`` is defined here, after Kansal et al., Phys. Rev. D 107, 076017, with the signature and defaults
jetnet documents:

  1. ``normalise``: both arrays are divided by the per-column ``max|real_features|`` (a column whose maximum is 0 stays);
  2. batch sizes ``(1 / linspace(1 / min_samples, 1 / max_samples, num_points)).astype(int32)``;
  3. per batch size, ``num_batches`` times: ``rs.choice(len(X), size=b)`` then ``rs.choice(len(Y), size=b)`` of
     ``rs = np.random.RandomState(seed)`` (the stream of ``np.random.seed(seed)`` and the global ``np.random.choice``);
  4. per pair the Frechet distance of the two Gaussians, ``|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2)``, averaged per size;
  5. a least-squares fit of ``a + b / N`` with ``a, b >= 0`` to those means; the result is ``(a, its standard error)``.

Step 3's 400 means and covariances of up to 50 000 gathered rows are the expensive part and run on the device
(``cd_fpd_moments``, include/calodiff.h: the Gram matrices on the fp64 matrix instruction): both arrays are uploaded once, as one
matrix, the draws stay on the host and their index lists go up one batch size at a time, ``2 num_batches`` sets a call.  Steps 4
and 5 are NumPy on the host (two symmetric eigen-decompositions per pair; no SciPy).  There is no host fallback for step 3.

The reference's metrics program (calodiffusion/tests/hgcal_metrics.py:401-432) scores the same feature matrix two more ways, and
both are here: ``jetnet.evaluation.kpd`` and a separation power per feature column.

``kpd(real_features, gen_features, num_batches=10, batch_size=5000, normalise=True, seed=42)`` -> ``(value, error)``, the kernel
physics distance.  This is a RESTATEMENT of jetnet's ``evaluation/gen_metrics.py`` and of Kansal et al., Phys. Rev. D 107, 076017,
written down without jetnet at hand; it is not a run of jetnet and has not been compared with one:

  1. ``normalise`` as for ``fpd`` (the same code);
  2. for batch i = 0 ... num_batches - 1: m = ``batch_size`` real row indices, then m generated ones, with replacement;
     X = real[idx1], Y = gen[idx2];
     ``mmd_i = (sum XX - tr XX) / (m (m - 1)) + (sum YY - tr YY) / (m (m - 1)) - 2 mean(XY)`` with ``XX = (X X^T gamma + 1)^4``,
     likewise YY and XY, gamma = 1 / d.  "tr" removes the entries at equal POSITIONS i = j of the list; two different positions
     that drew the same row are an ordinary off-diagonal pair and are counted;
  3. ``value = median(mmd)``;
  4. ``error = (percentile(mmd, 83.725) - percentile(mmd, 16.275)) / 2``, NumPy's default linear interpolation.

The draws (``kpd_index_lists``): per batch ``rs = np.random.RandomState(seed + 1000 * i)``, ``rs.choice(n_real, size=m)``, then
``rs.choice(n_gen, size=m)``.  jetnet seeds per batch with ``seed + 1000 i`` too but draws inside numba-compiled code, whose
generator stream is not promised to equal NumPy's: the index lists here are NOT claimed to equal jetnet's, and values agree with
jetnet's only within the metric's own error.  Everything downstream takes index lists as input.
The three kernel sums of a batch run on the device (``cd_kpd_sums``: Gram blocks on the fp64 matrix instruction, the 5000 x 5000
kernel matrices never formed); the division and the subtraction of step 2 and steps 3 and 4 are float64 Python on the host.

``separation_powers(real_features, gen_features, bins=50)`` -> ``(d,)`` float64, per column j the triangular discrimination of the
two histograms (``utils._separation_power``, utils/utils.py:167-175, over ``make_hist``'s defaults):
``edges = np.linspace(min(real[:, j]), max(real[:, j]), bins)`` (``bins - 1`` bins); counts as ``np.histogram`` (values outside
``[edges[0], edges[-1]]`` dropped, every bin ``[lo, hi)`` but the last, which is closed on the right); ``p = counts / counts.sum()`` per
set (``density=True`` times the bin widths); ``sep = 0.5 sum (p - q)^2 / (p + q + 1e-16)``.  A column whose real values are all equal
gives ``nan``, as the reference's own arithmetic does (its density is a division by a bin width of 0, then 0 / 0); so does a column
with no generated value inside the real range.  The column minima and maxima come from the device, the edges are made on the host
with ``np.linspace``, and the counts are one pass of ``cd_column_histograms`` per set.  ``separation_power_total`` is the plain sum
over the columns, the reference's ``TOTAL``.

Not provided: ``ComparisonNetwork`` and ``CNNCompare`` of the same reference module (a torchvision ResNet, not a dependency of
this package).
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np
import torch

from .abi import WorkspaceCache, _check, _stream, _upload, load_library, require_gpu
from .hlf import HighLevelFeatures

MAX_FEATURES = 256  # CD_FPD_MAX_D


class FDPCalculationError(Exception):
    def __init__(self, *args):
        super().__init__(*args)


# ---- step 2 and 3: the draws (host) ---------------------------------------------------------------------------------------

def fpd_batch_sizes(min_samples=20_000, max_samples=50_000, num_points=10):
    """The bootstrap sample sizes: equally spaced in 1 / N between ``min_samples`` and ``max_samples``."""
    if not (int(num_points) >= 1 and 2 <= int(min_samples) <= int(max_samples)):
        raise ValueError(f"fpd: needs 2 <= min_samples <= max_samples and num_points >= 1, got {min_samples}, {max_samples}, {num_points}")
    return (1 / np.linspace(1 / min_samples, 1 / max_samples, num_points)).astype("int32")


def fpd_index_lists(n_real, n_gen, batch_sizes, num_batches=20, seed=42):
    """Yields, per batch size in order, the int64 array (num_batches, 2, b) of row indices: [k, 0] into the real and [k, 1] into
    the generated features, drawn with replacement in the order ``fpd`` documents."""
    if n_real < 1 or n_gen < 1:
        raise ValueError(f"fpd: an array has no rows ({n_real} and {n_gen})")
    rs = np.random.RandomState(seed)
    for b in batch_sizes:
        out = np.empty((num_batches, 2, int(b)), dtype=np.int64)
        for k in range(num_batches):
            out[k, 0] = rs.choice(n_real, size=int(b))
            out[k, 1] = rs.choice(n_gen, size=int(b))
        yield out


# ---- step 3: the moments (device) -----------------------------------------------------------------------------------------

_workspaces = WorkspaceCache()  # kind: the device index; grown on demand


def _workspace(device, nbytes):
    return _workspaces.get(device.index, (), device, nbytes)


def moments_workspace_bytes(d, sets, max_count):
    nbytes = load_library().cd_fpd_workspace_bytes(int(d), int(sets), int(max_count))
    if nbytes == 0:
        _check(-1)
    return nbytes


def launch_moments(x, centre, idx, counts, mean, cov, status, workspace=None):
    """One ``cd_fpd_moments`` call on the current stream, nothing allocated (unless ``workspace`` is None), nothing
    synchronised.  x (rows, d) float64, centre (d,) float64, idx (sets, idx_stride) int32, mean (sets, d), cov (sets, d, d)
    float64 and status (1,) int32: contiguous tensors on one device; counts: a sequence of ``sets`` ints (host)."""
    lib = load_library()
    sets, d = idx.shape[0], x.shape[1]
    for t, dt, name in ((x, torch.float64, "x"), (centre, torch.float64, "centre"), (idx, torch.int32, "idx"), (mean, torch.float64, "mean"),
                        (cov, torch.float64, "cov"), (status, torch.int32, "status")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt and t.is_contiguous()):
            raise ValueError(f"launch_moments: {name} must be a contiguous {dt} CUDA tensor")
    if len(counts) != sets or centre.numel() != d or mean.numel() != sets * d or cov.numel() != sets * d * d or status.numel() < 1:
        raise ValueError(f"launch_moments: shapes do not match {sets} sets of {d} features")
    c_counts = (C.c_int32 * sets)(*[int(c) for c in counts])
    with torch.cuda.device(x.device):
        if workspace is None:
            workspace = _workspace(x.device, moments_workspace_bytes(d, sets, max(c_counts)))
        _check(lib.cd_fpd_moments(x.data_ptr(), x.shape[0], d, centre.data_ptr(), idx.data_ptr(), idx.shape[1], c_counts, sets,
                                  mean.data_ptr(), cov.data_ptr(), status.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                  _stream()))


def _feature_rows(a, name):
    """A float64 (rows, d) tensor on the device: a CUDA tensor is cast where it is, anything else is uploaded."""
    if not (isinstance(a, torch.Tensor) and a.is_cuda):
        require_gpu()
        if not isinstance(a, torch.Tensor):
            a = np.asarray(a, dtype=np.float64)  # (an object array of numbers is taken, as NumPy converts it)
    t = _upload(a, torch.float64, name, keep_device=True)
    if t.dim() != 2:
        raise ValueError(f"{name}: expected a (rows, features) array, got shape {tuple(t.shape)}")
    return t


def _pack_lists(index_lists, who="bootstrap_moments", least="a covariance needs at least 2 rows"):
    counts = [len(l) for l in index_lists]
    if not counts:
        raise ValueError(f"{who}: no index lists")
    idx = np.zeros((len(counts), max(max(counts), 1)), dtype=np.int32)
    for s, l in enumerate(index_lists):
        l = np.asarray(l)
        if l.ndim != 1 or l.size < 2:
            raise ValueError(f"{who}: set {s} holds {l.size} rows, {least}")
        if l.size and (l.min() < -2 ** 31 or l.max() >= 2 ** 31):
            raise ValueError(f"{who}: set {s} holds an index beyond int32")
        idx[s, :len(l)] = l
    return idx, counts


def _raise_on_status(status, stride, rows, who="bootstrap_moments"):
    word = int(status.item())
    if word:
        s, k = divmod(word - 1, stride)
        raise ValueError(f"{who}: set {s}, position {k} holds a row index outside [0, {rows})")


def bootstrap_moments(x, index_lists, centre=None):
    """np.mean(x[l], axis=0) and np.cov(x[l], rowvar=False) for every index list l, on the device: (sets, d) and (sets, d, d)
    float64 NumPy arrays.  ``x``: (rows, d), NumPy or CUDA tensor, cast to float64; lists may differ in length (at least 2
    entries each, duplicates allowed); ``centre`` (d,): the shift applied before the sums (default: the column mean of x).
    Raises ``ValueError`` naming the set and position of a row index outside x."""
    x = _feature_rows(x, "x")
    idx, counts = _pack_lists(index_lists)
    with torch.cuda.device(x.device):
        centre = x.mean(dim=0) if centre is None else _feature_rows(np.asarray(centre).reshape(1, -1), "centre").reshape(-1)
        idx_d = torch.from_numpy(idx).to(x.device)
        sets, d = idx.shape[0], x.shape[1]
        mean = torch.empty((sets, d), dtype=torch.float64, device=x.device)
        cov = torch.empty((sets, d, d), dtype=torch.float64, device=x.device)
        status = torch.zeros((1,), dtype=torch.int32, device=x.device)
        launch_moments(x, centre.contiguous(), idx_d, counts, mean, cov, status)
        _raise_on_status(status, idx.shape[1], x.shape[0])
        return mean.cpu().numpy(), cov.cpu().numpy()


# ---- step 4 and 5 (host) ---------------------------------------------------------------------------------------------------

def frechet_distance(mu1, sigma1, mu2, sigma2):
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2).  The last trace is the sum of the roots of the eigenvalues of
    R S2 R (symmetrised, negative ones clipped), R = S1^(1/2) from the eigen-decomposition of S1 with its eigenvalues clipped
    at 0: the same spectrum as S1 S2, through symmetric matrices only."""
    mu1, mu2 = np.asarray(mu1, dtype=np.float64), np.asarray(mu2, dtype=np.float64)
    s1, s2 = np.atleast_2d(np.asarray(sigma1, dtype=np.float64)), np.atleast_2d(np.asarray(sigma2, dtype=np.float64))
    if mu1.shape != mu2.shape or s1.shape != s2.shape or s1.shape != (mu1.size, mu1.size):
        raise ValueError(f"frechet_distance: shapes {mu1.shape}, {s1.shape}, {mu2.shape}, {s2.shape} do not belong together")
    w, v = np.linalg.eigh(s1)
    root = (v * np.sqrt(np.maximum(w, 0.0))) @ v.T
    m = root @ s2 @ root
    lam = np.linalg.eigvalsh((m + m.T) / 2)
    diff = mu1 - mu2
    return float(diff @ diff + np.trace(s1) + np.trace(s2) - 2.0 * np.sqrt(np.maximum(lam, 0.0)).sum())


def fit_extrapolation(batch_sizes, values):
    """Least squares of ``a + b / N`` with a >= 0 and b >= 0 -> (a, error of a).  The unconstrained solution where it is
    feasible, else the best of the edges a = 0 and b = 0 and the origin; error = sqrt(cov[0, 0]), cov = RSS / (M - 2) (A^T A)^-1
    with A = [1, 1 / N]."""
    x, y = 1.0 / np.asarray(batch_sizes, dtype=np.float64), np.asarray(values, dtype=np.float64)
    M = x.size
    if M < 3 or y.shape != x.shape:
        raise ValueError(f"fit_extrapolation: needs at least 3 points and as many values, got {M} and {y.size}")
    xm, ym = x.mean(), y.mean()
    sxx = ((x - xm) ** 2).sum()
    if not sxx > 0.0:
        raise ValueError("fit_extrapolation: all batch sizes are equal")
    b = ((x - xm) * (y - ym)).sum() / sxx
    a = ym - b * xm
    rss = lambda a, b: float(((y - a - b * x) ** 2).sum())  # noqa: E731
    if a < 0.0 or b < 0.0:
        edges = [(0.0, max(float((x * y).sum() / (x * x).sum()), 0.0)), (max(float(ym), 0.0), 0.0), (0.0, 0.0)]
        a, b = min(edges, key=lambda ab: rss(*ab))
    var_a = rss(a, b) / (M - 2) * (1.0 / M + xm * xm / sxx)  # (A^T A)^-1 [0, 0] = sum x^2 / (M sxx)
    return float(a), float(np.sqrt(var_a))


def _normalise(X, Y):
    """Both arrays divided by the per-column max|X|; a column whose maximum is 0 stays as it is."""
    m = X.abs().amax(dim=0)
    m = torch.where(m == 0, torch.ones_like(m), m)
    return X / m, Y / m


def fpd(real_features, gen_features, min_samples=20_000, max_samples=50_000, num_batches=20, num_points=10, normalise=True, seed=42):
    """The Frechet physics distance of two feature arrays (rows, d), extrapolated to infinite sample size: (value, error).
    NumPy arrays or CUDA tensors, cast to float64; see the module docstring for the definition."""
    X, Y = _feature_rows(real_features, "real_features"), _feature_rows(gen_features, "gen_features")
    if X.shape[1] != Y.shape[1]:
        raise ValueError(f"fpd: {X.shape[1]} real and {Y.shape[1]} generated features")
    if not 1 <= X.shape[1] <= MAX_FEATURES:
        raise ValueError(f"fpd: {X.shape[1]} features, the device kernel takes 1 to {MAX_FEATURES}")
    sizes = fpd_batch_sizes(min_samples, max_samples, num_points)
    if int(num_batches) < 1:
        raise ValueError(f"fpd: num_batches must be positive, got {num_batches}")
    for t, name in ((X, "real_features"), (Y, "gen_features")):
        if t.shape[0] == 0:
            raise ValueError(f"fpd: {name} has no rows")
        if t.shape[0] < min_samples:
            warnings.warn(f"fpd: {name} has {t.shape[0]} rows, fewer than min_samples = {min_samples}: the bootstrap draws with "
                          "replacement from too small a set and the result is unreliable", RuntimeWarning, stacklevel=2)
    with torch.cuda.device(X.device):
        Y = Y.to(X.device)
        if normalise:
            X, Y = _normalise(X, Y)
        n_real, d = X.shape
        Z = torch.cat([X, Y])  # one matrix: set 2 k of a call indexes the real rows, set 2 k + 1 the generated ones
        del X, Y
        centre = Z.mean(dim=0)
        status = torch.zeros((1,), dtype=torch.int32, device=Z.device)
        pending = []
        for b, lists in zip(sizes, fpd_index_lists(n_real, Z.shape[0] - n_real, sizes, num_batches, seed)):
            lists[:, 1] += n_real
            idx = torch.from_numpy(lists.reshape(2 * num_batches, int(b)).astype(np.int32)).to(Z.device)
            mean = torch.empty((2 * num_batches, d), dtype=torch.float64, device=Z.device)
            cov = torch.empty((2 * num_batches, d, d), dtype=torch.float64, device=Z.device)
            launch_moments(Z, centre, idx, [int(b)] * (2 * num_batches), mean, cov, status)
            pending.append((idx, mean, cov))
        values = []
        for idx, mean, cov in pending:  # the host's eigen-decompositions of one size run beside the device's later sizes
            mu, sigma = mean.cpu().numpy(), cov.cpu().numpy()
            values.append(np.mean([frechet_distance(mu[2 * k], sigma[2 * k], mu[2 * k + 1], sigma[2 * k + 1]) for k in range(num_batches)]))
    return fit_extrapolation(sizes, values)


# ---- kernel physics distance -----------------------------------------------------------------------------------------------

KPD_DEGREE = 4  # the polynomial kernel of jetnet's kpd; gamma = 1 / d


def kpd_index_lists(n_real, n_gen, num_batches=10, batch_size=5000, seed=42):
    """The int64 array (num_batches, 2, batch_size) of row indices: [i, 0] into the real and [i, 1] into the generated features of
    batch i, drawn with replacement from ``np.random.RandomState(seed + 1000 * i)``, real first.  jetnet seeds its batches the same
    way but draws inside numba-compiled code, whose stream is not promised to equal NumPy's: these lists are this package's
    definition, not jetnet's lists."""
    if n_real < 1 or n_gen < 1:
        raise ValueError(f"kpd: an array has no rows ({n_real} and {n_gen})")
    if int(num_batches) < 1:
        raise ValueError(f"kpd: num_batches must be positive, got {num_batches}")
    if int(batch_size) < 2:
        raise ValueError(f"kpd: batch_size must be at least 2, got {batch_size}")
    out = np.empty((int(num_batches), 2, int(batch_size)), dtype=np.int64)
    for i in range(int(num_batches)):
        rs = np.random.RandomState(seed + 1000 * i)
        out[i, 0] = rs.choice(n_real, size=int(batch_size))
        out[i, 1] = rs.choice(n_gen, size=int(batch_size))
    return out


def kpd_workspace_bytes(sets, max_count):
    nbytes = load_library().cd_kpd_workspace_bytes(int(sets), int(max_count))
    if nbytes == 0:
        _check(-1)
    return nbytes


def launch_kpd_sums(x, idx, counts, gamma, degree, sums, status, workspace=None):
    """One ``cd_kpd_sums`` call on the current stream, nothing allocated (unless ``workspace`` is None), nothing synchronised.
    x (rows, d) float64, idx (sets, idx_stride) int32, sums (sets / 2, 3) float64 and status (1,) int32: contiguous tensors on
    one device; counts: a sequence of ``sets`` ints (host); set 2 k lists the real and set 2 k + 1 the generated rows of batch k."""
    lib = load_library()
    sets, d = idx.shape[0], x.shape[1]
    for t, dt, name in ((x, torch.float64, "x"), (idx, torch.int32, "idx"), (sums, torch.float64, "sums"), (status, torch.int32, "status")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt and t.is_contiguous()):
            raise ValueError(f"launch_kpd_sums: {name} must be a contiguous {dt} CUDA tensor")
    if len(counts) != sets or sets % 2 or sums.numel() != sets // 2 * 3 or status.numel() < 1:
        raise ValueError(f"launch_kpd_sums: shapes do not match {sets} sets (an even number) of {d} features")
    c_counts = (C.c_int32 * sets)(*[int(c) for c in counts])
    with torch.cuda.device(x.device):
        if workspace is None:
            workspace = _workspace(x.device, kpd_workspace_bytes(sets, max(c_counts)))
        _check(lib.cd_kpd_sums(x.data_ptr(), x.shape[0], d, idx.data_ptr(), idx.shape[1], c_counts, sets, float(gamma), int(degree),
                               sums.data_ptr(), status.data_ptr(), workspace.data_ptr(), workspace.numel(), _stream()))


def kernel_sums(x, index_lists, gamma=None, degree=KPD_DEGREE):
    """For every pair of index lists (2 k: rows X, 2 k + 1: rows Y of ``x``) the three sums of the kernel
    ``(gamma a.b + 1)^degree``: over the ordered pairs of different positions of X, of Y, and over all pairs of one position of
    X and one of Y -- a (pairs, 3) float64 NumPy array, computed on the device.  ``gamma`` defaults to 1 / d.  Lists may differ in
    length (at least 2 entries each, duplicates allowed).  Raises ``ValueError`` naming the set and position of a row index outside x."""
    x = _feature_rows(x, "x")
    idx, counts = _pack_lists(index_lists, "kpd", "a kernel sum needs at least 2 rows")
    if len(counts) % 2:
        raise ValueError(f"kpd: {len(counts)} index lists, they come in pairs (real, generated)")
    with torch.cuda.device(x.device):
        sums = torch.empty((len(counts) // 2, 3), dtype=torch.float64, device=x.device)
        status = torch.zeros((1,), dtype=torch.int32, device=x.device)
        launch_kpd_sums(x, torch.from_numpy(idx).to(x.device), counts, 1.0 / x.shape[1] if gamma is None else gamma, degree, sums, status)
        _raise_on_status(status, idx.shape[1], x.shape[0], "kpd")
        return sums.cpu().numpy()


def mmd_from_sums(sums, m, n=None):
    """Step 2's estimate from the three sums of one batch of m real and n (default m) generated rows:
    ``xx / (m (m - 1)) + yy / (n (n - 1)) - 2 (xy / (m n))``, in float64 Python."""
    n = m if n is None else n
    xx, yy, xy = (float(v) for v in sums)
    return xx / (m * (m - 1)) + yy / (n * (n - 1)) - 2.0 * (xy / (m * n))


def median_and_error(mmds):
    """Steps 3 and 4: (median, half the width of the central 67.45 % interval) of the batches' estimates."""
    mmds = np.asarray(mmds, dtype=np.float64)
    return float(np.median(mmds)), float((np.percentile(mmds, 83.725) - np.percentile(mmds, 16.275)) / 2)


def _feature_pair(who, real_features, gen_features):
    X, Y = _feature_rows(real_features, "real_features"), _feature_rows(gen_features, "gen_features")
    if X.shape[1] != Y.shape[1]:
        raise ValueError(f"{who}: {X.shape[1]} real and {Y.shape[1]} generated features")
    if not 1 <= X.shape[1] <= MAX_FEATURES:
        raise ValueError(f"{who}: {X.shape[1]} features, the device kernel takes 1 to {MAX_FEATURES}")
    for t, name in ((X, "real_features"), (Y, "gen_features")):
        if t.shape[0] == 0:
            raise ValueError(f"{who}: {name} has no rows")
    return X, Y.to(X.device)


def kpd(real_features, gen_features, num_batches=10, batch_size=5000, normalise=True, seed=42):
    """The kernel physics distance of two feature arrays (rows, d): (median, error) over ``num_batches`` MMD estimates of
    ``batch_size`` rows each.  NumPy arrays or CUDA tensors, cast to float64; see the module docstring for the definition and
    for what is and is not claimed about jetnet's draws."""
    X, Y = _feature_pair("kpd", real_features, gen_features)
    lists = kpd_index_lists(X.shape[0], Y.shape[0], num_batches, batch_size, seed)
    num_batches, m = lists.shape[0], lists.shape[2]
    for t, name in ((X, "real_features"), (Y, "gen_features")):
        if t.shape[0] < m:
            warnings.warn(f"kpd: {name} has {t.shape[0]} rows, fewer than batch_size = {m}: the batches draw with replacement from "
                          "too small a set and the result is unreliable", RuntimeWarning, stacklevel=2)
    with torch.cuda.device(X.device):
        if normalise:
            X, Y = _normalise(X, Y)
        n_real, d = X.shape
        Z = torch.cat([X, Y])  # one matrix: set 2 i indexes the real rows, set 2 i + 1 the generated ones
        del X, Y
        lists[:, 1] += n_real
        idx = torch.from_numpy(lists.reshape(2 * num_batches, m).astype(np.int32)).to(Z.device)
        sums = torch.empty((num_batches, 3), dtype=torch.float64, device=Z.device)
        status = torch.zeros((1,), dtype=torch.int32, device=Z.device)
        launch_kpd_sums(Z, idx, [m] * (2 * num_batches), 1.0 / d, KPD_DEGREE, sums, status)
        _raise_on_status(status, m, Z.shape[0], "kpd")
        sums = sums.cpu().numpy()
    return median_and_error([mmd_from_sums(s, m) for s in sums])


# ---- separation powers -----------------------------------------------------------------------------------------------------

MAX_HISTOGRAM_EDGES = 64  # CD_HIST_MAX_EDGES: a workgroup keeps the edges and count tables of 64 columns in 64 KB of LDS


def histogram_workspace_bytes(row_count, d, nedges):
    nbytes = load_library().cd_column_histograms_workspace_bytes(int(row_count), int(d), int(nedges))
    if nbytes == 0:
        _check(-1)
    return nbytes


def launch_column_histograms(x, row_begin, row_count, edges, counts, workspace=None):
    """One ``cd_column_histograms`` call on the current stream over rows [row_begin, row_begin + row_count) of x (rows, d)
    float64; edges (d, nedges) float64; counts (d, nedges - 1) int32, read as uint32: contiguous tensors on one device."""
    lib = load_library()
    for t, dt, name in ((x, torch.float64, "x"), (edges, torch.float64, "edges"), (counts, torch.int32, "counts")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt and t.is_contiguous()):
            raise ValueError(f"launch_column_histograms: {name} must be a contiguous {dt} CUDA tensor")
    d = x.shape[1]
    if edges.dim() != 2 or edges.shape[0] != d or edges.shape[1] < 2 or counts.numel() != d * (edges.shape[1] - 1):
        raise ValueError(f"launch_column_histograms: shapes do not match {d} features")
    if not (0 <= int(row_begin) and 1 <= int(row_count) and int(row_begin) + int(row_count) <= x.shape[0]):
        raise ValueError(f"launch_column_histograms: rows [{row_begin}, {row_begin} + {row_count}) are not a range of the {x.shape[0]} rows of x")
    with torch.cuda.device(x.device):
        if workspace is None:
            workspace = _workspace(x.device, histogram_workspace_bytes(row_count, d, edges.shape[1]))
        _check(lib.cd_column_histograms(x.data_ptr(), int(row_begin), int(row_count), d, edges.data_ptr(), edges.shape[1], counts.data_ptr(),
                                        workspace.data_ptr(), workspace.numel(), _stream()))


def column_histograms(x, edges, row_ranges=None):
    """``np.histogram(x[lo : lo + n, j], bins=edges[j])[0]`` for every column j and every ``(lo, n)`` of ``row_ranges`` (default: all
    rows), on the device: a (ranges, d, nedges - 1) int64 NumPy array.  ``x``: (rows, d) NumPy or CUDA tensor; ``edges`` (d, nedges)."""
    x = _feature_rows(x, "x")
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    d = x.shape[1]
    if edges.ndim != 2 or edges.shape[0] != d or edges.shape[1] < 2:
        raise ValueError(f"column_histograms: edges of shape {edges.shape} for {d} features")
    if not 1 <= d <= MAX_FEATURES or edges.shape[1] > MAX_HISTOGRAM_EDGES:
        raise ValueError(f"column_histograms: {d} features and {edges.shape[1]} edges; the device kernel takes 1 to {MAX_FEATURES} features and "
                         f"at most {MAX_HISTOGRAM_EDGES} edges ({MAX_HISTOGRAM_EDGES - 1} bins)")
    row_ranges = [(0, x.shape[0])] if row_ranges is None else list(row_ranges)
    with torch.cuda.device(x.device):
        edges_d = torch.from_numpy(edges).to(x.device)
        counts = torch.empty((len(row_ranges), d, edges.shape[1] - 1), dtype=torch.int32, device=x.device)
        for k, (lo, n) in enumerate(row_ranges):
            launch_column_histograms(x, lo, n, edges_d, counts[k])
        return counts.cpu().numpy().view(np.uint32).astype(np.int64)


def separation_from_counts(real_counts, gen_counts, edges=None):
    """``0.5 sum (p - q)^2 / (p + q + 1e-16)`` per column with ``p = counts / counts.sum()`` of each set (utils/utils.py:167-175 on
    ``density=True`` histograms).  Where ``edges`` is given, a column whose first and last edge are equal is ``nan``: the
    reference's density divides by a bin width of 0 there."""
    c1, c2 = np.asarray(real_counts, dtype=np.float64), np.asarray(gen_counts, dtype=np.float64)
    if c1.shape != c2.shape or c1.ndim != 2:
        raise ValueError(f"separation_from_counts: counts of shapes {c1.shape} and {c2.shape}")
    with np.errstate(invalid="ignore", divide="ignore"):
        p, q = c1 / c1.sum(axis=1, keepdims=True), c2 / c2.sum(axis=1, keepdims=True)
        sep = 0.5 * ((p - q) ** 2 / (p + q + 1e-16)).sum(axis=1)
    if edges is not None:
        edges = np.asarray(edges)
        sep[edges[:, 0] == edges[:, -1]] = np.nan
    return sep


def separation_powers(real_features, gen_features, bins=50):
    """The reference's separation power of every feature column, a (d,) float64 array: see the module docstring.  ``bins`` is
    the number of EDGES (``make_hist``'s ``np.linspace(min, max, 50)``): ``bins - 1`` bins.  A column whose real values are all
    equal gives ``nan``."""
    X, Y = _feature_pair("separation_powers", real_features, gen_features)
    d, bins = X.shape[1], int(bins)
    if bins < 2:
        raise ValueError(f"separation_powers: bins must be at least 2 (edges), got {bins}")
    if bins > MAX_HISTOGRAM_EDGES:
        raise ValueError(f"separation_powers: bins = {bins}; the device kernel keeps the edges and counts of 64 columns in LDS: at most "
                         f"bins = {MAX_HISTOGRAM_EDGES}")
    with torch.cuda.device(X.device):
        lo, hi = X.amin(dim=0).cpu().numpy(), X.amax(dim=0).cpu().numpy()
        edges = np.stack([np.linspace(lo[j], hi[j], bins) for j in range(d)])
        n_real, n_gen = X.shape[0], Y.shape[0]
        counts = column_histograms(torch.cat([X, Y]), edges, [(0, n_real), (n_real, n_gen)])
    return separation_from_counts(counts[0], counts[1], edges)


def separation_power_total(real_features, gen_features, bins=50):
    """The plain sum of ``separation_powers`` over the columns: what the reference writes as ``TOTAL`` (hgcal_metrics.py:411-415)."""
    return float(np.sum(separation_powers(real_features, gen_features, bins)))


# ---- the reference's metric classes ----------------------------------------------------------------------------------------

class _FeatureMetric:
    """What ``FDP`` and ``KPD`` share: two ``HighLevelFeatures`` over one binning file and the feature arrays of a model's
    generated showers and of the loader's own (the feature-array half of the reference's ``FDP.__call__``)."""

    def __init__(self, binning_dataset, particle):
        self.hlf = HighLevelFeatures(particle, filename=binning_dataset)
        self.reference_hlf = HighLevelFeatures(particle, filename=binning_dataset)

    def pre_process(self, energies, hlf_class, label):
        """The reference's array, label column included (``feature_matrix`` builds the rest)."""
        features = hlf_class.feature_matrix(energies)
        return np.concatenate([features, label * np.ones((features.shape[0], 1))], axis=1)

    def feature_arrays(self, trained_model, eval_data):
        """(generated, Geant4) feature arrays, NaN replaced as the reference does before it calls jetnet."""
        reference_shower, reference_energy = [], []
        for energy, _, data in eval_data:
            reference_shower.append(_to_numpy(data))
            reference_energy.append(_to_numpy(energy))
        reference_shower = np.concatenate(reference_shower)
        reference_energy = np.concatenate(reference_energy)
        generated, energies = trained_model.generate(data_loader=eval_data, sample_steps=trained_model.config.get("NSTEPS"), sample_offset=0)
        self.hlf.CalculateFeatures(_flat(generated))
        self.reference_hlf.CalculateFeatures(_flat(reference_shower))
        source_array = self.pre_process(energies, self.hlf, 0.)[:, :-1]
        reference_array = self.pre_process(reference_energy, self.reference_hlf, 1.)[:, :-1]
        return np.nan_to_num(source_array), np.nan_to_num(reference_array)


class FDP(_FeatureMetric):
    """The reference's ``FDP`` (train/evaluate.py:21-79).  Its constructor is spelled ``_init__`` there and never runs; this
    one takes the same two arguments and works.  ``fpd_kwargs`` go to ``fpd`` (the reference uses jetnet's defaults)."""

    def __init__(self, binning_dataset, particle, **fpd_kwargs):
        super().__init__(binning_dataset, particle)
        self.fpd_kwargs = fpd_kwargs

    def __call__(self, trained_model, eval_data, kwargs=None) -> float:
        source_array, reference_array = self.feature_arrays(trained_model, eval_data)
        try:
            value, _ = fpd(source_array, reference_array, **self.fpd_kwargs)
        except ValueError as err:
            raise FDPCalculationError(err)
        return value


class KPD(_FeatureMetric):
    """The kernel physics distance as a metric object with ``FDP``'s constructor and call: the value of ``kpd`` between the
    Geant4 showers of the loader (the ``real_features``, whose column maxima normalise both arrays, as in
    hgcal_metrics.py:424) and the model's generated ones.  ``kpd_kwargs`` go to ``kpd``."""

    def __init__(self, binning_dataset, particle, **kpd_kwargs):
        super().__init__(binning_dataset, particle)
        self.kpd_kwargs = kpd_kwargs

    def __call__(self, trained_model, eval_data, kwargs=None) -> float:
        source_array, reference_array = self.feature_arrays(trained_model, eval_data)
        try:
            value, _ = kpd(reference_array, source_array, **self.kpd_kwargs)
        except ValueError as err:
            raise FDPCalculationError(err)
        return value


class ClassifierScore(_FeatureMetric):
    """The classifier two-sample test as a metric object with ``FDP``'s constructor and call: the AUC of a ``DNN`` trained to tell
    the model's generated showers (label 1) from the loader's Geant4 ones (label 0) in the space of the same feature arrays
    (hgcal_metrics.py:434-490; ``calodiffusion_amd.classifier.ClassifierTest``, whose keyword arguments ``classifier_kwargs`` are).
    0.5 is a perfect generator.  The full result of the last call (accuracy, JSD, calibrated figures) is kept in ``last_result``."""

    def __init__(self, binning_dataset, particle, rounded_scores=False, **classifier_kwargs):
        super().__init__(binning_dataset, particle)
        self.rounded_scores, self.classifier_kwargs, self.last_result = rounded_scores, classifier_kwargs, None

    def __call__(self, trained_model, eval_data, kwargs=None) -> float:
        from .classifier import ClassifierTest
        source_array, reference_array = self.feature_arrays(trained_model, eval_data)
        features = np.concatenate([source_array, reference_array], axis=0)
        labels = np.concatenate([np.ones(source_array.shape[0], dtype=np.float32), np.zeros(reference_array.shape[0], dtype=np.float32)])
        try:
            test = ClassifierTest(features.shape[1], **self.classifier_kwargs).fit(features, labels)
            self.last_result = test.evaluate(rounded_scores=self.rounded_scores)
        except ValueError as err:
            raise FDPCalculationError(err)
        return self.last_result.auc


def _to_numpy(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _flat(showers):
    showers = _to_numpy(showers)
    return showers.reshape(showers.shape[0], int(np.prod(showers.shape[1:])))
