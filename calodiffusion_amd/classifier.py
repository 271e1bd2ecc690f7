"""The classifier two-sample test of the reference's metrics program (calodiffusion/tests/hgcal_metrics.py:45-209, 434-490) on the
device: a ``DNN`` learns to tell generated from Geant4 rows of the feature matrix, and its accuracy, AUC and
``JSD = 1 - BCE / ln 2`` on held-out rows, before and after isotonic calibration, are the figures -- the CaloChallenge "classifier AUC".

Training and scoring run in the library (``cd_classifier_*``, include/calodiff.h "classifier two-sample test": fp32 parameters,
every matrix product an exact three-term bf16 split on the matrix cores, fused bias / LeakyReLU / dropout, ``cd_adam_step``);
the scaled feature matrix is uploaded once and an epoch is one call that enqueues all its steps.  There is no host fallback.
The bookkeeping around it is float64 NumPy on the host and needs neither scikit-learn nor SciPy:

  * ``standard_scale``        ``StandardScaler().fit_transform`` (:440-441), population variance, zero-variance columns scaled by 1;
  * ``ttv_split``             index lists (train, test, val) of sizes ``int(n f)`` (:255-265, 445-446).  The reference calls the 10 % part
                              "test" and reports on it, and picks ``best_epoch`` and calibrates on the 20 % "val" part; kept.  The lists
                              come from ``np.random.default_rng(seed).permutation`` -- this package's draw, NOT the reference's
                              ``np.random.shuffle`` stream (as for ``evaluate.kpd``'s index lists);
  * ``roc_auc``               the Mann-Whitney statistic with average ranks for ties = ``sklearn.metrics.roc_auc_score``;
  * ``IsotonicCalibrator``    ``IsotonicRegression(out_of_bounds='clip', y_min=1e-6, y_max=1 - 1e-6)`` (:180): pool adjacent violators,
                              linear interpolation between the kept knots;
  * ``calibration_curve``     sklearn's, uniform bins (:141).

Dropout masks and the per-epoch shuffles (``default_rng(seed + epoch)``) are this package's own streams, not torch's: runs agree with
the reference's within the spread of its own seeds, not step by step.  Not restored, as in the reference (:57-59 are commented out
there): the best epoch's weights.  ``cls_n_iters > 1``: call ``fit`` again.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from .abi import CdClassifierDesc, CdHlfDesc, _check, _dev32, _nbytes, _ptr, _stream, load_library, require_gpu

MAX_DIM, MAX_LAYERS, MAX_BATCH, MAX_ROWS_PER_CALL = 4096, 8, 256, 65536  # CD_CLS_* of include/calodiff.h
LEAKY_SLOPE = 0.01  # torch.nn.LeakyReLU()'s default, what the reference builds (:197)


# ---- the device entry points --------------------------------------------------------------------------------------------------

def _desc(input_dim, hidden, num_layer, slope=LEAKY_SLOPE, dropout=0.0):
    return CdClassifierDesc(C.sizeof(CdClassifierDesc), int(input_dim), int(hidden), int(num_layer), float(slope), float(dropout))


def _strict(t, name, dtype=torch.float32, ndim=None):
    """``t`` as it is, if it is a contiguous CUDA tensor of ``dtype`` (and of ``ndim`` dimensions, where given)."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and ndim in (None, t.dim())):
        raise ValueError(f"{name} must be a contiguous {'' if ndim is None else f'{ndim}-d '}{str(dtype)[len('torch.'):]} CUDA tensor")
    return t


def _weight_table(params):
    return (C.c_void_p * len(params))(*[_strict(p, "a parameter").data_ptr() for p in params])


def workspace_bytes(desc, max_rows_per_call):
    return _nbytes(load_library().cd_classifier_workspace_bytes, C.byref(desc), int(max_rows_per_call))


def num_params(desc):
    n = C.c_int64()
    _check(load_library().cd_classifier_num_params(C.byref(desc), C.byref(n)))
    return n.value


def _workspace(desc, rows, device):
    return torch.empty((workspace_bytes(desc, rows),), dtype=torch.uint8, device=device)


def forward_logits(desc, params, x, idx=None, count=None, max_rows_per_call=4096, workspace=None):
    """``cd_classifier_forward``: eval-mode logits (count,) float32 of the rows ``idx`` (device int32) of ``x`` (rows, d), or of its
    first ``count`` rows (default: all)."""
    x = _strict(x, "x")
    count = (x.shape[0] if count is None else int(count)) if idx is None else _strict(idx, "idx", torch.int32, 1).numel()
    with torch.cuda.device(x.device):
        out = torch.empty((count,), dtype=torch.float32, device=x.device)
        rows = max(1, min(int(max_rows_per_call), max(count, 1)))
        ws = _workspace(desc, rows, x.device) if workspace is None else workspace
        _check(load_library().cd_classifier_forward(
            C.byref(desc), _weight_table(params), x.data_ptr(), x.shape[0], None if idx is None else idx.data_ptr(), count, out.data_ptr(),
            rows, ws.data_ptr(), ws.numel(), _stream()))
    return out


def train_step(desc, params, x, labels, batch_idx, seed, step, grads, adam=None, workspace=None):
    """``cd_classifier_train_step``: the flat gradient into ``grads`` and the loss as a (1,) float64 device tensor.  ``adam``:
    None, or ``(exp_avg, exp_avg_sq, lr, beta1, beta2, eps, adam_step)`` to apply the update."""
    x, labels, grads = _strict(x, "x"), _strict(labels, "labels"), _strict(grads, "grads")
    batch = _strict(batch_idx, "batch_idx", torch.int32, 1).numel()
    with torch.cuda.device(x.device):
        loss = torch.empty((1,), dtype=torch.float64, device=x.device)
        ws = _workspace(desc, max(batch, 1), x.device) if workspace is None else workspace
        m, v, lr, b1, b2, eps, k = adam if adam is not None else (None, None, 0.0, 0.9, 0.999, 1e-8, 1)
        _check(load_library().cd_classifier_train_step(
            C.byref(desc), _weight_table(params), x.data_ptr(), labels.data_ptr(), x.shape[0], batch_idx.data_ptr(), batch, int(seed), int(step),
            grads.data_ptr(), loss.data_ptr(), int(adam is not None), _ptr(m), _ptr(v), float(lr), float(b1), float(b2), float(eps),
            int(k), ws.data_ptr(), ws.numel(), _stream()))
    return loss


def train_epoch(desc, params, x, labels, perm, batch_size, seed, first_step, grads, exp_avg, exp_avg_sq, lr, betas=(0.9, 0.999), eps=1e-8,
                workspace=None):
    """``cd_classifier_train_epoch``: every batch of ``perm`` (device int32) as a training step with Adam, all enqueued on the
    current stream; the per-step losses as a float64 device tensor."""
    x, labels, grads = _strict(x, "x"), _strict(labels, "labels"), _strict(grads, "grads")
    n_train = _strict(perm, "perm", torch.int32, 1).numel()
    steps = -(-n_train // int(batch_size)) if int(batch_size) > 0 else 0
    with torch.cuda.device(x.device):
        losses = torch.empty((max(steps, 1),), dtype=torch.float64, device=x.device)
        ws = _workspace(desc, max(1, min(int(batch_size), MAX_BATCH)), x.device) if workspace is None else workspace
        _check(load_library().cd_classifier_train_epoch(
            C.byref(desc), _weight_table(params), x.data_ptr(), labels.data_ptr(), x.shape[0], perm.data_ptr(), n_train, int(batch_size),
            int(seed), int(first_step), grads.data_ptr(), _strict(exp_avg, "exp_avg").data_ptr(), _strict(exp_avg_sq, "exp_avg_sq").data_ptr(),
            float(lr), float(betas[0]), float(betas[1]), float(eps), losses.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    return losses[:steps]


def dropout_mask(seed, step, layer, p, rows, n, device="cuda"):
    """``cd_classifier_dropout_mask``: the (rows, n) uint8 mask (1 = kept) the training kernels apply at (seed, step, layer)."""
    require_gpu()
    mask = torch.empty((int(rows), int(n)), dtype=torch.uint8, device=device)
    with torch.cuda.device(mask.device):
        _check(load_library().cd_classifier_dropout_mask(int(seed), int(step), int(layer), float(p), int(rows), int(n),
                                                         mask.data_ptr(), _stream()))
    return mask


def linear_act(x, w, bias, act=True, slope=LEAKY_SLOPE, dropout=0.0, seed=0, step=0, layer=0):
    """``cd_op_linear_act``: dropout(act(x w^T + bias)), the forward layer kernel on its own."""
    x, w = _strict(x, "x"), _strict(w, "w")
    with torch.cuda.device(x.device):
        y = torch.empty((x.shape[0], w.shape[0]), dtype=torch.float32, device=x.device)
        _check(load_library().cd_op_linear_act(
            x.data_ptr(), w.data_ptr(), None if bias is None else _strict(bias, "bias").data_ptr(), y.data_ptr(), x.shape[0], x.shape[1], w.shape[0],
            int(bool(act)), float(slope), float(dropout), int(seed), int(step), int(layer), _stream()))
    return y


def linear_act_backward(x, w, y, dy, mask=None, keep_scale=1.0, act=True, slope=LEAKY_SLOPE, need_dx=True):
    """``cd_op_linear_act_backward``: (dx or None, dw, db) for an arbitrary ``dy``; ``mask``: (rows, n_out) uint8 or None."""
    x, w, y, dy = _strict(x, "x"), _strict(w, "w"), _strict(y, "y"), _strict(dy, "dy")
    if mask is not None and not (mask.is_cuda and mask.dtype == torch.uint8 and mask.is_contiguous() and mask.shape == y.shape):
        raise ValueError("mask must be a contiguous uint8 CUDA tensor of y's shape")
    with torch.cuda.device(x.device):
        dx = torch.empty_like(x) if need_dx else None
        dw, db = torch.empty_like(w), torch.empty((w.shape[0],), dtype=torch.float32, device=x.device)
        ws = torch.empty((max(y.numel(), 4),), dtype=torch.float32, device=x.device)
        _check(load_library().cd_op_linear_act_backward(
            x.data_ptr(), w.data_ptr(), y.data_ptr(), dy.data_ptr(), _ptr(mask), float(keep_scale), int(bool(act)), float(slope),
            _ptr(dx), dw.data_ptr(), db.data_ptr(), x.shape[0], x.shape[1], w.shape[0], ws.data_ptr(), ws.numel() * 4, _stream()))
    return dx, dw, db


# ---- the network --------------------------------------------------------------------------------------------------------------

class DNN(torch.nn.Module):
    """The reference's classifier (hgcal_metrics.py:185-209), same attributes and therefore same ``state_dict`` keys and
    ``nn.Linear`` initialisation.  No sigmoid in the last layer: use with BCE-with-logits.  ``forward`` runs on the device in eval
    mode (or under ``no_grad``); training goes through ``ClassifierTest.fit``."""

    def __init__(self, num_layer, num_hidden, input_dim, dropout_probability=0.):
        super().__init__()
        self.dpo = dropout_probability
        self.inputlayer = torch.nn.Linear(input_dim, num_hidden)
        self.outputlayer = torch.nn.Linear(num_hidden, 1)
        all_layers = [self.inputlayer, torch.nn.LeakyReLU(), torch.nn.Dropout(self.dpo)]
        for _ in range(num_layer):
            all_layers.append(torch.nn.Linear(num_hidden, num_hidden))
            all_layers.append(torch.nn.LeakyReLU())
            all_layers.append(torch.nn.Dropout(self.dpo))
        all_layers.append(self.outputlayer)
        self.layers = torch.nn.Sequential(*all_layers)
        self.num_layer, self.num_hidden, self.input_dim = int(num_layer), int(num_hidden), int(input_dim)

    def desc(self):
        return _desc(self.input_dim, self.num_hidden, self.num_layer, LEAKY_SLOPE, self.dpo)

    def device_params(self):
        """The parameters in the library's order (``parameters()``: inputlayer, outputlayer, then the hidden layers)."""
        return [p.data for p in self.parameters()]

    def forward(self, x):
        if self.training and torch.is_grad_enabled():
            raise NotImplementedError("DNN.forward: training mode has no autograd path here; train with ClassifierTest.fit "
                                      "(cd_classifier_train_epoch), or call model.eval() / torch.no_grad() to score")
        if not (isinstance(x, torch.Tensor) and x.is_cuda):
            raise RuntimeError("DNN.forward: x must be a CUDA(ROCm) tensor: calodiffusion_amd computes on the GPU only")
        if x.dim() != 2 or x.shape[1] != self.input_dim:
            raise ValueError(f"DNN.forward: expected (rows, {self.input_dim}), got {tuple(x.shape)}")
        params = self.device_params()
        if not all(p.is_cuda for p in params):
            raise RuntimeError("DNN.forward: move the module to the device first (model.cuda())")
        x = _dev32(x.detach(), "x")
        if x.shape[0] == 0:
            return torch.empty((0, 1), dtype=torch.float32, device=x.device)
        return forward_logits(self.desc(), params, x).reshape(-1, 1)


# ---- host bookkeeping (float64 NumPy) --------------------------------------------------------------------------------------------

def standard_scale(feats):
    """``StandardScaler().fit_transform(feats)`` in float64: (x - mean) / sqrt(population variance) per column; a column whose
    variance is zero (within the rounding of its own mean, sklearn's rule) is scaled by 1.  Same operation order as sklearn's
    ``_incremental_mean_and_var`` for one batch."""
    x = np.array(feats, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] < 1:
        raise ValueError(f"standard_scale: expected a (rows, features) array with at least one row, got shape {x.shape}")
    n = x.shape[0]
    mean = np.sum(x, axis=0) / n
    temp = x - mean
    correction = np.sum(temp, axis=0)
    temp **= 2
    var = (np.sum(temp, axis=0) - correction ** 2 / n) / n
    eps = np.finfo(np.float64).eps
    constant = var <= n * eps * var + (n * mean * eps) ** 2
    scale = np.sqrt(var)
    scale[constant | (scale == 0.0)] = 1.0
    x -= mean
    x /= scale
    return x


def ttv_split(n, fractions=(0.7, 0.1, 0.2), seed=0):
    """(train, test, val) index arrays: a permutation of ``range(n)`` cut after ``int(n f0)`` and ``int(n f0) + int(n f1)``
    entries, the last part taking the rest (np.split in hgcal_metrics.py:259-261).  The permutation is
    ``np.random.default_rng(seed).permutation(n)``: not the reference's ``np.random.shuffle`` stream."""
    n = int(n)
    if n < 1 or len(fractions) != 3 or min(fractions) < 0 or sum(fractions) > 1 + 1e-12:
        raise ValueError(f"ttv_split: needs n >= 1 and three non-negative fractions summing to at most 1, got {n}, {fractions}")
    num = (n * np.asarray(fractions, dtype=np.float64)).astype(int)
    perm = np.random.default_rng(seed).permutation(n)
    train, test, val = np.split(perm, num.cumsum()[:-1])
    return train, test, val


def roc_auc(labels, scores):
    """Area under the ROC curve = P(score of a positive > score of a negative) + P(equal) / 2, from average ranks; the rank sum is
    an exact integer (twice the ranks), so only the final division rounds.  Equals ``sklearn.metrics.roc_auc_score``."""
    y = np.asarray(labels).reshape(-1)
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    if y.shape != s.shape:
        raise ValueError(f"roc_auc: {y.size} labels and {s.size} scores")
    pos = y > 0.5
    n_pos, n_neg = int(pos.sum()), int((~pos).sum())
    if n_pos == 0 or n_neg == 0:
        raise ValueError("roc_auc: only one class present")
    if np.isnan(s).any():
        raise ValueError("roc_auc: a score is NaN")
    order = np.argsort(s, kind="stable")
    ss = s[order]
    first = np.concatenate(([True], ss[1:] != ss[:-1]))
    start = np.flatnonzero(first)                       # first sorted position of every group of equal scores
    end = np.concatenate((start[1:], [s.size]))         # one past its last
    twice_rank = (start + end + 1)[np.cumsum(first) - 1]  # 2 x the average of the 1-based ranks start + 1 ... end
    twice_sum = int(twice_rank[pos[order]].astype(np.int64).sum())
    return (twice_sum - n_pos * (n_pos + 1)) / (2.0 * n_pos * n_neg)


def calibration_curve(y_true, y_prob, n_bins=10):
    """sklearn's ``calibration_curve(..., strategy='uniform')``: (fraction of positives, mean prediction) of every non-empty bin."""
    y_true, y_prob = np.asarray(y_true, dtype=np.float64).reshape(-1), np.asarray(y_prob, dtype=np.float64).reshape(-1)
    if y_prob.min() < 0 or y_prob.max() > 1:
        raise ValueError("calibration_curve: y_prob has values outside [0, 1]")
    bins = np.linspace(0.0, 1.0, n_bins + 1)
    binids = np.searchsorted(bins[1:-1], y_prob)
    bin_sums = np.bincount(binids, weights=y_prob, minlength=len(bins))
    bin_true = np.bincount(binids, weights=y_true, minlength=len(bins))
    bin_total = np.bincount(binids, minlength=len(bins))
    nonzero = bin_total != 0
    return bin_true[nonzero] / bin_total[nonzero], bin_sums[nonzero] / bin_total[nonzero]


class IsotonicCalibrator:
    """``IsotonicRegression(out_of_bounds='clip', y_min=..., y_max=...)`` in float64: samples sorted by (x, y), equal x pooled to
    their mean, pool-adjacent-violators, the fit clipped to [y_min, y_max], interior points of flat stretches dropped; ``predict``
    clips the query to the fitted range and interpolates linearly between the kept knots."""

    def __init__(self, y_min=1e-6, y_max=1.0 - 1e-6):
        self.y_min, self.y_max = y_min, y_max
        self.x_knots = self.y_knots = None

    def fit(self, x, y):
        x, y = np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(y, dtype=np.float64).reshape(-1)
        if x.shape != y.shape or x.size == 0:
            raise ValueError(f"IsotonicCalibrator.fit: {x.size} scores and {y.size} targets")
        order = np.lexsort((y, x))
        x, y = x[order], y[order]
        eps = np.finfo(np.float64).resolution
        ux, uy, uw = [], [], []
        cur_x, cur_y, cur_w = x[0], 0.0, 0.0
        for xi, yi in zip(x.tolist(), y.tolist()):
            if xi - cur_x >= eps:
                ux.append(cur_x); uy.append(cur_y / cur_w); uw.append(cur_w)
                cur_x, cur_y, cur_w = xi, yi, 1.0
            else:
                cur_y += yi
                cur_w += 1.0
        ux.append(cur_x); uy.append(cur_y / cur_w); uw.append(cur_w)
        fit = np.asarray(_pava(uy, uw), dtype=np.float64)
        if self.y_min is not None or self.y_max is not None:
            fit = np.clip(fit, self.y_min, self.y_max)
        ux = np.asarray(ux, dtype=np.float64)
        keep = np.ones(fit.size, dtype=bool)
        if fit.size > 2:
            keep[1:-1] = (fit[1:-1] != fit[:-2]) | (fit[1:-1] != fit[2:])
        self.x_knots, self.y_knots = ux[keep], fit[keep]
        return self

    def predict(self, t):
        if self.x_knots is None:
            raise RuntimeError("IsotonicCalibrator.predict: call fit first")
        t = np.asarray(t, dtype=np.float64)
        xk, yk = self.x_knots, self.y_knots
        if xk.size == 1:
            return np.full(t.shape, yk[0])
        tc = np.clip(t, xk[0], xk[-1])
        hi = np.clip(np.searchsorted(xk, tc), 1, xk.size - 1)
        lo = hi - 1
        slope = (yk[hi] - yk[lo]) / (xk[hi] - xk[lo])
        return slope * (tc - xk[lo]) + yk[lo]


def _pava(y, w):
    """Pool adjacent violators over blocks (the in-place single pass with backtracking): the weighted least-squares
    non-decreasing fit of y."""
    y, w = list(y), list(w)
    n = len(y)
    target = list(range(n))
    i = 0
    while i < n:
        k = target[i] + 1
        if k == n:
            break
        if y[i] < y[k]:
            i = k
            continue
        sum_wy, sum_w = w[i] * y[i], w[i]
        while True:  # inside a non-increasing run of blocks
            prev_y = y[k]
            sum_wy += w[k] * y[k]
            sum_w += w[k]
            k = target[k] + 1
            if k == n or prev_y < y[k]:
                y[i], w[i] = sum_wy / sum_w, sum_w
                target[i], target[k - 1] = k - 1, i
                if i > 0:
                    i = target[i - 1]  # the pooled block may now violate its predecessor
                break
    i = 0
    while i < n:
        k = target[i] + 1
        for j in range(i + 1, k):
            y[j] = y[i]
        i = k
    return y


def bce_with_logits(logits, labels):
    """mean(max(z, 0) - z y + log1p(exp(-|z|))) in float64 (torch.nn.BCEWithLogitsLoss, hgcal_metrics.py:123)."""
    z, y = np.asarray(logits, dtype=np.float64).reshape(-1), np.asarray(labels, dtype=np.float64).reshape(-1)
    return float(np.mean(np.maximum(z, 0.0) - z * y + np.log1p(np.exp(-np.abs(z)))))


def bce_of_probabilities(p, labels):
    """torch.nn.BCELoss (:152): -mean(y log p + (1 - y) log(1 - p)), each log clamped at -100."""
    p, y = np.asarray(p, dtype=np.float64).reshape(-1), np.asarray(labels, dtype=np.float64).reshape(-1)
    with np.errstate(divide="ignore"):
        lp, lq = np.maximum(np.log(p), -100.0), np.maximum(np.log1p(-p), -100.0)
    return float(-np.mean(y * lp + (1.0 - y) * lq))


def _sigmoid(z):
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


# ---- the test -----------------------------------------------------------------------------------------------------------------

@dataclass
class ClassifierResult:
    accuracy: float
    auc: float
    bce: float
    jsd: float
    accuracy_cal: float
    auc_cal: float
    jsd_cal: float
    best_epoch: int
    step_losses: np.ndarray = field(repr=False)
    rounded_scores: bool = False


class ClassifierTest:
    """``fit(features, labels)`` then ``evaluate()``: hgcal_metrics.py:434-490 with its hyper-parameters as defaults.  ``model`` (a
    ``DNN`` with ``nn.Linear``'s default initialisation under ``torch.manual_seed(seed)``, the global generator left untouched) is
    built here and may be re-initialised before ``fit``."""

    def __init__(self, input_dim, num_layer=2, num_hidden=2024, dropout=0.2, lr=1e-4, batch_size=256, n_epochs=50, seed=0):
        if not 1 <= int(input_dim) <= MAX_DIM or not 1 <= int(num_hidden) <= MAX_DIM:
            raise ValueError(f"ClassifierTest: input_dim and num_hidden must be in [1, {MAX_DIM}], got {input_dim} and {num_hidden}")
        if not 0 <= int(num_layer) <= MAX_LAYERS:
            raise ValueError(f"ClassifierTest: num_layer must be in [0, {MAX_LAYERS}], got {num_layer}")
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"ClassifierTest: dropout must be in [0, 1), got {dropout}")
        if not 1 <= int(batch_size) <= MAX_BATCH:
            raise ValueError(f"ClassifierTest: batch_size must be in [1, {MAX_BATCH}] (the weight gradient sums a batch in one pass), got {batch_size}")
        if not float(lr) > 0.0 or int(n_epochs) < 1:
            raise ValueError(f"ClassifierTest: needs lr > 0 and n_epochs >= 1, got {lr} and {n_epochs}")
        self.input_dim, self.num_layer, self.num_hidden = int(input_dim), int(num_layer), int(num_hidden)
        self.dropout, self.lr, self.batch_size, self.n_epochs, self.seed = float(dropout), float(lr), int(batch_size), int(n_epochs), int(seed)
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(self.seed)
            self.model = DNN(self.num_layer, self.num_hidden, self.input_dim, self.dropout)
        self.best_epoch = -1
        self.val_accuracies, self.step_losses = [], np.zeros((0,), dtype=np.float64)
        self._x = self._labels = self.split = None

    def epoch_permutation(self, epoch):
        """The order of the training rows in ``epoch`` (0-based): ``default_rng(seed + epoch).permutation`` of the train list."""
        return np.random.default_rng(self.seed + epoch).permutation(self.split[0])

    def fit(self, features, labels, fractions=(0.7, 0.1, 0.2)):
        require_gpu()
        feats = features.detach().cpu().numpy() if isinstance(features, torch.Tensor) else np.asarray(features)
        y = (labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)).reshape(-1).astype(np.float32)
        if feats.ndim != 2 or feats.shape[1] != self.input_dim or feats.shape[0] != y.size:
            raise ValueError(f"ClassifierTest.fit: expected features (rows, {self.input_dim}) and as many labels, got {feats.shape} and {y.size}")
        if not np.isin(y, (0.0, 1.0)).all():
            raise ValueError("ClassifierTest.fit: labels must be 0 (Geant4) or 1 (generated)")
        self.split = ttv_split(feats.shape[0], fractions, self.seed)
        if min(len(part) for part in self.split) < 1:
            raise ValueError(f"ClassifierTest.fit: {feats.shape[0]} rows leave a part of the split empty")
        self._x = torch.from_numpy(standard_scale(feats).astype(np.float32)).cuda()  # uploaded once
        self._labels = torch.from_numpy(y).to(self._x.device)
        device = self._x.device
        self.model.to(device)
        desc, params = self.model.desc(), self.model.device_params()
        with torch.cuda.device(device):
            n = num_params(desc)
            grads, m, v = (torch.zeros((n,), dtype=torch.float32, device=device) for _ in range(3))
            ws = _workspace(desc, self.batch_size, device)
            val_idx = torch.from_numpy(self.split[2].astype(np.int32)).to(device)
            val_y = self._labels[val_idx.long()]
            steps = -(-len(self.split[0]) // self.batch_size)
            best, losses = float("-inf"), []
            self.best_epoch, self.val_accuracies = -1, []
            for epoch in range(self.n_epochs):
                perm = torch.from_numpy(self.epoch_permutation(epoch).astype(np.int32)).to(device)
                losses.append(train_epoch(desc, params, self._x, self._labels, perm, self.batch_size, self.seed, epoch * steps, grads, m, v,
                                          self.lr, workspace=ws))
                z = forward_logits(desc, params, self._x, val_idx)
                acc = float((torch.round(torch.sigmoid(z)) == val_y).double().mean().item())
                self.val_accuracies.append(acc)
                if acc > best:
                    best, self.best_epoch = acc, epoch + 1
                if acc == 1.0:
                    break
            self.step_losses = torch.cat(losses).cpu().numpy()
        return self

    def logits(self, rows):
        """Eval-mode logits (float64 NumPy) of the given rows of the fitted matrix."""
        idx = torch.from_numpy(np.asarray(rows).astype(np.int32)).to(self._x.device)
        return forward_logits(self.model.desc(), self.model.device_params(), self._x, idx).cpu().numpy().astype(np.float64)

    def evaluate(self, rounded_scores=False):
        """The figures on the 10 % "test" part, calibrated on the 20 % "val" part (evaluate_cls(final_eval=True), :105-157).
        ``rounded_scores=False``: AUC and calibration take the continuous sigmoid scores (the CaloChallenge definition).  ``True``: the
        scores are rounded to 0 / 1 first, exactly as the reference does (:124-153) -- its "AUC" is then the balanced accuracy."""
        if self._x is None:
            raise RuntimeError("ClassifierTest.evaluate: call fit first")
        _, test, val = self.split
        y = self._labels.cpu().numpy().astype(np.float64)
        z = self.logits(test)
        bce = bce_with_logits(z, y[test])
        prob = _sigmoid(z)
        hard = np.clip(np.round(prob), 0.0, 1.0)
        scores = hard if rounded_scores else prob
        calibrator = IsotonicCalibrator().fit(_sigmoid(self.logits(val)), y[val])
        rescaled = calibrator.predict(scores)
        bce_cal = bce_of_probabilities(rescaled, y[test])
        return ClassifierResult(
            accuracy=float(np.mean(hard == y[test])), auc=roc_auc(y[test], scores), bce=bce, jsd=1.0 - bce / math.log(2.0),
            accuracy_cal=float(np.mean(np.clip(np.round(rescaled), 0.0, 1.0) == y[test])), auc_cal=roc_auc(y[test], rescaled),
            jsd_cal=1.0 - bce_cal / math.log(2.0), best_epoch=self.best_epoch, step_losses=self.step_losses, rounded_scores=bool(rounded_scores))


# ---- the feature matrix of hgcal_metrics.py ----------------------------------------------------------------------------------------

def hgcal_features(showers, incident_E, xmap, ymap):
    """``compute_feats`` (hgcal_metrics.py:216-252): float32 (N, 2 + 5 L) =
    ``[E_inc, E_tot / E_inc, log10(E_layer + 1e-8), x centre, x width, y centre, y width]`` of showers (N, L, C) with the per-layer
    coordinate tables ``xmap[:, :C]`` and ``ymap[:, :C]``, through ``cd_hlf_compute`` (one pass, fp64 sums).  An empty layer has
    centre and width 0, as the reference's masked division gives."""
    from .hlf import _E, _EC_ETA, _EC_PHI, _W_ETA, _W_PHI
    lib = load_library()
    require_gpu()
    if isinstance(showers, torch.Tensor):
        sh = showers.detach()
    else:
        sh = torch.from_numpy(np.ascontiguousarray(showers, dtype=np.float32))
    if sh.dim() != 3:
        raise ValueError(f"hgcal_features: expected showers (N, layers, cells), got {tuple(sh.shape)}")
    N, L, Cc = sh.shape
    xs, ys = np.asarray(xmap, dtype=np.float64), np.asarray(ymap, dtype=np.float64)
    if xs.ndim != 2 or xs.shape != ys.shape or xs.shape[0] != L or xs.shape[1] < Cc:
        raise ValueError(f"hgcal_features: xmap / ymap must be ({L}, >= {Cc}), got {xs.shape} and {ys.shape}")
    e_inc = np.asarray(incident_E.detach().cpu().numpy() if isinstance(incident_E, torch.Tensor) else incident_E, dtype=np.float64).reshape(-1, 1)
    if e_inc.shape[0] != N:
        raise ValueError(f"hgcal_features: {e_inc.shape[0]} incident energies for {N} showers")
    eta, phi = np.ascontiguousarray(xs[:, :Cc]).reshape(-1), np.ascontiguousarray(ys[:, :Cc]).reshape(-1)
    offsets = (C.c_int32 * (L + 1))(*[l * Cc for l in range(L + 1)])
    centres = (C.c_int32 * L)(*([1] * L))
    desc = CdHlfDesc(C.sizeof(CdHlfDesc), L, offsets, eta.ctypes.data_as(C.POINTER(C.c_double)),
                     phi.ctypes.data_as(C.POINTER(C.c_double)), centres)
    sh = _dev32(sh.cuda(), "showers").reshape(N, L * Cc)
    with torch.cuda.device(sh.device):
        handle = C.c_void_p()
        _check(lib.cd_hlf_create(C.byref(desc), C.byref(handle), _stream()))
        try:
            out = torch.empty((N, L, 8), dtype=torch.float64, device=sh.device)
            hits = torch.empty((N, L), dtype=torch.int32, device=sh.device)
            if N:
                _check(lib.cd_hlf_compute(handle, sh.data_ptr(), N, 0.0, out.data_ptr(), hits.data_ptr(), _stream()))
            rec = out.cpu().numpy()
        finally:
            lib.cd_hlf_destroy(handle)
    e_layer = rec[:, :, _E]
    e_tot = np.zeros((N,), dtype=np.float64)
    for l in range(L):
        e_tot += e_layer[:, l]
    blocks = [e_inc, e_tot.reshape(-1, 1) / e_inc, np.log10(e_layer + 1e-8), rec[:, :, _EC_ETA], rec[:, :, _W_ETA], rec[:, :, _EC_PHI],
              rec[:, :, _W_PHI]]
    return np.concatenate(blocks, axis=-1).astype(np.float32)
