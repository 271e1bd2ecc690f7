"""Oracle of the classifier two-sample test (calodiffusion_amd.classifier): a torch restatement, at any dtype, of the reference's
``DNN`` (calodiffusion/tests/hgcal_metrics.py:185-209), its training step (``BCEWithLogitsLoss`` + ``torch.optim.Adam``, :68-84, :461)
and its loop (:45-66), with the dropout masks passed IN (the device's own, ``cd_classifier_dropout_mask``), plus the exact-integer
layer cases and a float64 NumPy restatement of ``compute_feats`` (:216-252).  hgcal_metrics.py itself needs h5py and jetnet and
cannot be imported.  No test imports scikit-learn or SciPy: their results are in tests/golden/classifier_host.npz
(tools/gen_golden_classifier.py)."""
import math

import numpy as np
import torch

# (input_dim, hidden, num_layer, batch): hidden below, across and above a 32-wide tile, the production width 2024 = 63 * 32 + 8,
# a full and a ragged batch
SHAPES = [(1, 8, 0, 1), (5, 72, 2, 37), (33, 40, 1, 64), (226, 2024, 2, 256), (226, 2024, 2, 37)]
SLOPE = 0.01  # torch.nn.LeakyReLU() (:197)


class RestatedDNN(torch.nn.Module):
    """hgcal_metrics.py:185-209 verbatim in structure; ``forward`` takes the dropout masks instead of drawing them."""

    def __init__(self, num_layer, num_hidden, input_dim, dropout_probability=0.):
        super().__init__()
        self.dpo = dropout_probability
        self.inputlayer = torch.nn.Linear(input_dim, num_hidden)                   # :194
        self.outputlayer = torch.nn.Linear(num_hidden, 1)                          # :195
        all_layers = [self.inputlayer, torch.nn.LeakyReLU(), torch.nn.Dropout(self.dpo)]   # :197
        for _ in range(num_layer):                                                 # :198-201
            all_layers.append(torch.nn.Linear(num_hidden, num_hidden))
            all_layers.append(torch.nn.LeakyReLU())
            all_layers.append(torch.nn.Dropout(self.dpo))
        all_layers.append(self.outputlayer)                                        # :203
        self.layers = torch.nn.Sequential(*all_layers)                             # :204

    def forward(self, x, masks=None):
        """``masks``: None (eval mode) or one (rows, hidden) 0/1 tensor per Dropout; kept values are scaled by 1 / (1 - p)."""
        k = 0
        for layer in self.layers:
            if isinstance(layer, torch.nn.Dropout):
                if masks is not None:
                    x = x * masks[k].to(x.dtype) * (1.0 / (1.0 - float(np.float32(self.dpo))))
                k += 1
            else:
                x = layer(x)
        return x


def make_model(input_dim, hidden, num_layer, p=0.0, seed=0, dtype=torch.float64):
    """nn.Linear's default initialisation in float32 (what the device holds), then cast: every dtype starts from the same values."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        model = RestatedDNN(num_layer, hidden, input_dim, p)
    return model.to(dtype)


def clone_as(model, dtype):
    other = RestatedDNN(sum(isinstance(l, torch.nn.Linear) for l in model.layers) - 2, model.inputlayer.out_features,
                        model.inputlayer.in_features, model.dpo)
    other.load_state_dict({k: v.clone() for k, v in model.state_dict().items()})
    return other.to(dtype)


def loss_and_grads(model, x, y, masks):
    """One step of :77-83 without the update: (loss, [gradient per parameter, in parameters() order])."""
    for p in model.parameters():
        p.grad = None
    dtype = model.inputlayer.weight.dtype
    out = model(torch.as_tensor(x).to(dtype), masks)
    loss = torch.nn.BCEWithLogitsLoss()(out, torch.as_tensor(y).to(dtype).unsqueeze(1))
    loss.backward()
    return float(loss.item()), [p.grad.detach().clone() for p in model.parameters()]


def adam_steps(model, x_all, y_all, batches, masks_per_step, lr):
    """The steps of :68-84 over the given batches (index arrays) with torch.optim.Adam(lr) (:461); returns the losses."""
    dtype = model.inputlayer.weight.dtype
    optim = torch.optim.Adam(model.parameters(), lr=lr)
    x_all, y_all = torch.as_tensor(x_all).to(dtype), torch.as_tensor(y_all).to(dtype)
    losses = []
    for idx, masks in zip(batches, masks_per_step):
        idx = torch.as_tensor(np.asarray(idx), dtype=torch.long)
        out = model(x_all[idx], masks)
        loss = torch.nn.BCEWithLogitsLoss()(out, y_all[idx].unsqueeze(1))
        optim.zero_grad()
        loss.backward()
        optim.step()
        losses.append(float(loss.item()))
    return losses


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def abs_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64).ravel() - np.asarray(b, dtype=np.float64).ravel()))


def within_four_times(name, device, fp32, fp64, report):
    """The bound: the device's error against the fp64 evaluation is at most 4 x the error of the fp32 torch-CPU evaluation of the
    same restatement, as relative L2 per tensor (two bits: the three-term split drops product terms below 2^-24, and the matrix
    instruction adds its k terms in another order than BLAS); a tensor whose fp64 norm is zero is compared absolutely.  Appends
    (name, device error, fp32 error, ratio) to ``report`` and returns whether the bound holds."""
    want = np.asarray(fp64, dtype=np.float64)
    if np.linalg.norm(want) == 0.0:
        e_dev, e_32 = abs_l2(device, want), abs_l2(fp32, want)
    else:
        e_dev, e_32 = rel_l2(device, want), rel_l2(fp32, want)
    ratio = e_dev / e_32 if e_32 > 0 else (0.0 if e_dev == 0 else math.inf)
    report.append((name, e_dev, e_32, ratio))
    return e_dev <= 4.0 * e_32


def seeded_rows(rows, d, seed):
    """Standardised-looking features (float32 values) and 0/1 labels."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, d)).astype(np.float32)
    y = (rng.random(rows) < 0.5).astype(np.float32)
    return x, y


# ---- exact-integer layer cases ---------------------------------------------------------------------------------------------------

INT_SLOPE, INT_P, INT_SCALE = 2.0 ** -6, 0.5, 2.0


def integer_layer_case(rows, n_in, n_out, seed):
    """Integers in [-3, 3] for x, w, bias and dy.  With slope 2^-6 and keep scale 2 every value below is a multiple of 2^-5 and every
    partial sum, in any order, stays below 2^24 of that unit, so fp32 arithmetic (and the three-term bf16 split, which is exact) gives
    the float64 result bit for bit."""
    rng = np.random.default_rng(seed)
    draw = lambda *s: rng.integers(-3, 4, size=s).astype(np.float32)  # noqa: E731
    case = dict(x=draw(rows, n_in), w=draw(n_out, n_in), b=draw(n_out), dy=draw(rows, n_out))
    unit = 2.0 ** -5
    largest = max(9 * n_in + 3,                    # |x.w + b|
                  INT_SCALE * 3 * 3 * n_out,       # |dx| <= sum over n_out of |g| |w|, |g| <= 2 * 3
                  INT_SCALE * 3 * 3 * rows,        # |dw|
                  INT_SCALE * 3 * rows)            # |db|
    assert largest / unit < 2 ** 24, (rows, n_in, n_out, largest)
    return case


def integer_layer_reference(case, mask):
    """float64 NumPy: y = mask * 2 * leaky(x w^T + b); g = dy * mask * 2 * leaky'(pre); dx = g w, dw = g^T x, db = sum g.
    leaky'(0) = slope (torch's leaky_relu_backward)."""
    x, w, b, dy = (case[k].astype(np.float64) for k in ("x", "w", "b", "dy"))
    keep = np.asarray(mask, dtype=bool)
    pre = x @ w.T + b
    y = np.where(keep, INT_SCALE * np.where(pre > 0, pre, INT_SLOPE * pre), 0.0)
    g = np.where(keep, dy * INT_SCALE * np.where(pre > 0, 1.0, INT_SLOPE), 0.0)
    return dict(y=y, dx=g @ w, dw=g.T @ x, db=g.sum(axis=0))


def same_bits(got, want):
    """Bitwise equality as float32, with -0 and +0 identified (x + 0 turns -0 into +0: a sum of zeros has no defined sign order)."""
    got = np.asarray(got, dtype=np.float32) + np.float32(0)
    want64 = np.asarray(want, dtype=np.float64)
    want = want64.astype(np.float32) + np.float32(0)
    assert np.array_equal(want.astype(np.float64), want64 + 0.0), "the reference itself is not exact in float32"
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- AUC error, end to end ---------------------------------------------------------------------------------------------------------

def hanley_mcneil_se(auc, n_pos, n_neg):
    """Hanley & McNeil, Radiology 143 (1982) 29: the standard error of an AUC from its class counts."""
    q1, q2 = auc / (2.0 - auc), 2.0 * auc * auc / (1.0 + auc)
    return math.sqrt((auc * (1.0 - auc) + (n_pos - 1) * (q1 - auc * auc) + (n_neg - 1) * (q2 - auc * auc)) / (n_pos * n_neg))


def two_gaussians(rows_each, d, shift_length, seed):
    """(features, labels): unit-covariance Gaussians, the generated one (label 1) shifted by a vector of the given length."""
    rng = np.random.default_rng(seed)
    shift = np.zeros(d)
    shift[0] = shift_length
    gen = rng.standard_normal((rows_each, d)) + shift
    real = rng.standard_normal((rows_each, d))
    return np.concatenate([gen, real]).astype(np.float32), np.concatenate([np.ones(rows_each), np.zeros(rows_each)]).astype(np.float32)


def restated_fit(model, x_scaled, labels, split, permutations, lr, batch_size, n_epochs):
    """train_and_evaluate_cls (:45-66) without dropout on the given split and per-epoch orders; returns (test logits, best_epoch)."""
    dtype = model.inputlayer.weight.dtype
    train, test, val = split
    x, y = torch.as_tensor(x_scaled).to(dtype), torch.as_tensor(labels).to(dtype)
    optim = torch.optim.Adam(model.parameters(), lr=lr)
    best, best_epoch = float("-inf"), -1
    for epoch in range(n_epochs):
        order = permutations[epoch]
        for lo in range(0, len(order), batch_size):
            idx = torch.as_tensor(order[lo:lo + batch_size], dtype=torch.long)
            loss = torch.nn.BCEWithLogitsLoss()(model(x[idx]), y[idx].unsqueeze(1))
            optim.zero_grad()
            loss.backward()
            optim.step()
        with torch.no_grad():
            pred = torch.round(torch.sigmoid(model(x[torch.as_tensor(val, dtype=torch.long)]).reshape(-1)))
            acc = float((pred == y[torch.as_tensor(val, dtype=torch.long)]).double().mean())
        if acc > best:
            best, best_epoch = acc, epoch + 1
        if acc == 1.0:
            break
    with torch.no_grad():
        return model(x[torch.as_tensor(test, dtype=torch.long)]).reshape(-1).double().numpy(), best_epoch


# ---- compute_feats -----------------------------------------------------------------------------------------------------------------

def restate_compute_feats(showers, incident_E, xmap, ymap):
    """hgcal_metrics.py:216-252 in float64 (WeightedMean: utils/plots.py:17-21; GetWidth: :212-214), before the float32 cast."""
    showers = np.asarray(showers, dtype=np.float64)
    incident_E = np.asarray(incident_E, dtype=np.float64).reshape(-1, 1)
    C = showers.shape[2]

    def weighted_mean(coord, power=1):
        ec = np.sum(showers * np.power(coord, power), axis=2)
        return np.ma.divide(ec, np.sum(showers, axis=2)).filled(0)

    def width(mean, mean2):
        return np.ma.sqrt(mean2 - mean ** 2).filled(0)

    e_layer = np.log10(np.sum(showers, axis=2) + 1e-8)
    e_ratio = np.sum(showers, axis=(1, 2)).reshape(-1, 1) / incident_E
    xv, yv = np.asarray(xmap, dtype=np.float64)[:, :C], np.asarray(ymap, dtype=np.float64)[:, :C]
    xc, yc = weighted_mean(xv), weighted_mean(yv)
    xw, yw = width(xc, weighted_mean(xv, 2)), width(yc, weighted_mean(yv, 2))
    return np.concatenate([incident_E, e_ratio, e_layer, xc, xw, yc, yw], axis=-1)
