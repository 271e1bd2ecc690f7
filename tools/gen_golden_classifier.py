"""Writes tests/golden/classifier_host.npz: what scikit-learn gives for the host bookkeeping of the classifier test
(calodiffusion_amd.classifier: standard_scale, roc_auc, IsotonicCalibrator, calibration_curve), on seeded inputs that are stored
with the results.  Needs scikit-learn (written with 1.7.2); the tests read the file and need neither scikit-learn nor SciPy.

    python tools/gen_golden_classifier.py
"""
import os

import numpy as np
from sklearn.calibration import calibration_curve
from sklearn.isotonic import IsotonicRegression
from sklearn.metrics import roc_auc_score
from sklearn.preprocessing import StandardScaler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    rng = np.random.default_rng(20240)
    out = {}

    # StandardScaler: columns of very different size and offset, one constant, one constant at a value with rounding in its mean
    x = rng.standard_normal((257, 6)) * np.array([1.0, 1e-3, 50.0, 1.0, 1.0, 1.0]) + np.array([0.0, 5.0, -300.0, 0.0, 0.0, 1e6])
    x[:, 3] = 2.5
    x[:, 4] = 0.1
    out["scaler_in"], out["scaler_out"] = x, StandardScaler().fit_transform(x)

    # roc_auc_score: heavy ties (scores on a grid of 17 values), continuous scores, and already-rounded scores
    labels = (rng.random(1500) < 0.45).astype(np.float64)
    tied = np.round((rng.standard_normal(1500) * 0.2 + 0.5 + 0.1 * labels) * 16) / 16
    cont = 1.0 / (1.0 + np.exp(-(rng.standard_normal(1500) + labels)))
    out["auc_labels"] = labels
    out["auc_tied_scores"], out["auc_tied"] = tied, roc_auc_score(labels, tied)
    out["auc_cont_scores"], out["auc_cont"] = cont, roc_auc_score(labels, cont)
    out["auc_rounded_scores"], out["auc_rounded"] = np.round(cont), roc_auc_score(labels, np.round(cont))

    # IsotonicRegression as the reference builds it (hgcal_metrics.py:180): repeated x, out-of-range queries
    ix = np.round(1.0 / (1.0 + np.exp(-rng.standard_normal(800) * 1.5)), 2) * 0.9 + 0.05
    iy = (rng.random(800) < ix).astype(np.float64)
    iso = IsotonicRegression(out_of_bounds="clip", y_min=1e-6, y_max=1.0 - 1e-6).fit(ix, iy)
    query = np.concatenate([[-1.0, 0.0, 0.05, 1.0, 2.0, 0.95], rng.random(300), ix[:50]])
    out["iso_x"], out["iso_y"], out["iso_query"], out["iso_pred"] = ix, iy, query, iso.predict(query)
    out["iso_x_knots"], out["iso_y_knots"] = iso.X_thresholds_, iso.y_thresholds_
    # ... on continuous x and non-binary y (block means are not integers over counts)
    cx, cy = rng.random(400), rng.random(400) * 0.5 + 0.5 * np.sort(rng.random(400))
    iso2 = IsotonicRegression(out_of_bounds="clip", y_min=1e-6, y_max=1.0 - 1e-6).fit(cx, cy)
    out["iso2_x"], out["iso2_y"], out["iso2_query"], out["iso2_pred"] = cx, cy, query, iso2.predict(query)
    # ... and the reference's own use: predictions rounded to 0 / 1 (:124-144)
    out["iso_pred_rounded"] = iso.predict(np.round(query.clip(0, 1)))

    # calibration_curve (:141, :149)
    pt, pp = calibration_curve(labels, cont, n_bins=10)
    out["cal_true"], out["cal_pred"] = pt, pp
    pt, pp = calibration_curve(labels, np.round(cont), n_bins=10)
    out["cal_true_rounded"], out["cal_pred_rounded"] = pt, pp

    path = os.path.join(ROOT, "tests", "golden", "classifier_host.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
