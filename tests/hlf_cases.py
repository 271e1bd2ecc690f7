"""Shared by test_hlf_host.py and test_gpu_hlf.py: the fixture of the reference's HighLevelFeatures (tests/golden/hlf.npz, written
by tools/gen_golden_hlf.py), a plain NumPy float64 restatement of cd_hlf_compute's eight values, and the two sets of bounds.

Bounds against the REFERENCE (`assert_within_reference_bounds`).  The reference sums float32 showers pairwise in float32 and
divides its float64 products' sums by that float32 `energy.sum()`, so its own rounding is float32-sized.  With n the voxels of the
layer (all voxels for E_tot) and delta = (log2 n + 2) 2^-24:
    E_layers, E_tot   rtol delta
    centres           atol 2 delta max|c|
    width^2           atol 4 delta max c^2
Variances are compared, not widths: for a one-voxel layer the reference gives exactly 0, and sqrt turns a 1e-16 relative residue
of another summation into 1e-8.

Bounds against the RESTATEMENT (`assert_within_fp64_bounds`): both are float64 sums of the same terms, only the order differs, so
|d| <= 64 n 2^-53 x scale with scale = the shower's layer energy, max|c| and max c^2; hit counts and brightest voxels are exact.
"""
import os

import numpy as np

from conftest import GOLD, gold

TAGS = {  # tag: (binning file, particle)
    "small": ("binning_reg_small.xml", "electron"),
    "wide": ("binning_reg_wide.xml", "electron"),
    "photon": ("binning_ds1_synthetic.xml", "photon"),
    "pion": ("binning_ds0_synthetic.xml", "pion"),
}
E, EC_ETA, EC_PHI, VAR_ETA, VAR_PHI, W_ETA, W_PHI, MAX = range(8)
_fixture = None


def binning(tag):
    return os.path.join(GOLD, TAGS[tag][0])


def fixture(tag):
    """{name: array} of one geometry of hlf.npz (loaded once, never written to)."""
    global _fixture
    if _fixture is None:
        z = gold("hlf")
        _fixture = {k: z[k] for k in z.files}
        for v in _fixture.values():
            v.setflags(write=False)
    return {k[len(tag) + 1:]: v for k, v in _fixture.items() if k.startswith(tag + ".")}


class Geometry:
    """What the restatement needs of a binning: offsets, positions, layers with voxels, layers with centres."""

    def __init__(self, bin_edges, eta, phi, relevant, centres):
        self.edges = [int(b) for b in bin_edges]
        self.eta, self.phi = np.asarray(eta, dtype=np.float64), np.asarray(phi, dtype=np.float64)
        self.relevant, self.centres = [int(l) for l in relevant], [int(l) for l in centres]

    @classmethod
    def of_fixture(cls, tag):
        f = fixture(tag)
        return cls(f["bin_edges"], f["eta"], f["phi"], f["relevantLayers"], f["centre_layers"])

    def span(self, l):
        return self.edges[l], self.edges[l + 1]


def restate(showers, geo, threshold=0.0):
    """(B, R, 8) float64 records and (B, R) int32 hit counts of float32 showers, as include/calodiff.h defines them."""
    x = np.asarray(showers, dtype=np.float32)
    rec = np.zeros((x.shape[0], len(geo.relevant), 8), dtype=np.float64)
    hits = np.zeros((x.shape[0], len(geo.relevant)), dtype=np.int32)
    for k, l in enumerate(geo.relevant):
        lo, hi = geo.span(l)
        e = x[:, lo:hi].astype(np.float64)
        tot = e.sum(axis=-1)
        rec[:, k, E] = tot
        rec[:, k, MAX] = x[:, lo:hi].max(axis=-1)
        hits[:, k] = (x[:, lo:hi] > np.float32(threshold)).sum(axis=-1)
        if l in geo.centres:
            for c, (i_ec, i_var, i_w) in ((geo.eta[lo:hi], (EC_ETA, VAR_ETA, W_ETA)), (geo.phi[lo:hi], (EC_PHI, VAR_PHI, W_PHI))):
                ec = (c * e).sum(axis=-1) / (tot + 1e-16)
                var = np.maximum((c * c * e).sum(axis=-1) / (tot + 1e-16) - ec ** 2, 0.0)
                rec[:, k, i_ec], rec[:, k, i_var], rec[:, k, i_w] = ec, var, np.sqrt(var)
    return rec, hits


def total_energy(rec):
    """E_tot as the class defines it: the layer energies in layer order, in float64."""
    tot = np.zeros(rec.shape[0], dtype=np.float64)
    for k in range(rec.shape[1]):
        tot += rec[:, k, E]
    return tot


def _delta(n):
    return (np.log2(n) + 2.0) * 2.0 ** -24


def assert_within_reference_bounds(rec, e_tot, tag, rows=slice(None)):
    """records (B, R, 8) and E_tot (B,) of the fixture's showers[rows] against the reference's features."""
    f, geo = fixture(tag), Geometry.of_fixture(tag)
    worst = {}

    def check(name, got, want, bound):
        err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
        worst[name] = max(worst.get(name, 0.0), float(np.max(err / np.maximum(bound, 1e-300))))
        assert np.all(err <= bound), (tag, name, float(err.max()), float(np.max(bound)))

    check("E_tot", e_tot, f["E_tot"][rows], _delta(geo.edges[-1]) * np.abs(f["E_tot"][rows].astype(np.float64)))
    for k, l in enumerate(geo.relevant):
        lo, hi = geo.span(l)
        want = f["E_layers"][rows][:, k].astype(np.float64)
        check(f"E_layers[{l}]", rec[:, k, E], want, _delta(hi - lo) * np.abs(want))
        if l not in geo.centres:
            assert not rec[:, k, EC_ETA:MAX].any(), (tag, l)
            continue
        j = geo.centres.index(l)
        for c, i_ec, i_var, ec_name, w_name in ((geo.eta[lo:hi], EC_ETA, VAR_ETA, "EC_etas", "width_etas"),
                                                (geo.phi[lo:hi], EC_PHI, VAR_PHI, "EC_phis", "width_phis")):
            cmax = float(np.abs(c).max())
            check(f"{ec_name}[{l}]", rec[:, k, i_ec], f[ec_name][rows][:, j], 2.0 * _delta(hi - lo) * cmax)
            check(f"{w_name}[{l}]^2", rec[:, k, i_var], f[w_name][rows][:, j] ** 2, 4.0 * _delta(hi - lo) * cmax ** 2)
    return worst


def assert_within_fp64_bounds(rec, hits, want_rec, want_hits, geo):
    """device records against the restatement's: the summation order in float64 is the only difference."""
    assert rec.shape == want_rec.shape and hits.shape == want_hits.shape
    assert rec.dtype == np.float64 and np.array_equal(hits, want_hits)
    assert np.array_equal(rec[:, :, MAX], want_rec[:, :, MAX])
    for k, l in enumerate(geo.relevant):
        lo, hi = geo.span(l)
        eps = 64.0 * (hi - lo) * 2.0 ** -53
        assert np.all(np.abs(rec[:, k, E] - want_rec[:, k, E]) <= eps * want_rec[:, k, E]), (l, "E")
        if l not in geo.centres:
            assert not rec[:, k, EC_ETA:MAX].any(), l
            continue
        for c, i_ec, i_var, i_w in ((geo.eta[lo:hi], EC_ETA, VAR_ETA, W_ETA), (geo.phi[lo:hi], EC_PHI, VAR_PHI, W_PHI)):
            cmax = float(np.abs(c).max())
            assert np.all(np.abs(rec[:, k, i_ec] - want_rec[:, k, i_ec]) <= eps * cmax), (l, i_ec)
            assert np.all(np.abs(rec[:, k, i_var] - want_rec[:, k, i_var]) <= eps * cmax ** 2), (l, i_var)
            # the width is the correctly rounded root of the record's own variance, give or take an ulp
            assert np.all(np.abs(rec[:, k, i_w] - np.sqrt(rec[:, k, i_var])) <= 2.0 ** -51 * rec[:, k, i_w]), (l, i_w)


def write_binning(path, layers, particle="electron"):
    """A binning file with one layer of n_alpha x n_r voxels per (n_alpha, n_r) of `layers`, radial edges 0, 1.5, 3, ..."""
    rows = [f'    <Layer id="{l}" r_edges="{",".join(repr(1.5 * k) for k in range(n_r + 1))}" n_bin_alpha="{n_alpha}"/>'
            for l, (n_alpha, n_r) in enumerate(layers)]
    with open(path, "w") as fh:
        fh.write("\n".join(['<?xml version="1.0" encoding="UTF-8"?>', "<Bins>", f'  <Bin pid="11" etaMin="0" etaMax="130" name="{particle}">',
                            *rows, "  </Bin>", "</Bins>", ""]))


def seeded_showers(V, B, seed):
    """About 30 % occupancy, values over six decades, float32; row 0 empty (when B > 1)."""
    rng = np.random.default_rng(seed)
    x = np.where(rng.random((B, V)) < 0.3, 10.0 ** rng.uniform(-3.0, 3.0, (B, V)), 0.0).astype(np.float32)
    if B > 1:
        x[0] = 0.0
    return x
