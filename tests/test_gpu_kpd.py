"""GPU: cd_kpd_sums (the three kernel sums of a batch of the kernel physics distance, Gram blocks on the fp64 matrix instruction)
and cd_column_histograms against the float64 restatement of kpd_cases.py at the bounds derived there, and
calodiffusion_amd.evaluate.kpd / KPD / separation_powers end to end."""
import numpy as np
import pytest
import torch

import fpd_cases as F
import hlf_cases as H
import kpd_cases as K
from calodiffusion_amd import evaluate as E

pytestmark = pytest.mark.gpu

B = K.BLOCK  # the edge of a workgroup's Gram block, in list positions
# both sides of a block and of a 16-row tile of the matrix instruction; (2 B + 3, 5): three block rows, the generated rows in the last
EDGE_COUNTS = [(2, 2), (15, 17), (16, 16), (B - 1, B + 1), (B, B), (2 * B + 3, 5)]


def device_sums(x, pairs, gamma, degree, stride=None, pad_index=0, first_pair=0, n_pairs=None):
    """cd_kpd_sums as the library launches it, with the raw outputs: sums (NumPy) and the status word.  `x`: NumPy or a CUDA
    tensor (used in place); `pairs`: [(real list, generated list)], sitting at batches first_pair, ... of `n_pairs` (the others
    hold 2 x row 0); entries beyond a list's count hold `pad_index`."""
    xd = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    n_pairs = n_pairs or first_pair + len(pairs)
    counts = [2] * (2 * n_pairs)
    stride = stride or max(len(l) for p in pairs for l in p)
    idx = np.full((2 * n_pairs, stride), pad_index, dtype=np.int32)
    idx[:, :2] = 0
    for k, p in enumerate(pairs):
        for side, l in enumerate(p):
            s = 2 * (first_pair + k) + side
            idx[s, :len(l)] = l
            idx[s, len(l):] = pad_index
            counts[s] = len(l)
    sums = torch.full((n_pairs, 3), 7.0, dtype=torch.float64, device="cuda")  # a sentinel: every entry is written
    status = torch.full((1,), -5, dtype=torch.int32, device="cuda")            # the call zeroes it
    E.launch_kpd_sums(xd, torch.from_numpy(idx).cuda(), counts, gamma, degree, sums, status)
    return sums.cpu().numpy()[first_pair:first_pair + len(pairs)], int(status.item())


def pairs_of(rows, counts, seed):
    flat = F.draws(rows, [c for mn in counts for c in mn], seed)
    return [(flat[2 * k], flat[2 * k + 1]) for k in range(len(counts))]


def worst_share(sums, x, pairs, gamma, degree):
    """Asserts every sum within the derived bound of the restatement; returns the largest share of the bound used."""
    worst = 0.0
    for k, (lx, ly) in enumerate(pairs):
        want, bound = K.restate_sums(x, lx, ly, gamma, degree), K.sum_bounds(x, lx, ly, gamma, degree)
        err = np.abs(sums[k] - want)
        assert np.all(err <= bound), (k, len(lx), len(ly), err.tolist(), bound.tolist())
        worst = max(worst, float(np.max(err / bound)))
    return worst


@pytest.mark.parametrize("d", [1, 3, 4, 5, 16, 17, 33, 226, 256])
def test_layout_on_integers(d):
    """Entries in [-3, 3], gamma = 2^-4, degree 4: every kernel value is a multiple of 2^-16 and every sum of them below 2^37, so
    any summation order is exact and the three sums are BITWISE the restatement's.  A misplaced C/D element, a mis-weighted
    region, a diagonal masked by row instead of by position, or K padding that reads past d is an O(1) error here.  The last
    pair holds one row at three positions of the real list and at two of the generated one."""
    x = F.integer_matrix(97, d, 100 + d)
    pairs = pairs_of(97, EDGE_COUNTS, d)
    dup_x, dup_y = pairs[3][0].copy(), pairs[3][1].copy()
    dup_x[[0, 17, 40]] = 5
    dup_y[[3, 64]] = 5
    pairs.append((dup_x, dup_y))
    gamma = 2.0 ** -4
    for lx, ly in pairs:  # the precondition of exactness, from the data: the values are not negative, so no partial sum is larger
        l = np.concatenate([lx, ly])
        assert ((x[l] @ x[l].T * gamma + 1.0) ** 4).sum() < 2.0 ** 37
    sums, status = device_sums(x, pairs, gamma, 4)
    assert status == 0
    for k, (lx, ly) in enumerate(pairs):
        want = K.restate_sums(x, lx, ly, gamma, 4)
        assert np.array_equal(sums[k], want), (d, len(lx), len(ly), sums[k].tolist(), want.tolist())


def test_duplicates_count_as_pairs():
    x = F.integer_matrix(97, 17, 1)
    lx, ly = np.array([4, 9, 4, 30, 4, 77, 12], dtype=np.int32), np.array([9, 4, 50, 51, 52], dtype=np.int32)
    sums, status = device_sums(x, [(lx, ly)], 2.0 ** -4, 4)
    want = K.restate_sums(x, lx, ly, 2.0 ** -4, 4)
    k44 = (float(x[4] @ x[4]) * 2.0 ** -4 + 1.0) ** 4
    by_row = want[0] - 6 * k44  # what masking equal ROWS would give: the six ordered pairs of the three positions of row 4 dropped
    assert status == 0 and sums[0, 0] != by_row
    assert np.array_equal(sums[0], want), ("off-diagonal pairs of equal rows are counted; only equal POSITIONS are dropped", sums[0].tolist(),
                                           want.tolist(), by_row)


@pytest.mark.parametrize("d", [7, 100, 226])
def test_general_data_against_the_restatement(d):
    """Degree 4 and gamma = 1 / d, counts on both sides of the block edge and up to 1500; at d = 100 degrees 1 and 3 too."""
    x = F.feature_like(3000, d, d)
    pairs = pairs_of(3000, [(B - 1, B + 1), (B + 1, B - 1), (B, B), (2, 2 * B + 1), (1500, 700)], 2000 + d)
    sums, status = device_sums(x, pairs, 1.0 / d, 4)
    assert status == 0
    worst = worst_share(sums, x, pairs, 1.0 / d, 4)
    print(f"d = {d}, degree 4: worst share of the sum bound {worst:.3g}")
    if d == 100:
        for degree in (1, 3):
            sums, status = device_sums(x, pairs[:4], 1.0 / d, degree)
            assert status == 0
            print(f"d = {d}, degree {degree}: worst share of the sum bound {worst_share(sums, x, pairs[:4], 1.0 / d, degree):.3g}")


def test_determinism():
    d = 50
    x = F.feature_like(2500, d, 3)
    pairs = pairs_of(2500, [(700, 300), (B + 5, 2 * B), (33, 900)], 4)
    first, status = device_sums(x, pairs, 1.0 / d, 4)
    assert status == 0 and not np.any(first == 7.0)
    again, _ = device_sums(x, pairs, 1.0 / d, 4)
    assert np.array_equal(first, again)
    alone, _ = device_sums(x, pairs[:1], 1.0 / d, 4)
    among, _ = device_sums(x, pairs[:1], 1.0 / d, 4, stride=1201, first_pair=2, n_pairs=5)  # number 3 of 5, another idx_stride
    assert np.array_equal(alone, first[:1]) and np.array_equal(among, first[:1])
    far, _ = device_sums(x, pairs[1:2], 1.0 / d, 4, first_pair=33, n_pairs=35)  # more batches than one launch takes counts for
    assert np.array_equal(far, first[1:2])


def _nan_framed(x):
    """x as a view big[8 : 8 + rows] of a larger NaN-filled allocation."""
    big = torch.full((x.shape[0] + 16, x.shape[1]), float("nan"), dtype=torch.float64, device="cuda")
    big[8:8 + x.shape[0]] = torch.from_numpy(x).cuda()
    return big[8:8 + x.shape[0]]


def test_padding_is_never_read():
    d, rows = 33, 500
    x = F.feature_like(rows, d, 5)
    pairs = pairs_of(rows, [(37, 2), (B + 1, 70), (3, 200)], 6)
    plain, _ = device_sums(x, pairs, 1.0 / d, 4)
    framed, status = device_sums(_nan_framed(x), pairs, 1.0 / d, 4, stride=300, pad_index=rows + 3)  # entries at k >= counts[s]: NaN rows
    assert status == 0 and np.isfinite(framed).all()
    assert np.array_equal(plain, framed)


@pytest.mark.parametrize("bad", [-1, "rows"])
def test_index_guard(bad, monkeypatch):
    """The bad index lands inside the NaN frame, never outside the allocation: a broken guard shows as a wrong result."""
    d, rows = 20, 400
    x = F.feature_like(rows, d, 9)
    view = _nan_framed(x)
    pairs = pairs_of(rows, [(100, 90), (150, 200), (B, 3)], 10)
    good, status = device_sums(view, pairs, 1.0 / d, 4)
    assert status == 0
    broken = [(a.copy(), b.copy()) for a, b in pairs]
    broken[1][1][130] = rows if bad == "rows" else bad  # set 3 (the generated list of batch 1), position 130
    sums, status = device_sums(view, broken, 1.0 / d, 4)
    assert status == 1 + 3 * 200 + 130
    assert np.isnan(sums[1]).all()
    assert np.array_equal(sums[0], good[0]) and np.array_equal(sums[2], good[2])
    flat = [l for p in broken for l in p]
    with pytest.raises(ValueError, match=rf"kpd: set 3, position 130 holds a row index outside \[0, {rows}\)"):
        E.kernel_sums(view, flat)
    # kpd() itself, handed such a list by its draw
    lists = E.kpd_index_lists(200, 200, 2, 50, 42)
    lists[1, 0, 7] = 400 if bad == "rows" else -1  # the real list of batch 1 (set 2); 400 = the rows of kpd's joint matrix
    monkeypatch.setattr(E, "kpd_index_lists", lambda *a, **k: lists.copy())
    with pytest.raises(ValueError, match=r"kpd: set 2, position 7 holds a row index outside \[0, 400\)"):
        E.kpd(x[:200], x[200:], num_batches=2, batch_size=50)
    monkeypatch.undo()
    assert np.array_equal(E.kernel_sums(view, [l for p in pairs for l in p]), good)  # the next clean call works
    assert np.isfinite(E.kpd(x[:200], x[200:], num_batches=2, batch_size=50)).all()


def _normal_pair(shift):
    rng = np.random.default_rng(32)
    real, gen = rng.normal(size=(3000, 20)), rng.normal(size=(3000, 20))
    gen[:, 0] += shift
    return real, gen


_KW = dict(num_batches=5, batch_size=700, seed=42)


@pytest.mark.parametrize("normalise", [True, False])
def test_kpd_end_to_end(normalise):
    """D = 20, 3000 standard-normal rows: no shift and a shift of 1.0 in one coordinate, against the restatement on the same draws
    (which gives 3.5e-4 +- 2.7e-4 and 1.069e-2 +- 3.5e-4 normalised, 1.49e-2 +- 6.3e-3 and 0.240 +- 9.3e-3 as the data are), within
    the sum bound carried through the estimate (kpd_cases.py).  The two values differ by more than their summed errors, so a
    metric that returns a constant fails."""
    lists = E.kpd_index_lists(3000, 3000, 5, 700, 42)
    got = {}
    for shift in (0.0, 1.0):
        real, gen = _normal_pair(shift)
        value, err = E.kpd(real, gen, normalise=normalise, **_KW)
        want, want_err, bound = K.restate_kpd(real, gen, lists, normalise, with_bound=True)
        print(f"normalise {normalise}, shift {shift}: kpd = {value!r} +- {err!r}, restatement {want!r} +- {want_err!r}, "
              f"difference {value - want:.3e} {err - want_err:.3e}, bound {bound:.3e}")
        assert abs(value - want) <= bound and abs(err - want_err) <= bound
        assert E.kpd(torch.from_numpy(real).cuda(), torch.from_numpy(gen).cuda(), normalise=normalise, **_KW) == (value, err)
        got[shift] = (value, err)
    assert got[1.0][0] - got[0.0][0] > got[1.0][1] + got[0.0][1]


def test_kpd_warns_about_small_sets_and_refuses_mismatched_ones():
    x = np.random.default_rng(1).normal(size=(300, 5))
    with pytest.warns(RuntimeWarning, match="fewer than batch_size"):
        value, err = E.kpd(x, x[:250], num_batches=2, batch_size=280)  # with replacement: it still runs
    assert np.isfinite(value) and np.isfinite(err)
    with pytest.raises(ValueError, match="5 real and 4 generated features"):
        E.kpd(x, x[:, :4], **_KW)
    with pytest.raises(ValueError, match="has no rows"):
        E.kpd(x, x[:0], **_KW)
    with pytest.raises(ValueError, match="the device kernel takes 1 to 256"):
        E.kpd(np.zeros((10, 257)), np.zeros((10, 257)), **_KW)
    with pytest.raises(ValueError, match="batch_size must be at least 2"):
        E.kpd(x, x, num_batches=2, batch_size=1)
    with pytest.raises(ValueError, match="num_batches must be positive"):
        E.kpd(x, x, num_batches=0, batch_size=10)
    with pytest.raises(ValueError, match="they come in pairs"):
        E.kernel_sums(x, [[0, 1], [1, 2], [2, 3]])
    with pytest.raises(ValueError, match="a kernel sum needs at least 2 rows"):
        E.kernel_sums(x, [[0, 1], [1]])


class _StubModel:
    """What KPD.__call__ uses of a trained model: config["NSTEPS"] and generate()."""

    def __init__(self, showers, energies):
        self.config = {"NSTEPS": 7}
        self.showers, self.energies, self.calls = showers, energies, []

    def generate(self, data_loader, sample_steps, sample_offset):
        self.calls.append((sample_steps, sample_offset, data_loader))
        return self.showers, self.energies


def test_kpd_call():
    geo = H.Geometry.of_fixture("small")
    V, n = geo.edges[-1], 600
    rng = np.random.default_rng(41)
    ref_showers, gen_showers = H.seeded_showers(V, n, 42), H.seeded_showers(V, n, 43) * np.float32(1.2)
    ref_energy, gen_energy = rng.uniform(1e3, 1e6, (n, 1)), rng.uniform(1e3, 1e6, (n, 1))
    loader = [(torch.from_numpy(ref_energy[lo:lo + 200]), None, torch.from_numpy(ref_showers[lo:lo + 200])) for lo in range(0, n, 200)]
    model = _StubModel(gen_showers, gen_energy)
    kpd = E.KPD(H.binning("small"), "electron", num_batches=3, batch_size=200)
    value = kpd(model, loader, {})
    assert model.calls == [(7, 0, loader)]
    # the restatement from the same showers: the class's own features, nan_to_num, the loader's showers as the real set
    feats = []
    for showers, energy in ((ref_showers, ref_energy), (gen_showers, gen_energy)):
        hlf = E.HighLevelFeatures("electron", filename=H.binning("small"))
        hlf.CalculateFeatures(showers)
        feats.append(np.nan_to_num(hlf.feature_matrix(energy)))
        hlf.close()
    want, _, bound = K.restate_kpd(feats[0], feats[1], E.kpd_index_lists(n, n, 3, 200, 42), with_bound=True)
    print(f"KPD = {value!r}, restatement {want!r}, difference {value - want:.3e}, bound {bound:.3e}, {feats[0].shape[1]} features")
    assert isinstance(value, float) and abs(value - want) <= bound
    empty = [(torch.zeros((0, 1), dtype=torch.float64), None, torch.zeros((0, V)))]
    with pytest.raises(E.FDPCalculationError, match="no rows"):
        kpd(_StubModel(np.zeros((0, V), dtype=np.float32), np.zeros((0, 1))), empty, {})
    kpd.hlf.close()
    kpd.reference_hlf.close()


# ---- histograms and separation powers ---------------------------------------------------------------------------------------

def _histogram_pair(d, seed):
    """Real and generated sets of 5000 rows: the generated one scaled by 1.2, so values fall outside the real range on both
    sides; rows 0 and 1 of the real set ARE the column minima and maxima; every edge of every column is planted in both sets."""
    both = F.feature_like(10000, d, seed)
    real, gen = both[:5000].copy(), both[5000:] * 1.2
    real[0], real[1] = real.min(axis=0), real.max(axis=0)
    edges = K.restate_edges(real)
    real[2:52], gen[100:150] = edges.T, edges.T
    assert np.array_equal(K.restate_edges(real), edges)
    return real, gen, edges


@pytest.mark.parametrize("d", [1, 33, 64, 65, 226])
def test_histograms_equal_numpy(d):
    """A workgroup counts 64 columns: d = 64 and 65 sit on both sides of one group, 226 is three groups and a part."""
    real, gen, edges = _histogram_pair(d, 300 + d)
    z = np.concatenate([real, gen])
    # the generated range starts at row 5000 and the third at row 37: neither a multiple of a workgroup's 256 rows, nor their ends
    got = E.column_histograms(z, edges, [(0, 5000), (5000, 5000), (37, 4901)])
    for k, block in enumerate((real, gen, z[37:37 + 4901])):
        want = K.restate_histograms(block, edges)
        assert np.array_equal(got[k], want), (d, k, np.argwhere(got[k] != want)[:8].tolist())
    assert got[0].sum() == 5000 * d and got[1].sum() < 5000 * d  # every real value is inside its own range; generated ones are not
    assert np.array_equal(E.column_histograms(torch.from_numpy(real).cuda(), edges)[0], got[0])


def test_histogram_edges_need_not_be_even():
    """The correction runs against the edges as given: uneven ones, a repeated one and a column of equal edges."""
    x = F.feature_like(1000, 3, 8)
    edges = np.stack([np.sort(np.random.default_rng(j).choice(x[:, j], size=12, replace=False)) for j in range(3)])
    edges[1, 5] = edges[1, 4]
    edges[2, :] = x[17, 2]
    got = E.column_histograms(x, edges)[0]
    assert np.array_equal(got, K.restate_histograms(x, edges)) and got[2, -1] >= 1


@pytest.mark.parametrize("d", [1, 33, 226])
def test_separation_powers_against_the_restatement(d):
    real, gen, _ = _histogram_pair(d, 500 + d)
    got, want = E.separation_powers(real, gen), K.restate_separation_powers(real, gen)
    print(f"d = {d}: largest difference {np.max(np.abs(got - want)):.3e}, total {got.sum():.6g}")
    assert got.shape == (d,) and got.dtype == np.float64 and np.all(np.abs(got - want) <= 1e-12)
    assert abs(E.separation_power_total(real, gen) - want.sum()) <= 1e-12 * d
    assert np.array_equal(E.separation_powers(torch.from_numpy(real).cuda(), torch.from_numpy(gen).cuda()), got)


def test_separation_powers_discriminate():
    """Column 0 is 0.057 with a shift of 0.5 and 0.005 without; columns 1 and 2 are 0.0079 and 0.0063 in both runs."""
    (real, gen0), (_, gen1) = _normal_pair(0.0), _normal_pair(0.5)
    s0, s1 = E.separation_powers(real, gen0), E.separation_powers(real, gen1)
    print(f"column 0: {s0[0]:.4g} -> {s1[0]:.4g}; columns 1, 2: {s0[1]:.4g}, {s0[2]:.4g}")
    assert s1[0] - s0[0] > 0.03
    assert np.array_equal(s0[1:], s1[1:])
    assert np.all(np.abs(s0 - K.restate_separation_powers(real, gen0)) <= 1e-12)


def test_separation_powers_edge_cases():
    real, gen, _ = _histogram_pair(4, 9)
    real[:, 2] = 1.5  # all equal: nan, as the reference's arithmetic gives
    got = E.separation_powers(real, gen)
    assert np.isnan(got[2]) and np.isfinite(got[[0, 1, 3]]).all()
    assert np.isnan(E.separation_power_total(real, gen))
    assert np.all(np.abs(E.separation_powers(real, gen, bins=7)[[0, 1, 3]] - K.restate_separation_powers(real, gen, bins=7)[[0, 1, 3]]) <= 1e-12)
    with pytest.raises(ValueError, match=r"at most bins = 64"):
        E.separation_powers(real, gen, bins=65)
    assert np.all(np.abs(E.separation_powers(real, gen, bins=64)[[0, 1, 3]] - K.restate_separation_powers(real, gen, bins=64)[[0, 1, 3]]) <= 1e-12)
    with pytest.raises(ValueError, match="bins must be at least 2"):
        E.separation_powers(real, gen, bins=1)
    with pytest.raises(ValueError, match="4 real and 3 generated features"):
        E.separation_powers(real, gen[:, :3])
    with pytest.raises(ValueError, match="has no rows"):
        E.separation_powers(real, gen[:0])
