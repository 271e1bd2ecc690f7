"""GPU: cd_hlf_compute through calodiffusion_amd.hlf.HighLevelFeatures against the reference's own features (fixture of
tools/gen_golden_hlf.py, at the host test's float32-sized bounds) and against the float64 restatement of hlf_cases.py, where only
the order of the float64 sums differs (|d| <= 64 n 2^-53 x scale; hit counts and brightest voxels exact)."""
import numpy as np
import pytest
import torch

import hlf_cases as H
from calodiffusion_amd.hlf import HighLevelFeatures

pytestmark = pytest.mark.gpu

_classes = {}


@pytest.fixture(scope="module", autouse=True)
def _free_the_device_tables():
    yield
    for hlf in _classes.values():
        hlf.close()
    _classes.clear()


def hlf_of(tag):
    if tag not in _classes:
        _classes[tag] = HighLevelFeatures(H.TAGS[tag][1], filename=H.binning(tag))
    return _classes[tag]


def records(hlf, data, **kw):
    """cd_hlf_compute's records and hit counts as the class gets them."""
    return hlf._records(data, data.shape[0], float(kw.get("threshold", 0.0)), int(kw.get("chunk", 16384)))


@pytest.mark.parametrize("tag", list(H.TAGS))
def test_fixture_showers_against_the_reference(tag):
    f, hlf = H.fixture(tag), hlf_of(tag)
    hlf.CalculateFeatures(f["showers"])
    geo = H.Geometry.of_fixture(tag)
    rec = np.zeros((8, len(geo.relevant), 8))
    for k, l in enumerate(geo.relevant):
        rec[:, k, H.E] = hlf.E_layers[l]
        if l in geo.centres:
            rec[:, k, H.EC_ETA], rec[:, k, H.EC_PHI] = hlf.EC_etas[l], hlf.EC_phis[l]
            rec[:, k, H.VAR_ETA], rec[:, k, H.VAR_PHI] = hlf.width_etas[l] ** 2, hlf.width_phis[l] ** 2
    assert list(hlf.EC_etas) == geo.centres == list(hlf.width_phis)
    worst = H.assert_within_reference_bounds(rec, hlf.E_tot, tag)
    print(tag, "worst share of the bound:", round(max(worst.values()), 3))


@pytest.mark.parametrize("threshold", [0.0, 1.0])
@pytest.mark.parametrize("tag", list(H.TAGS))
def test_fixture_showers_against_the_restatement(tag, threshold):
    f, geo = H.fixture(tag), H.Geometry.of_fixture(tag)
    rec, hits = records(hlf_of(tag), f["showers"], threshold=threshold)
    want_rec, want_hits = H.restate(f["showers"], geo, threshold)
    H.assert_within_fp64_bounds(rec, hits, want_rec, want_hits, geo)


@pytest.mark.parametrize("tag, B", [("wide", 1), ("wide", 7), ("pion", 7)])
def test_odd_batches(tag, B):
    """wide: 900-voxel layers, four strides a lane and a tail; pion: 5-, 3- and 110-voxel layers in a 323-float row."""
    geo = H.Geometry.of_fixture(tag)
    x = H.seeded_showers(geo.edges[-1], B, 11 + B)
    rec, hits = records(hlf_of(tag), x)
    H.assert_within_fp64_bounds(rec, hits, *H.restate(x, geo), geo)


def test_layer_sizes_around_every_switch(tmp_path):
    """16 lanes sum a layer, four voxels ahead each: layers of 16 / 17 voxels (a lane's first second voxel), 63 / 64 / 65 (the
    first full trip of four strides), 256 / 258 / 260 (whole trips and what is left over), and one voxel without centres; five
    showers, so one lane group of the wave is full, one holds a single shower and two are idle."""
    path = str(tmp_path / "binning_switches.xml")
    H.write_binning(path, [(16, 16), (6, 43), (2, 8), (17, 1), (13, 5), (8, 8), (7, 9), (1, 1), (4, 65)])
    hlf = HighLevelFeatures("electron", filename=path)
    assert list(np.diff(hlf.bin_edges)) == [256, 258, 16, 17, 65, 64, 63, 1, 260] and hlf.layers_with_centres == [0, 1, 2, 3, 4, 5, 6, 8]
    geo = H.Geometry(hlf.bin_edges, np.concatenate(hlf.eta_all_layers), np.concatenate(hlf.phi_all_layers), hlf.relevantLayers,
                     hlf.layers_with_centres)
    x = H.seeded_showers(geo.edges[-1], 5, 21)
    for threshold in (0.0, 1.0):
        rec, hits = records(hlf, x, threshold=threshold)
        H.assert_within_fp64_bounds(rec, hits, *H.restate(x, geo, threshold), geo)


def test_chunks_and_repeats_are_bitwise_equal():
    geo = H.Geometry.of_fixture("pion")
    x = H.seeded_showers(geo.edges[-1], 12, 5)
    hlf = hlf_of("pion")
    rec, hits = records(hlf, x)
    again = records(hlf, x)
    assert np.array_equal(rec, again[0]) and np.array_equal(hits, again[1])
    chunked = records(hlf, x, chunk=5)  # 5 + 5 + 2: rows at other addresses, alignments and batch sizes
    assert np.array_equal(rec, chunked[0]) and np.array_equal(hits, chunked[1])
    hlf.CalculateFeatures(x)
    whole = (hlf.E_tot.copy(), {l: v.copy() for l, v in hlf.width_etas.items()}, {l: v.copy() for l, v in hlf.n_hits.items()})
    hlf.CalculateFeatures(x, chunk=5)
    assert np.array_equal(whole[0], hlf.E_tot)
    assert all(np.array_equal(whole[1][l], hlf.width_etas[l]) for l in whole[1])
    assert all(np.array_equal(whole[2][l], hlf.n_hits[l]) for l in whole[2])


def test_device_tensor_equals_host_array():
    geo = H.Geometry.of_fixture("photon")
    x = H.seeded_showers(geo.edges[-1], 9, 6)
    hlf = hlf_of("photon")
    rec, hits = records(hlf, x)
    dev = torch.from_numpy(x).cuda()
    rec_d, hits_d = records(hlf, dev)
    assert np.array_equal(rec, rec_d) and np.array_equal(hits, hits_d)
    assert np.array_equal(dev.cpu().numpy(), x)  # read in place, not written
    rec_64, _ = records(hlf, dev.double())  # cast to float32, as at every entry point
    assert np.array_equal(rec, rec_64)
    hlf.close()  # the tables are per device and come back on the next call
    assert not hlf._handles and np.array_equal(rec, records(hlf, dev)[0]) and list(hlf._handles) == [dev.device.index]
    with pytest.raises(ValueError, match=r"expected showers of shape \(N, 368\)"):
        hlf.CalculateFeatures(dev[:, :367])


def test_waves_make_several_trips_of_the_capped_grid(tmp_path):
    """The grid is capped at 16 384 workgroups of 64 showers a trip: with 45 layers that is 364 slices, 23 296 showers, and a wave
    loops beyond that -- the path of every evaluation-size call (100 000 Dataset-2 showers are five trips).  50 003 showers of 45
    small layers (150 floats a row, 30 MB): two full trips and a third that ends inside a workgroup, a wave and a lane group."""
    path = str(tmp_path / "binning_trips.xml")
    H.write_binning(path, [(2, 2), (1, 3), (3, 1)] * 15)
    hlf = HighLevelFeatures("electron", filename=path)
    assert len(hlf.relevantLayers) == 45 and hlf.total_voxels == 150
    geo = H.Geometry(hlf.bin_edges, np.concatenate(hlf.eta_all_layers), np.concatenate(hlf.phi_all_layers), hlf.relevantLayers,
                     hlf.layers_with_centres)
    B = 50003
    assert 2 * 64 * (16384 // 45) < B < 3 * 64 * (16384 // 45) and B % 64 == 19
    x = H.seeded_showers(150, B, 31)
    x[-1, :] = np.arange(1, 151, dtype=np.float32)  # the last shower is not empty
    rec, hits = records(hlf, torch.from_numpy(x).cuda())
    H.assert_within_fp64_bounds(rec, hits, *H.restate(x, geo), geo)
    hlf.close()


def test_batch_beyond_a_grid_dimension():
    """70 001 showers of the photon file in one call (103 MB): more (shower, layer) pairs than a grid dimension of 65 535 (one
    trip per wave; the capped grid's loop is test_waves_make_several_trips_of_the_capped_grid)."""
    geo = H.Geometry.of_fixture("photon")
    B, V = 70001, geo.edges[-1]
    block = H.seeded_showers(V, 4096, 9)
    x = np.concatenate([np.roll(block, i, axis=1) for i in range(B // 4096 + 1)])[:B]  # every block another alignment of the data
    rec, hits = records(hlf_of("photon"), torch.from_numpy(x).cuda())
    H.assert_within_fp64_bounds(rec, hits, *H.restate(x, geo), geo)
