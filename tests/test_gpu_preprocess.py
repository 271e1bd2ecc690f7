"""GPU (MI355X): the forward pre-processing on the device (cd_preprocess, calodiffusion_amd.preprocess) against the
reference's own preprocess_shower / DataLoaderCaloChall outputs (tests/golden/preprocess.npz, tools/gen_preprocess_golden.py)."""
import numpy as np
import pytest
import torch

from conftest import gold, rel_l2
from helpers import per_layer_worst

pytestmark = pytest.mark.gpu

SCALE = np.float32(0.001)  # DataLoaderCaloChall's shower_scale: the fixture's MeV -> the loader's GeV
CASES = [("d2", "dataset2", True), ("d2", "dataset2", False), ("d3", "dataset3", True)]


def _cfg(name, logE=True):
    from calodiffusion_amd.configs import load_config
    return dict(load_config(name), logE=logE)


@pytest.mark.parametrize("tag,name,logE", CASES)
def test_preprocess_matches_the_reference(tag, name, logE):
    """preprocess_shower (reference signature, numpy in / numpy out) and Preprocess (device tensors) against the reference:
    showers, layerE and energies each within rel-L2 1e-5 (the bar test_gpu_parity.py holds cd_reverse_norm to) and every
    (shower, layer) row of layerE and of the voxel tensor within 3e-5 (the per-row bar of the HGCal ReverseNorm case).  Every
    shower and every element is compared."""
    from calodiffusion_amd.preprocess import Preprocess, preprocess_shower
    g, cfg = gold("preprocess"), _cfg(name, logE)
    D = cfg["SHAPE_PAD"][2]
    raw, e = g[f"{tag}.showers"], g[f"{tag}.incident_energies"]
    want, want_l = g[f"{tag}.data"], (g[f"{tag}.layerE"] if f"{tag}.layerE" in g.files else None)
    want_E = g[f"{tag}.E"] if logE else g[f"{tag}.E_lin"]

    got, got_l = preprocess_shower(raw * SCALE, e * SCALE, cfg["SHAPE_PAD"], "", cfg["SHOWERMAP"], dataset_num=cfg["DATASET_NUM"],
                                   orig_shape=False, ecut=cfg["ECUT"], max_deposit=cfg["MAXDEP"])
    assert got.shape == want.shape and got.dtype == np.float32 and np.isfinite(got).all()
    e_all, e_row = rel_l2(got, want), per_layer_worst(got.reshape(8, D, -1), want.reshape(8, D, -1))
    print(f"[{tag} logE={logE}] voxels: rel L2 {e_all:.3e}, worst (shower, layer) row {e_row:.3e}")
    assert e_all < 1e-5 and e_row < 3e-5
    if want_l is None:
        assert got_l is None
    else:
        assert got_l.shape == want_l.shape == (8, D + 1) and got_l.dtype == np.float32
        l_all, l_row = rel_l2(got_l, want_l), per_layer_worst(got_l[:, :, None], want_l[:, :, None])
        print(f"[{tag} logE={logE}] layerE: rel L2 {l_all:.3e}, worst (shower, layer) element {l_row:.3e}")
        assert l_all < 1e-5 and l_row < 3e-5

    E, layers, data = Preprocess(cfg)(raw, e)
    assert E.is_cuda and data.is_cuda and E.shape == (8, 1) and data.shape == (8, 1) + tuple(cfg["SHAPE_PAD"][2:])
    assert E.dtype == data.dtype == torch.float32
    err_E = rel_l2(E.cpu().numpy(), want_E)
    print(f"[{tag} logE={logE}] E: rel L2 {err_E:.3e}")
    assert err_E < 1e-5
    # the loader's scaling happens inside the same call: the same float32 products, so the same bits
    assert np.array_equal(data.cpu().numpy().reshape(8, -1), got)
    assert (layers is None and got_l is None) or np.array_equal(layers.cpu().numpy(), got_l)


# The reference's own round trip, ReverseNormCaloChall(preprocess_shower(raw)) against raw on the fixture inputs (numpy, CPU;
# printed by tools/gen_preprocess_golden.py), energy-weighted rel L2:  d2 5.482e-07,  d3 3.734e-07.
REFERENCE_ROUND_TRIP = {"d2": 5.482e-07, "d3": 3.734e-07}


@pytest.mark.parametrize("tag,name", [("d2", "dataset2"), ("d3", "dataset3")])
def test_round_trip_through_reverse_norm(tag, name):
    """ReverseNorm(Preprocess(raw)) against raw.  The map is not exactly invertible (logit's alpha, the ECUT threshold), so the
    bar is the reference's own round trip on the same inputs (d2 5.482e-07, d3 3.734e-07: REFERENCE_ROUND_TRIP) times 2 for
    fp32 reordering: d2 1.096e-06, d3 7.468e-07.  The zero pattern must agree on >= 99.9 % of the voxels (every non-zero
    fixture voxel is above ECUT), the share test_reverse_norm uses."""
    from calodiffusion_amd.postprocess import ReverseNorm
    from calodiffusion_amd.preprocess import Preprocess
    g, cfg = gold("preprocess"), _cfg(name)
    raw, e = g[f"{tag}.showers"], g[f"{tag}.incident_energies"]
    E, layers, data = Preprocess(cfg)(raw, e)
    back, energy = ReverseNorm(data.cpu().numpy(), E.cpu().numpy(), emax=cfg["EMAX"], emin=cfg["EMIN"], max_deposit=cfg["MAXDEP"],
                               logE=cfg["logE"], layerE=None if layers is None else layers.cpu().numpy(),
                               showerMap=cfg["SHOWERMAP"], dataset_num=cfg["DATASET_NUM"], ecut=float(cfg["ECUT"]))
    want = raw * SCALE
    err, same = rel_l2(back, want), float(((back == 0) == (want == 0)).mean())
    print(f"[{tag}] round trip: rel L2 {err:.3e} (reference's own {REFERENCE_ROUND_TRIP[tag]:.3e}), zero pattern agrees on {same:.6f}")
    assert back.shape == want.shape
    assert err < 2 * REFERENCE_ROUND_TRIP[tag]
    assert same >= 0.999
    assert rel_l2(np.reshape(energy, (-1, 1)), e * SCALE) < 1e-5


@pytest.mark.parametrize("tag,name", [("d2", "dataset2"), ("d3", "dataset3")])
def test_rows_do_not_depend_on_the_batch_or_the_input_kind(tag, name):
    """Rows 0-3 and 4-7 processed separately are bitwise the rows of the 8-shower call; numpy input and device-tensor input
    give bitwise-equal output."""
    from calodiffusion_amd.preprocess import Preprocess
    g, cfg = gold("preprocess"), _cfg(name)
    raw, e = g[f"{tag}.showers"], g[f"{tag}.incident_energies"]
    pre = Preprocess(cfg)
    whole = pre(raw, e)
    lo, hi = pre(raw[:4], e[:4]), pre(raw[4:], e[4:])
    dev = pre(torch.from_numpy(raw).cuda(), torch.from_numpy(e).cuda())
    for w, a, b, d in zip(whole, lo, hi, dev):
        if w is None:
            assert a is None and b is None and d is None
            continue
        assert torch.equal(torch.cat([a, b]), w)
        assert torch.equal(d, w)
    assert whole[1] is not None or tag == "d3"


def test_one_training_step_from_raw_data():
    """compute_loss on Preprocess(raw) equals compute_loss on the reference-pre-processed tensors of the fixture (same noise,
    same sigma draw), within the relative 1e-5 tests/test_gpu_train.py holds the loss to."""
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    from calodiffusion_amd.preprocess import Preprocess
    g, cfg = gold("preprocess"), _cfg("dataset2")
    torch.manual_seed(1234)
    m = CaloDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"])
    E, layers, data = Preprocess(cfg)(g["d2.showers"], g["d2.incident_energies"])
    gen = torch.Generator().manual_seed(11)
    noise, rnd = torch.randn(data.shape, generator=gen).cuda(), torch.randn((8,), generator=gen).cuda()
    want_in = (torch.from_numpy(g["d2.data"]).reshape(data.shape).cuda(), torch.from_numpy(g["d2.E"]).cuda(),
               torch.from_numpy(g["d2.layerE"]).cuda())
    got = m.compute_loss(data, E, noise=noise, layers=layers, rnd_normal=rnd)
    want = m.compute_loss(want_in[0], want_in[1], noise=noise, layers=want_in[2], rnd_normal=rnd)
    assert got.requires_grad and got.dim() == 0
    got.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.model.parameters())
    print(f"loss from raw data {float(got):.8f}, from the reference's tensors {float(want):.8f}")
    assert np.isfinite(float(want)) and abs(float(got) - float(want)) <= 1e-5 * abs(float(want))


@pytest.mark.parametrize("tag,name", [("d2", "dataset2"), ("d3", "dataset3")])
def test_a_shower_without_energy_raises(tag, name):
    """A wholly empty shower, or a zero incident energy, raises ValueError naming the row: nothing of that call is returned."""
    from calodiffusion_amd.preprocess import Preprocess, preprocess_shower
    g, cfg = gold("preprocess"), _cfg(name)
    raw, e = g[f"{tag}.showers"], g[f"{tag}.incident_energies"]
    pre = Preprocess(cfg)
    empty = raw.copy()
    empty[5] = 0.0
    with pytest.raises(ValueError, match="shower 5 "):
        pre(empty, e)
    with pytest.raises(ValueError, match="shower 5 "):
        preprocess_shower(empty * SCALE, e * SCALE, cfg["SHAPE_PAD"], "", cfg["SHOWERMAP"], dataset_num=cfg["DATASET_NUM"],
                          max_deposit=cfg["MAXDEP"])
    no_e = e.copy()
    no_e[2] = 0.0
    with pytest.raises(ValueError, match="shower 2 "):
        pre(raw, no_e)
    # the flag is per call: the same object works on the next, clean batch
    E, layers, data = pre(raw, e)
    assert torch.isfinite(data).all() and torch.isfinite(E).all()


def test_bad_shapes_are_refused_before_the_launch():
    from calodiffusion_amd.preprocess import Preprocess
    pre = Preprocess(_cfg("dataset2"))
    with pytest.raises(ValueError, match="voxels"):
        pre(np.ones((2, 100), dtype=np.float32), np.ones((2,), dtype=np.float32))
    with pytest.raises(ValueError, match="incident energies"):
        pre(np.ones((2, 6480), dtype=np.float32), np.ones((3,), dtype=np.float32))
