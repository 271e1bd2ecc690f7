"""CPU: the HGCal geometry converter's host side (calodiffusion_amd/hgcal.py) against the reference's own maps on a synthetic
geometry (fixture: tools/gen_golden_hgcal_geom.py), and the float64 restatements the GPU tests use against the reference's
Embeder / Decoder outputs."""
import numpy as np
import pytest
import torch

from conftest import gold
from hgcal_geom_cases import apply64, bound, geometry, sparse64, sparse_bound, sparse_matrix, worst_ratio

from calodiffusion_amd import hgcal
from calodiffusion_amd.configs import load_config


@pytest.mark.parametrize("tag", ["g", "w"])
def test_from_geometry_reproduces_the_reference_maps(tag):
    """init_map restated: enc_mat and both masks exactly (g: the centre-cell-only layer, the 0.5 / 0.5 splits; w: the ring
    re-binning from 23 outwards); the pseudo-inverse to 1e-6 absolute (torch.linalg.pinv against itself on equal input: the
    bound only absorbs a different thread count's summation order)."""
    g = gold("hgcal_geom")
    conv = hgcal.HGCalConverter.from_geometry(geometry(g, tag), [-1, 1] + [int(b) for b in g[f"{tag}.bins"]])
    enc = conv.enc_mat.numpy()
    assert enc.shape == g[f"{tag}.enc_mat"].shape and np.array_equal(enc, g[f"{tag}.enc_mat"])
    assert np.array_equal(conv.enc_mask.numpy(), g[f"{tag}.enc_mask"]) and np.array_equal(conv.dec_mask.numpy(), g[f"{tag}.dec_mask"])
    err = float(np.abs(conv.dec_mat.numpy() - g[f"{tag}.dec_mat"]).max())
    print(f"[{tag}] pinv restated: max abs difference {err:.2e}")
    assert err <= 1e-6
    if tag == "g":
        assert np.count_nonzero(enc[2]) == 4 and np.all(enc[2][:, 1:] == 0)  # the centre cell over the 4 angular bins
        assert np.any((enc == 0.5).sum(1) == 2)
    else:
        assert g["w.ring_map"].max() >= 23 > g["w.ring_map"].min()
    assert conv.embeder.mat is conv.enc_mat and conv.decoder.dim1 == int(g[f"{tag}.bins"][1])


def test_norm_constants_and_constructors():
    g = gold("hgcal_geom")
    bins = [int(b) for b in g["g.bins"]]
    conv = hgcal.HGCalConverter.from_geometry(geometry(g, "g"), bins, norm=True, dataset_num=101)
    assert conv.norm and (conv.embed_mean, conv.embed_std) == (0.0835, 3.1083)
    assert tuple(g["norm"]) == hgcal.HGCAL_EMBED_PARAMS[111] == (0.0, 1.0)
    with pytest.raises(KeyError):
        conv.init(norm=True, dataset_num=100)  # the reference's set 100 has no embed constants either
    with pytest.raises(NotImplementedError, match="TRAINABLE_EMBED"):
        conv.init(noise_scale=0.1)
    m = hgcal.HGCalConverter.from_matrices(bins, g["g.enc_mat"], g["g.dec_mat"])
    assert np.array_equal(m.dec_mask.numpy(), g["g.dec_mask"]) and not m.norm
    r = hgcal.HGCalConverter.from_reference(conv)
    assert r.norm and r.embed_std == 3.1083 and torch.equal(r.enc_mat, conv.enc_mat)
    with pytest.raises(ValueError, match="enc_mat must be"):
        hgcal.HGCalConverter.from_matrices(bins, g["g.dec_mat"], g["g.dec_mat"])


def test_float64_restatement_matches_the_reference_outputs():
    """Encode, decode (with the converter's norm too) and the sparse decode on the recorded uniforms, restated in float64,
    against what the reference's Embeder / Decoder returned: within the derived bound, and with the reference's support."""
    g = gold("hgcal_geom")
    enc_mat, dec_mat = g["g.enc_mat"], g["g.dec_mat"]
    L, A, R = (int(b) for b in g["g.bins"])
    mean, std = g["norm"]
    z = g["z"].reshape(g["z"].shape[:3] + (A * R,))
    worst = {}
    for name, M, x, key in (("enc", enc_mat, g["x"], "enc"), ("dec", dec_mat, z, "dec")):
        want = g[key].reshape(g[key].shape[:3] + (-1,))
        worst[name] = worst_ratio(apply64(M, x), want, bound(M, x))
    worst["enc_norm"] = worst_ratio((apply64(enc_mat, g["x"]) - mean) / std, g["enc_norm"].reshape(g["x"].shape[:3] + (-1,)),
                                    bound(enc_mat, g["x"]) / std)
    worst["dec_norm"] = worst_ratio(apply64(dec_mat, z * std + mean), g["dec_norm"], bound(dec_mat, z * std + mean))
    for tag in ("sparse", "sparse_pb"):
        rand = g[f"{tag}.rand"]
        assert rand.shape[0] == (1 if tag == "sparse_pb" else z.shape[0])
        keep = dec_mat > 1e-6
        margin = np.abs((rand.astype(np.float32) + dec_mat)[np.broadcast_to(keep, rand.shape)] - 1.0).min()
        assert margin > 1e-6  # the fixture's seed condition
        sm = sparse_matrix(dec_mat, rand)
        got, want = sparse64(sm, z), g[f"{tag}.out"]
        worst[tag] = worst_ratio(got, want, sparse_bound(dec_mat, sm, z))
        assert np.array_equal(got != 0, want != 0)
        for l in range(L):  # the seed condition on the columns, and a decode that really samples
            if g["g.ncells"][l] > 1:
                assert keep[l].sum(0).max() >= 2
        assert 0 < (sm > 0).sum() < np.broadcast_to(keep, sm.shape).sum()
    print("float64 restatement vs reference, worst |err| / bound:", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0


def test_alias_module_exports_the_reference_names():
    import calodiffusion.utils.HGCal_utils as H
    from calodiffusion_amd import postprocess
    assert H.HGCalConverter is hgcal.HGCalConverter and H.Embeder is hgcal.Embeder and H.Decoder is hgcal.Decoder
    assert H.init_map is hgcal.init_map and H.load_geom is hgcal.load_geom and H.ReverseNormHGCal is postprocess.ReverseNormHGCal


def test_generate_without_geometry_still_raises_for_hgcal():
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    cfg = dict(load_config("hgcal"), EMAX=1000., EMIN=1., logE=True, MAXDEP=2, ECUT=0.0)
    m = CaloDiffusion(cfg, 50, "l2")
    with pytest.raises(ValueError, match="inverse pre-processing"):
        m.generate([], 2)
    with pytest.raises(ValueError, match="inverse pre-processing"):
        m.generate([], 2, geometry=None)
    with pytest.raises(TypeError, match="HGCalConverter"):
        m.generate([], 2, geometry=object())
    g = gold("hgcal_geom")
    conv = hgcal.HGCalConverter.from_matrices([int(b) for b in g["g.bins"]], g["g.enc_mat"], g["g.dec_mat"])
    assert m._physical_form(None, conv) == "device" and m._physical_form(False, conv) == "none"
    # a regular-grid config is what it was, with or without the keyword
    d2 = CaloDiffusion(dict(load_config("dataset2"), EMAX=1000., EMIN=1., logE=True, MAXDEP=2, ECUT=0.0), 50, "l2")
    assert d2._physical_form(None) == d2._physical_form(None, conv) == "device"


def test_geom_file_without_the_package_names_it(tmp_path):
    with pytest.raises(ImportError, match="HGCalShowers"):
        hgcal.HGCalConverter(bins=[28, 12, 21], geom_file=str(tmp_path / "geom.pkl"))
