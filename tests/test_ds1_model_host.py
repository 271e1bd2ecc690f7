"""CPU: the Dataset-1 model's host side -- the binning-file reader against what the reference's reads, construction of
``CaloDiffusion`` over SHOWER_EMBED 'orig-NN' (seeded weights and state_dict keys of the reference), and what is still refused."""
import numpy as np
import pytest
import torch

from conftest import gold
from helpers import SEED, verify_checksums
import ds1_geom_cases as G1
import ds1_model_cases as K


def _model(**over):
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    cfg = K.config(**over)
    state = torch.random.get_rng_state()
    torch.manual_seed(SEED)
    m = CaloDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"])
    torch.random.set_rng_state(state)
    return m


def test_xml_handler_reads_what_the_reference_reads():
    from calodiffusion.utils.utils import XMLHandler  # the alias, where the reference has it
    from calodiffusion_amd import xml_handler
    assert XMLHandler is xml_handler.XMLHandler
    g = gold("ds1_model")
    h = XMLHandler("photon", K.XML)
    assert np.array_equal(np.concatenate([np.asarray(e, dtype=np.float64) for e in h.r_edges]), g["xml.r_edges"])
    assert [len(e) for e in h.r_edges] == g["xml.n_edges"].tolist()
    assert h.r_bins == g["xml.r_bins"].tolist() and h.a_bins == g["xml.a_bins"].tolist()
    assert h.bin_edges == g["xml.bin_edges"].tolist() and h.GetBinEdges() == g["xml.bin_edges"].tolist()
    assert h.GetRelevantLayers() == g["xml.relevant"].tolist()
    assert [len(a[0]) if h.r_bins[i] > 0 else 0 for i, a in enumerate(h.alphaListPerLayer)] == g["xml.n_alpha"].tolist()
    assert np.array_equal(np.asarray(h.alphaListPerLayer[1][0], dtype=np.float64), g["xml.alpha0"])
    assert h.GetTotalNumberOfBins() == int(g["xml.total"]) == K.V
    with pytest.raises(ValueError, match="kaon"):
        XMLHandler("kaon", K.XML)


def test_orig_nn_model_constructs_with_the_reference_weights():
    g = gold("ds1_model")
    m = _model()
    assert m.do_embed and m.NN_embed is not None and m._data_shape == [K.V]
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["sd_keys"]]
    assert any(k == "NN_embed.encs.0.weight" for k in sd) and any(k == "NN_embed.decs.4.weight" for k in sd)
    verify_checksums(sd, g)
    gc = m.NN_embed.gc
    assert (gc.num_layers, int(gc.alpha_out), gc.dim_r_out) == K.GRID
    assert K.layout(gc) == ([0, 8, 168, 358, 363, 368], [1, 10, 10, 1, 1], [8, 16, 19, 5, 5])


def test_state_dict_with_a_foreign_prefix_loads():
    m = _model()
    other = _model()
    with torch.no_grad():
        for p in other.parameters():
            p.add_(1.0)
    m.load_state_dict({"module." + k: v for k, v in other.state_dict().items()})
    for (k, a), b in zip(m.state_dict().items(), other.state_dict().values()):
        assert torch.equal(a, b), k


def test_built_converter_in_the_config():
    """config['NN_EMBED']: an already built NNConverter, for callers without the XML"""
    from calodiffusion_amd import geom1, xml_handler
    conv = geom1.NNConverter(bins=xml_handler.XMLHandler("photon", K.XML))
    m = _model(NN_EMBED=conv, BIN_FILE="/nonexistent.xml")
    assert m.NN_embed is conv and m.do_embed
    with pytest.raises(TypeError, match="NNConverter"):
        _model(NN_EMBED=conv.gc)


def test_mismatched_geometry_is_refused():
    conv = G1.nn_converter("g1")  # 368 voxels onto (5, 10, 28)
    with pytest.raises(ValueError, match=r"\(5, 10, 28\).*\(5, 10, 30\)"):
        _model(NN_EMBED=conv)
    with pytest.raises(ValueError, match="SHAPE_ORIG"):
        _model(SHAPE_ORIG=[-1, 367])


def test_what_stays_refused_names_the_gap():
    from calodiffusion_amd.layerdiffusion import LayerDiffusion
    from calodiffusion_amd.sample import BespokeNonStationary
    with pytest.raises(NotImplementedError, match="orig-NN"):
        LayerDiffusion(K.config())
    m = _model(TIME_EMBED="sigma")
    bns = BespokeNonStationary(dict(m.config, SAMPLER_PATH="/nonexistent"))
    with pytest.raises(NotImplementedError, match="orig-NN"):
        bns.optimize_sampler(m, [], 4)
    with pytest.raises(NotImplementedError):
        _model(SHOWER_EMBED="orig-NN-FCN")
    with pytest.raises(NotImplementedError, match="pre-embed"):
        _model(HGCAL=True, SHOWER_EMBED="NN")
    with pytest.raises(ValueError, match="reverse_norm"):
        m.generate([], 4)
