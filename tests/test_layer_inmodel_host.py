"""CPU: ``LayerDiffusion`` over an in-model geometry embedding -- Dataset 0/1 with SHOWER_EMBED 'orig-NN' and HGCal with the
converter inside forward -- constructs as the reference's does (parameter order, layer-model widths), keeps the embedding out of
the layer state, and names the reference's latent SHAPE_PAD failure instead of reproducing it."""
import numpy as np
import pytest
import torch

from conftest import gold
from helpers import SEED, verify_checksums
import ds1_model_cases as K1
import layer_inmodel_cases as L
import narrow_cases as KN


def _record(rec):
    g = gold(L.FILE[rec])
    return {k[len(L.PREFIX[rec]):]: g[k] for k in g.files if k.startswith(L.PREFIX[rec])}


@pytest.mark.parametrize("rec", L.RECORDS)
def test_construction_draws_the_references_parameters(rec):
    """layer model, U-Net, then NN_embed: keys in the reference's order and every tensor's checksums"""
    from calodiffusion_amd.layerdiffusion import LayerDiffusion
    g = _record(rec)
    cfg = L.config(rec, NN_EMBED=L.nn_embed(rec)) if rec == "hg" else L.config(rec)
    torch.manual_seed(SEED)
    m = LayerDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type="l2")
    sd = L.flat_state_dict(m)
    if rec == "hg":  # the maps are the fixture's own here (config['NN_EMBED']); the reference's were not yet initialised
        sd = {k: v for k, v in sd.items() if not k.startswith("NN_embed.")}
        g = dict(g, ck_keys=np.array([k for k in g["ck_keys"] if not str(k).startswith("NN_embed.")]),
                 ck_vals=np.array([v for k, v in zip(g["ck_keys"], g["ck_vals"]) if not str(k).startswith("NN_embed.")]),
                 sd_keys=np.array([k for k in g["sd_keys"] if not str(k).startswith("NN_embed.")]))
    assert list(sd) == [str(k) for k in g["sd_keys"]]
    verify_checksums({k: v.cpu() for k, v in sd.items()}, g)
    assert isinstance(m.state_dict()["layer_model"], dict)
    assert m.layer_model.in_lay.weight.shape[1] == L.LAYERS[rec] + 1
    assert m.layer_model.cond_mlp[0].weight.shape[1] == (3 if rec == "hg" else 1)
    assert m.do_embed and tuple(m._data_shape) == L.STATE[rec] and m.model is m.base_model


@pytest.mark.parametrize("cases", [K1, KN])
def test_the_shipped_dataset1_shapes_name_the_latent_failure(cases):
    """SHAPE_PAD [-1, 1, V] (the shipped configs): refused at construction, by the name of what the reference fails on; a model
    whose shape_pad takes that form afterwards raises the named ValueError in every two-stage entry point, before it draws
    anything"""
    from calodiffusion_amd.layerdiffusion import LayerDiffusion
    from calodiffusion_amd import generator as G
    cfg = cases.config()
    assert cfg["SHAPE_PAD"] == [-1, 1, cases.V]
    final = rf"\[-1, 1, {cases.GRID[0]}, 10, {cases.GRID[2]}\]"
    with pytest.raises(NotImplementedError, match=rf"orig-NN.*SHAPE_PAD \[-1, 1, {cases.V}\].*SHAPE_PAD = SHAPE_FINAL = {final}"):
        LayerDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type="l2")
    m = L.model("ph" if cases is K1 else "pi")
    m.shape_pad = [-1, 1, cases.V]
    E = torch.rand((2, 1))
    want = rf"SHAPE_PAD\[2\] \+ 1 != SHAPE_FINAL\[2\] \+ 1 \({cases.V + 1} != {cases.GRID[0] + 1}\).*SHAPE_PAD = SHAPE_FINAL = \[-1, 1, {cases.GRID[0]}, 10, {cases.GRID[2]}\]"
    for call in (lambda: m.sample_layers(E), lambda: m.sample(E), lambda: m.generate([(E, None, None)], 3, geometry=m.NN_embed),
                 lambda: G.export_generator(m, 3)):
        with pytest.raises(ValueError, match=want):
            call()
        assert m.noise_offset == 0 and not m.layer_loss and m.model is m.base_model


@pytest.mark.parametrize("rec", L.RECORDS)
def test_the_layer_state_leaves_the_embedding_out(rec):
    """parameters that take gradients, the conditioning and the state switch: the layer state is the layer model alone"""
    m = L.model(rec)
    unet_params = m._params()
    assert len(unet_params) == len(list(m.base_model.parameters())) + len(list(m.NN_embed.parameters()))
    m.set_layer_state(True)
    try:
        assert m.model is m.layer_model
        assert [id(p) for p in m._params()] == [id(p) for p in m.layer_model.parameters()]
        E = torch.rand((2, L.ENERGY_COLS[rec]))
        assert m.cond_tensor(E, torch.zeros((2, L.LAYERS[rec] + 1))).shape == E.shape
    finally:
        m.set_layer_state(False)
    assert m.model is m.base_model and [id(p) for p in m._params()] == [id(p) for p in unet_params]
    assert m.cond_tensor(torch.rand((2, L.ENERGY_COLS[rec])), torch.zeros((2, L.LAYERS[rec] + 1))).shape == (2, L.ENERGY_COLS[rec] + L.LAYERS[rec] + 1)
    assert m._layer_dim() == L.LAYERS[rec] + 1


def test_hgcal_converter_is_built_from_the_geometry_file_when_none_is_given():
    """as CaloDiffusion builds it; where the file's package is missing the error says what to pass instead"""
    import importlib.util
    from calodiffusion_amd.layerdiffusion import LayerDiffusion
    if importlib.util.find_spec("HGCalShowers") is None:
        with pytest.raises(NotImplementedError, match=r"HGCalConverter inside forward.*BIN_FILE.*HGCalShowers.*config\['NN_EMBED'\]") as info:
            LayerDiffusion(L.config("hg"))
        assert isinstance(info.value.__cause__, ImportError)
    else:  # the package reads the file: a missing file is the file system's error, not a refusal
        with pytest.raises(OSError):
            LayerDiffusion(L.config("hg"))


def test_theta_training_stays_refused():
    from calodiffusion_amd.sample import BespokeNonStationary
    for rec, word in (("ph", "orig-NN"), ("hg", "HGCalConverter inside forward")):
        m = L.model(rec, time_embed="sigma")
        bns = BespokeNonStationary(dict(m.config, SAMPLER_PATH="/nonexistent"))
        with pytest.raises(NotImplementedError, match=word):
            bns.optimize_sampler(m, [], 4)
