"""CPU: what the layer model's gradient surface promises before any device work -- LayerDiffusion.denoise in the layer state
refuses a sigma or E that requires grad without touching the engine, the new entry points are declared in all three places
(tests/test_abi.py compares their argument lists), and theta training on the layer stage stays refused."""
import re

import pytest
import torch

from conftest import ROOT


def _model():
    from calodiffusion_amd.layerdiffusion import LayerDiffusion
    from calodiffusion_amd.configs import load_config
    cfg = load_config("dataset2")
    torch.manual_seed(1234)
    m = LayerDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"])
    m.set_layer_state(True)
    return m


def test_denoise_refuses_gradients_of_sigma_and_E_before_the_engine(monkeypatch):
    m = _model()

    def no_engine():
        raise AssertionError("the engine must not be touched")

    monkeypatch.setattr(m.layer_model, "engine", no_engine)
    x = torch.randn((2, 46), requires_grad=True)
    E, sigma = torch.rand((2, 1)), torch.ones(2)
    with pytest.raises(NotImplementedError, match="sigma"):
        m.denoise(x, E=E, sigma=sigma.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="E"):
        m.denoise(x, E=E.clone().requires_grad_(True), sigma=sigma)
    # every other call reaches the engine (here: the stub)
    with pytest.raises(AssertionError, match="engine"):
        m.denoise(x, E=E, sigma=sigma)
    with pytest.raises(AssertionError, match="engine"):
        m.denoise(x.detach(), E=E, sigma=sigma)


def test_new_entry_points_are_declared_everywhere():
    from calodiffusion_amd import engine
    header = open(f"{ROOT}/include/calodiff.h").read()
    guide = open(f"{ROOT}/INTEGRATION.md").read()
    for name in ("cd_layer_denoise_vjp", "cd_layer_vjp_workspace_bytes", "cd_layer_loss"):
        assert name in engine._SIGNATURES
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in guide, name
    assert engine.CD_ABI_VERSION == 3
    assert not hasattr(engine.LayerMlpEngine, "bns_theta_grad")
