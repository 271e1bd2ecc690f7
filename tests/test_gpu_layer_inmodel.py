"""GPU (MI355X): ``LayerDiffusion`` over an in-model geometry embedding -- the two-stage model whose U-Net state is the flat
Dataset-0/1 shower (cd_plan_set_radial) or HGCal's cell-space shower (cd_plan_set_geom) -- against the reference's own
``LayerDiffusion`` (tools/gen_golden_layer_inmodel.py) on the three records of layer_inmodel_cases.py.

Bounds, all existing ones: TOL_TRAJ for the generated layer energies and the final state (test_gpu_layer.py, helpers.py); the layer
state's loss to 2e-6 relative, its gradients to TOL_GRAD together and 1e-4 per tensor (test_gpu_layer.py); the inverse
pre-processing to rel L2 1e-5 with the zero pattern on > 99.9 % of the voxels (test_gpu_ds1_preprocess.py) or TOL_OP
(test_gpu_hgcal_model.py), on the reference's own final state and layers, so that it is this step that is measured and not the
trajectory in front of it; generate() from the fixture's start tensors is held to the reference's showers under the same rule, and
bitwise to that step applied to its own sampler output."""
import numpy as np
import pytest
import torch

from conftest import gold, rel_l2
from helpers import TOL_GRAD, TOL_OP, TOL_TRAJ, t
import layer_inmodel_cases as L

pytestmark = pytest.mark.gpu

_models = {}


def _record(rec):
    g = gold(L.FILE[rec])
    return {k[len(L.PREFIX[rec]):]: g[k] for k in g.files if k.startswith(L.PREFIX[rec])}


def _model(rec, time_embed="log"):
    if (rec, time_embed) not in _models:
        _models[rec, time_embed] = L.model(rec, time_embed=time_embed)
    return _models[rec, time_embed]


def _two_stage(m, g):
    return m.sample(t(g["E"]).cuda(), layers=None, num_steps=L.UNET_STEPS, sample_offset=0, return_layers=True,
                    start=t(g["start"]).cuda(), layer_start=t(g["layer_start"]).cuda())


@pytest.mark.parametrize("time_embed", L.TIME_EMBEDS)
@pytest.mark.parametrize("rec", L.RECORDS)
def test_two_stage_sample_against_the_reference(rec, time_embed):
    g, m = _record(rec), _model(rec, time_embed)
    out = _two_stage(m, g)
    assert out["x"].shape == (L.B,) + L.STATE[rec] and tuple(out["layers"].shape) == (L.B, L.LAYERS[rec] + 1)
    e_lay, e_x = rel_l2(out["layers"].cpu().numpy(), g[f"{time_embed}.layers"]), rel_l2(out["x"], g[f"{time_embed}.x"])
    print(f"[{rec} {time_embed}] layers {e_lay:.2e}  final state {e_x:.2e}")
    assert e_lay < TOL_TRAJ and e_x < TOL_TRAJ
    assert not m.layer_loss and m.model is m.base_model


@pytest.mark.parametrize("rec,objective,loss_type", [(r, o, lt) for r in L.RECORDS for o, lt in (L.LOSS_CASES if r != "pi" else L.LOSS_CASES[:1])])
def test_layer_state_loss_and_gradients_against_the_reference(rec, objective, loss_type):
    g = _record(rec)
    m = L.model(rec, objective, "log", loss_type)
    m.train()
    tag = f"loss.{objective}.{loss_type}"
    E, lay, lnoise, lrnd = (t(g[k]).cuda() for k in ("E", "lay", "lnoise", "lrnd"))
    m.set_layer_state(True)
    m.noise_generation = lambda shape: lnoise
    m.zero_grad()
    loss = m.compute_loss(None, E, None, lay, rnd_normal=lrnd)
    loss.backward()
    with torch.no_grad():
        value_only = float(m.compute_loss(None, E, None, lay, rnd_normal=lrnd))
    m.set_layer_state(False)
    want = float(g[tag + ".loss"])
    print(f"[{rec} {tag}] loss {float(loss.detach()):.7f} against {want:.7f}")
    assert abs(float(loss.detach()) - want) < 2e-6 * abs(want) and abs(value_only - want) < 2e-6 * abs(want)
    grads = {k: p.grad for k, p in m.layer_model.named_parameters()}
    num = den = worst = 0.0
    for k in g:
        if k.startswith(tag + ".grad."):
            a, b = grads[k[len(tag) + 6:]].cpu().double().numpy(), g[k].astype(np.float64)
            num += float(((a - b) ** 2).sum()); den += float((b ** 2).sum())
            worst = max(worst, rel_l2(a, b))
    print(f"[{rec} {tag}] stored gradients together {(num / den) ** 0.5:.2e}, worst tensor {worst:.2e}")
    assert (num / den) ** 0.5 < TOL_GRAD and worst < 1e-4
    for k, (s1, s2) in zip(g[tag + ".ck_keys"], g[tag + ".ck_vals"]):
        gr = grads[str(k)].double()
        assert abs(float((gr * gr).sum()) - s2) <= 2e-4 * max(s2, 1e-30), (tag, k)
    # the U-Net and the embedding are not part of the layer state's graph
    assert all(p.grad is None for p in m.base_model.parameters()) and all(p.grad is None for p in m.NN_embed.parameters())


@pytest.mark.parametrize("rec", L.RECORDS)
def test_layer_state_denoise_is_the_layer_model_alone(rec):
    """bitwise cd_layer_denoise of the same weights in a model without a U-Net, before and after the embedding is bound to the
    U-Net's plan, with and without a graph"""
    from calodiffusion_amd.resnet import ResNet
    g, m = _record(rec), _model(rec)
    alone = ResNet(dim_in=L.LAYERS[rec] + 1, num_layers=5, cond_size=L.ENERGY_COLS[rec])
    alone.load_state_dict(m.layer_model.state_dict())
    alone._engine_opts = dict(m.layer_model._engine_opts)
    alone.cuda()
    x, E = t(g["lay"]).cuda(), t(g["E"]).cuda()
    sigma = torch.tensor([40.0, 1.0, 0.03125], device="cuda")
    want = alone.engine().denoise(x, sigma, E)

    def layer_denoise(grad=False):
        m.set_layer_state(True)
        try:
            assert m.engine() is m.layer_model.engine()
            if not grad:
                with torch.no_grad():
                    return m.denoise(x, E=E, sigma=sigma, layers=None)
            xg = x.clone().requires_grad_(True)
            y = m.denoise(xg, E=E, sigma=sigma, layers=None)
            y.sum().backward()
            assert xg.grad is not None and torch.isfinite(xg.grad).all()
            return y.detach()
        finally:
            m.set_layer_state(False)

    assert torch.equal(layer_denoise(), want)
    eng = m.engine()  # the U-Net's engine: binds the embedding
    assert eng is m.base_model.engine() and eng.embedding is m.NN_embed
    assert torch.equal(layer_denoise(), want) and torch.equal(layer_denoise(grad=True), want)
    assert m.engine().embedding is m.NN_embed
    # and the U-Net state with layers given: CaloDiffusion's denoise of the same weights
    start, layers = t(g["start"]).cuda(), t(g["log.layers"]).cuda()
    with torch.no_grad():
        y = m.denoise(start, E=E, sigma=sigma, layers=layers)
    assert tuple(y.shape) == (L.B,) + L.STATE[rec] and torch.isfinite(y).all()


@pytest.mark.parametrize("rec", L.RECORDS)
def test_generate_ends_in_physical_showers(rec):
    g, m = _record(rec), _model(rec)
    geometry = None if rec == "hg" else m.NN_embed
    got, en = m._to_physical(g["log.x"], g["E"], g["log.layers"], None, geometry=geometry)
    got = np.asarray(got, dtype=np.float32).reshape(L.B, -1)
    err, same = rel_l2(got, g["log.phys"]), float(((got == 0) == (g["log.phys"] == 0)).mean())
    print(f"[{rec}] inverse pre-processing of the reference's state and layers: rel L2 {err:.3e}, zero pattern agrees on {same:.6f}")
    assert err < (TOL_OP if rec == "hg" else 1e-5) and same > 0.999 and np.isfinite(got).all()
    assert np.allclose(np.reshape(en, (L.B, -1))[:, 0], np.reshape(g["log.phys_e"], (L.B, -1))[:, 0], rtol=1e-6)
    # generate(): the same two stages from injected start tensors, then that step on its own output
    own = _two_stage(m, g)
    draws = [t(g["start"]).cuda(), t(g["layer_start"]).cuda()]
    m.noise_generation = lambda shape: draws.pop(0)
    try:
        showers, energies = m.generate([(t(g["E"]), None, None)], L.UNET_STEPS, geometry=geometry)
    finally:
        del m.noise_generation
    assert not draws
    want, _ = m._to_physical(own["x"], g["E"], own["layers"].cpu().numpy(), None, geometry=geometry)
    assert np.array_equal(np.asarray(showers), np.asarray(want)) and energies.shape == (L.B, L.ENERGY_COLS[rec])
    assert showers.shape == ((L.B, L.STATE[rec][0]) if rec != "hg" else (L.B,) + L.STATE[rec][1:])
    # and against the reference's own showers, under the same rule
    flat = np.reshape(showers, (L.B, -1))
    err, same = rel_l2(flat, g["log.phys"]), float(((flat == 0) == (g["log.phys"] == 0)).mean())
    print(f"[{rec}] generate() against the reference's showers: rel L2 {err:.3e}, zero pattern agrees on {same:.6f}")
    assert err < (TOL_OP if rec == "hg" else 1e-5) and same > 0.999


def test_device_noise_is_reproducible_and_advances_the_stream_by_its_tensors():
    """sample() from the Philox stream: start tensor of the flat state, layer start, start.numel() * steps per stage"""
    m = _model("ph")
    E = t(_record("ph")["E"]).cuda()
    m.noise_offset = 0
    a = m.sample(E, return_layers=True, num_steps=L.UNET_STEPS)
    after = m.noise_offset
    m.noise_offset = 0
    b = m.sample(E, return_layers=True, num_steps=L.UNET_STEPS)
    V, dim = L.STATE["ph"][0], L.LAYERS["ph"] + 1
    assert after == L.B * V + L.B * dim + L.B * dim * L.LAYER_STEPS + L.B * V * L.UNET_STEPS
    assert np.array_equal(a["x"], b["x"]) and torch.equal(a["layers"], b["layers"]) and np.isfinite(a["x"]).all()
    m.noise_offset = 0
