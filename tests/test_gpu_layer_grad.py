"""GPU (MI355X): the gradient surface of LayerDiffusion's layer-energy model -- cd_layer_denoise_vjp against torch autograd
through the CPU oracle's denoise (models/calodiffusion.py:154-169 on the ResNet MLP) for the three objectives and both time
embeddings, autograd through LayerDiffusion.denoise in the layer state, the input-only mode, consistency with the training step,
the training step for noise_pred / mean_pred against autograd through the reference's loss (models/loss.py:163-210, restated
below), the forward-only loss, and the refusal of bad arguments.

The docstrings give the figures measured on one MI355X against the fp32 oracle."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from oracle import torch_oracle as O

pytestmark = pytest.mark.gpu

DIM = 46
OBJECTIVES = ["hybrid_weight", "noise_pred", "mean_pred"]


def _model(**extra):
    from calodiffusion_amd.layerdiffusion import LayerDiffusion
    from calodiffusion_amd.configs import load_config
    cfg = load_config("dataset2")
    cfg["LAYER_STEPS"] = 12
    cfg.update(extra)
    torch.manual_seed(1234)
    return LayerDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"])


def _oracle(m):
    sd = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.layer_model.state_dict().items()}
    return O.OracleLayerModel(m.config, sd), sd


def _inputs(B, seed=11):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((B, DIM), generator=gen)
    E = torch.rand((B, 1), generator=gen)
    gy = torch.randn((B, DIM), generator=gen)
    sigma = torch.tensor([0.02, 0.3, 2.5, 11.0, 60.0][:B], dtype=torch.float32)  # spread over the range the samplers visit
    return x, E, gy, sigma


def _grad_errors(got: dict, sd: dict):
    """(all gradients concatenated, worst single tensor with its name) rel-L2 of {name: grad} against the oracle's sd[name].grad."""
    worst = max((rel_l2(got[k].cpu().numpy(), sd[k].grad.numpy()), k) for k in got)
    g = np.concatenate([got[k].cpu().numpy().ravel() for k in got])
    w = np.concatenate([sd[k].grad.numpy().ravel() for k in got])
    return rel_l2(g, w), worst


def _named_grads(m, flat):
    eng = m.layer_model.engine()
    return {k: g for (k, _), g in zip(m.layer_model.named_parameters(), eng.param_grads(flat))}


# models/loss.py:97-116 (Loss._loss) and :163-210 (the three loss_function bodies), on the oracle's denoise
def _ref_reduce(lt, pred, target, weight):
    if lt == "l1":
        return F.l1_loss(pred, target)
    if lt == "mse":
        return F.mse_loss(pred, target)
    if lt == "huber":
        return F.smooth_l1_loss(pred, target)
    return (weight * ((pred - target) ** 2)).sum() / (torch.mean(weight) * float(np.prod(target.shape)))


def _ref_loss(om, objective, lt, data, E, noise, sigma):
    sigma = sigma.reshape(-1, 1)
    x_noisy = data + sigma * noise
    x0_pred = om.denoise(x_noisy, E, sigma)
    if objective == "hybrid_weight":
        return _ref_reduce(lt, x0_pred, data, 1.0 + (1.0 / sigma ** 2))
    if objective == "noise_pred":
        x0_pred = data - sigma * x0_pred
        pred = (data - x0_pred) / sigma
        return _ref_reduce(lt, pred, noise, torch.ones_like(pred))
    assert objective == "mean_pred"
    return _ref_reduce(lt, x0_pred, data, 1.0 / (sigma ** 2))


@pytest.mark.parametrize("time_embed", ["sigma", "log"])
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_vjp_matches_autograd(objective, time_embed):
    """dx and every parameter gradient of L = <gy, denoise(x)> from one cd_layer_denoise_vjp call.  Bounds: those of the U-Net's
    VJP (test_gpu_denoise_grad.py).  Measured over the six cases: dx 3.8e-8 ... 3.6e-7, worst tensor 6.7e-7 ... 8.6e-7, concatenated 1.5e-7 ... 1.9e-7."""
    m = _model(TRAINING_OBJ=objective, TIME_EMBED=time_embed)
    m.set_layer_state(True)
    x, E, gy, sigma = _inputs(5)
    om, sd = _oracle(m)
    xo = x.clone().requires_grad_(True)
    (om.denoise(xo, E, sigma) * gy).sum().backward()

    eng = m.engine()
    dx, flat = eng.denoise_vjp(x.cuda(), sigma.cuda(), E.cuda(), gy.cuda(), param_grads=True)
    e_x = rel_l2(dx.cpu().numpy(), xo.grad.numpy())
    e_all, worst = _grad_errors(_named_grads(m, flat), sd)
    print(f"[{objective}/{time_embed}] vjp: dx rel-L2 {e_x:.3e}, worst tensor {worst[0]:.3e} ({worst[1]}), concatenated {e_all:.3e}")
    assert e_x < 2e-5
    assert worst[0] < 1e-4, worst
    assert e_all < 5e-6


def _chain(den, x0, theta, sigmas):
    x = x0
    for i in range(theta.shape[1]):
        x = theta[0, i] * x + theta[1, i] * den(x, sigmas[i])
    return x


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_chained_denoise_through_autograd(objective):
    """x <- a_i x + b_i denoise(x, sigma_i), 4 calls, through LayerDiffusion.denoise and torch autograd: theta and the start get
    their gradients through every call; the parameters too (they accumulate over the calls and over a second backward).
    Measured (worst objective): theta.grad 2.1e-7, x0.grad 1.3e-7, parameters 1.6e-7."""
    m = _model(TRAINING_OBJ=objective)
    m.set_layer_state(True)
    B = 3
    x, E, gy, _ = _inputs(B, seed=5)
    theta0 = torch.tensor([[0.9, 0.8, 0.7, 0.6], [0.3, 0.5, 0.6, 0.4]])
    sigmas = [torch.full((B,), s) for s in (20.0, 4.0, 0.8, 0.1)]

    om, sd = _oracle(m)
    th_o = theta0.clone().requires_grad_(True)
    x_o = x.clone().requires_grad_(True)
    (_chain(lambda xi, s: om.denoise(xi, E, s), x_o, th_o, sigmas) * gy).sum().backward()

    def run():
        th = theta0.cuda().requires_grad_(True)
        xg = x.cuda().requires_grad_(True)
        Ec = E.cuda()
        out = _chain(lambda xi, s: m.denoise(xi, E=Ec, sigma=s.cuda(), layers=None), xg, th, sigmas)
        assert out.requires_grad
        (out * gy.cuda()).sum().backward()
        return th, xg

    m.zero_grad()
    th, xg = run()
    e_th = rel_l2(th.grad.cpu().numpy(), th_o.grad.numpy())
    e_x = rel_l2(xg.grad.cpu().numpy(), x_o.grad.numpy())
    params = dict(m.layer_model.named_parameters())
    e_all, worst = _grad_errors({k: p.grad for k, p in params.items()}, sd)
    print(f"[{objective}] chain: theta.grad rel-L2 {e_th:.3e}, x0.grad {e_x:.3e}, parameters {e_all:.3e} (worst {worst[0]:.3e} {worst[1]})")
    assert e_th < 1e-4 and e_x < 1e-4
    assert e_all < 1e-4
    # a second backward without zero_grad accumulates, as torch does
    first = {k: p.grad.clone() for k, p in params.items()}
    run()
    for k, p in params.items():
        assert torch.allclose(p.grad, 2 * first[k], rtol=1e-5, atol=1e-7), k
    assert all(p.grad is None for p in m.base_model.parameters())


def test_graph_free_calls_are_unchanged():
    m = _model()
    m.set_layer_state(True)
    x, E, _, sigma = _inputs(4, seed=3)
    xc, Ec, sc = x.cuda(), E.cuda(), sigma.cuda()
    eng = m.engine()
    want = eng.denoise(xc, sc, Ec)
    out = m.denoise(xc, E=Ec, sigma=sc, layers=None)  # x does not require grad (the parameters do)
    assert not out.requires_grad and out.grad_fn is None
    assert torch.equal(out, want)
    with torch.no_grad():
        out2 = m.denoise(xc.clone().requires_grad_(True), E=Ec, sigma=sc, layers=None)
    assert not out2.requires_grad and out2.grad_fn is None
    assert torch.equal(out2, want)
    xg = xc.clone().requires_grad_(True)
    out3 = m.denoise(xg, E=Ec, sigma=sc, layers=None)
    assert out3.requires_grad and torch.equal(out3.detach(), want)  # the graph's forward is the same call
    with pytest.raises(NotImplementedError, match="sigma"):
        m.denoise(xg, E=Ec, sigma=sc.clone().requires_grad_(True), layers=None)
    with pytest.raises(NotImplementedError, match="E"):
        m.denoise(xg, E=Ec.clone().requires_grad_(True), sigma=sc, layers=None)
    # frozen parameters: the input-only call
    for p in m.layer_model.parameters():
        p.requires_grad_(False)
    (m.denoise(xg, E=Ec, sigma=sc, layers=None) * xc).sum().backward()
    assert xg.grad is not None and all(p.grad is None for p in m.layer_model.parameters())
    assert torch.equal(xg.grad, eng.denoise_vjp(xc, sc, Ec, xc, param_grads=False)[0])


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_input_only_mode(objective):
    """grads == NULL: the same dx bits from one launch, no tape, no weight-gradient launch; neither mode allocates after its first
    call; the full call's sums have a fixed order."""
    from calodiffusion_amd import engine
    m = _model(TRAINING_OBJ=objective)
    m.set_layer_state(True)
    x, E, gy, sigma = _inputs(5, seed=9)
    eng = m.engine()
    args = (x.cuda(), sigma.cuda(), E.cuda(), gy.cuda())
    dx_full, flat = eng.denoise_vjp(*args, param_grads=True)
    dx_only, none = eng.denoise_vjp(*args, param_grads=False)
    assert none is None and flat is not None
    assert torch.equal(dx_full, dx_only)
    assert torch.isfinite(dx_full).all() and torch.isfinite(flat).all()

    engine.profile_begin()
    eng.denoise_vjp(*args, param_grads=False)
    prof = engine.profile_end()
    assert set(prof) == {"layer_mlp_vjp"} and prof["layer_mlp_vjp"]["launches"] == 1, prof
    engine.profile_begin()
    eng.denoise_vjp(*args, param_grads=True)
    prof = engine.profile_end()
    assert set(prof) == {"layer_mlp_vjp", "linear_wgrad"}, prof
    assert prof["layer_mlp_vjp"]["launches"] == 1 and prof["linear_wgrad"]["launches"] == 1, prof

    sizes = []
    for mode in (0, 1):
        n = C.c_size_t()
        assert eng.lib.cd_layer_vjp_workspace_bytes(C.byref(eng.desc), 5, mode, C.byref(n)) == 0
        sizes.append(n.value)
    assert sizes[0] < sizes[1], sizes

    for mode in (True, False):
        dx, fl = eng.denoise_vjp(*args, param_grads=mode)  # (the first call of this mode sizes its workspace)
        del dx, fl
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        for _ in range(2):
            dx, fl = eng.denoise_vjp(*args, param_grads=mode)
            del dx, fl
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before, (mode, before, torch.cuda.memory_allocated())
    _, flat2 = eng.denoise_vjp(*args, param_grads=True)
    assert torch.equal(flat, flat2)


def test_vjp_reproduces_training_step_gradients():
    """gy = d(hybrid_weight l2 loss)/dD formed in torch: cd_layer_denoise_vjp then gives cd_layer_train_step's flat gradient.
    Measured: 2.2e-7."""
    m = _model()
    m.set_layer_state(True)
    B = 9
    gen = torch.Generator().manual_seed(21)
    data, E = torch.randn((B, DIM), generator=gen).cuda(), torch.rand((B, 1), generator=gen).cuda()
    noise = torch.randn((B, DIM), generator=gen).cuda()
    sigma = (torch.randn((B,), generator=gen) * 1.2 - 1.2).exp().cuda()
    eng = m.engine()
    _, flat_train = eng.train_step(data, noise, sigma, E, "l2")
    x = data + sigma.view(-1, 1) * noise
    D = eng.denoise(x, sigma, E)
    wgt = (1.0 + sigma.double() ** -2).view(-1, 1)
    gy = (2.0 * wgt * (D.double() - data.double()) / (wgt.mean() * D.numel())).float().contiguous()
    dx, flat = eng.denoise_vjp(x, sigma, E, gy, param_grads=True)
    err = rel_l2(flat.cpu().numpy(), flat_train.cpu().numpy())
    print(f"layer vjp vs training step: flat gradient rel-L2 {err:.3e}")
    assert err < 1e-6
    assert torch.isfinite(dx).all()


@pytest.mark.parametrize("lt", ["l2", "huber", "l1", "mse"])
@pytest.mark.parametrize("objective", ["noise_pred", "mean_pred"])
def test_layer_training_objectives_against_autograd(objective, lt):
    """LayerDiffusion.compute_loss(...).backward() in the layer state for TRAINING_OBJ noise_pred / mean_pred and every LOSS_TYPE,
    on the inputs and with the bounds of test_gpu_layer.py::test_layer_model_training_step_against_autograd, against autograd
    through the reference's loss on the oracle; FusedAdam then steps the layer model; under no_grad the loss is cd_layer_loss.
    Measured: loss <= 2.2e-7, concatenated <= 3.1e-7, worst tensor <= 8.7e-7 over the eight cases, l1 included."""
    from calodiffusion_amd.optim import FusedAdam
    from calodiffusion_amd import engine
    m = _model(LOSS_TYPE=lt, TRAINING_OBJ=objective)
    assert m.loss_function.loss_type == lt and type(m.loss_function).__name__ == objective
    gen = torch.Generator().manual_seed(21)
    B = 9
    layers = torch.randn((B, DIM), generator=gen)
    E = torch.rand((B, 1), generator=gen)
    noise = torch.randn((B, DIM), generator=gen)
    rnd = torch.randn((B,), generator=gen)
    om, sd = _oracle(m)
    assert "log" in m.config["NOISE_SCHED"]
    sigma = (rnd * 1.2 + (-1.2)).exp()  # Loss.__call__ (models/loss.py:139-140) with the 'log' schedule's P_mean / P_std
    want = _ref_loss(om, objective, lt, layers, E, noise, sigma)
    want.backward()
    want = float(want.detach())

    m.set_layer_state(True)
    m.noise_generation = lambda shape: noise.cuda()
    params = dict(m.layer_model.named_parameters())
    opt = FusedAdam(m.layer_model.parameters(), lr=1e-3)
    opt.zero_grad()
    loss = m.compute_loss(None, E.cuda(), None, layers.cuda(), rnd_normal=rnd.cuda())
    loss.backward()
    e_loss = abs(float(loss.detach()) - want) / abs(want)
    e_all, worst = _grad_errors({k: p.grad for k, p in params.items()}, sd)
    print(f"[{objective}/{lt}] loss rel {e_loss:.3e}, gradients concatenated {e_all:.3e}, worst tensor {worst[0]:.3e} ({worst[1]})")
    assert e_loss < 2e-6
    # (l1: the gradient is sign(d) / N -- a residual within rounding of zero may flip one of the 414 signs)
    assert e_all < (2e-3 if lt == "l1" else 5e-6) and worst[0] < (2e-2 if lt == "l1" else 1e-4), (e_all, worst)
    engine.profile_begin()
    with torch.no_grad():
        val = float(m.compute_loss(None, E.cuda(), None, layers.cuda(), rnd_normal=rnd.cuda()))
    prof = engine.profile_end()
    assert abs(val - want) < 2e-6 * abs(want)
    assert "layer_mlp_loss" in prof and "layer_mlp_train" not in prof and "linear_wgrad" not in prof, prof
    before = m.layer_model.out_lay.weight.detach().clone()
    opt.step()
    assert not torch.equal(before, m.layer_model.out_lay.weight)
    m.set_layer_state(False)
    assert all(p.grad is None for p in m.base_model.parameters())


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_forward_only_loss_is_the_training_steps_value(objective):
    from calodiffusion_amd import engine
    gen = torch.Generator().manual_seed(4)
    B = 7
    data, E = torch.randn((B, DIM), generator=gen).cuda(), torch.rand((B, 1), generator=gen).cuda()
    noise = torch.randn((B, DIM), generator=gen).cuda()
    sigma = (torch.randn((B,), generator=gen) * 1.2 - 1.2).exp().cuda()
    m = _model(TRAINING_OBJ=objective)
    m.set_layer_state(True)
    eng = m.engine()
    for lt in ("l2", "l1", "mse", "huber"):
        loss_t, _ = eng.train_step(data, noise, sigma, E, lt)
        engine.profile_begin()
        loss_f = eng.loss(data, noise, sigma, E, lt)
        prof = engine.profile_end()
        assert loss_f.dtype == torch.float64 and torch.equal(loss_f, loss_t), (objective, lt, float(loss_f), float(loss_t))
        assert set(prof) == {"layer_mlp_loss", "layer_loss_final"}, prof
        assert prof["layer_mlp_loss"]["launches"] == 1
        assert float(eng.loss_hybrid(data, noise, sigma, E, lt)) == float(loss_t.to(torch.float32))
    engine.profile_begin()
    eng.train_step(data, noise, sigma, E, "l2")
    prof = engine.profile_end()
    assert set(prof) == {"layer_mlp_train", "layer_loss_final", "linear_wgrad"}, prof


def test_bad_arguments_are_refused_before_any_launch():
    from calodiffusion_amd import engine
    m = _model()
    m.set_layer_state(True)
    eng = m.engine()
    B = 3
    x, E, gy, sigma = (t.cuda() for t in _inputs(B))
    w, n = eng._weights()
    ws = eng.vjp_workspace(B, True)
    dx = torch.empty_like(x)
    _, total = eng.grad_layout()
    flat = torch.empty(total, device="cuda")
    d = C.byref(eng.desc)
    st = engine._stream()

    def call(n_weights=n, dx_ptr=dx.data_ptr(), grads=flat.data_ptr(), ws_bytes=ws.numel(), x_ptr=x.data_ptr()):
        return eng.lib.cd_layer_denoise_vjp(d, w, n_weights, B, x_ptr, sigma.data_ptr(), E.data_ptr(), gy.data_ptr(), dx_ptr, grads,
                                            ws.data_ptr(), ws_bytes, st)

    engine.profile_begin()
    assert call(ws_bytes=ws.numel() // 2) == -1 and b"workspace" in eng.lib.cd_last_error()
    assert call(n_weights=n - 2) == -1 and b"n_weights" in eng.lib.cd_last_error()
    assert call(dx_ptr=None) == -1
    assert call(x_ptr=None) == -1
    assert call(grads=None, ws_bytes=16) == -1  # the input-only call wants its (small) workspace too
    # the forward-only loss and the training step check theirs the same way
    tws = eng.train_workspace(B)
    loss = torch.empty((), dtype=torch.float64, device="cuda")
    assert eng.lib.cd_layer_loss(d, w, n, B, x.data_ptr(), gy.data_ptr(), sigma.data_ptr(), E.data_ptr(), 0, loss.data_ptr(),
                                 tws.data_ptr(), 64, st) == -1
    assert eng.lib.cd_layer_loss(d, w, n, B, x.data_ptr(), gy.data_ptr(), sigma.data_ptr(), E.data_ptr(), 7, loss.data_ptr(),
                                 tws.data_ptr(), tws.numel(), st) == -1
    assert eng.lib.cd_layer_train_step_loss(d, w, n, B, x.data_ptr(), gy.data_ptr(), sigma.data_ptr(), E.data_ptr(), 0,
                                            loss.data_ptr(), None, tws.data_ptr(), tws.numel(), st) == -1
    assert engine.profile_end() == {}  # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(dx).all()
