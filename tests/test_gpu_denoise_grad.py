"""GPU (MI355X): autograd through CaloDiffusion.denoise (cd_denoise_vjp) against torch autograd through the CPU oracle's
denoise (models/calodiffusion.py:154-169): the input gradient, every parameter gradient, a chain of denoise calls shaped like
the reference's BNS sampler (models/sample.py:1050-1105), consistency with the training step, the input-only mode, and the
calls that must keep today's graph-free path."""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from helpers import seeded_model_cfg
from oracle import torch_oracle as O

pytestmark = pytest.mark.gpu


def _inputs(cfg, B, seed=11):
    gen = torch.Generator().manual_seed(seed)
    shape = [B] + list(cfg["SHAPE_PAD"][1:])
    x = torch.randn(shape, generator=gen)
    E = torch.rand((B, 3 if cfg.get("HGCAL") else 1), generator=gen)
    layers = torch.randn((B, 1 + cfg["SHAPE_FINAL"][2]), generator=gen) if "layer" in cfg["SHOWERMAP"] else None
    sigma = torch.tensor([0.3, 2.5, 0.05, 11.0][:B], dtype=torch.float32)  # per-sample distinct noise levels
    w = torch.randn(shape, generator=gen)
    return x, E, layers, sigma, w


def _cuda(t):
    return None if t is None else t.cuda()


def _oracle(cfg, m):
    sd = {k[6:]: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    return O.OracleModel(cfg, sd)


CASES = [("tiny", 3, None), ("tiny", 2, "noise_pred"), ("tiny", 2, "mean_pred"), ("dataset2", 2, None), ("dataset3", 1, None),
         ("hgcal", 1, None)]


@pytest.mark.parametrize("name,B,objective", CASES)
def test_input_and_parameter_gradients_match_autograd(name, B, objective):
    m, cfg = seeded_model_cfg(name, {} if objective is None else {"TRAINING_OBJ": objective})
    x, E, layers, sigma, w = _inputs(cfg, B)
    om = _oracle(cfg, m)
    xo = x.clone().requires_grad_(True)
    (om.denoise(xo, E, sigma, layers) * w).sum().backward()

    m.zero_grad()
    xg = x.cuda().requires_grad_(True)
    out = m.denoise(xg, E=E.cuda(), sigma=sigma.cuda(), layers=_cuda(layers))
    assert out.requires_grad
    (out * w.cuda()).sum().backward()
    err_x = rel_l2(xg.grad.cpu().numpy(), xo.grad.numpy())
    print(f"[{name}/{cfg['TRAINING_OBJ']}] input gradient rel-L2 {err_x:.3e}")
    assert err_x < 2e-5

    worst = []
    for kname, p in m.model.named_parameters():
        assert p.grad is not None, kname
        worst.append((rel_l2(p.grad.cpu().numpy(), om.sd[kname].grad.numpy()), kname))
    worst.sort(reverse=True)
    print(f"[{name}] worst per-tensor gradient errors: {[(round(e, 8), k) for e, k in worst[:3]]}")
    assert worst[0][0] < 1e-4, worst[:8]
    got_all = np.concatenate([p.grad.cpu().numpy().ravel() for _, p in m.model.named_parameters()])
    want_all = np.concatenate([om.sd[k].grad.numpy().ravel() for k, _ in m.model.named_parameters()])
    assert rel_l2(got_all, want_all) < 5e-6


def _chain(den, x0, theta, sigmas):
    x = x0
    for i in range(theta.shape[1]):
        x = theta[0, i] * x + theta[1, i] * den(x, sigmas[i])
    return x


@pytest.mark.parametrize("name,B", [("tiny", 2), ("dataset2", 1)])
def test_chained_denoise_gradients(name, B):
    """x_{i+1} = theta[0,i] x_i + theta[1,i] denoise(x_i, sigma_i): the gradients reach theta and x_0 through every call."""
    m, cfg = seeded_model_cfg(name)
    x, E, layers, _, w = _inputs(cfg, B, seed=5)
    theta0 = torch.tensor([[0.9, 0.8, 0.7], [0.3, 0.5, 0.6]])
    sigmas = [torch.full((B,), s) for s in (8.0, 1.5, 0.2)]

    om = _oracle(cfg, m)
    th_o = theta0.clone().requires_grad_(True)
    x_o = x.clone().requires_grad_(True)
    (_chain(lambda xi, s: om.denoise(xi, E, s, layers), x_o, th_o, sigmas) * w).sum().backward()

    th = theta0.cuda().requires_grad_(True)
    xg = x.cuda().requires_grad_(True)
    Ec, lc = E.cuda(), _cuda(layers)
    out = _chain(lambda xi, s: m.denoise(xi, E=Ec, sigma=s.cuda(), layers=lc), xg, th, sigmas)
    (out * w.cuda()).sum().backward()
    e_th = rel_l2(th.grad.cpu().numpy(), th_o.grad.numpy())
    e_x = rel_l2(xg.grad.cpu().numpy(), x_o.grad.numpy())
    print(f"[{name}] chain: theta.grad rel-L2 {e_th:.3e}, x0.grad rel-L2 {e_x:.3e}")
    assert e_th < 1e-4 and e_x < 1e-4


def test_vjp_reproduces_training_step_gradients():
    """gy = d(hybrid l2 loss)/dD formed in torch: cd_denoise_vjp then gives cd_train_step's flat gradient."""
    m, cfg = seeded_model_cfg("dataset2")
    B = 2
    gen = torch.Generator().manual_seed(21)
    shape = [B] + list(cfg["SHAPE_PAD"][1:])
    data, noise = torch.randn(shape, generator=gen).cuda(), torch.randn(shape, generator=gen).cuda()
    E = torch.rand((B, 1), generator=gen).cuda()
    layers = torch.randn((B, 1 + cfg["SHAPE_FINAL"][2]), generator=gen).cuda() if "layer" in cfg["SHOWERMAP"] else None
    sigma = torch.tensor([0.4, 3.0]).cuda()
    eng = m.engine()
    cond = m.cond_tensor(E, layers)
    _, flat_train = eng.train_step(data, noise, sigma, cond, "l2")
    x = data + sigma.view(-1, 1, 1, 1, 1) * noise
    D = eng.denoise(x, sigma, cond)
    wgt = (1.0 + sigma.double() ** -2).view(-1, 1, 1, 1, 1)
    gy = (2.0 * wgt * (D.double() - data.double()) / (wgt.mean() * D.numel())).float().contiguous()
    dx, flat = eng.denoise_vjp(x, sigma, cond, gy, param_grads=True)
    # (the parameters' slices only: the flat buffer's alignment gaps are written by neither call)
    got = torch.cat([g.reshape(-1) for g in eng.param_grads(flat)]).cpu().numpy()
    want = torch.cat([g.reshape(-1) for g in eng.param_grads(flat_train)]).cpu().numpy()
    err = rel_l2(got, want)
    print(f"vjp vs training step: flat gradient rel-L2 {err:.3e}")
    assert err < 1e-6
    assert torch.isfinite(dx).all()


@pytest.mark.parametrize("name,B", [("dataset2", 3), ("hgcal", 2)])
def test_input_only_mode_is_the_same_dx(name, B):
    import ctypes as C
    m, cfg = seeded_model_cfg(name)
    x, E, layers, sigma, w = _inputs(cfg, B, seed=9)
    eng = m.engine()
    cond = m.cond_tensor(E.cuda(), _cuda(layers))
    xg, sg, gy = x.cuda(), sigma.cuda(), w.cuda()
    dx_full, flat = eng.denoise_vjp(xg, sg, cond, gy, param_grads=True)
    dx_only, none = eng.denoise_vjp(xg, sg, cond, gy, param_grads=False)
    assert none is None and flat is not None
    assert torch.equal(dx_full, dx_only)
    sizes = []
    for mode in (0, 1):
        n = C.c_size_t()
        assert eng.lib.cd_plan_vjp_workspace_bytes(eng.plan, B, mode, C.byref(n)) == 0
        sizes.append(n.value)
    print(f"[{name}] vjp workspace: input only {sizes[0] / 2**20:.1f} MiB, with grads {sizes[1] / 2**20:.1f} MiB")
    assert sizes[0] < sizes[1]


def test_graph_free_calls_are_unchanged():
    m, cfg = seeded_model_cfg("tiny")
    x, E, layers, sigma, _ = _inputs(cfg, 3, seed=3)
    xc, Ec, lc, sc = x.cuda(), E.cuda(), _cuda(layers), sigma.cuda()
    eng = m.engine()
    want = eng.denoise(xc, sc, m.cond_tensor(Ec, lc))
    out = m.denoise(xc, E=Ec, sigma=sc, layers=lc)  # x does not require grad (the parameters do)
    assert not out.requires_grad and out.grad_fn is None
    assert torch.equal(out, want)
    with torch.no_grad():
        out2 = m.denoise(xc.clone().requires_grad_(True), E=Ec, sigma=sc, layers=lc)
    assert not out2.requires_grad
    assert torch.equal(out2, want)
    xg = xc.clone().requires_grad_(True)
    out3 = m.denoise(xg, E=Ec, sigma=sc, layers=lc)
    assert out3.requires_grad and torch.equal(out3.detach(), want)  # the graph's forward is the same call
    with pytest.raises(NotImplementedError, match="sigma"):
        m.denoise(xg, E=Ec, sigma=sc.clone().requires_grad_(True), layers=lc)
    with pytest.raises(NotImplementedError, match="E"):
        m.denoise(xg, E=Ec.clone().requires_grad_(True), sigma=sc, layers=lc)


def test_parameter_only_gradients_via_requires_grad_x():
    """x.requires_grad_() is the documented switch for parameter gradients alone; a frozen model gets the input-only call."""
    m, cfg = seeded_model_cfg("tiny")
    x, E, layers, sigma, w = _inputs(cfg, 2, seed=4)
    xc, Ec, lc, sc, wc = x.cuda(), E.cuda(), _cuda(layers), sigma.cuda(), w.cuda()
    m.zero_grad()
    xg = xc.clone().requires_grad_(True)
    (m.denoise(xg, E=Ec, sigma=sc, layers=lc) * wc).sum().backward()
    g1 = [p.grad.clone() for p in m.model.parameters()]
    dx1 = xg.grad.clone()
    # a second backward without zero_grad accumulates, as torch does
    xg2 = xc.clone().requires_grad_(True)
    (m.denoise(xg2, E=Ec, sigma=sc, layers=lc) * wc).sum().backward()
    for a, p in zip(g1, m.model.parameters()):
        assert torch.allclose(p.grad, 2 * a, rtol=1e-5, atol=1e-7)
    # frozen parameters: input gradient only, the same bits
    for p in m.model.parameters():
        p.requires_grad_(False)
        p.grad = None
    xg3 = xc.clone().requires_grad_(True)
    (m.denoise(xg3, E=Ec, sigma=sc, layers=lc) * wc).sum().backward()
    assert torch.equal(xg3.grad, dx1)
    assert all(p.grad is None for p in m.model.parameters())


def test_vjp_allocates_nothing_after_the_first_call():
    m, cfg = seeded_model_cfg("tiny")
    x, E, layers, sigma, w = _inputs(cfg, 3, seed=8)
    eng = m.engine()
    cond = m.cond_tensor(E.cuda(), _cuda(layers))
    args = (x.cuda(), sigma.cuda(), cond, w.cuda())
    free = []
    for _ in range(2):
        dx, flat = eng.denoise_vjp(*args, param_grads=True)
        del dx, flat
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert free[1] == free[0], free
