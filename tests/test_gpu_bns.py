"""GPU (MI355X): the BespokeNonStationary sampler (calodiffusion_amd/sample.py; reference models/sample.py:1013-1122) on the
device -- trajectories against the reference's loop restated on the CPU oracle's denoise with the same sigmas, graph replay,
batch shards and the sigma stream, the layer stage (cd_layer_sampler_run), the refusal of bad DENOISE_PS programs -- and the
theta training: cd_bns_theta_grad against torch autograd through the oracle chain, its determinism and its workspace, and one
optimize_sampler epoch against torch.optim.Adam on the oracle's gradients."""
import copy

import numpy as np
import pytest
import torch

from conftest import rel_l2
from helpers import seeded_model_cfg
from oracle import torch_oracle as O

pytestmark = pytest.mark.gpu


def _cfg(name):
    from calodiffusion_amd.configs import load_config
    cfg = dict(load_config(name))
    cfg["TIME_EMBED"] = "sigma"  # (tiny / dataset2 ship 'log', which BNS refuses; the parameter shapes are the same)
    return cfg


def _model(name):
    return seeded_model_cfg(_cfg(name))


def _oracle(cfg, m):
    return O.OracleModel(cfg, {k[6:]: v.detach().cpu().clone() for k, v in m.state_dict().items()})


def _sampler(cfg, path=None, **opts):
    from calodiffusion_amd.sample import BespokeNonStationary
    c = copy.deepcopy(cfg)
    c["SAMPLER_OPTIONS"] = dict(opts, **({"SAMPLER_PATH": str(path)} if path else {}))
    return BespokeNonStationary(c)


def _inputs(cfg, B, seed):
    gen = torch.Generator().manual_seed(seed)
    shape = [B] + list(cfg["SHAPE_PAD"][1:])
    start = torch.randn(shape, generator=gen)
    E = torch.rand((B, 3 if cfg.get("HGCAL") else 1), generator=gen)
    layers = torch.randn((B, 1 + cfg["SHAPE_FINAL"][2]), generator=gen) if "layer" in cfg["SHOWERMAP"] else None
    return start, E, layers, gen


def _theta(N, gen):
    return torch.stack([0.6 + 0.4 * torch.rand(N, generator=gen), 0.1 + 0.5 * torch.rand(N, generator=gen)])


def _cuda(t):
    return None if t is None else t.cuda()


def _reference_loop(den, x, theta, sigma):
    """BespokeNonStationary.sampler (models/sample.py:1050-1063) with model_fn's sigma draws injected."""
    xs, us = [], []
    for i, (a, b) in enumerate(zip(theta[0], theta[1])):
        us.append(den(x, sigma[i]))
        x = x * a + us[i] * b
        xs.append(x)
    return x, xs, us


def _reference_loss(x, x_prime):
    """models/sample.py:1052-1059."""
    mse = torch.mean((x - x_prime) ** 2)
    if mse == 0:
        return 100
    max_val = torch.max(x, axis=-1).values
    return 20 * torch.log10(max_val / torch.sqrt(mse))


@pytest.mark.parametrize("name,B,N,off", [("tiny", 3, 6, 0), ("dataset3", 2, 4, 0), ("tiny", 3, 6, 2)])
def test_trajectory_matches_the_reference_loop(tmp_path, name, B, N, off):
    m, cfg = _model(name)
    start, E, layers, gen = _inputs(cfg, B, seed=31)
    theta = _theta(N, gen)
    torch.save(torch.nn.Parameter(theta.clone()), tmp_path / "bns.pth")
    sigma = torch.randn((N - off, B), generator=gen)
    smp = _sampler(cfg, tmp_path / "bns.pth")
    smp.step_sigma = sigma
    x, xs, x0s = smp(m, start.cuda(), E.cuda(), _cuda(layers), N, off, True)
    om = _oracle(cfg, m)
    with torch.no_grad():
        wx, wxs, wus = _reference_loop(lambda xi, s: om.denoise(xi, E, s, layers), start, theta[:, off:], sigma)
    assert len(xs) == len(x0s) == N - off
    errs = [rel_l2(x.cpu().numpy(), wx.numpy())]
    errs += [rel_l2(g.cpu().numpy(), w.numpy()) for g, w in zip(xs, wxs)]
    errs += [rel_l2(g.cpu().numpy(), w.numpy()) for g, w in zip(x0s, wus)]
    print(f"[{name} B={B} N={N} off={off}] worst rel-L2 {max(errs):.3e}")
    assert max(errs) <= 2e-5, errs


def test_graph_replay_shards_and_the_sigma_stream(tmp_path):
    from calodiffusion_amd.engine import randn
    m, cfg = _model("tiny")
    G, N = 4, 5
    start, E, layers, gen = _inputs(cfg, G, seed=41)
    torch.save(torch.nn.Parameter(_theta(N, gen)), tmp_path / "bns.pth")
    start, E, layers = start.cuda(), E.cuda(), _cuda(layers)
    base = 12345

    def run(lo, B, graph=True):
        smp = _sampler(cfg, tmp_path / "bns.pth", HIP_GRAPH=graph)
        m.noise_offset = base
        m.set_noise_shard(lo, G if B != G else 0)
        try:
            x, _, _ = smp(m, start[lo:lo + B], E[lo:lo + B], None if layers is None else layers[lo:lo + B], N, 0, False)
        finally:
            m.set_noise_shard(0, 0)
        return x, smp

    x_graph, smp = run(0, G, True)
    x_eager, _ = run(0, G, False)
    assert torch.equal(x_graph, x_eager), "graph replay must equal the eager steps bitwise"
    assert torch.isfinite(x_graph).all()
    # the sigmas: element base + k * G + row of the device stream (base: the model's offset, the start tensor is given)
    want = randn((N, G), "cuda", m.noise_seed, base)
    assert torch.equal(smp.last_sigma, want)
    assert smp.noise_tensors_drawn == 1
    h0, s0 = run(0, G // 2)
    h1, s1 = run(G // 2, G // 2)
    assert torch.equal(s0.last_sigma, want[:, :G // 2]) and torch.equal(s1.last_sigma, want[:, G // 2:])
    assert torch.equal(torch.cat([h0, h1]), x_graph), "two shards must be the rows of the full batch"
    # Diffusion.sample advances the stream past the draws (rounded up to whole tensors)
    smp = _sampler(cfg, tmp_path / "bns.pth")
    m.sampler_algorithm = smp
    m.noise_offset = 0
    m.sample(E, layers, num_steps=N)
    assert m.noise_offset == start.numel() * 2


def test_layer_stage_matches_the_oracle(tmp_path):
    from calodiffusion_amd.configs import load_config
    from calodiffusion_amd.layerdiffusion import LayerDiffusion
    cfg = load_config("dataset2")
    cfg["TIME_EMBED"] = "sigma"
    torch.manual_seed(1234)
    m = LayerDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"])
    B, N, DIM = 3, 6, cfg["SHAPE_FINAL"][2] + 1
    gen = torch.Generator().manual_seed(51)
    start, E = torch.randn((B, DIM), generator=gen), torch.rand((B, 1), generator=gen) + 0.5
    theta = _theta(N, gen)
    torch.save(torch.nn.Parameter(theta.clone()), tmp_path / "bns.pth")
    sigma = torch.randn((N, B), generator=gen)
    smp = _sampler(cfg, tmp_path / "bns.pth")
    smp.step_sigma = sigma
    m.set_layer_state(is_layer=True)
    try:
        x, xs, x0s = smp(m, start.cuda(), E.cuda(), None, N, 0, True)
        with pytest.raises(NotImplementedError, match="layer stage"):
            smp.optimize_sampler(m, [(E, None, start)], N)
    finally:
        m.set_layer_state(is_layer=False)
    om = O.OracleLayerModel(m.config, {k: v.detach().cpu() for k, v in m.layer_model.state_dict().items()})
    with torch.no_grad():
        wx, wxs, wus = _reference_loop(lambda xi, s: om.denoise(xi, E, s), start, theta, sigma)
    errs = [rel_l2(x.cpu().numpy(), wx.numpy())] + [rel_l2(g.cpu().numpy(), w.numpy()) for g, w in zip(xs + x0s, wxs + wus)]
    print(f"layer stage worst rel-L2 {max(errs):.3e}")
    assert max(errs) <= 1e-5, errs


class _Prog:
    def __init__(self, ops, n_bufs=2, n_steps=2, n_coef=3):
        self.ops, self.op_begin, self.n_bufs, self.start_scale, self.n_randn = ops, None, n_bufs, 1.0, 0
        self.coefs = np.full((n_steps, n_coef), 0.5, dtype=np.float32)


def test_out_of_range_sigma_columns_are_refused():
    from calodiffusion_amd.engine import SOP_DENOISE_PS, SOP_LINCOMB
    from calodiffusion_amd.layerdiffusion import LayerDiffusion
    m, cfg = _model("tiny")
    B = 2
    start, E, layers, _ = _inputs(cfg, B, seed=61)
    cond = m.cond_tensor(E.cuda(), _cuda(layers))
    good = [(SOP_DENOISE_PS, 1, (0,), 2), (SOP_LINCOMB, 0, (0, 1), 0)]  # sigma columns 2, 3: n_coef 4
    bad = [(SOP_DENOISE_PS, 1, (0,), 3), (SOP_LINCOMB, 0, (0, 1), 0)]   # columns 3, 4 of 4
    eng = m.engine()
    x, _, _ = eng.sampler_run(start.cuda(), cond, _Prog(good, n_coef=4))
    assert torch.isfinite(x).all()
    with pytest.raises(ValueError, match="sigma columns"):
        eng.sampler_run(start.cuda(), cond, _Prog(bad, n_coef=4))

    lcfg = _cfg("dataset2")
    torch.manual_seed(1234)
    lm = LayerDiffusion(lcfg, n_steps=lcfg["NSTEPS"], loss_type=lcfg["LOSS_TYPE"])
    leng = lm.layer_model.engine()
    ls = torch.randn((B, lcfg["SHAPE_FINAL"][2] + 1)).cuda()
    lE = torch.rand((B, 1)).cuda() + 0.5
    x, _, _ = leng.sampler_run(ls, lE, _Prog(good, n_coef=4))
    assert torch.isfinite(x).all()
    with pytest.raises(ValueError, match="sigma columns"):
        leng.sampler_run(ls, lE, _Prog(bad, n_coef=4))


def _theta_grad_case(name, B, N, seed):
    m, cfg = _model(name)
    start, E, layers, gen = _inputs(cfg, B, seed)
    data = start.abs() + 0.05  # (positive row maxima: a finite loss)
    theta = _theta(N, gen)
    sigma = torch.randn((N, B), generator=gen)
    return m, cfg, data, E, layers, theta, sigma


def _oracle_theta_grad(cfg, m, data, E, layers, theta, sigma):
    om = _oracle(cfg, m)
    th = theta.clone().requires_grad_(True)
    xn, _, _ = _reference_loop(lambda xi, s: om.denoise(xi, E, s, layers), data, th, sigma)
    loss = torch.mean(_reference_loss(data, xn))
    loss.backward()
    return float(loss.detach()), th.grad


@pytest.mark.parametrize("name,B,N", [("tiny", 2, 3), ("tiny", 2, 5), ("dataset3", 1, 3)])
def test_theta_gradient_matches_autograd(name, B, N):
    m, cfg, data, E, layers, theta, sigma = _theta_grad_case(name, B, N, seed=71)
    want_loss, want_g = _oracle_theta_grad(cfg, m, data, E, layers, theta, sigma)
    eng = m.engine()
    cond = m.cond_tensor(E.cuda(), _cuda(layers))
    loss, dth = eng.bns_theta_grad(data.cuda(), cond, theta.cuda(), sigma.cuda())
    e_loss = abs(float(loss) - want_loss) / abs(want_loss)
    e_th = rel_l2(dth.cpu().numpy(), want_g.numpy())
    print(f"[{name} B={B} N={N}] loss {float(loss):.6f} vs {want_loss:.6f} (rel {e_loss:.2e}), dtheta rel-L2 {e_th:.2e}")
    assert e_loss <= 1e-6 and e_th <= 1e-5
    loss2, dth2 = eng.bns_theta_grad(data.cuda(), cond, theta.cuda(), sigma.cuda())
    assert torch.equal(dth, dth2) and float(loss) == float(loss2), "repeated calls must be bitwise equal"
    assert all(p.grad is None for p in m.parameters())


def test_theta_gradient_allocates_nothing():
    m, cfg, data, E, layers, theta, sigma = _theta_grad_case("tiny", 2, 4, seed=81)
    eng = m.engine()
    cond = m.cond_tensor(E.cuda(), _cuda(layers))
    args = (data.cuda(), cond, theta.cuda(), sigma.cuda())
    eng.bns_theta_grad(*args)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(2):
        eng.bns_theta_grad(*args)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0


def test_optimize_sampler_epoch_matches_adam_on_oracle_gradients(tmp_path):
    m, cfg = _model("tiny")
    B, N = 2, 3
    gen = torch.Generator().manual_seed(91)
    batches, sigmas = [], []
    for _ in range(2):
        start, E, layers, _ = _inputs(cfg, B, seed=int(torch.randint(1 << 20, (1,), generator=gen)))
        batches.append((E, layers, start.abs() + 0.05))
        sigmas.append(torch.randn((N, B), generator=gen))
    path = tmp_path / "out" / "theta.pt"
    smp = _sampler(cfg, path, TRAIN_SAMPLER=True, MAX_ITER=1, LR=0.01)
    smp.step_sigma = sigmas
    loader = [(E.cuda(), _cuda(ly), d.cuda()) for E, ly, d in batches]
    theta = smp.optimize_sampler(m, loader, N)

    ref = torch.nn.Parameter(torch.ones(2, N))
    opt = torch.optim.Adam([ref], lr=0.01)
    for (E, ly, d), s in zip(batches, sigmas):
        _, g = _oracle_theta_grad(cfg, m, d, E, ly, ref.detach(), s)
        opt.zero_grad()
        ref.grad = g
        opt.step()
    err = float((theta - ref.detach()).abs().max())
    print(f"theta after one epoch: max |diff| {err:.2e}; losses {smp.losses}")
    assert err <= 1e-6 and len(smp.losses) == 2
    assert all(p.grad is None for p in m.parameters())
    loaded = torch.load(path)
    assert torch.equal(loaded.detach(), theta)
    # TRAIN_SAMPLER: the call samples with the trained theta; a fresh sampler reading the saved file gives the same showers
    start, E, layers, _ = _inputs(cfg, B, seed=92)
    sig = torch.randn((N, B), generator=gen)
    smp.step_sigma = sig
    x1, _, _ = smp(m, start.cuda(), E.cuda(), _cuda(layers), N, 0, False)
    fresh = _sampler(cfg, path)
    fresh.step_sigma = sig
    x2, _, _ = fresh(m, start.cuda(), E.cuda(), _cuda(layers), N, 0, False)
    assert torch.equal(fresh.theta, theta) and torch.equal(x1, x2)
