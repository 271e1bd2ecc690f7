"""GPU (MI355X): the Dataset-1 model -- ``CaloDiffusion`` over SHOWER_EMBED 'orig-NN', whose denoise, samplers, loss and gradients
act on the flat 368-voxel shower with NNConverter's enc / dec inside the device calls (cd_plan_set_radial) -- against the
reference's own results (tools/gen_golden_ds1_model.py) on the synthetic binning file.

Bounds: TOL_OP 1e-5 per call and TOL_TRAJ 1e-4 per trajectory (helpers.py), 2e-6 for batch independence and for two forms of
one computation, 5e-6 for gradients (test_gpu_train.py).  The NN_embed gradients are held to 5e-6 per matrix; the reference's own
float32 gradients lie up to 1.8e-6 (encs) and 3.3e-7 (decs) from a float64 restatement (fixture, ``f64.dist``), so twice that
distance would be the tighter bound where 5e-6 were missed."""
import numpy as np
import pytest
import torch

from conftest import gold, rel_l2
from helpers import SEED, TOL_GRAD, TOL_OP, TOL_ROW, TOL_TRAJ, t
import ds1_model_cases as K
from ds1_model_cases import inputs as _inputs, model as _model

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("objective", K.OBJECTIVES)
@pytest.mark.parametrize("time_embed", K.TIME_EMBEDS)
def test_denoise_against_the_reference(objective, time_embed):
    g = gold("ds1_model")
    m = _model(objective, time_embed)
    x, E, layers, sigma = _inputs("x", "E", "layers", "sigma")
    with torch.no_grad():
        y3 = m.denoise(x, E=E, sigma=sigma.reshape(3, 1), layers=layers)
        assert tuple(y3.shape) == (3, K.V)
        e3 = rel_l2(y3.cpu().numpy(), g[f"den.{objective}.{time_embed}.b3"])
        y1 = m.denoise(x[:1], E=E[:1], sigma=sigma[:1], layers=layers[:1])
        e1 = rel_l2(y1.cpu().numpy(), g[f"den.{objective}.{time_embed}.b1"])
        rows = [rel_l2(m.denoise(x[i:i + 1], E=E[i:i + 1], sigma=sigma[i:i + 1], layers=layers[i:i + 1]).cpu().numpy(),
                       y3[i:i + 1].cpu().numpy()) for i in range(3)]
    print(f"[{objective} {time_embed}] B=3 {e3:.2e}  B=1 {e1:.2e}  rows of B=3 against B=1 runs {[f'{r:.1e}' for r in rows]}")
    assert e3 < TOL_OP and e1 < TOL_OP
    assert max(rows) < TOL_ROW


def test_denoise_rows_do_not_depend_on_the_batch():
    """B = 130 crosses every per-shower stride loop of embed-in and embed-out"""
    m = _model()
    x, E, layers, sigma = _inputs("x", "E", "layers", "sigma")
    gen = torch.Generator().manual_seed(11)
    B = 130
    xb = torch.cat([x, K.eighths(gen, (B - 3, K.V), -16, 16).cuda()])
    Eb = torch.cat([E, K.eighths(gen, (B - 3, 1), 1, 8).cuda()])
    lb = torch.cat([layers, K.eighths(gen, (B - 3, 6), -8, 8).cuda()])
    sb = torch.cat([sigma, (torch.rand((B - 3,), generator=gen) * 4 - 3).exp().cuda()])
    with torch.no_grad():
        y3 = m.denoise(x, E=E, sigma=sigma, layers=layers)
        yb = m.denoise(xb, E=Eb, sigma=sb, layers=lb)
    err = rel_l2(yb[:3].cpu().numpy(), y3.cpu().numpy())
    print(f"rows [0:3] of B = 130 against B = 3: {err:.2e}")
    assert torch.isfinite(yb).all() and err < TOL_ROW


def test_identity_embedding_is_the_grid_denoiser():
    """every layer has all 31 edges and alpha 10, the matrices are the exact identity: the flat state is the grid"""
    from calodiffusion_amd import geom1
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    from calodiffusion_amd.utils import _R_EDGES
    edges = [float(e) for e in _R_EDGES[1]]
    gc = geom1.GeomConverter(all_r_edges=torch.tensor(edges), lay_r_edges=[edges] * 5, alpha_out=10, lay_alphas=[10] * 5,
                             layer_boundaries=[300 * i for i in range(6)])
    conv = geom1.NNConverter(geomconverter=gc)
    with torch.no_grad():
        for p in conv.parameters():
            p.copy_(torch.eye(30))
    for objective in K.OBJECTIVES:
        cfg = K.config(objective, NN_EMBED=conv, SHAPE_ORIG=[-1, 1500])
        torch.manual_seed(SEED)
        flat = CaloDiffusion(cfg, n_steps=400)
        cfg_grid = K.config(objective, SHOWER_EMBED="", SHAPE_PAD=[-1, 1, 5, 10, 30])
        torch.manual_seed(SEED)
        grid = CaloDiffusion(cfg_grid, n_steps=400)
        gen = torch.Generator().manual_seed(3)
        x = torch.randn((3, 1500), generator=gen).cuda()
        E, layers = torch.rand((3, 1), generator=gen).cuda(), torch.randn((3, 6), generator=gen).cuda()
        sigma = torch.tensor(K.SIGMAS).cuda()
        with torch.no_grad():
            a = flat.denoise(x, E=E, sigma=sigma, layers=layers)
            b = grid.denoise(x.reshape(3, 1, 5, 10, 30), E=E, sigma=sigma, layers=layers)
        err = rel_l2(a.cpu().numpy(), b.reshape(3, 1500).cpu().numpy())
        print(f"[{objective}] identity embedding against the grid denoise: {err:.2e}")
        assert err < TOL_ROW


def _check_grads(tag, m, g, prefix):
    unet = dict(m.model.named_parameters())
    worst = 0.0
    for k in g.files:
        if k.startswith(prefix + ".grad."):
            err = rel_l2(unet[k[len(prefix) + 6:]].grad.cpu().numpy(), g[k])
            worst = max(worst, err)
            print(f"[{tag}] U-Net {k[len(prefix) + 6:]}: {err:.2e}")
    for k, (s1, s2) in zip(g[prefix + ".ck_keys"], g[prefix + ".ck_vals"]):
        gr = unet[str(k)].grad.double()
        assert abs(float((gr * gr).sum()) - s2) <= 2e-4 * max(s2, 1e-30), (tag, k)
    nn_worst = 0.0
    for k, p in m.NN_embed.named_parameters():
        err = rel_l2(p.grad.cpu().numpy(), g[f"{prefix}.nn.{k}"])
        nn_worst = max(nn_worst, err)
        print(f"[{tag}] NN_embed {k}: {err:.2e}")
    assert worst < TOL_GRAD, (tag, worst)
    assert nn_worst < TOL_GRAD, (tag, nn_worst)


def _loss_backward(m):
    data, E, layers, noise, rnd = _inputs("data", "E", "layers", "noise", "rnd_normal")
    m.zero_grad()
    loss = m.compute_loss(data, E, noise=noise, layers=layers, rnd_normal=rnd)
    loss.backward()
    return loss


@pytest.mark.parametrize("objective,loss_type", K.LOSS_CASES)
def test_loss_and_gradients_against_the_reference(objective, loss_type):
    g = gold("ds1_model_grads")
    m = _model(objective, "log", loss_type, fresh=True)
    tag = f"loss.{objective}.{loss_type}"
    loss = _loss_backward(m)
    want = float(g[tag + ".loss"])
    print(f"[{tag}] loss {float(loss):.7f} against {want:.7f}")
    assert abs(float(loss) - want) <= 1e-5 * abs(want)
    with torch.no_grad():
        data, E, layers, noise, rnd = _inputs("data", "E", "layers", "noise", "rnd_normal")
        assert abs(float(m.compute_loss(data, E, noise=noise, layers=layers, rnd_normal=rnd)) - want) <= 1e-5 * abs(want)
    _check_grads(tag, m, g, tag)


@pytest.mark.parametrize("objective", K.OBJECTIVES)
def test_denoise_backward_against_the_reference(objective):
    g = gold("ds1_model_grads")
    m = _model(objective, fresh=True)
    x, E, layers, sigma, cot = _inputs("x", "E", "layers", "sigma", "cot")
    x.requires_grad_(True)
    y = m.denoise(x, E=E, sigma=sigma, layers=layers)
    (y * cot).sum().backward()
    err = rel_l2(x.grad.cpu().numpy(), g[f"vjp.{objective}.dx"])
    print(f"[vjp {objective}] dx {err:.2e}")
    assert err < TOL_GRAD
    _check_grads(f"vjp.{objective}", m, g, f"vjp.{objective}")
    # input gradient only: the same bits, and no parameter gets a gradient
    m.zero_grad()
    for p in m.parameters():
        p.requires_grad_(False)
    x2 = x.detach().clone().requires_grad_(True)
    (m.denoise(x2, E=E, sigma=sigma, layers=layers) * cot).sum().backward()
    assert torch.equal(x2.grad, x.grad) and all(p.grad is None for p in m.parameters())


def test_embedding_gradients_repeat_bitwise_and_freeze():
    m = _model(fresh=True)
    _loss_backward(m)
    first = [p.grad.clone() for p in m.NN_embed.parameters()]
    unet_first = [p.grad.clone() for p in m.model.parameters()]
    _loss_backward(m)
    for a, p in zip(first, m.NN_embed.parameters()):
        assert torch.equal(a, p.grad)
    # accumulation without zero_grad: the second gradient is added
    m.zero_grad()
    data, E, layers, noise, rnd = _inputs("data", "E", "layers", "noise", "rnd_normal")
    for _ in range(2):
        m.compute_loss(data, E, noise=noise, layers=layers, rnd_normal=rnd).backward()
    for a, p in zip(first, m.NN_embed.parameters()):
        assert torch.equal(a + a, p.grad)
    # frozen matrices: no gradient, and the U-Net's unchanged to the bit
    m.NN_embed.requires_grad_(False)
    _loss_backward(m)
    assert all(p.grad is None for p in m.NN_embed.parameters())
    for a, p in zip(unet_first, m.model.parameters()):
        assert torch.equal(a, p.grad)


def test_one_adam_step_moves_the_embedding_as_torch_adam_on_the_reference_gradients():
    from calodiffusion_amd.optim import FusedAdam
    g = gold("ds1_model_grads")
    m = _model(fresh=True)
    ref = [p.detach().cpu().clone().requires_grad_(True) for p in m.NN_embed.parameters()]
    for (k, _), r in zip(m.NN_embed.named_parameters(), ref):
        r.grad = t(g[f"loss.hybrid_weight.l2.nn.{k}"]).clone()
    torch.optim.Adam(ref, lr=1e-3).step()
    opt = FusedAdam(m.parameters(), lr=1e-3)
    _loss_backward(m)
    opt.step()
    for (k, p), r in zip(m.NN_embed.named_parameters(), ref):
        err = rel_l2(p.detach().cpu().numpy(), r.detach().numpy())
        assert err < 1e-6, (k, err)
    x, E, layers, sigma = _inputs("x", "E", "layers", "sigma")
    with torch.no_grad():  # the next call reads the moved matrices
        y = m.denoise(x, E=E, sigma=sigma, layers=layers)
        y0 = _model().denoise(x, E=E, sigma=sigma, layers=layers)
    assert torch.isfinite(y).all() and not torch.equal(y, y0)


def _sampler(name, cfg_over=None):
    from calodiffusion_amd import sample
    return getattr(sample, name)(K.config(**(cfg_over or {})))


@pytest.mark.parametrize("name", ["ddim", "ddpm"])
def test_trajectories_against_the_reference(name):
    g = gold("ds1_model_samplers")
    m = _model()
    start, E, layers = t(g["start"]).cuda(), t(g["E"]).cuda(), t(g["layers"]).cuda()
    smp = _sampler("DDim" if name == "ddim" else "DDPM")
    if name == "ddpm":
        smp.step_noise = t(g["ddpm.noise"]).cuda()
    x, xs, x0s = smp(m, start, E, layers, K.TRAJ_STEPS, 0, True)
    ex = rel_l2(x.cpu().numpy(), g[f"{name}.x"])
    exs = rel_l2(torch.stack(xs).cpu().numpy(), g[f"{name}.xs"])
    ex0 = rel_l2(torch.stack(x0s).cpu().numpy(), g[f"{name}.x0s"])
    print(f"[{name}] final {ex:.2e}  xs {exs:.2e}  x0s {ex0:.2e}")
    assert ex < TOL_TRAJ and exs < TOL_TRAJ and ex0 < TOL_TRAJ
    # the graph-replayed loop (no trajectories) ends in the same state
    if name == "ddim":
        x2, _, _ = smp(m, start, E, layers, K.TRAJ_STEPS, 0, False)
        assert rel_l2(x2.cpu().numpy(), x.cpu().numpy()) < TOL_ROW


@pytest.mark.parametrize("tag,cls,n,over", K.OTHER_SAMPLERS)
def test_other_samplers_where_the_reference_runs(tag, cls, n, over):
    g = gold("ds1_model_samplers")
    m = _model()
    rows = int(g[f"smp.{tag}.rows"])  # 3, or 1 where the reference's (B,) sigma broadcasts against (B, 368) at B = 1 only
    start, E, layers = t(g["start"][:rows]).cuda(), t(g["E"][:rows]).cuda(), t(g["layers"][:rows]).cuda()
    x, _, _ = _sampler(cls, over)(m, start, E, layers, n, 0, False)
    assert tuple(x.shape) == (rows, K.V)
    if bool(g[f"smp.{tag}.ran"]):
        err = rel_l2(x.cpu().numpy(), g[f"smp.{tag}.x"])
        print(f"[{tag}] final state at B = {rows}: {err:.2e}")
        assert torch.isfinite(x).all() and err < TOL_TRAJ
    else:  # (the fixture: Heun and DPM2 end in NaN at 4 steps of this untrained model in the reference)
        print(f"[{tag}] no reference result on the flat state: the device program ran, finite {bool(torch.isfinite(x).all())}")


def test_step_program_graph_replay_equals_the_eager_run():
    g = gold("ds1_model_samplers")
    m = _model()
    eng = m.engine()
    start, E, layers = t(g["start"]).cuda(), t(g["E"]).cuda(), t(g["layers"]).cuda()
    smp = _sampler("Euler")
    prog = smp.build(m, 4, 0).finalize()
    assert prog.op_begin is None  # a uniform program: the one a step graph replays
    cond = m.cond_tensor(E, layers)
    eager, _, _ = eng.sampler_run(start, cond, prog, use_graph=False)
    r1, _, _ = eng.sampler_run(start, cond, prog, use_graph=True)
    r2, _, _ = eng.sampler_run(start, cond, prog, use_graph=True)
    err = rel_l2(r1.cpu().numpy(), eager.cpu().numpy())
    print(f"graph replay against eager: {err:.2e}")
    assert err < TOL_ROW and torch.equal(r1, r2)


def test_sample_and_generate_on_the_flat_state():
    m = _model()
    _, E, layers = _inputs("x", "E", "layers")
    out = m.sample(E, layers, num_steps=4)
    assert out.shape == (3, K.V) and np.isfinite(out).all()
    loader = [(E.cpu(), layers.cpu(), None), (E[:2].cpu(), layers[:2].cpu(), None)]
    gen, en = m.generate(loader, 4, reverse_norm=False)
    assert gen.shape == (5, K.V) and en.shape == (5, 1) and np.isfinite(gen).all()
    offset = m.noise_offset
    with pytest.raises(ValueError, match="reverse_norm"):
        m.generate(loader, 4)
    assert m.noise_offset == offset  # raised before sampling


def test_cleared_embedding_leaves_the_grid_plan_as_it_was():
    """After cd_plan_set_radial(plan, NULL, ...) a Dataset-1-grid plan's cd_denoise equals a fresh plan's to the bit; and a map of
    another grid is refused with CD_EINVAL"""
    from calodiffusion_amd import engine as eng_mod
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    import ds1_geom_cases as G1
    cfg_grid = K.config(SHOWER_EMBED="", SHAPE_PAD=[-1, 1, 5, 10, 30])
    gen = torch.Generator().manual_seed(5)
    x = torch.randn((3, 1, 5, 10, 30), generator=gen).cuda()
    E, layers = torch.rand((3, 1), generator=gen).cuda(), torch.randn((3, 6), generator=gen).cuda()
    sigma = torch.tensor(K.SIGMAS).cuda()
    outs = []
    for use in (False, True):
        torch.manual_seed(SEED)
        m = CaloDiffusion(cfg_grid, n_steps=400)
        eng = m.engine()
        if use:
            eng.set_embedding(_model().NN_embed)
            with torch.no_grad():
                eng.denoise(x.reshape(3, -1)[:, :K.V].contiguous(), sigma, m.cond_tensor(E, layers))
            bad = G1.nn_converter("g1").gc.radial_map()  # (5, 10, 28)
            buf = torch.zeros(bad.wtotal, device="cuda")
            code = eng.lib.cd_plan_set_radial(eng.plan, bad.handle, buf.data_ptr(), buf.data_ptr(), 1, eng_mod._stream())
            assert code == -1 and b"(5, 10, 28)" in eng.lib.cd_last_error() and b"(5, 10, 30)" in eng.lib.cd_last_error()
            eng.set_embedding(None)
        with torch.no_grad():
            outs.append(m.denoise(x, E=E, sigma=sigma, layers=layers))
        if use:
            with pytest.raises(NotImplementedError):  # BNS theta training stays refused on an embedded model
                _sampler("BespokeNonStationary", dict(TIME_EMBED="sigma", SAMPLER_PATH="/nonexistent")).optimize_sampler(
                    _model("hybrid_weight", "sigma"), [], 4)
    assert torch.equal(outs[0], outs[1])


def test_a_state_of_the_other_form_is_refused_on_the_host():
    """with an embedding bound the state is (B, V), without one the grid: every entry point checks before the device sees it"""
    m = _model()
    eng = m.engine()
    x, E, layers, sigma = _inputs("x", "E", "layers", "sigma")
    cond = m.cond_tensor(E, layers)
    grid = torch.zeros((3, 1) + K.GRID, device="cuda")
    prog = _sampler("Euler").build(m, 4, 0).finalize()
    from calodiffusion_amd import schedule
    table = schedule.ddim_step_table(4, 0.0, 0)
    for call in (lambda: eng.denoise(grid, sigma, cond), lambda: eng.train_step(grid, grid, sigma, cond),
                 lambda: eng.loss_hybrid(grid, grid, sigma, cond), lambda: eng.ddim_sample(grid, cond, table),
                 lambda: eng.sampler_run(grid, cond, prog), lambda: eng.denoise_vjp(grid, sigma, cond, grid, False),
                 lambda: eng.train_step(x, x[:2], sigma, cond)):
        with pytest.raises(ValueError):
            call()
