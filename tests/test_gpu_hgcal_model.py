"""GPU (MI355X): HGCal's in-model geometry embedding -- ``CaloDiffusion`` over HGCAL with SHOWER_EMBED 'NN' (no 'pre-embed'), whose
denoise, samplers, loss and gradients act on the cell-space shower (B, 1, 8, 61) with HGCalConverter's enc / dec inside the device
calls (cd_plan_set_geom) and whose two maps train through ``mat * mask`` -- against the reference's own results
(tools/gen_golden_hgcal_model.py) on the synthetic geometry "m".

Bounds: TOL_OP 1e-5 per call and TOL_TRAJ 1e-4 per trajectory (helpers.py), 2e-6 for batch independence and for two forms of
one computation, 5e-6 for gradients (test_gpu_train.py).  The two ``mat`` gradients are held to the larger of 5e-6 and twice the
fixture's ``f64.dist``, the distance of the reference's own float32 gradients from a float64 restatement: 1.9e-6 (embeder.mat)
and 1.6e-6 (decoder.mat) as generated, so the bound is 5e-6 for both."""
import numpy as np
import pytest
import torch

from conftest import gold, rel_l2
from helpers import SEED, TOL_GRAD, TOL_OP, TOL_ROW, TOL_TRAJ, t
import hgcal_model_cases as K

pytestmark = pytest.mark.gpu

BINS = [-1, 1] + list(K.GRID)
_models = {}


def _converter(trainable=True):
    """the fixture's perturbed maps over init()'s masks; frozen: init()'s own maps, as the shipped TRAINABLE_EMBED False has them"""
    from calodiffusion_amd import hgcal
    g = gold("hgcal_model")
    if trainable:
        return hgcal.HGCalConverter.from_matrices(BINS, g["nn.embeder.mat"], g["nn.decoder.mat"], g["init.enc_mask"], g["init.dec_mask"],
                                                  trainable=True)
    return hgcal.HGCalConverter.from_matrices(BINS, g["init.enc_mat"], g["init.dec_mat"])


def _model(objective="hybrid_weight", time_embed="log", loss_type="l2", fresh=False, trainable=True):
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    key = (objective, time_embed, loss_type, trainable)
    if fresh or key not in _models:
        cfg = K.config(objective, time_embed, LOSS_TYPE=loss_type, TRAINABLE_EMBED=trainable, NN_EMBED=_converter(trainable))
        torch.manual_seed(SEED)
        m = CaloDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=loss_type)
        m.eval()
        if fresh:
            return m
        _models[key] = m
    return _models[key]


def _inputs(*names):
    g = gold("hgcal_model")
    return [t(g[n]).cuda() for n in names]


@pytest.mark.parametrize("objective", K.OBJECTIVES)
@pytest.mark.parametrize("time_embed", K.TIME_EMBEDS)
def test_denoise_against_the_reference(objective, time_embed):
    g = gold("hgcal_model")
    m = _model(objective, time_embed)
    x, E, layers, sigma = _inputs("x", "E", "layers", "sigma")
    with torch.no_grad():
        y3 = m.denoise(x, E=E, sigma=sigma.reshape(3, 1, 1, 1), layers=layers)
        assert tuple(y3.shape) == (3,) + K.STATE
        e3 = rel_l2(y3.cpu().numpy(), g[f"den.{objective}.{time_embed}.b3"])
        y1 = m.denoise(x[:1], E=E[:1], sigma=sigma[:1], layers=layers[:1])
        e1 = rel_l2(y1.cpu().numpy(), g[f"den.{objective}.{time_embed}.b1"])
        rows = [rel_l2(m.denoise(x[i:i + 1], E=E[i:i + 1], sigma=sigma[i:i + 1], layers=layers[i:i + 1]).cpu().numpy(),
                       y3[i:i + 1].cpu().numpy()) for i in range(3)]
    print(f"[{objective} {time_embed}] B=3 {e3:.2e}  B=1 {e1:.2e}  rows of B=3 against B=1 runs {[f'{r:.1e}' for r in rows]}")
    assert e3 < TOL_OP and e1 < TOL_OP
    assert max(rows) < TOL_ROW


def test_denoise_rows_do_not_depend_on_the_batch():
    """B = 130 crosses the batch stride of embed-in and embed-out"""
    m = _model()
    x, E, layers, sigma = _inputs("x", "E", "layers", "sigma")
    gen = torch.Generator().manual_seed(11)
    B = 130
    xb = torch.cat([x, K.eighths(gen, (B - 3,) + K.STATE, -16, 16).cuda()])
    Eb = torch.cat([E, K.eighths(gen, (B - 3, 3), 1, 8).cuda()])
    lb = torch.cat([layers, K.eighths(gen, (B - 3, 1 + K.LAYERS), -8, 8).cuda()])
    sb = torch.cat([sigma, (torch.rand((B - 3,), generator=gen) * 4 - 3).exp().cuda()])
    with torch.no_grad():
        y3 = m.denoise(x, E=E, sigma=sigma, layers=layers)
        yb = m.denoise(xb, E=Eb, sigma=sb, layers=lb)
    err = rel_l2(yb[:3].cpu().numpy(), y3.cpu().numpy())
    print(f"rows [0:3] of B = 130 against B = 3: {err:.2e}")
    assert torch.isfinite(yb).all() and err < TOL_ROW


def test_frozen_maps_against_the_reference():
    """TRAINABLE_EMBED False: denoise, loss and the U-Net's gradients; the converter has no parameters and no gradient slots"""
    g, gg = gold("hgcal_model"), gold("hgcal_model_grads")
    m = _model(trainable=False, fresh=True)
    x, E, layers, sigma = _inputs("x", "E", "layers", "sigma")
    with torch.no_grad():
        err = rel_l2(m.denoise(x, E=E, sigma=sigma, layers=layers).cpu().numpy(), gg["frozen.den"])
    loss = _loss_backward(m)
    want = float(gg["frozen.loss"])
    print(f"[frozen] denoise {err:.2e}  loss {float(loss):.7f} against {want:.7f}")
    assert err < TOL_OP and abs(float(loss) - want) <= 1e-5 * abs(want)
    assert _check_unet_grads("frozen", m, gg, "frozen") < TOL_GRAD
    lay, total = m.engine().grad_layout()
    assert not [k for k in lay if k.startswith("NN_embed")]
    # the input gradient of the frozen model (cd_denoise_vjp launches enc's VJP too)
    xg = x.clone().requires_grad_(True)
    (m.denoise(xg, E=E, sigma=sigma, layers=layers) * _inputs("cot")[0]).sum().backward()
    assert torch.isfinite(xg.grad).all() and bool(xg.grad.any())


def test_identity_maps_are_the_grid_denoiser():
    """cells = alpha * r and identity maps: the cell-space state is the grid"""
    from calodiffusion_amd import hgcal
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    eye = torch.eye(K.E_GRID).expand(K.LAYERS, -1, -1).contiguous()
    for objective in K.OBJECTIVES:
        conv = hgcal.HGCalConverter.from_matrices(BINS, eye, eye, trainable=(objective == "hybrid_weight"))
        cfg = K.config(objective, NN_EMBED=conv, SHAPE_PAD=[-1, 1, K.LAYERS, K.E_GRID])
        torch.manual_seed(SEED)
        cells = CaloDiffusion(cfg, n_steps=cfg["NSTEPS"])
        torch.manual_seed(SEED)
        grid = CaloDiffusion(K.config(objective, SHOWER_EMBED="NN-pre-embed", SHAPE_PAD=[-1, 1] + list(K.GRID)), n_steps=cfg["NSTEPS"])
        gen = torch.Generator().manual_seed(3)
        x = torch.randn((3, 1, K.LAYERS, K.E_GRID), generator=gen).cuda()
        E, layers = torch.rand((3, 3), generator=gen).cuda(), torch.randn((3, 1 + K.LAYERS), generator=gen).cuda()
        sigma = torch.tensor(K.SIGMAS).cuda()
        with torch.no_grad():
            a = cells.denoise(x, E=E, sigma=sigma, layers=layers)
            b = grid.denoise(x.reshape((3, 1) + K.GRID), E=E, sigma=sigma, layers=layers)
        err = rel_l2(a.cpu().numpy(), b.reshape(a.shape).cpu().numpy())
        print(f"[{objective}] identity maps against the grid denoise: {err:.2e}")
        assert err < TOL_ROW


def _check_unet_grads(tag, m, g, prefix):
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
    return worst


def _check_grads(tag, m, g, prefix):
    worst = _check_unet_grads(tag, m, g, prefix)
    f64 = dict(zip((str(n) for n in gold("hgcal_model")["f64.names"]), gold("hgcal_model")["f64.dist"]))
    nn_worst = 0.0
    for name, mod in (("embeder.mat", m.NN_embed.embeder), ("decoder.mat", m.NN_embed.decoder)):
        grad, mask = mod.mat.grad.cpu(), torch.as_tensor(mod.mask).cpu()
        assert grad.shape == mod.mat.shape and bool((grad[~mask] == 0).all()), (tag, name)  # exact zeros outside the mask
        err = rel_l2(K.masked(grad.numpy(), mask.numpy()), g[f"{prefix}.nn.{name}"])
        bound = max(TOL_GRAD, 2.0 * float(f64[name]))
        print(f"[{tag}] NN_embed {name}: {err:.2e} (bound {bound:.1e})")
        nn_worst = max(nn_worst, err / bound)
    assert worst < TOL_GRAD, (tag, worst)
    assert nn_worst < 1.0, (tag, nn_worst)


def _loss_backward(m):
    data, E, layers, noise, rnd = _inputs("data", "E", "layers", "noise", "rnd_normal")
    m.zero_grad()
    loss = m.compute_loss(data, E, noise=noise, layers=layers, rnd_normal=rnd)
    loss.backward()
    return loss


@pytest.mark.parametrize("objective,loss_type", K.LOSS_CASES)
def test_loss_and_gradients_against_the_reference(objective, loss_type):
    g = gold("hgcal_model_grads")
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
    g = gold("hgcal_model_grads")
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


def test_map_gradients_repeat_bitwise_and_freeze():
    m = _model(fresh=True)
    _loss_backward(m)
    first = [p.grad.clone() for p in m.NN_embed.parameters()]
    unet_first = [p.grad.clone() for p in m.model.parameters()]
    assert len(first) == 2
    _loss_backward(m)
    for a, p in zip(first, m.NN_embed.parameters()):
        assert torch.equal(a, p.grad)
    # frozen by requires_grad: no gradient, no slots, and the U-Net's unchanged to the bit
    m.NN_embed.requires_grad_(False)
    _loss_backward(m)
    assert all(p.grad is None for p in m.NN_embed.parameters())
    assert not [k for k in m.engine().grad_layout()[0] if k.startswith("NN_embed")]
    for a, p in zip(unet_first, m.model.parameters()):
        assert torch.equal(a, p.grad)


def test_one_adam_step_moves_the_masked_entries_only():
    from calodiffusion_amd.optim import FusedAdam
    g = gold("hgcal_model_grads")
    m = _model(fresh=True)
    before = [p.detach().clone() for p in m.NN_embed.parameters()]
    masks = [torch.as_tensor(m.NN_embed.enc_mask).cuda(), torch.as_tensor(m.NN_embed.dec_mask).cuda()]
    ref = [p.detach().cpu().clone().requires_grad_(True) for p in m.NN_embed.parameters()]
    for name, r, mask in zip(("embeder.mat", "decoder.mat"), ref, masks):
        r.grad = torch.zeros_like(r)
        r.grad[mask.cpu()] = t(g[f"loss.hybrid_weight.l2.nn.{name}"])
    torch.optim.Adam(ref, lr=1e-3).step()
    opt = FusedAdam(m.parameters(), lr=1e-3)
    _loss_backward(m)
    opt.step()
    for p, b, mask, r in zip(m.NN_embed.parameters(), before, masks, ref):
        moved = p.detach() != b
        assert torch.equal(moved, mask)  # every masked entry moved (its gradient is not 0), nothing else did
        err = rel_l2(p.detach().cpu().numpy(), r.detach().numpy())
        assert err < 1e-6, err
    x, E, layers, sigma = _inputs("x", "E", "layers", "sigma")
    with torch.no_grad():  # the next call reads the moved maps (cd_geom_refresh)
        y = m.denoise(x, E=E, sigma=sigma, layers=layers)
        y0 = _model().denoise(x, E=E, sigma=sigma, layers=layers)
    assert torch.isfinite(y).all() and not torch.equal(y, y0)


def _sampler(name, cfg_over=None):
    from calodiffusion_amd import sample
    return getattr(sample, name)(K.config(**(cfg_over or {})))


@pytest.mark.parametrize("name", ["ddim", "ddpm"])
def test_trajectories_against_the_reference(name):
    g = gold("hgcal_model_samplers")
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
    # the graph-replayed loop (no trajectories, the fused update inside embed-out) ends in the same state
    if name == "ddim":
        x2, _, _ = smp(m, start, E, layers, K.TRAJ_STEPS, 0, False)
        assert rel_l2(x2.cpu().numpy(), x.cpu().numpy()) < TOL_ROW


@pytest.mark.parametrize("tag,cls,n,over", K.OTHER_SAMPLERS)
def test_other_samplers_where_the_reference_runs(tag, cls, n, over):
    g = gold("hgcal_model_samplers")
    m = _model()
    rows = int(g[f"smp.{tag}.rows"])  # 3, or 1 where the reference's (B,) sigma broadcasts against the state at B = 1 only
    start, E, layers = t(g["start"][:rows]).cuda(), t(g["E"][:rows]).cuda(), t(g["layers"][:rows]).cuda()
    x, _, _ = _sampler(cls, over)(m, start, E, layers, n, 0, False)
    assert tuple(x.shape) == (rows,) + K.STATE
    if bool(g[f"smp.{tag}.ran"]):
        err = rel_l2(x.cpu().numpy(), g[f"smp.{tag}.x"])
        print(f"[{tag}] final state at B = {rows}: {err:.2e}")
        assert torch.isfinite(x).all() and err < TOL_TRAJ
    else:  # (the fixture: Heun and DPM2 end in NaN at 4 steps of this untrained model in the reference)
        print(f"[{tag}] no reference result on the cell-space state: the device program ran, finite {bool(torch.isfinite(x).all())}")


def test_step_program_graph_replay_equals_the_eager_run():
    g = gold("hgcal_model_samplers")
    m = _model()
    eng = m.engine()
    start, E, layers = t(g["start"]).cuda(), t(g["E"]).cuda(), t(g["layers"]).cuda()
    prog = _sampler("Euler").build(m, 4, 0).finalize()
    assert prog.op_begin is None  # a uniform program: the one a step graph replays
    cond = m.cond_tensor(E, layers)
    eager, _, _ = eng.sampler_run(start, cond, prog, use_graph=False)
    r1, _, _ = eng.sampler_run(start, cond, prog, use_graph=True)
    r2, _, _ = eng.sampler_run(start, cond, prog, use_graph=True)
    assert torch.equal(r1, eager) and torch.equal(r1, r2)


def test_generate_ends_in_physical_cells():
    """generate() on the cell-space state needs no geometry: ReverseNormHGCal(embed=False) of what the sampler returns, held to
    the reference's output on the fixture's batch"""
    g = gold("hgcal_model")
    cfg = dict(EMAX=K.RN["emax"], EMIN=K.RN["emin"], logE=K.RN["logE"], MAXDEP=K.RN["max_deposit"], ECUT=0.0)
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    torch.manual_seed(SEED)
    m = CaloDiffusion(K.config(NN_EMBED=_converter(), **cfg), n_steps=50)
    m.eval()
    got, en = m._to_physical(g["rn.vox"], g["rn.e"], g["rn.layerE"], None)
    err = rel_l2(got, g["rn.data"])
    print(f"ReverseNormHGCal(embed=False) of the fixture's cells: {err:.2e}")
    assert got.shape == (3, K.LAYERS, K.CELLS) and err < TOL_OP and np.allclose(en, g["rn.gen"], rtol=1e-6)
    _, E, layers = _inputs("x", "E", "layers")
    out = m.sample(E, layers, num_steps=4)
    assert out.shape == (3,) + K.STATE and np.isfinite(out).all()
    loader = [(E.cpu(), layers.cpu(), None), (E[:2].cpu(), layers[:2].cpu(), None)]
    gen, en = m.generate(loader, 4)
    assert gen.shape == (5, K.LAYERS, K.CELLS) and en.shape == (5, 3) and np.isfinite(gen).all()


def test_refusals_on_the_device_side():
    """maps of another grid, of disagreeing cell counts or without a transposed view: CD_EINVAL; setting one kind of embedding
    clears the other and clearing leaves the grid plan as it was; BNS theta training refuses the plan"""
    from calodiffusion_amd import engine as eng_mod, hgcal
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    import ctypes as C
    cfg_grid = K.config(SHOWER_EMBED="NN-pre-embed", SHAPE_PAD=[-1, 1] + list(K.GRID))
    gen = torch.Generator().manual_seed(5)
    x = torch.randn((3, 1) + K.GRID, generator=gen).cuda()
    E, layers = torch.rand((3, 3), generator=gen).cuda(), torch.randn((3, 1 + K.LAYERS), generator=gen).cuda()
    sigma = torch.tensor(K.SIGMAS).cuda()
    outs = []
    for use in (False, True):
        torch.manual_seed(SEED)
        m = CaloDiffusion(cfg_grid, n_steps=50)
        eng = m.engine()
        if use:
            conv = _converter()
            eng.set_embedding(conv)
            assert eng.state_shape == K.STATE
            with torch.no_grad():
                eng.denoise(x.reshape(3, -1)[:, :K.LAYERS * K.CELLS].reshape((3,) + K.STATE).contiguous(), sigma, m.cond_tensor(E, layers))
            with pytest.raises(ValueError):
                eng.denoise(x, sigma, m.cond_tensor(E, layers))  # a grid-shaped state is refused on the host
            enc, dec = conv.embeder.packed(), conv.decoder.packed()
            lib, s = eng.lib, eng_mod._stream()
            other = hgcal._PackedMap(torch.zeros((K.LAYERS, 32, K.CELLS)), False)          # another grid
            short = hgcal._PackedMap(torch.zeros((K.LAYERS, K.CELLS - 1, K.E_GRID)), False)  # another cell count
            assert lib.cd_plan_set_geom(eng.plan, other.handle, dec.handle, 1, s) == -1 and b"(8, 32, cells)" in lib.cd_last_error()
            assert lib.cd_plan_set_geom(eng.plan, enc.handle, short.handle, 1, s) == -1 and b"60" in lib.cd_last_error()
            bare = C.c_void_p()
            dense = conv.enc_mat.cuda().contiguous()
            eng_mod._check(lib.cd_geom_create(dense.data_ptr(), K.LAYERS, K.E_GRID, K.CELLS, 0, C.byref(bare), s))
            assert lib.cd_plan_set_geom(eng.plan, bare, dec.handle, 1, s) == -1 and b"transposed" in lib.cd_last_error()
            dx = torch.empty_like(dense)
            assert lib.cd_geom_apply_vjp(bare, None, dense.data_ptr(), dx.data_ptr(), None, 1, 1.0, 0.0, 0, s) == -1
            lib.cd_geom_destroy(bare)
            with pytest.raises(ValueError, match="flat-state embedding"):
                eng.bns_theta_grad(x, m.cond_tensor(E, layers), torch.ones((2, 4), device="cuda"), torch.ones((4, 3), device="cuda"))
            eng.set_embedding(None)
        with torch.no_grad():
            outs.append(m.denoise(x, E=E, sigma=sigma, layers=layers))
    assert torch.equal(outs[0], outs[1])
