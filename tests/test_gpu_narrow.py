"""GPU (MI355X): narrow U-Net widths.  A plan whose config has 8-, 16-, 24- or 48-channel levels runs them widened (DESIGN,
"Narrow U-Net widths"): the Dataset-1 pion config ([16, 16, 16, 32], in-model NNConverter on 7 x 10 x 23) and [16, 16, 32, 64] on
the 8 x 8 x 8 grid of ``tiny`` against the reference's own results (tools/gen_golden_narrow.py), the device's map against the
restated one (narrow_cases.py), and the widths the rule refuses.

Bounds, the project's own (test_gpu_ds1_model.py, test_gpu_train.py): 1e-5 one denoise call, 1e-4 a trajectory, 2e-6 rows of a batch
against the same rows alone, 1e-5 relative the loss, 1e-4 the worst gradient tensor, 5e-6 all gradients together, 2e-5 dx.  The whole
gradient of a model does not fit a fixture: the fixture holds a few whole tensors, checksums of all and the NN_embed gradients in
full; "all together" is taken against float32 autograd through the CPU oracle, which test_narrow_host.py holds to the fixture."""
import numpy as np
import pytest
import torch

from conftest import gold, rel_l2
from helpers import SEED, TOL_GRAD, TOL_OP, TOL_ROW, TOL_TRAJ, t
from oracle import torch_oracle as O
import narrow_cases as N

pytestmark = pytest.mark.gpu

TOL_LOSS, TOL_GRAD_WORST, TOL_GRAD_ALL, TOL_DX = 1e-5, 1e-4, TOL_GRAD, 2e-5
_models = {}


def _model(objective="hybrid_weight", time_embed="log", loss_type="l2", fresh=False):
    """The seeded pion model with the fixture's perturbed NN_embed matrices (one per case, shared by the tests that only read it)."""
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    key = (objective, time_embed, loss_type)
    if fresh or key not in _models:
        cfg = N.config(objective, time_embed, LOSS_TYPE=loss_type)
        torch.manual_seed(SEED)
        m = CaloDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=loss_type)
        g = gold("narrow_pion")
        m.NN_embed.load_state_dict({k[3:]: t(g[k]) for k in g.files if k.startswith("nn.")})
        m.eval()
        if fresh:
            return m
        _models[key] = m
    return _models[key]


def _grid_model(widths, sd=None):
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    cfg = N.tiny_config(widths)
    torch.manual_seed(SEED)
    m = CaloDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"])
    if sd is not None:
        m.model.load_state_dict(sd)
    return m, cfg


def _inputs(*names, fixture="narrow_pion"):
    g = gold(fixture)
    return [t(g[n]).cuda() for n in names]


def _sampler(name):
    from calodiffusion_amd import sample
    return getattr(sample, name)(N.config())


@pytest.mark.parametrize("objective", N.OBJECTIVES)
@pytest.mark.parametrize("time_embed", N.TIME_EMBEDS)
def test_pion_denoise_against_the_reference(objective, time_embed):
    g = gold("narrow_pion")
    m = _model(objective, time_embed)
    x, E, layers, sigma = _inputs("x", "E", "layers", "sigma")
    with torch.no_grad():
        y3 = m.denoise(x, E=E, sigma=sigma.reshape(3, 1), layers=layers)
        assert tuple(y3.shape) == (3, N.V)
        e3 = rel_l2(y3.cpu().numpy(), g[f"den.{objective}.{time_embed}.b3"])
        y1 = m.denoise(x[:1], E=E[:1], sigma=sigma[:1], layers=layers[:1])
        e1 = rel_l2(y1.cpu().numpy(), g[f"den.{objective}.{time_embed}.b1"])
        row = rel_l2(y1.cpu().numpy(), y3[:1].cpu().numpy())
    print(f"[{objective} {time_embed}] B=3 {e3:.2e}  B=1 {e1:.2e}  rows [0:1] of B=3 against the B=1 run {row:.2e}")
    assert e3 < TOL_OP and e1 < TOL_OP
    assert row < TOL_ROW


def _check_fixture_grads(tag, m, g, prefix):
    """the fixture's whole tensors (worst of them), the checksums of every U-Net gradient, the NN_embed gradients"""
    unet = dict(m.model.named_parameters())
    worst = (0.0, "")
    for k in g.files:
        if k.startswith(prefix + ".grad."):
            name = k[len(prefix) + 6:]
            worst = max(worst, (rel_l2(unet[name].grad.cpu().numpy(), g[k]), name))
    for k, (s1, s2) in zip(g[prefix + ".ck_keys"], g[prefix + ".ck_vals"]):
        gr = unet[str(k)].grad.double()
        assert abs(float((gr * gr).sum()) - s2) <= 2e-4 * max(s2, 1e-30), (tag, k)
    nn_worst = (0.0, "")
    for k, p in m.NN_embed.named_parameters():
        nn_worst = max(nn_worst, (rel_l2(p.grad.cpu().numpy(), g[f"{prefix}.nn.{k}"]), k))
    print(f"[{tag}] worst stored U-Net tensor {worst[0]:.2e} ({worst[1]}), worst NN_embed matrix {nn_worst[0]:.2e} ({nn_worst[1]})")
    assert worst[0] < TOL_GRAD_WORST, (tag, worst)
    assert nn_worst[0] < TOL_GRAD_WORST, (tag, nn_worst)


def _check_all_together(tag, named, want):
    """every gradient against float32 autograd through the oracle: the worst tensor and all together"""
    errs = sorted(((rel_l2(p.grad.cpu().numpy(), want[k].numpy()), k) for k, p in named if float(want[k].abs().max()) > 0), reverse=True)
    got_all = np.concatenate([p.grad.cpu().numpy().ravel() for _, p in named])
    want_all = np.concatenate([want[k].numpy().ravel() for k, _ in named])
    e_all = rel_l2(got_all, want_all)
    print(f"[{tag}] against the oracle: worst tensors {[(f'{e:.2e}', k) for e, k in errs[:3]]}, all together {e_all:.2e}")
    assert errs[0][0] < TOL_GRAD_WORST, errs[:8]
    assert e_all < TOL_GRAD_ALL, e_all


def _pion_oracle_grads(m, cfg, loss_type):
    g = gold("narrow_pion")
    sd = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.model.state_dict().items()}
    Ws = [lay.weight.detach().cpu().clone().requires_grad_(True) for lay in m.NN_embed.encs]
    Ds = [lay.weight.detach().cpu().clone().requires_grad_(True) for lay in m.NN_embed.decs]
    sigma = (t(g["rnd_normal"]) * m.loss_function.P_std + m.loss_function.P_mean).exp()
    loss = N.oracle_loss(cfg, sd, Ws, Ds, N.layout(m.NN_embed.gc), t(g["data"]), t(g["E"]), t(g["noise"]), sigma, t(g["layers"]), loss_type)
    loss.backward()
    want = {"model." + k: v.grad for k, v in sd.items()}
    for i in range(len(Ws)):
        want[f"NN_embed.encs.{i}.weight"], want[f"NN_embed.decs.{i}.weight"] = Ws[i].grad, Ds[i].grad
    return want


def _loss_backward(m):
    data, E, layers, noise, rnd = _inputs("data", "E", "layers", "noise", "rnd_normal")
    m.zero_grad()
    loss = m.compute_loss(data, E, noise=noise, layers=layers, rnd_normal=rnd)
    loss.backward()
    return loss


@pytest.mark.parametrize("objective,loss_type", N.LOSS_CASES)
def test_pion_loss_and_gradients_against_the_reference(objective, loss_type):
    g = gold("narrow_pion_grads")
    m = _model(objective, "log", loss_type, fresh=True)
    tag = f"loss.{objective}.{loss_type}"
    loss = _loss_backward(m).detach()
    want = float(g[tag + ".loss"])
    print(f"[{tag}] loss {float(loss):.7f} against {want:.7f}")
    assert abs(float(loss) - want) <= TOL_LOSS * abs(want)
    with torch.no_grad():
        data, E, layers, noise, rnd = _inputs("data", "E", "layers", "noise", "rnd_normal")
        assert abs(float(m.compute_loss(data, E, noise=noise, layers=layers, rnd_normal=rnd)) - want) <= TOL_LOSS * abs(want)
    for k, p in m.model.named_parameters():  # the caller-facing shapes are the config's own
        assert p.grad is not None and p.grad.shape == p.shape, k
    _check_fixture_grads(tag, m, g, tag)
    _check_all_together(tag, list(m.named_parameters()), _pion_oracle_grads(m, N.config(objective, "log", LOSS_TYPE=loss_type), loss_type))


@pytest.mark.parametrize("objective", N.OBJECTIVES)
def test_pion_denoise_backward_against_the_reference(objective):
    g = gold("narrow_pion_grads")
    m = _model(objective, fresh=True)
    x, E, layers, sigma, cot = _inputs("x", "E", "layers", "sigma", "cot")
    x.requires_grad_(True)
    y = m.denoise(x, E=E, sigma=sigma, layers=layers)
    (y * cot).sum().backward()
    err = rel_l2(x.grad.cpu().numpy(), g[f"vjp.{objective}.dx"])
    print(f"[vjp {objective}] dx {err:.2e}")
    assert err < TOL_DX
    _check_fixture_grads(f"vjp.{objective}", m, g, f"vjp.{objective}")
    # input gradient only: the same bits, and no parameter gets a gradient
    m.zero_grad()
    for p in m.parameters():
        p.requires_grad_(False)
    x2 = x.detach().clone().requires_grad_(True)
    (m.denoise(x2, E=E, sigma=sigma, layers=layers) * cot).sum().backward()
    assert torch.equal(x2.grad, x.grad) and all(p.grad is None for p in m.parameters())


@pytest.mark.parametrize("name", ["ddim", "ddpm"])
def test_pion_trajectories_against_the_reference(name):
    g = gold("narrow_pion_samplers")
    m = _model()
    start, E, layers = t(g["start"]).cuda(), t(g["E"]).cuda(), t(g["layers"]).cuda()
    smp = _sampler("DDim" if name == "ddim" else "DDPM")
    if name == "ddpm":
        smp.step_noise = t(g["ddpm.noise"]).cuda()
    x, xs, x0s = smp(m, start, E, layers, N.TRAJ_STEPS, 0, True)
    ex = rel_l2(x.cpu().numpy(), g[f"{name}.x"])
    exs = rel_l2(torch.stack(xs).cpu().numpy(), g[f"{name}.xs"])
    ex0 = rel_l2(torch.stack(x0s).cpu().numpy(), g[f"{name}.x0s"])
    print(f"[{name}] final {ex:.2e}  xs {exs:.2e}  x0s {ex0:.2e}")
    assert ex < TOL_TRAJ and exs < TOL_TRAJ and ex0 < TOL_TRAJ


def test_pion_step_program_graph_replay_equals_the_eager_run_and_another_sampler_ends_finite():
    g = gold("narrow_pion_samplers")
    m = _model()
    eng = m.engine()
    start, E, layers = t(g["start"]).cuda(), t(g["E"]).cuda(), t(g["layers"]).cuda()
    prog = _sampler("Euler").build(m, 4, 0).finalize()
    assert prog.op_begin is None  # a uniform program: the one a step graph replays
    cond = m.cond_tensor(E, layers)
    eager, _, _ = eng.sampler_run(start, cond, prog, use_graph=False)
    r1, _, _ = eng.sampler_run(start, cond, prog, use_graph=True)
    r2, _, _ = eng.sampler_run(start, cond, prog, use_graph=True)
    print(f"graph replay against eager: {rel_l2(r1.cpu().numpy(), eager.cpu().numpy()):.2e}")
    assert torch.isfinite(eager).all() and torch.equal(r1, eager) and torch.equal(r1, r2)
    x, _, _ = _sampler("LMS")(m, start, E, layers, 5, 0, False)
    assert tuple(x.shape) == (3, N.V) and torch.isfinite(x).all()


def test_pion_sample_and_generate_on_the_flat_state():
    m = _model()
    _, E, layers = _inputs("x", "E", "layers")
    out = m.sample(E, layers, num_steps=4)
    assert out.shape == (3, N.V) and np.isfinite(out).all()
    loader = [(E.cpu(), layers.cpu(), None), (E[:2].cpu(), layers[:2].cpu(), None)]
    gen, en = m.generate(loader, 4, geometry=m.NN_embed)
    assert gen.shape == (5, N.V) and en.shape == (5, 1) and np.isfinite(gen).all() and (gen >= 0).all()


def _tiny_batch(fixture="narrow_tiny"):
    return _inputs("data", "E", "layers", "noise", "rnd_normal", fixture=fixture)


def _tiny_oracle_grads(cfg, sd_cpu):
    g = gold("narrow_tiny")
    om = O.OracleModel(cfg, {k: v.detach().clone().requires_grad_(True) for k, v in sd_cpu.items()})
    loss = om.hybrid_l2_loss(t(g["data"]), t(g["E"]), t(g["noise"]), t(g["layers"]), rnd_normal=t(g["rnd_normal"]))
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in om.sd.items()}


def test_narrow_tiny_against_the_reference():
    """[16, 16, 32, 64] without an embedding: a widened level next to unwidened ones, 16 -> 32 blocks that keep their shortcut"""
    g = gold("narrow_tiny")
    m, cfg = _grid_model(N.TINY_WIDTHS)
    x, E, layers, sigma = _inputs("x", "E", "layers", "sigma", fixture="narrow_tiny")
    with torch.no_grad():
        err = rel_l2(m.denoise(x, E=E, sigma=sigma, layers=layers).cpu().numpy(), g["den.b2"])
    print(f"[narrow tiny] denoise {err:.2e}")
    assert err < TOL_OP
    data, E, layers, noise, rnd = _tiny_batch()
    m.zero_grad()
    loss = m.compute_loss(data, E, noise=noise, layers=layers, rnd_normal=rnd)
    loss.backward()
    loss = loss.detach()
    want = float(g["loss.loss"])
    assert abs(float(loss) - want) <= TOL_LOSS * abs(want)
    unet = dict(m.model.named_parameters())
    worst = max((rel_l2(unet[k[10:]].grad.cpu().numpy(), g[k]), k[10:]) for k in g.files if k.startswith("loss.grad."))
    print(f"[narrow tiny] loss {float(loss):.7f} against {want:.7f}; worst stored tensor {worst[0]:.2e} ({worst[1]})")
    assert worst[0] < TOL_GRAD_WORST, worst
    for k, (s1, s2) in zip(g["loss.ck_keys"], g["loss.ck_vals"]):
        gr = unet[str(k)].grad.double()
        assert abs(float((gr * gr).sum()) - s2) <= 2e-4 * max(s2, 1e-30), k
    _, og = _tiny_oracle_grads(cfg, {k: v.detach().cpu() for k, v in m.model.state_dict().items()})
    _check_all_together("narrow tiny", list(m.model.named_parameters()), og)


def test_device_map_is_the_restated_map():
    """[16, 16, 16, 16] on 8x8x8 (no shortcut conv on either side) against a [32, 32, 32, 32] model loaded with the restated widened
    state_dict: the same launches on the same bits, so denoise is equal to the bit; the narrow plan's gradients are the restated
    fold of the wide model's"""
    narrow, cfg = _grid_model(N.MAP_WIDTHS)
    sd = N.seeded_unet_sd(cfg, SEED, perturb=0.05)
    narrow.model.load_state_dict(sd)
    wide, wcfg = _grid_model([32, 32, 32, 32], N.widen_state_dict(sd, cfg))
    assert list(wide.model.state_dict()) == list(sd)
    x, E, layers, sigma = _inputs("x", "E", "layers", "sigma", fixture="narrow_tiny")
    with torch.no_grad():
        yn = narrow.denoise(x, E=E, sigma=sigma, layers=layers)
        yw = wide.denoise(x, E=E, sigma=sigma, layers=layers)
    assert torch.isfinite(yn).all() and torch.equal(yn, yw)
    data, E, layers, noise, rnd = _tiny_batch()
    grads = []
    for m in (narrow, wide):
        m.zero_grad()
        m.compute_loss(data, E, noise=noise, layers=layers, rnd_normal=rnd).backward()
        grads.append({k: p.grad.cpu() for k, p in m.model.named_parameters()})
    folded = N.fold_grads(grads[1], cfg)
    worst = max((rel_l2(grads[0][k].numpy(), folded[k].numpy()), k) for k in folded if float(folded[k].abs().max()) > 0)
    print(f"narrow plan's gradients against the restated fold of the wide model's: worst tensor {worst[0]:.2e} ({worst[1]})")
    assert worst[0] < 1e-6, worst
    for k in folded:
        assert grads[0][k].shape == sd[k].shape, k


def test_two_fused_adam_steps_follow_torch_adam_on_the_oracle_gradients():
    """All parameters together at test_gpu_train.py's 1e-6 after each of two steps, at the learning rate of that file's
    training-loop test (2e-5).  Adam's first updates are lr g / (|g| + eps): an element whose gradient is of eps's size (1e-8)
    moves by its gradient's ABSOLUTE error, so two float32 gradients that agree to 1e-6 give updates that agree to 6.4e-5
    (measured; 4.4e-4 on downs.1.0.block1.norm.bias, which starts at zero and so IS its updates).  The parameters are held to
    1e-6; a tensor whose gradient had the wrong sign or layout would move them by 2 lr per element, 3e-6 for 16 channels alone."""
    from calodiffusion_amd.optim import FusedAdam
    m, cfg = _grid_model(N.TINY_WIDTHS)
    names = [k for k, _ in m.model.named_parameters()]
    ref = {k: p.detach().cpu().clone().requires_grad_(True) for k, p in m.model.named_parameters()}
    assert sorted(ref) == sorted(m.model.state_dict())
    o_ref = torch.optim.Adam([ref[k] for k in names], lr=2e-5)
    o_dev = FusedAdam(m.parameters(), lr=2e-5)
    data, E, layers, noise, rnd = _tiny_batch()
    start = np.concatenate([ref[k].detach().numpy().ravel() for k in names])
    for step in range(2):
        _, og = _tiny_oracle_grads(cfg, {k: v.detach() for k, v in ref.items()})
        for k in names:
            ref[k].grad = og[k].clone()
        o_ref.step()
        m.zero_grad()
        m.compute_loss(data, E, noise=noise, layers=layers, rnd_normal=rnd).backward()
        o_dev.step()
        got = np.concatenate([p.detach().cpu().numpy().ravel() for _, p in m.model.named_parameters()])
        want = np.concatenate([ref[k].detach().numpy().ravel() for k in names])
        worst = max((rel_l2(p.detach().cpu().numpy(), ref[k].detach().numpy()), k) for k, p in m.model.named_parameters())
        print(f"step {step}: all parameters against torch.optim.Adam {rel_l2(got, want):.2e}, the step itself {rel_l2(got - start, want - start):.2e}; "
              f"worst tensor {worst[0]:.2e} ({worst[1]})")
        assert rel_l2(got, want) < 1e-6, step
        assert rel_l2(want, start) > 1e-5 * (step + 1)  # (the parameters moved: 2e-5 an element, of size ~0.04)


def _train_args(m):
    data, E, layers, noise, rnd = _tiny_batch()
    sigma = m.loss_function.draw_sigma(data, rnd_normal=rnd)
    return data, noise, sigma.reshape(-1), m.cond_tensor(E, layers)


def test_two_train_steps_give_the_same_bits_and_take_no_device_memory():
    m, _ = _grid_model(N.TINY_WIDTHS)
    eng = m.engine()
    args = _train_args(m)
    steps = []
    for _ in range(2):
        loss, flat = eng.train_step(*args)
        steps.append((float(loss), torch.cat([g.flatten() for g in eng.param_grads(flat)]).cpu()))
    assert steps[0][0] == steps[1][0] and torch.equal(steps[0][1], steps[1][1])
    assert steps[0][1].numel() == sum(p.numel() for p in m.model.parameters())
    del flat
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        eng.train_step(*args)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0


@pytest.mark.parametrize("widths,groups,what", [([32, 32, 64, 72], 8, "72"), ([32, 32, 96, 96], 32, "96"), ([32, 32, 64, 288], 8, "288")])
def test_widths_the_rule_rejects_are_refused_at_plan_creation(widths, groups, what):
    """no k of {1, 2, 4} (72 k > 256 before 72 k % 32 == 0; 96 / 32 = 3 a group needs k = 4: 384; 288 > 256): CD_EINVAL from
    cd_plan_create's argument checks, naming the rule"""
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    assert N.widen_factor(int(what), groups) == 0
    cfg = N.tiny_config(widths, BLOCK_GROUPS=groups)
    m = CaloDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"])
    with pytest.raises(ValueError, match=rf"LAYER_SIZE_UNET entry {what} with BLOCK_GROUPS {groups}.*k in \{{1, 2, 4\}}.*multiple of 32"):
        m.engine()
