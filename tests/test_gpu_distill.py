"""GPU (MI355X): consistency distillation on the device -- the ODE step and the EMA update against their formulas, the training
step against a given target against autograd through the CPU oracle, the composition stage by stage (each stage fed the
device's own output of the one before, so the errors of two denoise calls are never amplified through student - T), three
optimizer steps, and the distilled student through the Consistency sampler."""
import numpy as np
import pytest
import torch

from distill_cases import (N_GRID, batch, frozen_teacher, ode_formula, oracle_of, oracle_step, perturb_, rel, target_away_from)
from grad_cases import check_parameter_gradients, inputs
from helpers import TOL_OP, TOL_TRAJ, seeded_model

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- cd_ode_step
@pytest.mark.parametrize("per", [1, 105, 512, 2053])  # (105: rows off the 16-byte grid; 2053: two workgroups a row, both scalar ends)
@pytest.mark.parametrize("form", ["euler", "heun", "heun_in_place"])
def test_ode_step_matches_the_formula(per, form):
    from calodiffusion_amd.ops import ode_step
    gen = torch.Generator().manual_seed(per)
    B = 3
    x_hi, d_hi, x_e, d_e = (torch.randn((B, per), generator=gen) for _ in range(4))
    s_hi, s_lo = torch.tensor([25.65, 1.184, 0.1295]), torch.tensor([19.7, 1.07, 0.0821])
    guard = torch.full((B * per + 64,), 7.0).cuda()  # the output inside a larger buffer: nothing past its end is written
    out = guard[:B * per].view(B, per)
    if form == "euler":
        want = ode_formula(x_hi, d_hi, s_hi, s_lo)
        got = ode_step(x_hi.cuda(), d_hi.cuda(), s_hi.cuda(), s_lo.cuda(), out=out)
    else:
        want = ode_formula(x_hi, d_hi, s_hi, s_lo, x_e, d_e)
        if form == "heun_in_place":
            out.copy_(x_e)
            got = ode_step(x_hi.cuda(), d_hi.cuda(), s_hi.cuda(), s_lo.cuda(), x_e=out, d_e=d_e.cuda(), out=out)
        else:
            got = ode_step(x_hi.cuda(), d_hi.cuda(), s_hi.cuda(), s_lo.cuda(), x_e=x_e.cuda(), d_e=d_e.cuda(), out=out)
    assert got.data_ptr() == out.data_ptr()
    err = rel(got.cpu().numpy(), want.numpy())
    print(f"ode_step {form} per {per}: rel L2 {err:.2e}")
    assert err <= 1e-6
    for b in range(B):  # every sample with its own pair
        assert rel(got[b].cpu().numpy(), want[b].numpy()) <= 1e-6, b
    assert bool((guard[B * per:] == 7.0).all())


def test_ode_step_without_out_and_refusals():
    from calodiffusion_amd.ops import ode_step
    gen = torch.Generator().manual_seed(2)
    x, d = torch.randn((2, 1, 4, 4, 5), generator=gen).cuda(), torch.randn((2, 1, 4, 4, 5), generator=gen).cuda()
    s_hi, s_lo = torch.tensor([2.0, 0.5]).cuda(), torch.tensor([1.5, 0.4]).cuda()
    got = ode_step(x, d, s_hi, s_lo)
    assert got.shape == x.shape and rel(got.cpu().numpy(), ode_formula(x.cpu(), d.cpu(), s_hi.cpu(), s_lo.cpu()).numpy()) <= 1e-6
    with pytest.raises(ValueError, match="come together"):
        ode_step(x, d, s_hi, s_lo, x_e=x)
    with pytest.raises(ValueError, match="per sample"):
        ode_step(x, d, s_hi[:1], s_lo)


# ---------------------------------------------------------------------------------------------- cd_ema_step
def test_ema_step_matches_torch_over_the_launch_boundary():
    from calodiffusion_amd.ops import ema_step
    gen = torch.Generator().manual_seed(9)
    sizes = [1, 3, 255, 256, 257, 4099] + [int(v) for v in torch.randint(1, 3000, (44,), generator=gen)]
    assert len(sizes) == 50  # two launches: 48 + 2
    mu = 0.95
    ref_dst = [torch.randn(n, generator=gen) for n in sizes]
    ref_src = [torch.randn(n, generator=gen) for n in sizes]
    dst, src = [v.cuda() for v in ref_dst], [v.cuda() for v in ref_src]
    # one pair off the 16-byte grid (views into larger buffers, as a flat parameter buffer's slices are): the one-float-a-lane path
    big_d, big_s = torch.randn(300, generator=gen), torch.randn(300, generator=gen)
    ref_dst[7], ref_src[7] = big_d[1:258].clone(), big_s[3:260].clone()
    dev_d, dev_s = big_d.cuda(), big_s.cuda()
    dst[7], src[7] = dev_d[1:258], dev_s[3:260]
    keep_src = [v.clone() for v in src]
    versions = [v._version for v in dst]
    for _ in range(3):
        ema_step(dst, src, mu)
        ref_dst = [d.mul(mu).add(s, alpha=1 - mu) for d, s in zip(ref_dst, ref_src)]
    worst = max(rel(d.cpu().numpy(), r.numpy()) for d, r in zip(dst, ref_dst))
    print(f"ema_step: worst tensor rel L2 {worst:.2e}")
    for n, d, r in zip(sizes, dst, ref_dst):
        assert rel(d.cpu().numpy(), r.numpy()) <= 1e-6, n
    assert all(torch.equal(a, b) for a, b in zip(src, keep_src))
    assert all(v._version > v0 for v, v0 in zip(dst, versions))
    # the floats around the unaligned view stay what they were
    assert torch.equal(dev_d[:1].cpu(), big_d[:1]) and torch.equal(dev_d[258:].cpu(), big_d[258:])
    # mu = 0 copies
    ema_step(dst, src, 0.0)
    assert all(torch.equal(a, b) for a, b in zip(dst, src))
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        ema_step(dst, src, 1.0)


# ---------------------------------------------------------------------------------------------- cd_train_step_target
def _assign_grads(m, flat):
    for p, g in zip(m._params(), m.engine().param_grads(flat)):
        p.grad = g


@pytest.mark.parametrize("name,B,obj,lt", [("tiny", 3, obj, lt) for obj in ("hybrid_weight", "noise_pred", "mean_pred")
                                           for lt in ("mse", "l1", "huber")] + [("dataset2", 2, "hybrid_weight", "mse")])
def test_train_step_target_matches_autograd(name, B, obj, lt):
    """Loss and every parameter gradient of loss_type(denoise(data + sigma noise) - target), target random, against autograd
    through the oracle's denoise; the project's bounds for these kernels: loss 1e-5, worst tensor 1e-4, all together TOL_GRAD
    (l1 too: the target keeps every |r| above 1e-2, asserted below, so no sign is within rounding of flipping)."""
    m = seeded_model(name, {"TRAINING_OBJ": obj})
    cfg = m.config
    data, noise, E, layers, sigma, _ = inputs(cfg, B, 41)
    om = oracle_of(m, grads=True)
    x_hi = data + sigma.reshape(-1, 1, 1, 1, 1) * noise
    made = {}

    def target_of(out):
        made["T"] = target_away_from(out, 43)
        return made["T"]
    want_loss, want, out = oracle_step(om, x_hi, E, sigma, layers, target_of, lt)
    target = made["T"]
    r = (out - target).abs()
    assert float(r.min()) >= 1e-4 and float(r.min()) < 1.0 < float(r.max())
    eng = m.engine()
    cond = m.cond_tensor(E.cuda(), None if layers is None else layers.cuda())
    loss, flat = eng.train_step_target(data.cuda(), noise.cuda(), sigma.cuda(), cond, target.cuda(), lt)
    err = abs(float(loss) - want_loss) / abs(want_loss)
    print(f"[{name} {obj} {lt}] loss {float(loss):.6f} (oracle {want_loss:.6f}), rel {err:.2e}")
    assert err <= 1e-5
    _assign_grads(m, flat)
    check_parameter_gradients(f"{name} {obj} {lt} target", m, want)
    eng.check_status()


@pytest.mark.parametrize("lt", ["mse", "l1", "huber"])
def test_train_step_target_with_data_is_train_step_bitwise(lt):
    m = seeded_model("tiny")  # (hybrid_weight)
    data, noise, E, layers, sigma, _ = inputs(m.config, 3, 47)
    eng = m.engine()
    args = (data.cuda(), noise.cuda(), sigma.cuda(), m.cond_tensor(E.cuda(), layers.cuda()))
    loss_a, flat_a = eng.train_step(*args, lt)
    loss_b, flat_b = eng.train_step_target(*args, data.cuda(), lt)
    # (every parameter's slice of the flat buffer: the alignment gaps between the slices are never written, by either call)
    grads_a, grads_b = (torch.cat([g.flatten() for g in eng.param_grads(f)]) for f in (flat_a, flat_b))
    assert float(loss_a) == float(loss_b) and torch.equal(grads_a, grads_b)
    assert grads_a.numel() == sum(p.numel() for p in m.model.parameters()) and float(grads_a.abs().sum()) > 0
    with pytest.raises(ValueError, match="'mse'"):
        eng.train_step_target(*args, data.cuda(), "l2")
    with pytest.raises(ValueError, match="data's shape"):
        eng.train_step_target(*args, data[:, :, :4].cuda(), lt)


# ---------------------------------------------------------------------------------------------- the composition
def _three_weight_sets(over):
    """teacher, student and target as three different seeded perturbations of the seeded model: a mix-up of weight sets fails a stage"""
    from calodiffusion_amd.distill import ConsistencyDistillation
    teacher = perturb_(frozen_teacher("tiny", over), 11).requires_grad_(False)
    d = ConsistencyDistillation(teacher)
    perturb_(d.student, 12)
    perturb_(d.target, 13)
    return d


@pytest.mark.parametrize("solver", ["heun", "euler"])
def test_composition_stage_by_stage(solver):
    from calodiffusion_amd.ops import axpy_sigma
    d = _three_weight_sets({"CONSIS_SOLVER": solver})
    assert d.solver == solver
    cfg = d.teacher.config
    B = 3
    data, noise, E, layers, index = batch(cfg, B, 31)
    staged = {}
    x_hi, x_lo, T, s_hi, s_lo = d.inputs(data, E, layers, noise, index, staged)
    grid = d.sigma_grid()
    assert torch.equal(s_lo.cpu(), grid[index]) and torch.equal(s_hi.cpu(), grid[index + 1])
    cpu = lambda v: v.detach().cpu()  # noqa: E731
    # 1. the noised shower: the bits of the launch the training step forms its own input with
    assert torch.equal(x_hi, axpy_sigma(data.cuda(), noise.cuda(), s_hi))
    assert rel(cpu(x_hi).numpy(), (data + grid[index + 1].reshape(-1, 1, 1, 1, 1) * noise).numpy()) <= 1e-6
    ot, og = oracle_of(d.teacher), oracle_of(d.target)
    with torch.no_grad():
        # 2. the teacher at sigma_hi
        e = rel(cpu(staged["D_hi"]).numpy(), ot.denoise(cpu(x_hi), E, cpu(s_hi), layers).numpy())
        print(f"[{solver}] D_hi {e:.2e}")
        assert e < TOL_OP
        # 3. the ODE step on the device's own denoiser outputs
        if solver == "heun":
            assert rel(cpu(staged["x_e"]).numpy(), ode_formula(cpu(x_hi), cpu(staged["D_hi"]), cpu(s_hi), cpu(s_lo)).numpy()) <= 1e-6
            e = rel(cpu(staged["D_e"]).numpy(), ot.denoise(cpu(staged["x_e"]), E, cpu(s_lo), layers).numpy())
            print(f"[{solver}] D_e {e:.2e}")
            assert e < TOL_OP
            want_lo = ode_formula(cpu(x_hi), cpu(staged["D_hi"]), cpu(s_hi), cpu(s_lo), cpu(staged["x_e"]), cpu(staged["D_e"]))
        else:
            assert "x_e" not in staged
            want_lo = ode_formula(cpu(x_hi), cpu(staged["D_hi"]), cpu(s_hi), cpu(s_lo))
        e = rel(cpu(x_lo).numpy(), want_lo.numpy())
        print(f"[{solver}] x_lo {e:.2e}")
        assert e <= 1e-6
        # 4. the target network at the device's x_lo
        e = rel(cpu(T).numpy(), og.denoise(cpu(x_lo), E, cpu(s_lo), layers).numpy())
        print(f"[{solver}] T {e:.2e}")
        assert e < TOL_OP
    # 5. loss and gradients: the student's weights against the device's T
    want_loss, want, out = oracle_step(oracle_of(d.student, grads=True), cpu(x_hi), E, cpu(s_hi), layers, cpu(T), d.loss_type)
    sep = float((out - cpu(T)).norm() / cpu(T).norm())
    print(f"[{solver}] |student - T| / |T| = {sep:.3f}")
    assert sep >= 0.1  # (the last stage compares something)
    loss = d.loss(data, E, layers, noise=noise, index=index)
    assert loss.requires_grad and loss.dim() == 0 and loss.dtype == torch.float32
    loss.backward()
    got_loss = float(loss.detach())
    err = abs(got_loss - want_loss) / abs(want_loss)
    print(f"[{solver}] loss {got_loss:.6f} (oracle {want_loss:.6f}), rel {err:.2e}")
    assert err <= 1e-5
    check_parameter_gradients(f"distill {solver}", d.student, want)
    assert all(p.grad is None for p in d.teacher.parameters()) and all(p.grad is None for p in d.target.parameters())


# ---------------------------------------------------------------------------------------------- steps and the sampler
def _flat(model):
    return torch.cat([p.detach().flatten() for p in model.parameters()]).cpu()


def _three_steps():
    """Three step() calls with FusedAdam on fixed batches -> (distillation, (teacher, student) before the first,
    [(target before, target after, student after, loss) of each step])."""
    from calodiffusion_amd.optim import FusedAdam
    d = _three_weight_sets({})
    start = (_flat(d.teacher), _flat(d.student))
    opt = FusedAdam(d.student.parameters(), lr=1e-4)
    trace = []
    for i in range(3):
        data, noise, E, layers, index = batch(d.teacher.config, 3, 60 + i)
        before = _flat(d.target)
        loss = d.step(opt, data, E, layers, noise=noise, index=index)
        trace.append((before, _flat(d.target), _flat(d.student), float(loss)))
    return d, start, trace


def test_three_steps_and_the_consistency_sampler():
    from calodiffusion_amd import sample
    from oracle import samplers_oracle as S
    from oracle import torch_oracle as O
    _three_steps()  # (the process's kernel choices are made: the two runs below launch the same kernels)
    d, (teacher0, student0), trace = _three_steps()
    d2, start2, trace2 = _three_steps()
    assert torch.equal(start2[0], teacher0) and torch.equal(start2[1], student0) and not torch.equal(teacher0, student0)
    assert torch.equal(_flat(d.teacher), teacher0)  # frozen, to the bit
    prev = student0
    for i, (before, after, student, loss) in enumerate(trace):
        assert np.isfinite(loss) and not torch.equal(student, prev), i
        want = before.mul(d.mu).add(student, alpha=1 - d.mu)  # the lerp of its previous value and the NEW student
        assert rel(after.numpy(), want.numpy()) <= 1e-6, i
        prev = student
    for a, b in zip(trace, trace2):  # two runs from the same seeds
        assert a[3] == b[3] and all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
    assert d.n_steps == 3 and d.checkpoint()["step"] == 3
    for m in (d.teacher, d.student, d.target):
        m.engine().check_status()
        assert m.engine().range_fallbacks == 0

    # end of the road: the student's checkpoint under SAMPLER: Consistency, two denoise calls a shower
    m = seeded_model("tiny", {"SAMPLER": "Consistency", "CONSIS_NSTEPS": N_GRID}, seed=5)
    m.load_state_dict(d.checkpoint()["model_state_dict"])
    assert isinstance(m.sampler_algorithm, sample.Consistency)
    gen = torch.Generator().manual_seed(71)
    B = 3
    start, step_noise = torch.randn((B, 1, 8, 8, 8), generator=gen), torch.randn((B, 1, 8, 8, 8), generator=gen)
    E, layers = torch.rand((B, 3), generator=gen), torch.randn((B, 9), generator=gen)
    m.sampler_algorithm.step_noise = step_noise[None].cuda()
    got = m.sample(E.cuda(), layers.cuda(), num_steps=2, start=start.cuda())
    om = oracle_of(d.student)
    with torch.no_grad():
        den = lambda x, s: om.denoise(x, E, torch.as_tensor(s, dtype=torch.float32).expand(B), layers)  # noqa: E731
        want, _, _ = S.consistency(den, start, O.ddim_tables(N_GRID), N_GRID, 2, iter([step_noise]))
    err = rel(got, want.numpy())
    print(f"Consistency, 2 steps, distilled student: rel L2 {err:.2e}")
    assert np.isfinite(got).all() and err < TOL_TRAJ
