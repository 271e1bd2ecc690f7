"""CPU: consistency distillation's host side (calodiffusion_amd/distill.py) -- the noise grid against the one sample.Consistency
queries, the refusals by name, the checkpoint an ordinary CaloDiffusion loads -- and the include graph of its stateless unit."""
import os
import re

import pytest
import torch

from calodiffusion_amd import sample
from calodiffusion_amd.build import CSRC, SOURCES
from calodiffusion_amd.distill import ConsistencyDistillation
from distill_cases import N_GRID, frozen_teacher, perturb_
from helpers import seeded_model


def test_grid_is_the_consistency_samplers_read_backwards():
    teacher = frozen_teacher()
    d = ConsistencyDistillation(teacher)
    grid = d.sigma_grid()
    assert grid.dtype == torch.float32 and grid.shape == (N_GRID,) and bool((grid[1:] > grid[:-1]).all())
    # t_all_steps as Consistency.build forms it (sample.py; models/sample.py:968-985): element by element, from the loss's tables
    lf = teacher.loss_function
    lf.update_step(N_GRID)
    t_all = torch.stack([lf.sqrt_one_minus_alphas_cumprod[N_GRID - t - 1] / lf.sqrt_alphas_cumprod[N_GRID - t - 1] for t in range(N_GRID)])
    lf.update_step(teacher.nsteps)
    assert torch.equal(grid.flip(0), t_all)
    # ... and the levels its 5-step program hands to denoise are grid points, to the bit
    prog = sample.Consistency(teacher.config).build(teacher, 5, 0)
    idx = [0, int(round(N_GRID * 0.5)), int(round(N_GRID * 0.7)), int(round(N_GRID * 0.9)), int(round(N_GRID * 0.95))]
    assert [st.coefs[0] for st in prog._steps] == [float(grid[N_GRID - 1 - i]) for i in idx]
    assert prog.start_scale == float(grid[-1])


def test_pairs():
    d = ConsistencyDistillation(frozen_teacher())
    grid = d.sigma_grid()
    for k in (0, 7, N_GRID - 2):
        lo, hi = d.pairs(k)
        assert float(lo) == float(grid[k]) and float(hi) == float(grid[k + 1])
    lo, hi = d.pairs(torch.tensor([3, 0, N_GRID - 2]))
    assert torch.equal(lo, grid[[3, 0, N_GRID - 2]]) and torch.equal(hi, grid[[4, 1, N_GRID - 1]])
    for bad in (N_GRID - 1, -1, torch.tensor([0, N_GRID - 1])):
        with pytest.raises(ValueError, match=f"0..{N_GRID - 2}"):
            d.pairs(bad)


def test_student_and_target_start_as_copies_of_the_teacher():
    teacher = frozen_teacher()
    d = ConsistencyDistillation(teacher)
    assert d.teacher is teacher and d.solver == "heun" and d.loss_type == "mse" and d.mu == 0.95
    for (k, a), b, c in zip(teacher.state_dict().items(), d.student.state_dict().values(), d.target.state_dict().values()):
        assert torch.equal(a, b) and torch.equal(a, c) and a.data_ptr() != b.data_ptr() != c.data_ptr(), k
    assert all(p.requires_grad for p in d.student.parameters())
    assert not any(p.requires_grad for p in d.target.parameters()) and not any(p.requires_grad for p in teacher.parameters())


def test_construction_leaves_the_callers_rng_stream_alone():
    teacher = frozen_teacher()
    torch.manual_seed(99)
    want = torch.rand(4)
    torch.manual_seed(99)
    ConsistencyDistillation(teacher)
    assert torch.equal(torch.rand(4), want)


def test_refusals_by_name():
    # a teacher that still trains
    with pytest.raises(ValueError, match=r"requires_grad_\(False\)"):
        ConsistencyDistillation(seeded_model("tiny"))
    # an in-model geometry embedding
    emb = frozen_teacher()
    emb.do_embed = True
    with pytest.raises(NotImplementedError, match="in-model geometry embedding"):
        ConsistencyDistillation(emb)
    # LayerDiffusion: its base model is distilled as a CaloDiffusion
    from calodiffusion_amd.layerdiffusion import LayerDiffusion
    torch.manual_seed(1)
    layer = LayerDiffusion(dict(frozen_teacher().config), n_steps=50, loss_type="l2").requires_grad_(False)
    with pytest.raises(NotImplementedError, match="base_model as a CaloDiffusion"):
        ConsistencyDistillation(layer)
    teacher = frozen_teacher()
    with pytest.raises(ValueError, match="'mse'"):
        ConsistencyDistillation(teacher, {"CONSIS_NSTEPS": N_GRID, "CONSIS_LOSS": "l2"})
    with pytest.raises(ValueError, match="CONSIS_LOSS"):
        ConsistencyDistillation(teacher, {"CONSIS_NSTEPS": N_GRID, "CONSIS_LOSS": "lpips"})
    for mu in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            ConsistencyDistillation(teacher, {"CONSIS_NSTEPS": N_GRID, "CONSIS_EMA": mu})
    with pytest.raises(ValueError, match="CONSIS_SOLVER"):
        ConsistencyDistillation(teacher, {"CONSIS_NSTEPS": N_GRID, "CONSIS_SOLVER": "rk4"})
    with pytest.raises(ValueError, match="CONSIS_NSTEPS"):
        ConsistencyDistillation(teacher, {"CONSIS_NSTEPS": 1})
    d = ConsistencyDistillation(teacher, {"CONSIS_NSTEPS": 12, "CONSIS_SOLVER": "euler", "CONSIS_LOSS": "huber", "CONSIS_EMA": 0.0})
    assert (d.n_grid, d.solver, d.loss_type, d.mu) == (12, "euler", "huber", 0.0)


def test_engine_refuses_the_weighted_loss_against_a_target():
    """UnetEngine.train_step_target names 'mse' before it touches the device."""
    from calodiffusion_amd.engine import UnetEngine
    with pytest.raises(ValueError, match="'mse'"):
        UnetEngine.train_step_target(None, None, None, None, None, None, "l2")


def test_checkpoint_loads_into_a_consistency_sampling_model():
    d = ConsistencyDistillation(frozen_teacher())
    perturb_(d.student, 5)
    perturb_(d.target, 6)
    d.n_steps = 3
    ck = d.checkpoint()
    assert sorted(ck) == ["model_state_dict", "step", "target_state_dict"] and ck["step"] == 3
    m = seeded_model("tiny", {"SAMPLER": "Consistency", "CONSIS_NSTEPS": N_GRID}, seed=77)
    assert type(m.sampler_algorithm).__name__ == "Consistency"
    m.load_state_dict(ck["model_state_dict"])
    for (k, a), b in zip(d.student.state_dict().items(), m.state_dict().values()):
        assert torch.equal(a, b), k
    # the reference's loader strips a wrapper's prefix (calodiffusion.py:31-37): the same dict under one loads too
    m2 = seeded_model("tiny", {"SAMPLER": "Consistency", "CONSIS_NSTEPS": N_GRID}, seed=78)
    m2.load_state_dict({"module." + k: v for k, v in ck["target_state_dict"].items()})
    for (k, a), b in zip(d.target.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(a, b), k
    # a snapshot, not a view of the live weights
    perturb_(d.student, 7)
    assert torch.equal(next(iter(ck["model_state_dict"].values())), next(iter(m.state_dict().values())))


# ---------------------------------------------------------------------------------------------- the stateless unit
def _closure(name):
    seen, todo = set(), [name]
    while todo:
        text = open(os.path.join(CSRC, todo.pop())).read()
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', text, re.M):
            path = os.path.normpath(inc)
            if path not in seen and os.path.exists(os.path.join(CSRC, path)):
                seen.add(path)
                todo.append(path)
    return seen


def test_the_distillation_unit_does_not_reach_the_plan():
    """kernels_distill.hip holds kernels and two C-ABI entry points but no launch sequence of the network: it takes guarded() and
    never CdPlan's definition (as tests/test_headers_host.py asks of the other stateless units)."""
    headers = [f for f in os.listdir(CSRC) if f.endswith(".h")]
    defining = [h for h in headers if re.search(r"^struct CdPlan\s*\{", open(os.path.join(CSRC, h)).read(), re.M)]
    assert len(defining) == 1, defining
    assert "kernels_distill.hip" in SOURCES
    reached = _closure("kernels_distill.hip")
    assert "guarded.h" in reached and defining[0] not in reached, reached
    text = open(os.path.join(CSRC, "kernels_distill.hip")).read()
    assert "cd_ode_step" in text and "cd_ema_step" in text and "asm" not in text
