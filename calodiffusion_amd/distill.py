"""Consistency distillation (Song et al. 2023, Algorithm 2) on the noise grid ``sample.Consistency`` queries: trains the model
that sampler needs from an ordinarily trained ``CaloDiffusion``.  Neither the reference at the commit this package mirrors nor
its ``slurm/submit_training.py`` (which still lists ``consis``) has a trainer for it.

Three weight sets of one architecture: the frozen ``teacher``, the ``student`` that trains, and the ``target``, the EMA of the
student, which is never differentiated.  Per sample, with the grid sigma_0 < ... < sigma_{N-1} (N = CONSIS_NSTEPS) and a drawn
pair (sigma_lo, sigma_hi) = (sigma_k, sigma_{k+1}):

    x_hi = data + sigma_hi noise                         (the launch the training step forms its own input with: the same bits)
    x_lo = one ODE step of the teacher from sigma_hi to sigma_lo            (CONSIS_SOLVER 'heun' (default) | 'euler'; cd_ode_step)
    T    = target.denoise(x_lo, sigma_lo)                                   (a constant)
    loss = CONSIS_LOSS('mse' (default) | 'l1' | 'huber') of student.denoise(x_hi, sigma_hi) - T        (cd_train_step_target)
    after the optimizer's step:  target <- mu target + (1 - mu) student     (CONSIS_EMA, default 0.95; cd_ema_step)

The parametrisation of ``denoise`` is untouched (the boundary condition is left to c_skip / c_out), so the
student is an ordinary ``CaloDiffusion`` checkpoint: load it and set ``SAMPLER: Consistency``."""
from __future__ import annotations

import torch

from . import schedule
from .loss import _TrainStep
from .ops import axpy_sigma, ema_step, ode_step


class _TargetStep:
    """What ``loss._TrainStep`` asks of an engine, with the step's target bound: its one call becomes cd_train_step_target."""

    def __init__(self, engine, target):
        self.engine, self.target = engine, target

    def train_step(self, data, noise, sigma, cond, loss_type):
        return self.engine.train_step_target(data, noise, sigma, cond, self.target, loss_type)

    def param_grads(self, flat):
        return self.engine.param_grads(flat)


class ConsistencyDistillation:
    SOLVERS = ("heun", "euler")
    LOSS_TYPES = ("mse", "l1", "huber")

    def __init__(self, teacher, config=None):
        """``teacher``: a frozen ``CaloDiffusion`` on a regular grid (pre-embedded HGCal included).  ``config``: where the
        CONSIS_* keys are read (the teacher's own config by default)."""
        from .calodiffusion import CaloDiffusion
        from .layerdiffusion import LayerDiffusion
        if isinstance(teacher, LayerDiffusion) or not isinstance(teacher, CaloDiffusion):
            raise NotImplementedError("ConsistencyDistillation: LayerDiffusion's layer stage is not provided (the layer MLP samples "
                                      "in one launch already); distil its base_model as a CaloDiffusion")
        if getattr(teacher, "do_embed", False):
            raise NotImplementedError("ConsistencyDistillation: a model with an in-model geometry embedding (SHOWER_EMBED 'orig-NN', "
                                      "or HGCal's HGCalConverter inside forward) is not provided: cd_train_step_target compares on "
                                      "the grid")
        if any(p.requires_grad for p in teacher.parameters()):
            raise ValueError("ConsistencyDistillation: the teacher's parameters require gradients; the teacher is frozen -- call "
                             "teacher.requires_grad_(False) (the student is the copy that trains)")
        opts = teacher.config if config is None else config
        self.n_grid = int(opts.get("CONSIS_NSTEPS", 100))
        self.solver = opts.get("CONSIS_SOLVER", "heun")
        self.loss_type = opts.get("CONSIS_LOSS", "mse")
        self.mu = float(opts.get("CONSIS_EMA", 0.95))
        if self.n_grid < 2:
            raise ValueError(f"ConsistencyDistillation: CONSIS_NSTEPS = {self.n_grid} leaves no pair of noise levels")
        if self.solver not in self.SOLVERS:
            raise ValueError(f"ConsistencyDistillation: CONSIS_SOLVER {self.solver!r} is not one of {self.SOLVERS}")
        if self.loss_type == "l2":
            raise ValueError("ConsistencyDistillation: CONSIS_LOSS 'l2' is the sigma-weighted form of the training objectives, which "
                             "has no meaning against the target network's output; use 'mse'")
        if self.loss_type not in self.LOSS_TYPES:
            raise ValueError(f"ConsistencyDistillation: CONSIS_LOSS {self.loss_type!r} is not one of {self.LOSS_TYPES}")
        if not 0.0 <= self.mu < 1.0:
            raise ValueError(f"ConsistencyDistillation: CONSIS_EMA = {self.mu} must lie in [0, 1)")
        self.teacher = teacher
        self.student = self._copy_of_teacher(trains=True)
        self.target = self._copy_of_teacher(trains=False)
        self.n_steps = 0
        self._grid = self.sigma_grid()
        self._grid_dev = None

    def _copy_of_teacher(self, trains: bool):
        """A fresh model of the teacher's class and config with the teacher's weights (a deep copy would share the teacher's
        HIP plan); the construction's parameter draws leave the caller's RNG stream where it was."""
        t = self.teacher
        with torch.random.fork_rng(devices=[]):
            m = type(t)(dict(t.config), n_steps=t.nsteps, loss_type=t.loss_type)
        m.load_state_dict(t.state_dict())
        m.to(t.device)
        m.requires_grad_(trains)
        return m

    # ------------------------------------------------------------------ the noise grid
    def sigma_grid(self) -> torch.Tensor:
        """sigma_k = sqrt(1 - acp_k) / sqrt(acp_k) of ``schedule.tables(CONSIS_NSTEPS)``, k = 0..N-1, ascending: the levels
        ``sample.Consistency`` builds as ``t_all_steps``, read backwards (the same bits)."""
        tb = schedule.tables(self.n_grid)
        return tb["sqrt_one_minus_alphas_cumprod"] / tb["sqrt_alphas_cumprod"]

    def pairs(self, index):
        """(sigma_lo, sigma_hi) = (sigma_k, sigma_{k+1}) for every k of ``index`` (an int or an integer tensor), k in 0..N-2."""
        idx = torch.as_tensor(index, dtype=torch.long)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) > self.n_grid - 2):
            raise ValueError(f"ConsistencyDistillation.pairs: pair k is (sigma_k, sigma_k+1) of a grid of {self.n_grid} levels, "
                             f"k in 0..{self.n_grid - 2}; got {index}")
        grid = self._grid
        if idx.is_cuda:
            if self._grid_dev is None or self._grid_dev.device != idx.device:
                self._grid_dev = grid.to(idx.device)
            grid = self._grid_dev
        return grid[idx], grid[idx + 1]

    # ------------------------------------------------------------------ one step
    def inputs(self, data, E, layers, noise, index, staged=None):
        """The constants of one step: (x_hi, x_lo, T, sigma_hi, sigma_lo) on the device.  ``index`` (B,): the pair of every
        sample.  ``staged``: a dict that receives the teacher's outputs D_hi (and, for Heun, x_e and D_e) -- the tests' hook."""
        dev = self.teacher.device
        data, noise = data.to(dev, torch.float32), noise.to(dev, torch.float32)
        E, layers = E.to(dev), None if layers is None else layers.to(dev)
        s_lo, s_hi = self.pairs(torch.as_tensor(index).reshape(-1))
        s_lo, s_hi = s_lo.to(dev), s_hi.to(dev)
        x_hi = axpy_sigma(data, noise, s_hi)
        with torch.no_grad():
            d_hi = self.teacher.denoise(x_hi, E=E, sigma=s_hi, layers=layers)
            x_lo = ode_step(x_hi, d_hi, s_hi, s_lo)
            if staged is not None:
                staged["D_hi"] = d_hi
            if self.solver == "heun":
                d_e = self.teacher.denoise(x_lo, E=E, sigma=s_lo, layers=layers)
                if staged is not None:
                    staged["x_e"], staged["D_e"] = x_lo.clone(), d_e
                ode_step(x_hi, d_hi, s_hi, s_lo, x_e=x_lo, d_e=d_e, out=x_lo)  # (in place over the Euler point)
            target = self.target.denoise(x_lo, E=E, sigma=s_lo, layers=layers)
        return x_hi, x_lo, target, s_hi, s_lo

    def loss(self, data, E, layers, noise=None, index=None):
        """The distillation loss of one batch: an autograd scalar whose ``backward()`` hands the student's parameters their
        gradients as ``compute_loss`` does (``loss._TrainStep``: views of one flat buffer, all-reduced in a data-parallel job).
        ``noise``: unit normals of data's shape; ``index`` (B,): the pair per sample -- both drawn with torch when not given."""
        dev = self.teacher.device
        data = data.to(dev, torch.float32)
        E, layers = E.to(dev), None if layers is None else layers.to(dev)
        B = data.shape[0]
        if noise is None:
            noise = torch.randn_like(data)
        if index is None:
            index = torch.randint(0, self.n_grid - 1, (B,), device=dev).long()
        _, _, target, s_hi, _ = self.inputs(data, E, layers, noise, index)
        step = _TargetStep(self.student.engine(), target)
        cond = self.student.cond_tensor(E, layers)
        noise = noise.to(dev, torch.float32)
        if not torch.is_grad_enabled():
            return step.train_step(data, noise, s_hi, cond, self.loss_type)[0].to(torch.float32)
        return _TrainStep.apply(step, self.loss_type, data, noise, s_hi, cond, *self.student._params())

    @torch.no_grad()
    def update_target(self):
        """target <- mu target + (1 - mu) student over all parameter tensors (cd_ema_step)."""
        ema_step(list(self.target.parameters()), list(self.student.parameters()), self.mu)

    def step(self, optimizer, data, E, layers, noise=None, index=None):
        """zero_grad -> loss -> backward -> optimizer.step -> update_target.  Returns the loss (detached, on the device)."""
        optimizer.zero_grad()
        loss = self.loss(data, E, layers, noise=noise, index=index)
        loss.backward()
        optimizer.step()
        self.update_target()
        self.n_steps += 1
        return loss.detach()

    def fit(self, loader, optimizer, epochs: int = 1):
        """``epochs`` passes over ``loader``, an iterable of (E, layers, data) batches (as ``BespokeNonStationary.optimize_sampler``
        takes them); ``optimizer`` holds the student's parameters (``optim.FusedAdam(d.student.parameters(), lr)``).  Returns
        the losses."""
        dev = self.teacher.device
        losses = []
        for _ in range(int(epochs)):
            for E, layers, data in loader:
                losses.append(self.step(optimizer, data.to(dev, torch.float32), E.to(dev), None if layers is None else layers.to(dev)))
        return [float(v) for v in losses]

    def checkpoint(self) -> dict:
        """``model_state_dict`` is the student's, an ordinary ``CaloDiffusion`` state dict (what ``Train.save`` writes and
        ``load_state_dict`` of either implementation takes); ``target_state_dict`` the EMA network's, to resume from."""
        snap = lambda m: {k: v.detach().clone() for k, v in m.state_dict().items()}  # noqa: E731
        return {"model_state_dict": snap(self.student), "target_state_dict": snap(self.target), "step": self.n_steps}
