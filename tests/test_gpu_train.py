"""GPU (MI355X): the training step (loss + every parameter gradient from cd_train_step) against torch autograd through the
CPU oracle, and one optimizer step through the reference's training-loop protocol."""
import numpy as np
import pytest
import torch

from conftest import gold, rel_l2
from grad_cases import oracle_grads, steps_across_batch_sizes
from helpers import seeded_model, seeded_model_cfg, t

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,B", [("tiny", 3), ("dataset2", 2), ("dataset3", 1)])
def test_parameter_gradients_match_autograd(name, B):
    m, cfg = seeded_model_cfg(name)
    gen = torch.Generator().manual_seed(77)
    shape = [B] + list(cfg["SHAPE_PAD"][1:])
    data = torch.randn(shape, generator=gen)
    noise = torch.randn(shape, generator=gen)
    E = torch.rand((B, 3 if cfg.get("HGCAL") else 1), generator=gen)
    layers = torch.randn((B, 1 + cfg["SHAPE_FINAL"][2]), generator=gen) if "layer" in cfg["SHOWERMAP"] else None
    rnd = torch.randn((B,), generator=gen)
    tsteps = torch.randint(0, cfg["NSTEPS"], (B,), generator=gen)  # Dataset-3 (cosine schedule) draws sigma from the table
    sd_cpu = {k[6:]: v.detach().cpu() for k, v in m.state_dict().items()}
    want_loss, want = oracle_grads(cfg, sd_cpu, data, E, noise, layers, rnd, tsteps)

    # Two identical steps (the weight gradients' slot reductions queued and run as one launch, WgradReduceQueue): both against the
    # reference's gradients, and against each other.
    got_steps = []
    for rep in range(2):
        m.zero_grad()
        sigma = m.loss_function.draw_sigma(data.cuda(), time=tsteps.cuda(), rnd_normal=rnd.cuda())
        loss = m.loss_function.loss_function(m, data.cuda(), E.cuda(), sigma=sigma, noise=noise.cuda(),
                                             layers=None if layers is None else layers.cuda())
        assert loss.requires_grad and loss.dim() == 0
        assert abs(float(loss) - want_loss) <= 1e-5 * abs(want_loss)
        loss.backward()
        worst = []
        for kname, p in m.model.named_parameters():
            assert p.grad is not None, kname
            err = rel_l2(p.grad.cpu().numpy(), want[kname].numpy())
            worst.append((err, kname))
        worst.sort(reverse=True)
        print(f"[{name}] step {rep}: worst per-tensor gradient errors: {[(round(e, 8), k) for e, k in worst[:3]]}")
        assert worst[0][0] < 1e-4, worst[:8]
        # all gradients together
        got_all = np.concatenate([p.grad.cpu().numpy().ravel() for _, p in m.model.named_parameters()])
        want_all = np.concatenate([want[k].numpy().ravel() for k, _ in m.model.named_parameters()])
        print(f"[{name}] step {rep}: all gradients together: {rel_l2(got_all, want_all):.3e}")
        assert rel_l2(got_all, want_all) < 5e-6
        got_steps.append(got_all)
    assert rel_l2(got_steps[1], got_steps[0]) < 1e-6


def test_training_loop_protocol_one_adam_step():
    """zero_grad -> compute_loss -> backward -> Adam.step, as TrainDiffusion.training_loop does (train_diffusion.py:52-63);
    the updated weights are picked up by the next forward."""
    m, cfg = seeded_model_cfg("tiny")
    opt = torch.optim.Adam(m.parameters(), lr=2e-5)  # small steps: the loss must go down monotonically on a fixed batch
    gen = torch.Generator().manual_seed(5)
    data = torch.randn((4, 1, 8, 8, 8), generator=gen).cuda()
    E, layers = torch.rand((4, 3), generator=gen).cuda(), torch.randn((4, 9), generator=gen).cuda()
    noise, rnd = torch.randn(data.shape, generator=gen).cuda(), torch.randn((4,), generator=gen).cuda()
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss = m.compute_loss(data, E, noise=noise, layers=layers, rnd_normal=rnd)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert np.isfinite(losses).all() and losses[3] < losses[2] < losses[1] < losses[0], losses
    with torch.no_grad():
        l_eval = m.compute_loss(data, E, noise=noise, layers=layers, rnd_normal=rnd)
    assert not l_eval.requires_grad and float(l_eval) < losses[0]


def test_fused_adam_matches_torch_adam():
    """cd_adam_step against torch.optim.Adam on the CPU (the optimizer of train/train.py:144): parameters, both moments and the
    checkpointable state after several steps, odd sizes, a learning-rate change in between, weight decay."""
    from calodiffusion_amd.optim import FusedAdam
    gen = torch.Generator().manual_seed(5)
    shapes = [(32, 32, 3, 3, 3), (96,), (7, 13), (1,), (64, 128)]
    for wd in (0.0, 1e-2):
        ref = [torch.randn(s, generator=gen).requires_grad_() for s in shapes]
        dev = [p.detach().clone().cuda().requires_grad_() for p in ref]
        o_ref = torch.optim.Adam(ref, lr=3e-3, weight_decay=wd)
        o_dev = FusedAdam(dev, lr=3e-3, weight_decay=wd)
        for it in range(6):
            for p, q in zip(ref, dev):
                g = torch.randn(p.shape, generator=gen) * (10.0 ** (it - 3))
                p.grad = g.clone()
                q.grad = g.clone().cuda()
            if it == 3:
                for o in (o_ref, o_dev):
                    o.param_groups[0]["lr"] = 1e-3
            o_ref.step()
            o_dev.step()
        for p, q in zip(ref, dev):
            assert rel_l2(q.detach().cpu().numpy(), p.detach().numpy()) < 1e-6
            assert rel_l2(o_dev.state[q]["exp_avg"].cpu().numpy(), o_ref.state[p]["exp_avg"].numpy()) < 1e-6
            assert rel_l2(o_dev.state[q]["exp_avg_sq"].cpu().numpy(), o_ref.state[p]["exp_avg_sq"].numpy()) < 1e-6
        # state_dict interchange with torch.optim.Adam
        o_t = torch.optim.Adam(dev, lr=1e-3, weight_decay=wd)
        o_t.load_state_dict(o_dev.state_dict())
        assert int(o_t.state[dev[0]]["step"]) == 6


def test_queued_weight_gradient_reductions_follow_the_batch_size():
    """The weight gradients' partials wait for their single reduction launch in blocks of the step's own workspace, which the
    engine sizes per batch size: batch 2, 2, 5, 5, 2 on one model -- every step, the first at a new batch size included, queues
    the same way -- every step against autograd through the oracle."""
    steps_across_batch_sizes()


def test_immediate_weight_gradient_reductions_follow_the_batch_size():
    """The same steps with every slot reduction launched where it arises (CD_NO_WGRAD_QUEUE=1), in a child process: the library
    reads the switch once."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys; sys.path[:0] = [%r, %r]; from grad_cases import steps_across_batch_sizes; steps_across_batch_sizes()"
    subprocess.run([sys.executable, "-c", code % (root, os.path.join(root, "tests"))], check=True,
                   env=dict(os.environ, CD_NO_WGRAD_QUEUE="1"), timeout=900)


def _dataset2_step(m, B, seed):
    gen = torch.Generator().manual_seed(seed)
    data = torch.randn((B, 1, 45, 16, 9), generator=gen)
    noise = torch.randn(data.shape, generator=gen)
    E, layers = torch.rand((B, 1), generator=gen), torch.randn((B, 46), generator=gen)
    sigma = 0.05 + 30.0 * torch.rand((B,), generator=gen)
    return data.cuda(), noise.cuda(), sigma.cuda(), m.cond_tensor(E.cuda(), layers.cuda())


def test_a_training_step_allocates_no_device_memory_of_its_own():
    """cd_train_step keeps all its scratch -- the queued weight gradients' partials, the input-gradient weight images, the max-|x|
    words -- in the caller's workspace (include/calodiff.h): on a fresh Dataset-2 engine, steps at batch 1, 2, 1 take no device
    memory besides what torch allocates (workspaces, gradient buffers).  Kernels and the autotune are warmed on a throwaway engine
    first (code objects and the tuner's timing runs are the process's, not the step's)."""
    warm, _ = seeded_model_cfg("dataset2")
    for B in (1, 2):
        warm.engine().train_step(*_dataset2_step(warm, B, B))
    torch.cuda.synchronize()
    m, _ = seeded_model_cfg("dataset2")
    eng = m.engine()
    torch.cuda.synchronize()
    free0, reserved0 = torch.cuda.mem_get_info()[0], torch.cuda.memory_reserved()
    for B in (1, 2, 1):
        eng.train_step(*_dataset2_step(m, B, 10 + B))
    torch.cuda.synchronize()
    free1, reserved1 = torch.cuda.mem_get_info()[0], torch.cuda.memory_reserved()
    own = (free0 - free1) - (reserved1 - reserved0)
    print(f"device memory taken by the steps: {(free0 - free1) / 2**20:.1f} MiB, by torch: {(reserved1 - reserved0) / 2**20:.1f} MiB, "
          f"by the library: {own / 2**20:.1f} MiB")
    assert own < 64 << 20


def test_the_first_training_step_equals_the_steady_state():
    """A fresh plan's first cd_train_step takes the path of every later one (the reductions queued from the start): two steps on
    identical inputs give bitwise-equal loss and gradients.  The autotune (per process, keyed by shape) is warmed on a throwaway
    engine first, so that both steps run the same kernels."""
    B = 2
    warm, _ = seeded_model_cfg("dataset2")
    warm.engine().train_step(*_dataset2_step(warm, B, 21))
    m, _ = seeded_model_cfg("dataset2")
    eng = m.engine()
    args = _dataset2_step(m, B, 21)
    steps = []
    for _ in range(2):
        loss, flat = eng.train_step(*args)
        steps.append((float(loss), torch.cat([g.flatten() for g in eng.param_grads(flat)]).cpu()))
    assert steps[0][0] == steps[1][0], (steps[0][0], steps[1][0])
    assert torch.equal(steps[0][1], steps[1][1])


@pytest.mark.parametrize("obj", ["noise_pred", "mean_pred"])
def test_objectives_match_the_reference(obj):
    """TRAINING_OBJ noise_pred / mean_pred: cd_denoise objectives 1 / 2 (calodiffusion.py:161-165) at three noise levels, a 6-step
    DDIM trajectory on that denoiser, and the loss classes of models/loss.py:181-210 -- value (cd_loss_hybrid) and every
    gradient (cd_train_step) for LOSS_TYPE l2 and huber -- against the reference (tests/golden/objectives_tiny.npz)."""
    g = gold("objectives_tiny")
    data, E, noise, layers = (t(g[k]).cuda() for k in ("data", "E", "noise", "layers"))
    rnd = t(g["rnd_normal"]).cuda()
    m = seeded_model("tiny", {"TRAINING_OBJ": obj, "LOSS_TYPE": "l2", "SAMPLER": "DDim"})  # (the tiny config's own sampler is DDPM)
    assert type(m.loss_function).__name__ == obj and type(m.sampler_algorithm).__name__ == "DDim"
    with torch.no_grad():
        for i, sg in enumerate(g["sigmas"]):
            xin = data * float(np.sqrt(1.0 + float(sg) ** 2))
            got = m.denoise(xin, E=E, sigma=torch.full((4,), float(sg)).cuda(), layers=layers)
            err = rel_l2(got.cpu().numpy(), g[f"{obj}.denoise_{i}"])
            assert err < 1e-5, (obj, i, err)
        x = m.sample(E, layers, num_steps=6, start=data)
        assert rel_l2(x, g[f"{obj}.ddim_6"]) < 1e-4
    for lt in ("l2", "huber"):
        m = seeded_model("tiny", {"TRAINING_OBJ": obj, "LOSS_TYPE": lt})
        m.zero_grad()
        loss = m.compute_loss(data, E, noise=noise, layers=layers, rnd_normal=rnd)
        loss.backward()
        want = float(g[f"{obj}.{lt}.loss"])
        assert abs(float(loss) - want) <= 1e-5 * abs(want), (obj, lt, float(loss), want)
        with torch.no_grad():
            assert abs(float(m.compute_loss(data, E, noise=noise, layers=layers, rnd_normal=rnd)) - want) <= 1e-5 * abs(want)
        grads = dict(m.model.named_parameters())
        pre, worst = f"{obj}.{lt}.grad.", 0.0
        for k in g.files:
            if k.startswith(pre):
                err = rel_l2(grads[k[len(pre):]].grad.cpu().numpy(), g[k])
                worst = max(worst, err)
                assert err < 1e-4, (k, err)
        for k, (s1, s2) in zip(g[f"{obj}.{lt}.ck_keys"], g[f"{obj}.{lt}.ck_vals"]):
            gr = grads[str(k)].grad.double()
            assert abs(float((gr * gr).sum()) - s2) <= 2e-4 * max(s2, 1e-30), (obj, lt, k)
        print(f"[{obj}/{lt}] loss {float(loss):.6f} (reference {want:.6f}); worst whole-tensor gradient error {worst:.2e}")
