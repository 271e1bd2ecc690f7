"""Training steps against autograd through the fp32 CPU oracle, shared by the gradient tests and the child interpreter of
test_gpu_train.py (CD_NO_WGRAD_QUEUE is read once per process)."""
import time

import numpy as np
import torch

from conftest import rel_l2
from helpers import TOL_GRAD, seeded_model_cfg
from oracle import torch_oracle as O


def cuda(t):
    return None if t is None else t.cuda()


def inputs(cfg, B, seed):
    """One batch on the CPU: shower, noise (the VJP's weights w), conditions, and one sigma per sample, log-uniform over
    [0.05, 30]."""
    gen = torch.Generator().manual_seed(seed)
    shape = [B] + list(cfg["SHAPE_PAD"][1:])
    x = torch.randn(shape, generator=gen)
    w = torch.randn(shape, generator=gen)
    E = torch.rand((B, 3 if cfg.get("HGCAL") else 1), generator=gen)
    layers = torch.randn((B, 1 + cfg["SHAPE_FINAL"][2]), generator=gen) if "layer" in cfg["SHOWERMAP"] else None
    sigma = torch.exp(np.log(0.05) + np.log(30.0 / 0.05) * torch.rand((B,), generator=gen))
    tsteps = torch.randint(0, cfg["NSTEPS"], (B,), generator=gen)
    return x, w, E, layers, sigma, tsteps


def oracle_of(cfg, m):
    sd = {k[6:]: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    return O.OracleModel(cfg, sd)


def check_parameter_gradients(tag, m, want):
    """Every parameter tensor of the model against `want` {name: gradient}: the worst tensor and all of them together."""
    worst = []
    for kname, p in m.model.named_parameters():
        assert p.grad is not None, kname
        worst.append((rel_l2(p.grad.cpu().numpy(), want[kname].numpy()), kname))
    worst.sort(reverse=True)
    got_all = np.concatenate([p.grad.cpu().numpy().ravel() for _, p in m.model.named_parameters()])
    want_all = np.concatenate([want[k].numpy().ravel() for k, _ in m.model.named_parameters()])
    err_all = rel_l2(got_all, want_all)
    print(f"[{tag}] worst tensor {worst[0][0]:.3e} ({worst[0][1]}), all gradients together {err_all:.3e}")
    assert worst[0][0] < 1e-4, worst[:8]
    assert err_all < TOL_GRAD
    return got_all


def train_steps_vs_oracle(tag, m, cfg, B, seed, steps=1):
    """`steps` identical training steps, each against autograd through the oracle's loss (test_parameter_gradients_match_autograd's
    assertions); returns [(loss, all gradients)] per step.  The noise level is the loss's own draw from the inputs: exp(1.2 rnd -
    1.2) with rnd placed so that sigma is log-uniform over [0.05, 30] (log schedule), the table's entry of `time` (cosine)."""
    data, noise, E, layers, sigma, tsteps = inputs(cfg, B, seed)
    rnd = (sigma.log() + 1.2) / 1.2
    om = oracle_of(cfg, m)
    t0 = time.perf_counter()
    want_loss = om.hybrid_l2_loss(data, E, noise, layers, rnd_normal=rnd, time=tsteps, n_steps=cfg["NSTEPS"])
    want_loss.backward()
    want_loss, want = float(want_loss.detach()), {k: v.grad for k, v in om.sd.items()}
    t_oracle = time.perf_counter() - t0
    sig = m.loss_function.draw_sigma(data, time=tsteps, rnd_normal=rnd).cuda()  # (on the CPU: the oracle's bits)
    dev = [data.cuda(), E.cuda(), noise.cuda(), cuda(layers)]
    out = []
    for rep in range(steps):
        m.zero_grad()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = m.loss_function.loss_function(m, dev[0], dev[1], sigma=sig, noise=dev[2], layers=dev[3])
        assert loss.requires_grad and loss.dim() == 0
        loss.backward()
        torch.cuda.synchronize()
        t_dev = time.perf_counter() - t0
        got_loss = float(loss.detach())
        err_loss = abs(got_loss - want_loss) / abs(want_loss)
        print(f"[{tag}] step {rep}: loss rel {err_loss:.3e}, device {t_dev:.3f} s, oracle {t_oracle:.2f} s")
        assert err_loss <= 1e-5
        out.append((got_loss, torch.from_numpy(check_parameter_gradients(f"{tag} step {rep}", m, want))))
    return out


def oracle_grads(cfg, sd, data, E, noise, layers, rnd, tsteps):
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    om = O.OracleModel(cfg, sd)
    loss = om.hybrid_l2_loss(data, E, noise, layers, rnd_normal=rnd, time=tsteps)
    loss.backward()
    return float(loss), {k: v.grad for k, v in om.sd.items()}


def steps_across_batch_sizes():
    m, cfg = seeded_model_cfg("tiny")
    sd_cpu = {k[6:]: v.detach().cpu() for k, v in m.state_dict().items()}
    for step, B in enumerate((2, 2, 5, 5, 2)):
        gen = torch.Generator().manual_seed(100 + step)
        shape = [B] + list(cfg["SHAPE_PAD"][1:])
        data, noise = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
        E = torch.rand((B, 3 if cfg.get("HGCAL") else 1), generator=gen)
        layers = torch.randn((B, 1 + cfg["SHAPE_FINAL"][2]), generator=gen) if "layer" in cfg["SHOWERMAP"] else None
        rnd = torch.randn((B,), generator=gen)
        tsteps = torch.randint(0, cfg["NSTEPS"], (B,), generator=gen)
        want_loss, want = oracle_grads(cfg, sd_cpu, data, E, noise, layers, rnd, tsteps)
        m.zero_grad()
        sigma = m.loss_function.draw_sigma(data.cuda(), time=tsteps.cuda(), rnd_normal=rnd.cuda())
        loss = m.loss_function.loss_function(m, data.cuda(), E.cuda(), sigma=sigma, noise=noise.cuda(),
                                             layers=None if layers is None else layers.cuda())
        assert abs(float(loss) - want_loss) <= 1e-5 * abs(want_loss), (step, B)
        loss.backward()
        got_all = np.concatenate([p.grad.cpu().numpy().ravel() for _, p in m.model.named_parameters()])
        want_all = np.concatenate([want[k].numpy().ravel() for k, _ in m.model.named_parameters()])
        assert rel_l2(got_all, want_all) < TOL_GRAD, (step, B, rel_l2(got_all, want_all))
