"""CPU: the BespokeNonStationary sampler's host side (calodiffusion_amd/sample.py) -- construction, theta loading with the
reference's paths and errors (models/sample.py:1036-1047, 1113-1122), sample_offset, the step program it hands the engine, the
sigma positions in the noise stream, the 'log' refusal -- and the PSNR loss of cd_bns_theta_grad with its closed-form seed
gradient against torch autograd on the reference's loss_function (:1052-1059)."""
import math
import types

import numpy as np
import pytest
import torch

from calodiffusion_amd import engine
from calodiffusion_amd.engine import SOP_DENOISE_PS, SOP_LINCOMB, SOP_RECORD
from calodiffusion_amd.sample import BespokeNonStationary


def _cfg(tmp_path=None, **opts):
    cfg = {"TIME_EMBED": "sigma", "SAMPLER": "BespokeNonStationary", "SAMPLER_OPTIONS": dict(opts)}
    if tmp_path is not None:
        cfg["flags"] = types.SimpleNamespace(data_folder=str(tmp_path))
    return cfg


class _FakeEngine:
    """Records the program cd_sampler_run would receive."""

    def __init__(self):
        self.calls = []

    def sampler_run(self, start, cond, prog, **kw):
        self.calls.append((prog, kw))
        n = prog.coefs.shape[0]
        traj = torch.zeros((n,) + tuple(start.shape))
        return start.clone(), traj, traj.clone()


class _FakeModel:
    """The attributes of Diffusion the sampler reads: the noise stream (Diffusion.step_noise_stream's arithmetic) and the
    engine."""

    def __init__(self, time_embed="sigma", noise_offset=0, shard=None):
        self.time_embed, self.noise_offset, self.noise_shard, self.noise_seed = time_embed, noise_offset, shard, 7
        self.eng = _FakeEngine()

    def engine(self):
        return self.eng

    def cond_tensor(self, E, layers):
        return E

    def step_noise_stream(self, start):
        per = start[0].numel()
        lo, gb = self.noise_shard or (0, start.shape[0])
        return self.noise_offset + lo * per, gb * per


def _save_theta(path, theta):
    torch.save(torch.nn.Parameter(theta.clone()), path)


def test_constructs():
    smp = BespokeNonStationary(_cfg())
    assert smp.theta is None and smp.step_sigma is None
    BespokeNonStationary(dict(_cfg(), TIME_EMBED="log"))  # (refused when it samples or trains)
    with pytest.raises(NotImplementedError, match="TIME_EMBED 'sigma'"):
        BespokeNonStationary({})  # the default 'sin' embedding: no reference trajectory exists


def test_theta_loading_errors(tmp_path):
    m = _FakeModel()
    start, E = torch.zeros(2, 1, 2, 2, 3), torch.ones(2, 1)
    smp = BespokeNonStationary(_cfg(tmp_path))
    with pytest.raises(ValueError, match="No sampler path provided, set it with 'SAMPLER_PATH' in the config"):
        smp(m, start, E, None, 4, 0, False)
    smp = BespokeNonStationary(_cfg(SAMPLER_PATH=str(tmp_path / "missing.pth")))
    with pytest.raises(ValueError, match="No sampler path provided"):
        smp(m, start, E, None, 4, 0, False)
    # the default file name: data_folder + '/bns_sampler.pth'; a theta for another step count is refused
    _save_theta(tmp_path / "bns_sampler.pth", torch.ones(2, 5))
    smp = BespokeNonStationary(_cfg(tmp_path))
    assert smp.sampler_path() == str(tmp_path) + "/bns_sampler.pth"
    assert smp.save_path() == str(tmp_path) + "/bns_sampler.pt"
    with pytest.raises(ValueError, match="Number of steps must match"):
        smp(m, start, E, None, 4, 0, False)


def test_train_sampler_without_a_loader_names_optimize_sampler(tmp_path):
    smp = BespokeNonStationary(_cfg(tmp_path, TRAIN_SAMPLER=True))
    with pytest.raises(RuntimeError, match="optimize_sampler"):
        smp(_FakeModel(), torch.zeros(1, 1, 2, 2, 2), torch.ones(1, 1), None, 3, 0, False)


def test_log_time_embedding_is_refused(tmp_path):
    _save_theta(tmp_path / "t.pth", torch.ones(2, 3))
    smp = BespokeNonStationary(_cfg(SAMPLER_PATH=str(tmp_path / "t.pth")))
    with pytest.raises(ValueError, match=r"NaN.*sigma <= 0"):
        smp(_FakeModel(time_embed="log"), torch.zeros(1, 1, 2, 2, 2), torch.ones(1, 1), None, 3, 0, False)
    with pytest.raises(ValueError, match="NaN"):
        smp.optimize_sampler(_FakeModel(time_embed="log"), [], 3)


@pytest.mark.parametrize("offset", [0, 2])
def test_program_columns_and_sample_offset(tmp_path, offset):
    N, B = 5, 3
    theta = torch.arange(2 * N, dtype=torch.float32).reshape(2, N) / 7 + 0.25
    _save_theta(tmp_path / "t.pth", theta)
    smp = BespokeNonStationary(_cfg(SAMPLER_PATH=str(tmp_path / "t.pth")))
    sigma = torch.randn(N - offset, B)
    smp.step_sigma = sigma
    m = _FakeModel(noise_offset=1000)
    start = torch.zeros(B, 1, 2, 2, 3)
    x, xs, x0s = smp(m, start, torch.ones(B, 1), None, N, offset, True)
    assert len(xs) == len(x0s) == N - offset
    prog, kw = m.eng.calls[-1]
    assert prog.op_begin is None, "uniform: one captured step graph"
    assert prog.n_bufs == 2 and prog.start_scale == 1.0 and prog.n_randn == 0
    kinds = [o[0] for o in prog.ops]
    assert kinds == [SOP_DENOISE_PS, SOP_RECORD, SOP_LINCOMB, SOP_RECORD]
    dn, rec_u, lin, rec_x = prog.ops
    assert dn[1:] == (1, (0,), 2) and lin[1:] == (0, (0, 1), 0) and rec_u[1] == 1 and rec_x[1] == 0
    assert prog.coefs.shape == (N - offset, 2 + B)
    np.testing.assert_array_equal(prog.coefs[:, 0], theta[0, offset:].numpy())
    np.testing.assert_array_equal(prog.coefs[:, 1], theta[1, offset:].numpy())
    np.testing.assert_array_equal(prog.coefs[:, 2:], sigma.numpy())
    assert kw["use_graph"] is True and kw["debug"] is True
    # the draws took N - offset rows of B sigmas: rounded up to one whole (B,1,2,2,3) tensor
    assert smp.ran_program and smp.noise_tensors_drawn == 1
    with pytest.raises(ValueError, match="step_sigma"):
        smp.step_sigma = torch.zeros(N, B + 1)
        smp(m, start, torch.ones(B, 1), None, N, offset, False)


def test_sigma_stream_positions_whole_and_sharded(tmp_path, monkeypatch):
    """sigma of step k, global row r = element offset + k * B_global + r of the stream behind the start tensor: two half-batch
    shards are the rows of one full batch.  (The fake randn returns the stream position of every element.)"""
    def fake_randn(shape, device, seed, offset=0):
        assert seed == 7
        n = int(np.prod(shape))
        return torch.arange(offset, offset + n, dtype=torch.float64).reshape(shape)

    monkeypatch.setattr(engine, "randn", fake_randn)
    N, G, per = 4, 6, 12
    _save_theta(tmp_path / "t.pth", torch.ones(2, N))
    base = 5000  # the model's running offset after the start tensor was drawn
    want = base + np.arange(N)[:, None] * G + np.arange(G)[None, :]

    def run(lo, B):
        smp = BespokeNonStationary(_cfg(SAMPLER_PATH=str(tmp_path / "t.pth")))
        m = _FakeModel(noise_offset=base, shard=(lo, G) if B != G else None)
        smp(m, torch.zeros(B, 1, 2, 2, 3), torch.ones(B, 1), None, N, 0, False)
        prog, kw = m.eng.calls[-1]
        return prog.coefs[:, 2:].astype(np.float64), kw

    full, kw = run(0, G)
    np.testing.assert_array_equal(full, want)
    assert kw["offset"] == base and kw["noise_stride"] == G * per
    h0, _ = run(0, G // 2)
    h1, kw1 = run(G // 2, G // 2)
    np.testing.assert_array_equal(np.concatenate([h0, h1], axis=1), full)
    assert kw1["offset"] == base + (G // 2) * per


# ---- the loss of cd_bns_theta_grad ----------------------------------------------------------------------------------
LN10 = math.log(10.0)


def _reference_loss(x, x_prime):
    """models/sample.py:1052-1059 as written."""
    mse = torch.mean((x - x_prime) ** 2)
    if mse == 0:
        return 100
    max_val = torch.max(x, axis=-1).values
    psnr = 20 * torch.log10(max_val / torch.sqrt(mse))
    return psnr


def _restated(data, x_n):
    """What bns_loss_partial / bns_loss_final / bns_seed compute: fp64 mse and loss, the seed g_N = c (x_N - data) with
    c = -20 / (ln 10 mse numel); NaN everywhere if a row maximum is 0; loss 100 and a zero seed if mse == 0."""
    d = data.astype(np.float64)
    xn = x_n.astype(np.float64)
    mse = np.mean((d - xn) ** 2)
    if mse == 0:
        return 100.0, np.zeros_like(d)
    m = d.max(axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = np.mean(20.0 * np.log10(m / np.sqrt(mse)))
    c = np.nan if (m == 0).any() else -20.0 / (LN10 * mse * d.size)
    return loss, c * (xn - d)


def _case(kind):
    gen = torch.Generator().manual_seed(3)
    data = torch.rand((2, 1, 3, 4, 5), generator=gen) + 0.1
    x_n = data + 0.3 * torch.randn(data.shape, generator=gen)
    if kind == "negative":
        data[1, 0, 2, 1, :] = -torch.rand(5, generator=gen) - 0.5
    elif kind == "zero":
        data[0, 0, 1, 3, :] = -torch.rand(5, generator=gen)
        data[0, 0, 1, 3, 2] = 0.0
    return data, x_n


@pytest.mark.parametrize("kind", ["positive", "negative", "zero"])
def test_psnr_loss_and_seed_gradient_match_autograd(kind):
    data, x_n = _case(kind)
    xp = x_n.clone().double().requires_grad_(True)
    ref = torch.mean(_reference_loss(data.double(), xp))
    ref.backward()
    want_loss, want_g = float(ref.detach()), xp.grad.numpy()
    loss, g = _restated(data.numpy(), x_n.numpy())
    if kind == "positive":
        assert np.isfinite(loss) and np.isfinite(g).all()
        assert abs(loss - want_loss) <= 1e-12 * abs(want_loss)
        np.testing.assert_allclose(g, want_g, rtol=1e-10, atol=0)
    elif kind == "negative":  # log10 of a negative maximum: NaN loss, the gradient does not see the maxima
        assert math.isnan(loss) and math.isnan(want_loss)
        assert np.isfinite(g).all() and np.isfinite(want_g).all()
        np.testing.assert_allclose(g, want_g, rtol=1e-10, atol=0)
    else:  # a zero maximum: -inf loss, and log10's backward makes torch's whole gradient NaN
        assert loss == -math.inf and want_loss == -math.inf
        assert np.isnan(want_g).all() and np.isnan(g).all()


def test_psnr_loss_at_zero_mse():
    data, _ = _case("positive")
    loss, g = _restated(data.numpy(), data.numpy())
    assert loss == 100.0 and not g.any()
    assert _reference_loss(data, data.clone()) == 100  # (an int: the reference's torch.mean raises on it)
