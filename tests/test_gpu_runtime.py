"""GPU (MI355X): the C ABI's runtime state -- a HIP error left behind by someone else does not fail the next entry point, and the
engine's workspace cache follows precision changes, launch-sequence switches and batch sizes."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_l2
from helpers import seeded_layer_models, seeded_model

pytestmark = pytest.mark.gpu


def test_a_stale_hip_error_does_not_fail_the_next_entry_point():
    """The launchers check hipGetLastError() after every launch, which reports the thread's last error whoever caused it (round 3:
    a refused hipEventElapsedTime made the next cd_randn fail with 'invalid resource handle').  Every C-ABI entry point now
    clears the error state on the way in: provoke a HIP error outside the library, then call into it."""
    from calodiffusion_amd import engine
    lib = engine.load_library()
    torch.cuda.init()
    # the HIP runtime this process already runs on (torch ships its own copy: a second one would keep its own error state)
    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
    hip = ctypes.CDLL(path)
    hip.hipFree.argtypes, hip.hipFree.restype = [ctypes.c_void_p], ctypes.c_int
    hip.hipPeekAtLastError.restype = ctypes.c_int
    torch.cuda.synchronize()
    assert hip.hipFree(ctypes.c_void_p(0x1234)) != 0      # not an allocation: fails and leaves the error behind
    assert hip.hipPeekAtLastError() != 0
    out = torch.empty(4096, dtype=torch.float32, device="cuda")
    rc = lib.cd_randn(out.data_ptr(), out.numel(), 7, 0, engine._stream())
    assert rc == 0, lib.cd_last_error().decode(errors="replace")
    torch.cuda.synchronize()
    assert abs(float(out.mean())) < 0.1 and 0.9 < float(out.std()) < 1.1
    # ... and a failing entry point leaves nothing behind for the next one either
    assert lib.cd_randn(None, 16, 7, 0, engine._stream()) != 0
    assert lib.cd_randn(out.data_ptr(), out.numel(), 7, 0, engine._stream()) == 0


def test_workspace_cache_follows_precision_and_switches(monkeypatch):
    """A cached workspace stays valid when the arithmetic mode changes after the first call (the library sizes for the largest of
    its modes), a launch-sequence switch gets its own workspace, and at most one network / one sampler workspace is kept (ADVICE
    r03: a ragged last batch doubled the footprint, a precision switch after the first call failed with CD_EWORKSPACE)."""
    from calodiffusion_amd import engine
    m = seeded_model("dataset2", {"SAMPLER": "Heun"})
    eng = m.engine()
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, 1, 45, 16, 9), generator=g).cuda()
    E, layers = torch.rand((2, 1), generator=g).cuda(), torch.randn((2, 46), generator=g).cuda()
    sig = torch.tensor([2.0, 0.3]).cuda()
    ref = m.denoise(x, E=E, sigma=sig, layers=layers)
    try:
        for mode in ("f32", "bf16x3"):
            engine.set_conv_precision(mode)
            y = m.denoise(x, E=E, sigma=sig, layers=layers)
            assert rel_l2(y.cpu().numpy(), ref.cpu().numpy()) < 1e-5, mode
    finally:
        engine.set_conv_precision("f16x2")
    monkeypatch.setenv("CD_NO_DEEP_LEVEL", "1")
    y = m.denoise(x, E=E, sigma=sig, layers=layers)
    assert rel_l2(y.cpu().numpy(), ref.cpu().numpy()) < 3e-6
    monkeypatch.delenv("CD_NO_DEEP_LEVEL")
    m.denoise(x[:1], E=E[:1], sigma=sig[:1], layers=layers[:1])  # another batch size: the previous workspace is evicted
    m.sample(E, layers, num_steps=3, start=x)
    m.sample(E[:1], layers[:1], num_steps=3, start=x[:1])
    kinds = [k[0] for k in eng._ws]
    assert kinds.count("net") == 1 and kinds.count("sampler") == 1, list(eng._ws)


def _tiny_step(m, B, seed):
    """(data, noise, sigma, cond) of one training step of the tiny model at batch B, on the device."""
    gen = torch.Generator().manual_seed(seed)
    data = torch.randn((B, 1, 8, 8, 8), generator=gen)
    noise = torch.randn(data.shape, generator=gen)
    E, layers = torch.rand((B, 3), generator=gen), torch.randn((B, 9), generator=gen)
    sigma = 0.05 + 30.0 * torch.rand((B,), generator=gen)
    return data.cuda(), noise.cuda(), sigma.cuda(), m.cond_tensor(E.cuda(), layers.cuda())


def _train(eng, args):
    loss, flat = eng.train_step(*args)
    return float(loss), torch.cat([g.flatten() for g in eng.param_grads(flat)]).cpu()


def test_training_workspaces_share_the_cache_and_leave_results_alone(monkeypatch):
    """The training, VJP and theta-gradient workspaces live in the engine's one cache beside the network's: a training step repeated
    after steps at another batch size, both VJP modes and a theta gradient is bitwise the first one, one workspace of each kind is
    kept, a launch-sequence switch gives the training workspace another key, and set_embedding empties the cache.  (The autotune
    is warmed on a throwaway engine first, as in test_the_first_training_step_equals_the_steady_state.)"""
    warm = seeded_model("tiny")
    for B in (2, 1):
        warm.engine().train_step(*_tiny_step(warm, B, 31))
    m = seeded_model("tiny")
    eng = m.engine()
    two, one = _tiny_step(m, 2, 31), _tiny_step(m, 1, 31)
    data, noise, sigma, cond = two
    first = _train(eng, two)
    _train(eng, one)
    for param_grads in (True, False):
        eng.denoise_vjp(data, sigma, cond, noise, param_grads=param_grads)
    theta = torch.tensor([[0.9, 0.8, 0.7], [0.3, 0.4, 0.5]]).cuda()
    eng.bns_theta_grad(data.abs() + 0.05, cond, theta, sigma.expand(3, 2).contiguous())
    again = _train(eng, two)
    assert again[0] == first[0], (again[0], first[0])
    assert torch.equal(again[1], first[1])
    kinds = [k[0] for k in eng._ws]
    assert [kinds.count(k) for k in ("train", "vjp", "bns")] == [1, 1, 1], list(eng._ws)

    def train_key():
        return next(k for k in eng._ws if k[0] == "train")

    before = train_key()
    monkeypatch.setenv("CD_NO_DEEP_LEVEL", "1")
    switched = _train(eng, two)
    assert train_key() != before and [k[0] for k in eng._ws].count("train") == 1, list(eng._ws)
    assert np.isfinite(again[0]) and np.isfinite(switched[0]) and torch.isfinite(again[1]).all() and torch.isfinite(switched[1]).all()
    monkeypatch.delenv("CD_NO_DEEP_LEVEL")
    eng.set_embedding(None)
    assert list(eng._ws) == []


def test_layer_engine_keeps_one_workspace_of_each_kind():
    layer, _ = seeded_layer_models()
    eng = layer.cuda().engine()
    gen = torch.Generator().manual_seed(41)
    for B in (3, 2):
        x, noise = torch.randn((B, eng.dim), generator=gen).cuda(), torch.randn((B, eng.dim), generator=gen).cuda()
        E, sigma = torch.rand((B, 1), generator=gen).cuda(), (0.05 + 5.0 * torch.rand((B,), generator=gen)).cuda()
        loss, flat = eng.train_step(x, noise, sigma, E)
        dx, grads = eng.denoise_vjp(x, sigma, E, noise, param_grads=True)
        assert np.isfinite(float(loss)) and torch.isfinite(flat).all() and torch.isfinite(dx).all() and torch.isfinite(grads).all()
        assert sorted(eng._ws) == [("train", B), ("vjp", B, True)]
