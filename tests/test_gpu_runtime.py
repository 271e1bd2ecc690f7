"""GPU (MI355X): the C ABI's runtime state -- a HIP error left behind by someone else does not fail the next entry point, and the
engine's workspace cache follows precision changes, launch-sequence switches and batch sizes."""
import ctypes

import pytest
import torch

from conftest import rel_l2
from helpers import seeded_model

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
