"""GPU (MI355X): where the convolution kernels write.  cd_op_cyl_conv into a buffer with guard bands either side of its output:
the bands keep their fill value bit for bit, every output element is written, and the result equals the ordinary launch exactly."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_full_resolution_conv_writes_nothing_outside_its_output():
    """Guard bands around the output of the z-slide convolution at the chunk lengths the sampling loop runs (the parity tests
    compare what lies INSIDE the output): long chunks of whole planes (Dataset-2 at batch 64: 4 chunks of 26 steps per sample), the
    continuation launch of a 64-channel input, phi strips with a 5-plane ring (Dataset-3, HGCal).  Written after round 3's
    unexplained core dump: every store of the shipped instances -- the row stores of the reduction and the
    partial-statistics stores -- stays inside its tensor."""
    import ctypes as C
    from calodiffusion_amd import engine
    ops = engine.Ops()
    gen = torch.Generator().manual_seed(17)
    pad = 1 << 16  # floats either side
    for B, cin, cout, shape in ((64, 32, 32, (45, 16, 9)), (64, 64, 32, (45, 16, 9)), (8, 32, 32, (45, 50, 18)), (16, 32, 32, (28, 12, 21)),
                                (3, 32, 64, (7, 16, 8))):
        D, H, W = shape
        x = torch.randn((B, D, H, W, cin), generator=gen).cuda()
        w = (torch.randn((cout, cin, 3, 3, 3), generator=gen) / (27 * cin) ** 0.5).cuda()
        bias = torch.randn((cout,), generator=gen).cuda()
        n = B * D * H * W * cout
        big = torch.full((pad + n + pad,), 7.25, dtype=torch.float32, device="cuda")
        sc = ops.scratch(B, max(cin, cout), D * H * W)
        engine._check(ops.lib.cd_op_cyl_conv(x.data_ptr(), cin, None, 0, w.data_ptr(), bias.data_ptr(), big.data_ptr() + 4 * pad, B,
                                             cout, engine._i32x3((D, H, W)), engine._i32x3((3, 3, 3)), engine._i32x3((1, 1, 1)),
                                             sc.data_ptr(), engine._stream()))
        torch.cuda.synchronize()
        assert bool((big[:pad] == 7.25).all()) and bool((big[pad + n:] == 7.25).all()), (B, cin, cout, shape)
        y = big[pad:pad + n].view(B, D, H, W, cout)
        assert bool(torch.isfinite(y).all()) and not bool((y == 7.25).any()), (B, cin, cout, shape)  # every element written
        ref = ops.cyl_conv(x, w, bias)
        assert torch.equal(ref, y)  # (deterministic: the same launch into an ordinary tensor)
