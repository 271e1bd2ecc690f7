"""GPU (MI355X): the deepest level's launch with a side job (kernels_deep_side.hip).  On the Dataset-2 grid (45 x 16 x 9, widths
32 / 64) the skip half of level 0's concat conv runs on the CUs the deepest level leaves idle, as the first of the conv's two
K-blocks; the x half follows as one continuation launch.  CD_NO_DEEP_SIDE_CONV=1 forces the earlier sequence (the whole conv after
the level), which every test here uses as the in-process reference for the reassociation (skip + bias) + x against (x + bias) + skip."""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from helpers import TOL_ORACLE, TOL_REASSOC, seeded_model_cfg
from oracle import torch_oracle as O

pytestmark = pytest.mark.gpu

SWITCH = "CD_NO_DEEP_SIDE_CONV"
BMAX = 66
_SIGMAS = [0.3, 2.5, 0.05, 11.0, 80.0, 1.0, 0.02, 5.0]


@pytest.fixture(scope="module")
def ds2():
    """One Dataset-2 model, one seeded batch of BMAX samples (smaller batches are prefixes) and the CPU oracle's denoise of the first
    three samples (the oracle treats samples independently)."""
    m, cfg = seeded_model_cfg("dataset2")
    gen = torch.Generator().manual_seed(29)
    x = torch.randn([BMAX] + list(cfg["SHAPE_PAD"][1:]), generator=gen)
    E = torch.rand((BMAX, 1), generator=gen)
    layers = torch.randn((BMAX, 1 + cfg["SHAPE_FINAL"][2]), generator=gen)
    sigma = torch.tensor([_SIGMAS[i % len(_SIGMAS)] for i in range(BMAX)], dtype=torch.float32)
    om = O.OracleModel(cfg, {k: v.detach().cpu() for k, v in m.state_dict().items()})
    with torch.no_grad():
        want3 = om.denoise(x[:3], E[:3], sigma[:3], layers[:3]).numpy()
    return m, cfg, (x.cuda(), E.cuda(), layers.cuda(), sigma.cuda()), want3


def _launches(fn):
    from calodiffusion_amd import engine
    engine.profile_begin()
    fn()
    return {k: v["launches"] for k, v in engine.profile_end().items()}


def _is_side(cat):
    return cat.startswith("deep_level") and "K-block" in cat


@pytest.mark.parametrize("B", [1, 3, 66])
def test_batch_edges_new_sequence_against_old_and_oracle(ds2, monkeypatch, B):
    """B = 66 makes the grid larger than one round of the chip's 256 CUs; the level's workgroups must still come out right."""
    m, cfg, (x, E, layers, sigma), want3 = ds2
    eng = m.engine()
    monkeypatch.setattr(eng, "safe_denoise", False)
    run = lambda: m.denoise(x[:B], E=E[:B], sigma=sigma[:B], layers=layers[:B])
    new = run()
    cats = _launches(run)
    assert sum(n for c, n in cats.items() if _is_side(c)) == 1, sorted(cats)
    monkeypatch.setenv(SWITCH, "1")
    old = run()
    cats_old = _launches(run)
    monkeypatch.delenv(SWITCH)
    eng.check_status()
    assert not any(_is_side(c) for c in cats_old) and any(c.startswith("deep_level") for c in cats_old), sorted(cats_old)
    err = float((new - old).norm() / old.norm())
    worst = max(float((new[i] - old[i]).norm() / old[i].norm()) for i in range(B))
    print(f"B={B}: new vs old sequence rel L2 {err:.3e} (worst sample {worst:.3e})")
    assert torch.isfinite(new).all() and err < TOL_REASSOC and worst < TOL_REASSOC
    assert torch.equal(run(), new)  # deterministic
    if B <= 3:
        e_o = rel_l2(new.cpu().numpy(), want3[:B])
        print(f"B={B}: new sequence vs oracle rel L2 {e_o:.3e}")
        assert e_o < TOL_ORACLE


def test_chunking_of_the_skip_half_changes_no_output_bit():
    """The skip half alone through the z-slide launcher, dealt in 3 chunks per sample (the side job's count at batch 64) and in the
    launcher's own 4: chunking along voxels changes no output's summation order, only the grouping of the statistics partials."""
    from calodiffusion_amd.engine import Ops
    ops = Ops()
    gen = torch.Generator().manual_seed(41)
    B, D, H, W = 5, 45, 16, 9
    x = ops.to_channels_last(torch.randn((B, 32, D, H, W), generator=gen).cuda())
    w = (torch.randn((32, 32, 3, 3, 3), generator=gen) * 0.05).cuda()
    bias = torch.randn((32,), generator=gen).cuda()
    y4, s4 = ops.zslide_conv_chunked(x, w, bias, 0)
    y3, s3 = ops.zslide_conv_chunked(x, w, bias, 3)
    for b in range(B):
        assert torch.equal(y3[b], y4[b]), b
    # Relative to what was summed: the sum of squares to itself, the plain sum to sum |y| -- a channel whose values cancel has a sum
    # far below its terms, and fp32 partial sums carry errors in proportion to the terms (the fp64 sums are printed as the scale).
    ref = y4.double().reshape(B, -1, 32)
    scale = torch.stack([ref.abs().sum(1), (ref * ref).sum(1)], -1)  # [B][C][2]
    want = torch.stack([ref.sum(1), (ref * ref).sum(1)], -1)
    for name, st in (("3 chunks", s3), ("default", s4)):
        print(f"channel statistics, {name}: max error against fp64 sums {float(((st - want).abs() / scale).max()):.2e} of the summed terms")
    err = float(((s3 - s4).abs() / scale).max())
    print(f"channel statistics, 3 chunks vs default: max difference {err:.2e} of the summed terms")
    assert err <= 1e-6


def test_range_flag_of_the_side_job_and_the_safe_fallback(ds2):
    """A skip tensor beyond the fp16 range raises the sticky status from inside the fused launch, and the safe denoise returns the
    full-range result.  (The public entry points cannot plant a single element in an internal tensor: one channel of skips[0] is
    driven to 1e5 through the bias of the closing GroupNorm of level 0's attention block.  The skip's other consumer, the strided
    conv into level 1, flags the same tensor, so this test shows that the flag survives the new sequence, not which launch set it.)"""
    from calodiffusion_amd import engine
    m, cfg, (x, E, layers, sigma), _ = ds2
    B = 2
    eng = m.engine()
    safe0 = eng.safe_denoise
    gn = m.model.downs_attn[0].fn.fn.to_out[1]
    keep = gn.bias.detach().clone()
    run = lambda: m.denoise(x[:B], E=E[:B], sigma=sigma[:B], layers=layers[:B])
    try:
        with torch.no_grad():
            gn.bias[5] = 1.0e5
        eng.safe_denoise = False
        cats = _launches(run)
        assert any(_is_side(c) for c in cats)
        with pytest.raises(FloatingPointError):
            eng.check_status()
        eng.safe_denoise = True
        before = getattr(eng, "range_fallbacks", 0)
        got = run()
        assert torch.isfinite(got).all() and eng.range_fallbacks == before + 1
        engine.set_conv_precision("bf16x3")
        try:
            want = run()
        finally:
            engine.set_conv_precision("f16x2")
        assert torch.equal(got, want)  # (the bound of test_fp16_range_flag_and_fallback_of_plain_denoise)
    finally:
        with torch.no_grad():
            gn.bias.copy_(keep)
        eng.safe_denoise = False
        run()
        eng.check_status()
        eng.safe_denoise = safe0


def test_graph_replay_equals_eager_bitwise_with_the_side_job(ds2):
    from calodiffusion_amd import sample
    m, cfg, (x, E, layers, sigma), _ = ds2
    B = 2
    outs = {}
    for use_graph in (True, False):
        c = dict(cfg)
        c["SAMPLER_OPTIONS"] = dict(cfg.get("SAMPLER_OPTIONS", {}), HIP_GRAPH=use_graph)
        m.sampler_algorithm = sample.DDim(c)
        outs[use_graph] = m.sample(E[:B], layers[:B], num_steps=4, start=x[:B])
    cats = _launches(lambda: m.sample(E[:B], layers[:B], num_steps=4, start=x[:B]))  # (eager: the new sequence is what ran)
    assert sum(n for k, n in cats.items() if _is_side(k)) == 4, sorted(cats)
    assert np.isfinite(outs[True]).all() and np.array_equal(outs[True], outs[False])


def test_training_and_vjp_do_not_take_the_new_sequence(ds2, monkeypatch):
    """The training tape and the VJP run the concat conv whole: bitwise the same loss and gradients with the switch on and off."""
    m, cfg, (x, E, layers, sigma), _ = ds2
    B = 2
    eng = m.engine()
    gen = torch.Generator().manual_seed(3)
    noise = torch.randn(x[:B].shape, generator=gen).cuda()
    gy = torch.randn(x[:B].shape, generator=gen).cuda()
    cond = m.cond_tensor(E[:B], layers[:B])
    res = {}
    for off in (False, True):
        if off:
            monkeypatch.setenv(SWITCH, "1")
        cats = _launches(lambda: res.__setitem__(off, (eng.train_step(x[:B], noise, sigma[:B], cond, "l2"),
                                                       eng.denoise_vjp(x[:B], sigma[:B], cond, gy, param_grads=True))))
        assert not any(_is_side(c) for c in cats), sorted(cats)
    monkeypatch.delenv(SWITCH)
    (l0, f0), (dx0, g0) = res[False]
    (l1, f1), (dx1, g1) = res[True]
    assert float(l0) == float(l1) and torch.equal(dx0, dx1)
    # (the parameters' slices only: the flat buffers' alignment gaps are written by neither call)
    for a, b in ((f0, f1), (g0, g1)):
        assert all(torch.equal(p, q) for p, q in zip(eng.param_grads(a), eng.param_grads(b)))
