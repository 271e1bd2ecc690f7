"""GPU (MI355X): every forward form of Residual(PreNorm(LinearAttention)) (attn_block, csrc/forward.hip) at 64 .. 128 channels and
at the edges of its work splits, through engine.Ops().linear_attention against oracle.torch_oracle.attn_residual in float64.

    form           kernels                                               taken when
    single launch  attn_small_kernel<1..4>                               f16x2, vox <= 1024
    two pass       attn_kv_context_kernel<1..4> + attn_out_kernel<1..4>  f16x2, vox > 1024
    moment form    the <1, true> instances of both                       as above, C == 32, B vox C >= CD_ATTN_MOM_MIN
    unfused        attn_context_kernel + attn_combine_kernel + the       bf16x3 / f32 (and the range-fallback re-run, and
                   pointwise kernel's 32-way softmax prologue            attn_block_train)

The other attention tests stop at four 32-voxel tiles for more than 32 channels (test_linear_attention_blocks: 120, 60, 30 voxels)
and at 32 channels for more than 1024 voxels (the moment-form test, every shipped config).  The shapes here are the smallest at which
each path can still go wrong: a wave that loops over a second tile, a ragged last tile, a last workgroup of one voxel, one workgroup
looping over every tile of its sample (batch 256), 128 workgroups per sample (the cap of both split rules, and the size of
attn_combine_kernel's factor table).  The profiler's launch categories say which form ran: a case that silently takes another form
tests nothing.

Bars, per case (all errors relative L2 against float64):
    block output   < 1e-5 (TOL_OP)
    branch alone   < max(2e-6, 4 e32), the branch being y - x (the residual x is common to both sides and larger than the branch).
                   e32 is the error of the same oracle evaluated in float32, measured in the test from the reference alone; 2e-6
                   is the bar the moment-form test holds at 32 channels.  The floor binds for default-scale and peaked-q weights
                   (e32 1e-7 .. 5e-7); a to_out bias of 3 puts e32 at 2e-6 .. 5e-6 (the closing GroupNorm's variance is then a
                   small difference of large sums in float32 too), k weights x 12 with a ramp at 3e-7 .. 9e-7.

Weight settings (helpers.attn_block_weights: to_qkv / sqrt(C), to_out / sqrt(32), norm parameters 1 + 0.1 randn):
    a  default
    b  q rows x 12: a peaked softmax over the channels
    c  k rows x 12, the input carrying a ramp of +-20 along z in its first four channels and the k weights of those four
       channels made positive and x 4: k then rises by 200 .. 500 along z, so for some channels the maximum over a sample's first
       workgroup lies more than 104 below the sample's (asserted on the reference) and the factor exp(m_split - M) of the
       log-sum-exp merge is 0 in float32.  Normalised x stays below 10 and v below 7: this is no range-flag case.
    d  to_out bias + 3

Split counts (workgroups x tiles each) are those of attn_fused_nsplit_for / attn_nsplit_for, restated below and asserted."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from helpers import TOL_OP, attn_block_weights, profiled_launches, seeded_model_cfg, seeded_unet, unet_kwargs

pytestmark = pytest.mark.gpu

BRANCH_FLOOR = 2e-6
SETTINGS = {"a": {}, "b": {"qscale": 12.0}, "c": {"kscale": 12.0}, "d": {"bias": 3.0}}

# (grid, C, B): vox <= 1024, one launch
SMALL = [
    ((11, 6, 4), 128, 2),    # 264 voxels, 9 tiles (last: 8 voxels): one wave gets a second tile
    ((11, 7, 9), 96, 2),     # 693 voxels, 22 tiles (last: 21 voxels): uneven tiles per wave, ragged
    ((11, 31, 3), 64, 1),    # 1023 voxels, 32 tiles (last: 31 voxels): four tiles per wave, ragged
    ((32, 8, 4), 128, 1),    # 1024 voxels, 32 full tiles: the eligibility bound itself
]
# (grid, C, B, workgroups per sample, tiles per workgroup): vox > 1024, two passes
TWO_PASS = [
    ((41, 5, 5), 64, 1, 3, 16),       # 1025 voxels, 33 tiles: the last workgroup holds one tile of one voxel
    ((13, 9, 9), 96, 2, 3, 16),       # 1053 voxels, 33 tiles
    ((9, 13, 37), 128, 1, 9, 16),     # 4329 voxels, 136 tiles (last: 9 voxels): the last workgroup half full
    ((45, 16, 9), 64, 1, 13, 16),     # Dataset-2's grid (6480 voxels, 203 tiles) at a width no config uses
    ((11, 19, 5), 32, 256, 1, 40),    # 1045 voxels: one workgroup loops over every tile; grid.y = 256
    ((64, 32, 32), 32, 1, 128, 16),   # 65536 voxels: nsplit at its cap (the unfused rule's cap is 128 too)
]
UNFUSED = [((41, 5, 5), 64, 1, "acd"), ((9, 13, 37), 128, 1, "acd"), ((11, 7, 9), 96, 2, "ab"), ((64, 32, 32), 32, 1, "acd")]


def _fused_split(vox, B):
    """(workgroups per sample, tiles per workgroup) of both fused passes: attn_fused_nsplit_for / tiles_per_wg_for
    (kernels_attn.hip) with the default of 256 workgroups per launch."""
    T = -(-vox // 32)
    n = max(1, min(-(-256 // B), -(-T // 16), 128))
    per = -(-(-(-T // n)) // 8) * 8
    return -(-T // per), per


def _unfused_split(vox, B):
    """Voxel ranges per sample of attn_context_kernel: attn_nsplit_for (kernels_attn_unfused.hip)."""
    return max(1, min(-(-1024 // B), -(-vox // 512), 128))


@functools.lru_cache(maxsize=None)
def _case(grid, C, B, setting):
    """Inputs and reference of one case, computed once on the CPU and shared by every test that runs it (never modified): x
    (B, D, H, W, C) float32, the block's weights, the attention branch in float64 (channels-last), e32, and for setting c the
    largest gap over (sample, channel) between the k maximum of the whole sample and that of its first 16 tiles."""
    from oracle import torch_oracle as O
    D, H, W = grid
    gen = torch.Generator().manual_seed(1000 * C + 10 * B + D + ord(setting))
    x = torch.randn((B, D, H, W, C), generator=gen) * 1.5 + 0.3
    sd = attn_block_weights(C, gen, **SETTINGS[setting])
    if setting == "c":
        x[..., :4] += torch.linspace(-20.0, 20.0, D).view(1, D, 1, 1, 1)
        wk = sd["fn.fn.to_qkv.conv.weight"][32:64]
        wk[:, :4] = wk[:, :4].abs() * 4.0
    with torch.no_grad():
        sd64 = {"a." + k: v.double() for k, v in sd.items()}
        x64 = x.double().permute(0, 4, 1, 2, 3)
        branch = O.attn_residual(sd64, "a", x64, True) - x64
        y32 = O.attn_residual({"a." + k: v for k, v in sd.items()}, "a", x.permute(0, 4, 1, 2, 3), True)
        e32 = float((y32.double() - x64 - branch).norm() / branch.norm())
        gap = 0.0
        if setting == "c":
            xn = F.group_norm(x64, 1, sd64["a.fn.norm.weight"], sd64["a.fn.norm.bias"], eps=1e-5)
            qkv = torch.einsum("oc,bcn->bon", sd64["a.fn.fn.to_qkv.conv.weight"].view(96, C), xn.reshape(B, C, -1))
            assert float(xn.abs().max()) < 100 and float(qkv[:, 64:].abs().max()) < 100  # far inside the fp16 range
            k = qkv[:, 32:64]
            gap = float((k.amax(-1) - k[:, :, :512].amax(-1)).max())
    return {"x": x, "sd": sd, "branch": branch.permute(0, 2, 3, 4, 1).contiguous().numpy(), "e32": e32, "gap": gap}


def _run(ops, case):
    """The block on the device under the per-launch profiler -> (y, the launch categories that ran)."""
    from calodiffusion_amd import engine
    x = case["x"].cuda()
    sd = {k: v.cuda().contiguous() for k, v in case["sd"].items()}
    engine.profile_begin()
    try:
        y = ops.linear_attention(x, sd)
        torch.cuda.synchronize()
    finally:
        ran = set(engine.profile_end())
    return y, ran


def _assert_form(ran, form, C, vox):
    attn = sorted(k for k in ran if k.startswith("attn_"))
    want, never = {
        "small": ([f"attn_small C{C} n{vox}"], ("attn_kv_context", "attn_out", "attn_context")),
        "two_pass": ([f"attn_kv_context C{C} n{vox}", f"attn_out C{C} n{vox}"], ("attn_small", "attn_context")),
        "unfused": (["attn_context", "attn_combine"], ("attn_small", "attn_kv_context", "attn_out")),
    }[form]
    assert all(k in attn for k in want), (form, attn)
    assert not [k for k in attn if k.split(" ")[0] in never], (form, attn)


def _check(tag, y, case):
    """Both bars; prints the block error, the branch error and e32."""
    x64 = case["x"].double().numpy()
    got = y.double().cpu().numpy()
    e_block = rel_l2(got, case["branch"] + x64)
    e_branch = rel_l2(got - x64, case["branch"])
    bar = max(BRANCH_FLOOR, 4.0 * case["e32"])
    print(f"[attention {tag}] block {e_block:.2e}, branch {e_branch:.2e} (bar {bar:.2e}), e32 {case['e32']:.2e}")
    assert np.isfinite(got).all(), tag
    assert e_block < TOL_OP, (tag, e_block)
    assert e_branch < bar, (tag, e_branch, bar, case["e32"])
    return e_branch


def _f16x2_only():
    if os.environ.get("CD_CONV_PRECISION", "f16x2") != "f16x2":
        pytest.skip("the fused attention passes run in the default f16x2 mode only")


@pytest.fixture(scope="module")
def ops():
    from calodiffusion_amd import engine
    return engine.Ops()


@pytest.mark.parametrize("setting", ["a", "b"])
@pytest.mark.parametrize("grid,C,B", SMALL)
def test_single_launch_form(ops, grid, C, B, setting):
    """attn_small_kernel<2..4> with more tiles than waves: 9, 22 and 32 tiles on 8 waves, ragged last tiles, and 1024 voxels, the
    largest grid that takes this form."""
    _f16x2_only()
    vox = grid[0] * grid[1] * grid[2]
    case = _case(grid, C, B, setting)
    y, ran = _run(ops, case)
    _assert_form(ran, "small", C, vox)
    _check(f"small C{C} {grid} B{B} {setting}", y, case)


@pytest.mark.parametrize("setting", ["a", "c", "d"])
@pytest.mark.parametrize("grid,C,B,wgs,per", TWO_PASS)
def test_two_pass_form(ops, grid, C, B, wgs, per, setting, monkeypatch):
    """attn_kv_context_kernel + attn_out_kernel at 64, 96 and 128 channels, and at 32 channels with one workgroup per sample
    (batch 256) and with 128 (65536 voxels); the 32-channel rows in the moment form and without it."""
    _f16x2_only()
    vox = grid[0] * grid[1] * grid[2]
    assert _fused_split(vox, B) == (wgs, per)
    case = _case(grid, C, B, setting)
    if setting == "c" and wgs > 1:
        assert case["gap"] > 104.0, case["gap"]  # exp(-104) < 2^-149: the first workgroup's factor is 0 for some channel
    tag = f"C{C} {grid} B{B} {setting}"
    if C != 32:
        y, ran = _run(ops, case)
        _assert_form(ran, "two_pass", C, vox)
        _check("two-pass " + tag, y, case)
        return
    monkeypatch.setenv("CD_ATTN_MOM_MIN", "0")  # (read per call; the plan takes the moment form from 4 M elements per tensor)
    y_mom, ran = _run(ops, case)
    _assert_form(ran, "two_pass", C, vox)
    assert not [k for k in ran if k.startswith("gn_apply")], sorted(ran)  # (pass 2 closes the block itself)
    monkeypatch.setenv("CD_NO_ATTN_MOMENTS", "1")
    y_sep, ran = _run(ops, case)
    _assert_form(ran, "two_pass", C, vox)
    assert [k for k in ran if k.startswith("gn_apply")], sorted(ran)  # (the closing GroupNorm as a pass of its own)
    assert not torch.equal(y_mom, y_sep)  # (the two forms really are different launches)
    _check("moment form " + tag, y_mom, case)
    _check("two-pass " + tag, y_sep, case)


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
@pytest.mark.parametrize("grid,C,B,settings", UNFUSED)
def test_unfused_form(ops, grid, C, B, settings, mode):
    """attn_context_kernel + attn_combine_kernel + the pointwise softmax prologue, the form of the full-range precisions, of a
    range fallback's re-run and of training: voxel ranges rounded up to an even length with a short, odd last one (1025 voxels:
    342 + 342 + 341; 693: 348 + 345) and 128 ranges per sample (65536 voxels), the size of attn_combine_kernel's factor table."""
    from calodiffusion_amd import engine
    if "CD_CONV_PRECISION" in os.environ:
        pytest.skip("CD_CONV_PRECISION is preset: this test switches the precision itself")
    vox = grid[0] * grid[1] * grid[2]
    assert _unfused_split(vox, B) == {1025: 3, 4329: 9, 693: 2, 65536: 128}[vox]
    before = engine.get_conv_precision()
    engine.set_conv_precision(mode)
    try:
        for setting in settings:
            case = _case(grid, C, B, setting)
            y, ran = _run(ops, case)
            _assert_form(ran, "unfused", C, vox)
            _check(f"unfused {mode} C{C} {grid} B{B} {setting}", y, case)
    finally:
        engine.set_conv_precision(before)


def test_two_pass_form_is_independent_of_the_batch(ops):
    """The same two showers at batch 2, as the first two rows of batch 40, and as the first two rows of batch 128: (13, 9, 9) at 96
    channels.  Batches 2 and 40 both run 3 workgroups of 16 tiles per sample (the 33 tiles cap the split at 3 until 256 / B drops
    below it), batch 128 runs 2 of 24: another tile-to-wave assignment and another merge order."""
    _f16x2_only()
    grid, C = (13, 9, 9), 96
    vox = grid[0] * grid[1] * grid[2]
    assert _fused_split(vox, 2) == (3, 16) and _fused_split(vox, 40) == (3, 16) and _fused_split(vox, 128) == (2, 24)
    two = _case(grid, C, 2, "a")
    y2, ran = _run(ops, two)
    _assert_form(ran, "two_pass", C, vox)
    _check(f"two-pass C{C} {grid} B2", y2, two)
    x2 = two["x"].double().numpy()
    for B in (40, 128):
        gen = torch.Generator().manual_seed(B)
        x = torch.cat([two["x"], torch.randn((B - 2,) + tuple(two["x"].shape[1:]), generator=gen) * 1.5 + 0.3])
        y, ran = _run(ops, {"x": x, "sd": two["sd"]})
        _assert_form(ran, "two_pass", C, vox)
        first = {"x": two["x"], "sd": two["sd"], "branch": two["branch"], "e32": two["e32"]}
        _check(f"two-pass C{C} {grid} rows 0-1 of B{B}", y[:2], first)
        err = rel_l2(y[:2].double().cpu().numpy() - x2, y2.double().cpu().numpy() - x2)
        print(f"[attention batch independence] rows 0-1 of B{B} against B2: branch rel L2 {err:.2e}")
        assert err < 1e-6, (B, err)


# ------------------------------------------------------------------------------------------------------------
# through the plan: the primitive passes neither the range-status word nor the plan's workspace sizing
# ------------------------------------------------------------------------------------------------------------
PLAN_GRID, PLAN_SIZES = (21, 20, 20), (32, 32, 64)  # level 1: 11 x 10 x 10 = 1100 voxels at 64 channels, too large for the
                                                    # one-launch deep level: it runs per-op


def test_two_pass_form_at_64_channels_through_unet_forward():
    """CondUnet.forward on a net whose 64-channel level has 1100 voxels, against the oracle: attn_kv_context / attn_out <2> as the
    plan calls them."""
    from oracle import torch_oracle as O
    _f16x2_only()
    B = 2
    net = seeded_unet(unet_kwargs(PLAN_GRID, PLAN_SIZES), 77).cuda()
    g = torch.Generator().manual_seed(5)
    x = torch.randn([B, 3] + list(PLAN_GRID), generator=g)
    cond, time = torch.randn((B, 9), generator=g), torch.rand((B,), generator=g)
    spec = O.UnetSpec(layer_sizes=list(PLAN_SIZES), channels=3, cond_size=9, data_shape=PLAN_GRID)
    with torch.no_grad():
        want = O.cond_unet_forward({k: v.cpu() for k, v in net.state_dict().items()}, spec, x, cond, time)
    launches = profiled_launches(lambda: net(x.cuda(), cond=cond.cuda(), time=time.cuda()))
    assert "attn_kv_context C64 n1100" in launches and "attn_out C64 n1100" in launches, sorted(launches)
    got = net(x.cuda(), cond=cond.cuda(), time=time.cuda())
    err = rel_l2(got.cpu().numpy(), want.numpy())
    print(f"[attention through the plan] grid {PLAN_GRID} sizes {PLAN_SIZES}: unet_forward rel L2 {err:.2e}")
    assert err < TOL_OP


def test_training_step_with_1100_voxels_at_64_channels():
    """One training step of the same layer sizes and grid (the tiny config otherwise): loss and every gradient tensor against
    autograd through the fp32 oracle at test_gpu_grad_batch's bars -- attn_block_train / attn_block_bwd, the per-sample attention
    weight gradient and the exp-norm pointwise prologue at 64 channels and more than 1024 voxels (elsewhere <= 120)."""
    from oracle import torch_oracle as O
    from grad_cases import train_steps_vs_oracle
    shape = [-1, 1] + list(PLAN_GRID)
    m, cfg = seeded_model_cfg("tiny", dict(LAYER_SIZE_UNET=list(PLAN_SIZES), SHAPE_PAD=shape, SHAPE_FINAL=shape))
    assert O.spec_from_config(cfg).layer_sizes == list(PLAN_SIZES)
    assert tuple(O.spec_from_config(cfg).data_shape) == PLAN_GRID == tuple(m.engine().grid)
    train_steps_vs_oracle(f"tiny {PLAN_GRID} {PLAN_SIZES} B=2 train", m, cfg, 2, seed=11)


@pytest.mark.parametrize("parts", [2, 4])
def test_cooperating_workgroups_attention_equals_the_single_workgroup_form(parts, tmp_path):
    """attn_coop_kernel (CD_ATTN_COOP: a sample's voxels dealt to several co-operating workgroups with two in-launch barriers)
    against the one-workgroup-per-sample attn_small_kernel at Dataset-2's level-1 grids (736 voxels, 32 and 64 channels, batch a
    multiple of 8 so that a sample's workgroups share an XCD) -- run in a child process, CD_ATTN_COOP is read once.  The two forms
    merge their {max, sum, context} partials differently, so they agree to rounding, not bit for bit; the range flag must stay
    clear (a barrier that times out raises it)."""
    import os
    import subprocess
    import sys
    code = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
from helpers import seeded_model
m = seeded_model("dataset2")
g = torch.Generator().manual_seed(5)
B = 16
x = torch.randn((B, 1, 45, 16, 9), generator=g).cuda()
E, layers = torch.rand((B, 1), generator=g).cuda(), torch.randn((B, 46), generator=g).cuda()
sig = torch.linspace(0.05, 30.0, B).cuda()
eng = m.engine()
eng.safe_denoise = False
y = m.denoise(x, E=E, sigma=sig, layers=layers)
torch.cuda.synchronize()
eng.check_status()
np.save(sys.argv[1], y.cpu().numpy())
"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = {}
    for tag, env in (("single", {}), ("coop", {"CD_ATTN_COOP": str(parts)})):
        path = str(tmp_path / f"coop_{parts}_{tag}.npy")
        e = dict(os.environ, **env)
        subprocess.run([sys.executable, "-c", code % (root, os.path.join(root, "tests")), path], check=True, env=e, timeout=600)
        outs[tag] = np.load(path)
    err = rel_l2(outs["coop"], outs["single"])
    print(f"co-operative attention ({parts} workgroups per sample) vs single workgroup: rel L2 {err:.2e}")
    assert err < 3e-6


@pytest.mark.parametrize("shape,batch", [((45, 16, 9), 4), ((28, 12, 21), 3), ((45, 50, 18), 2)])
def test_attention_moment_form_equals_the_separate_closing_pass(shape, batch, monkeypatch):
    """Level-0 attention (32 channels, > 1024 voxels): the moment form -- pass 1 also accumulates sum(softmax(q) - 1/32) and its
    32 x 32 second moment, pass 2 derives the closing GroupNorm(1)'s mean / variance from them and the folded weights and writes
    gn(y) + x directly -- beside the three-launch form (y written, channel sums, gn_apply), both against the oracle in float64, on grids with a ragged last tile,
    for near-uniform softmaxes (default-init scale), peaked ones (q weights x 12) and an output projection with a large bias
    (mean^2 >> variance: the cancellation case of E[y^2] - mean^2)."""
    import os
    from calodiffusion_amd import engine
    if os.environ.get("CD_CONV_PRECISION", "f16x2") != "f16x2":
        pytest.skip("the fused attention passes (and with them the moment form) run in the default f16x2 mode only")
    monkeypatch.setenv("CD_ATTN_MOM_MIN", "0")  # (the plan takes this form from 4 M elements per tensor)
    ops = engine.Ops()
    gen = torch.Generator().manual_seed(23)
    D, H, W = shape
    C = 32
    x = (torch.randn((batch, D, H, W, C), generator=gen) * 1.5 + 0.3).cuda()
    for qscale, bias in ((1.0, 0.0), (12.0, 0.0), (1.0, 3.0)):
        sd = {k: v.cuda().contiguous() for k, v in attn_block_weights(C, gen, qscale=qscale, bias=bias).items()}
        y_mom = ops.linear_attention(x, sd)
        monkeypatch.setenv("CD_NO_ATTN_MOMENTS", "1")
        y_sep = ops.linear_attention(x, sd)
        monkeypatch.delenv("CD_NO_ATTN_MOMENTS")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(y_mom).all())
        assert not torch.equal(y_mom, y_sep)  # (the two forms really are different launches)
        # both against the oracle in float64, on the attention branch alone (the residual x is common and larger than it)
        from oracle import torch_oracle
        sd64 = {"a." + k: v.double().cpu() for k, v in sd.items()}
        x64 = x.double().cpu().permute(0, 4, 1, 2, 3)
        want = (torch_oracle.attn_residual(sd64, "a", x64, True) - x64).permute(0, 2, 3, 4, 1).numpy()
        e_mom = rel_l2((y_mom.double().cpu() - x.double().cpu()).numpy(), want)
        e_sep = rel_l2((y_sep.double().cpu() - x.double().cpu()).numpy(), want)
        print(f"{shape} q x{qscale} bias {bias}: rel L2 of the branch against float64 -- moment form {e_mom:.2e}, closing pass {e_sep:.2e}")
        assert e_mom < 2e-6, (shape, qscale, bias, e_mom, e_sep)
