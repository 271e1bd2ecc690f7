"""GPU (MI355X): cd_train_step and cd_denoise_vjp against torch autograd through the fp32 CPU oracle at batches where the
backward path's work splits are limited by the batch, not by the voxel count, and on nets deep enough to overflow the two
deferred-reduction queues mid-step.

Every other gradient test runs at batch <= 6 (largest B*vox 40 500), where each split below takes its voxel-limited branch
("cap"); the shipped configs train at batch 128 / 64 / 256, where almost all of them take the batch-limited one ("want").

    where                                  split                                        batch-limited when
    gn_nsplit_for (kernels_gn.hip)         min(ceil(2048/B), ceil(vox/256))             B*vox > 524 288
    attn_nsplit_for                        min(ceil(1024/B), ceil(vox/512))             B*vox > 524 288
    gn_apply_blocks_per_sample             min(ceil(1024/B), ceil(vox/(8*rows))),       C = 32 (rows = 32): B*vox > 262 144
                                           rows = 256/(C/4)
    launch_gn_backward, folded form        bps_cap = ceil(256/B) on the line above      queued (training / VJP with grads) only
    wgrad_chunks, 27 taps                  min(ceil(512/B), ceil(vox/128)), 32 MiB cap  B*vox > 65 536
    wgrad_chunks, 1 tap                    min(ceil(4096/B), ceil(vox/64))              B*vox > 262 144
    head_bwd_blocks                        min(1024, ceil(B*vox/256))                   B*vox > 262 144 (more than 8 loop trips)
    launch_init_dgrad                      ceil(512/(B*nbands)) z-chunks vs (D+2)/3;    dataset2: B >= 35, dataset3: B >= 8
                                           bands of rows with a halo when H*W > 256
    GnParamJobs::kMax = 64,                a full queue is flushed mid-step             six resp. seven LAYER_SIZE_UNET entries
    WgradReduceQueue::kMax = 80

The arithmetic of each chosen batch (level 0 unless said otherwise):

  dataset2 (vox 45*16*9 = 6480), B = 97 (prime: every ceil is ragged), B*vox = 628 560
    gn_nsplit     ceil(2048/97) = 22  <  ceil(6480/256) = 26
    attn_nsplit   ceil(1024/97) = 11  <  ceil(6480/512) = 13
    gn_apply      ceil(1024/97) = 11  <  ceil(6480/256) = 26;  folded backward: bps_cap = ceil(256/97) = 3
    wgrad 27 taps ceil(512/97)  = 6   <  ceil(6480/128) = 51;  1 tap: ceil(4096/97) = 43 < ceil(6480/64) = 102; the 32 MiB cap
                  binds for the 96-channel concat convs
    head          ceil(628560/256) = 2456 blocks wanted, 1024 launched: a block takes 32 voxels per trip, so the loop makes 19 or
                  20 trips of 32 768 voxels where an uncapped grid makes exactly 8
    init_dgrad    (cd_denoise_vjp only) H*W = 144 <= 256: one band; ceil(512/97) = 6 z-chunks of ceil(45/6) = 8 planes, the last
                  one 5 planes
  dataset3 (vox 45*50*18 = 40 500), B = 9, B*vox = 364 500
    init_dgrad    H*W = 900 > 256: 5 bands of 12 rows (the last 2 rows) with halo rows; ceil(512/45) = 12 z-chunks of 4 planes
                  (the last 1 plane);  head: ceil(364500/256) = 1424 blocks wanted, 1024 launched (11 or 12 trips)
  hgcal (vox 28*12*21 = 7056), B = 90, B*vox = 635 040
    gn_nsplit     ceil(2048/90) = 23  <  ceil(7056/256) = 28;  attn_nsplit ceil(1024/90) = 12 < ceil(7056/512) = 14
    gn_apply      ceil(1024/90) = 12  <  28;  bps_cap = ceil(256/90) = 3;  head 2481 -> 1024 blocks
    init_dgrad    H*W = 252 <= 256: one band; ceil(512/90) = 6 z-chunks of ceil(28/6) = 5 planes, the last one 3 planes (the one-band
                  ragged-last-chunk form of dataset2's B = 97 line, here against the oracle)
  tiny (vox 512), B = 300, B*vox = 153 600
    one workgroup per sample in gn_bwd_small_kernel, the per-sample attention dctx weight gradient, embed_bwd and linear_wgrad:
    300 of each; bps_cap = 1; wgrad 27 taps: ceil(512/300) = 2 chunks < ceil(512/128) = 4

The level-1 and level-2 GroupNorm / attention splits stay voxel-limited here: their B*vox thresholds are the same, their voxel
counts 8 and 64 times smaller, so they turn batch-limited at batches in the thousands only.

The bars are the suite's own (test_gpu_train.py, test_gpu_denoise_grad.py): loss 1e-5 relative, worst parameter tensor 1e-4, all
parameter gradients together 5e-6, input gradient 2e-5 (whole batch and every sample's row), VJP against the training step 1e-6,
a repeated step bitwise.  The fp32 oracle's own error against an fp64 evaluation of the same graph does not grow with the batch
(all gradients 7e-7, worst tensor 2e-6, loss 3e-7 at dataset2 batch 2 and 24 and tiny batch 160).  The oracle runs on torch's
intra-op thread pool, which takes its size from OMP_NUM_THREADS."""
import time

import numpy as np
import pytest
import torch

from conftest import rel_l2
from grad_cases import check_parameter_gradients, cuda, inputs, oracle_of, train_steps_vs_oracle
from helpers import seeded_model_cfg
from oracle import torch_oracle as O

pytestmark = pytest.mark.gpu


def _vjp_vs_oracle(tag, m, cfg, B, seed, params=True):
    """dx and every parameter gradient of sum(w * denoise(x)) through CaloDiffusion.denoise against autograd through
    OracleModel.denoise (test_input_and_parameter_gradients_match_autograd's assertions); the input gradient also per sample.
    `params=False`: the input gradient alone.  Returns the device tensors (x, sigma, cond, w, dx) for a caller that goes on with
    the engine."""
    x, w, E, layers, sigma, _ = inputs(cfg, B, seed)
    om = oracle_of(cfg, m)
    xo = x.clone().requires_grad_(True)
    t0 = time.perf_counter()
    (om.denoise(xo, E, sigma, layers) * w).sum().backward()
    t_oracle = time.perf_counter() - t0

    m.zero_grad()
    xg, sg, wg = x.cuda().requires_grad_(True), sigma.cuda(), w.cuda()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = m.denoise(xg, E=E.cuda(), sigma=sg, layers=cuda(layers))
    assert out.requires_grad
    (out * wg).sum().backward()
    torch.cuda.synchronize()
    t_dev = time.perf_counter() - t0
    got, want = xg.grad.cpu().numpy(), xo.grad.numpy()
    err_x = rel_l2(got, want)
    rows = [rel_l2(got[b], want[b]) for b in range(B)]
    print(f"[{tag}] input gradient rel-L2 {err_x:.3e}, worst sample row {max(rows):.3e} (sample {int(np.argmax(rows))}, "
          f"sigma {float(sigma[int(np.argmax(rows))]):.3g}), device {t_dev:.3f} s, oracle {t_oracle:.2f} s")
    assert err_x < 2e-5
    assert max(rows) < 2e-5, sorted(zip(rows, range(B)), reverse=True)[:4]  # (a whole-batch norm averages one bad sample away)
    if params:
        check_parameter_gradients(tag, m, {k: v.grad for k, v in om.sd.items()})
    return xg.detach(), sg, m.cond_tensor(E.cuda(), cuda(layers)), wg, xg.grad


def test_dataset2_training_step_batch97():
    """Level 0 of Dataset-2 with every split of the backward path in its batch-limited branch (the table's B = 97 lines).  The first
    step carries the warm-up and the autotune; the two after it run the same kernels and must agree bitwise."""
    m, cfg = seeded_model_cfg("dataset2")
    steps = train_steps_vs_oracle("dataset2 B=97 train", m, cfg, 97, seed=97, steps=3)
    assert steps[1][0] == steps[2][0], (steps[1][0], steps[2][0])
    assert torch.equal(steps[1][1], steps[2][1])


def test_dataset3_training_step_batch9():
    """The cosine schedule (sigma from the table's entry of `time`) and the head's loop (1424 -> 1024 blocks)."""
    m, cfg = seeded_model_cfg("dataset3")
    train_steps_vs_oracle("dataset3 B=9 train", m, cfg, 9, seed=9)


def test_dataset3_denoise_vjp_input_gradient_batch9():
    """The banded init_dgrad (H*W = 900: 5 bands of 12 rows with halo rows, the last band 2 rows; 12 z-chunks of 4 planes, the last
    1 plane) with more than one sample.  launch_init_dgrad belongs to cd_denoise_vjp alone -- a training step needs no input
    gradient -- so the batch of test_dataset3_training_step_batch9 goes through the VJP as well, for its input gradient: against the
    oracle, whole and per sample, and bitwise the same in the input-only mode.

    The parameter gradients of this batch are the training-step test's.  Here they are not compared: for these inputs the fp32
    oracle's own error against an fp64 evaluation of the same graph is 7.8e-6 on all gradients together (1.0e-5 on
    ups.2.0.block1.proj.conv.weight: 364 500 fp32 terms per weight) where the device is 1.9e-6 away from that fp64 evaluation, so
    the 5e-6 bar lies below what this reference resolves (device against the fp32 oracle: 5.9e-6).  Its input gradient is good to
    6.5e-7 (device against fp64: 3.1e-7)."""
    m, cfg = seeded_model_cfg("dataset3")
    x, sigma, cond, w, dx = _vjp_vs_oracle("dataset3 B=9 vjp", m, cfg, 9, seed=19, params=False)
    dx_only, none = m.engine().denoise_vjp(x, sigma, cond, w, param_grads=False)
    assert none is None
    assert torch.equal(dx_only, dx)


def test_hgcal_denoise_vjp_batch90():
    """cd_denoise_vjp with three E columns and the phi input channel at B*vox = 635 040: dx and every parameter gradient; then the
    input-only mode (the GroupNorm queue's `discard` path, no weight-gradient queue) gives bitwise the same dx."""
    m, cfg = seeded_model_cfg("hgcal")
    x, sigma, cond, w, dx = _vjp_vs_oracle("hgcal B=90 vjp", m, cfg, 90, seed=90)
    eng = m.engine()
    dx_full, flat = eng.denoise_vjp(x, sigma, cond, w, param_grads=True)
    dx_only, none = eng.denoise_vjp(x, sigma, cond, w, param_grads=False)
    assert none is None and flat is not None
    assert torch.equal(dx_full, dx)
    assert torch.equal(dx_only, dx_full)


def test_dataset2_vjp_reproduces_training_step_batch97():
    """gy = d(hybrid l2 loss)/dD formed in torch: cd_denoise_vjp then gives cd_train_step's flat gradient
    (test_vjp_reproduces_training_step_gradients at the batch of test_dataset2_training_step_batch97)."""
    m, cfg = seeded_model_cfg("dataset2")
    B = 97
    data, noise, E, layers, sigma, _ = (cuda(t) for t in inputs(cfg, B, seed=21))
    eng = m.engine()
    cond = m.cond_tensor(E, layers)
    _, flat_train = eng.train_step(data, noise, sigma, cond, "l2")
    x = data + sigma.view(-1, 1, 1, 1, 1) * noise
    D = eng.denoise(x, sigma, cond)
    wgt = (1.0 + sigma.double() ** -2).view(-1, 1, 1, 1, 1)
    gy = (2.0 * wgt * (D.double() - data.double()) / (wgt.mean() * D.numel())).float().contiguous()
    dx, flat = eng.denoise_vjp(x, sigma, cond, gy, param_grads=True)
    # (the parameters' slices only: the flat buffer's alignment gaps are written by neither call)
    got = torch.cat([g.reshape(-1) for g in eng.param_grads(flat)]).cpu().numpy()
    want = torch.cat([g.reshape(-1) for g in eng.param_grads(flat_train)]).cpu().numpy()
    err = rel_l2(got, want)
    print(f"[dataset2 B=97] vjp vs training step: flat gradient rel-L2 {err:.3e}")
    assert err < 1e-6
    assert torch.isfinite(dx).all()


def test_tiny_training_step_batch300():
    """Many small samples: 300 workgroups (one per sample) in gn_bwd_small_kernel, the attention's per-sample dctx weight gradient,
    embed_bwd and linear_wgrad; the 27-tap weight gradient in 2 chunks against a cap of 4."""
    m, cfg = seeded_model_cfg("tiny")
    train_steps_vs_oracle("tiny B=300 train", m, cfg, 300, seed=300)


# Deeper than the shipped four-entry nets: nets whose steps fill GnParamJobs (64 jobs) resp. WgradReduceQueue (80 jobs) and flush them
# mid-step.  The jobs were counted on the device with a temporary counter in launch_gn_param_jobs / wgrad_queue_flush: see the test.
DEEP = {
    "five": dict(LAYER_SIZE_UNET=[32, 32, 32, 64, 32], SHAPE_PAD=[-1, 1, 16, 16, 8], SHAPE_FINAL=[-1, 1, 16, 16, 8]),
    "six": dict(LAYER_SIZE_UNET=[32, 32, 32, 32, 64, 32], SHAPE_PAD=[-1, 1, 32, 32, 16], SHAPE_FINAL=[-1, 1, 32, 32, 16]),
    "seven": dict(LAYER_SIZE_UNET=[32, 32, 32, 64, 32, 64, 32], SHAPE_PAD=[-1, 1, 32, 32, 32], SHAPE_FINAL=[-1, 1, 32, 32, 32]),
}


@pytest.mark.parametrize("depth", ["five", "six", "seven"])
def test_deeper_nets_flush_the_queues_mid_step(depth):
    """The tiny config with five LAYER_SIZE_UNET entries on a 16x16x8 grid (levels 16.16.8 -> 8.8.4 -> 4.4.2 -> 2.2.1), six on
    32x32x16 and seven on 32x32x32 (down to 1.1.1), batch 2: the training step and the VJP with parameter gradients against the
    oracle built from the same overrides.

    Queued jobs per step, counted on the device (the same for the training step and the VJP; the shipped four-entry nets: 44
    GroupNorm jobs, 44 to 57 weight-gradient reductions):
        five   56 GroupNorm jobs, 74 weight-gradient reductions: neither queue fills (the next depth up from the shipped nets)
        six    68 GroupNorm jobs: flushed at 64, 4 at the end;  78 weight-gradient reductions: not yet 80, hence the third net
        seven  80 GroupNorm jobs: flushed at 64, 16 at the end;  94 weight-gradient reductions: flushed at 80, 14 at the end"""
    m, cfg = seeded_model_cfg("tiny", DEEP[depth])
    assert O.spec_from_config(cfg).layer_sizes == DEEP[depth]["LAYER_SIZE_UNET"]
    assert tuple(O.spec_from_config(cfg).data_shape) == tuple(DEEP[depth]["SHAPE_FINAL"][2:]) == tuple(m.engine().grid)
    train_steps_vs_oracle(f"tiny/{depth} B=2 train", m, cfg, 2, seed=6)
    _vjp_vs_oracle(f"tiny/{depth} B=2 vjp", m, cfg, 2, seed=7)
