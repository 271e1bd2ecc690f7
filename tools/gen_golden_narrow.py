"""Generate the narrow-width fixtures from the reference's own classes: tests/golden/narrow_pion.npz, narrow_pion_grads.npz and
narrow_pion_samplers.npz from its ``CaloDiffusion`` on the Dataset-1 pion config (LAYER_SIZE_UNET [16, 16, 16, 32], SHOWER_EMBED
'orig-NN', DATASET_NUM 0) over a SYNTHETIC binning file, tests/golden/binning_ds0_synthetic.xml, and narrow_tiny.npz from the
``tiny`` config with LAYER_SIZE_UNET [16, 16, 32, 64] (no embedding, 8x8x8).  The synthetic file has what the model needs from the
CaloChallenge pion file: seven layers with voxels (alpha 1, 10, 10, 10, 1, 10, 1; 5, 9, 11, 6, 5, 5 and 3 radial bins: 323 voxels) and
one without between them, edges that are subsets of the 24 Dataset-0 edges the reference's ``create_R_Z_image`` hard-codes and
together cover all of them (dim_r_out 23); layers 0 and 5 start above 0.

TEST INFRASTRUCTURE, like oracle/gen_golden.py: runs only where the reference is mounted, on the CPU, and imports it through that
script's stub-import preamble (by importing the script).  Only data is written.

    python tools/gen_golden_narrow.py [--out-dir DIR]      # default tests/golden

Stored, as tools/gen_golden_ds1_model.py stores them (tests/narrow_cases.py has the cases):
  xml.*, lay.*   what the reference's XMLHandler reads from the file; the layout of the reference's GeomConverter
  ck_keys / ck_vals / sd_keys, nn.*   checksums of the seeded state_dict, the perturbed NN_embed matrices
  den.<objective>.<time embed>.b3 / .b1     denoise at B = 3 and at B = 1 (rows [0:1])
  loss.<objective>.<loss type>.*            loss, U-Net gradient checksums and a few whole tensors, NN_embed gradients in full
  vjp.<objective>.*                         the same for sum(denoise(x) * cot), with dx
  ddim.* / ddpm.*                           4-step trajectories (xs, x0s), the start tensor and DDPM's per-step noise
  f64.names / f64.dist / f64.all            distance of the reference's float32 gradients from a float64 restatement (oracle U-Net
                                            between two matmul maps), per tensor (worst over the loss cases) and all together
narrow_tiny.npz: ck_*, inputs, den.b2, loss.loss, loss.ck_*, loss.grad.<picked>, f64.*
"""
from __future__ import annotations

import argparse
import copy
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from oracle import gen_golden as G  # noqa: E402  (stubs the absent modules and puts the reference on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from calodiffusion.utils.XMLHandler import XMLHandler as RefXMLHandler  # noqa: E402
import narrow_cases as N  # noqa: E402

# (whole tensors kept small: seven gradient records share one file)
PICK = ["init_conv.conv.weight", "downs_attn.1.fn.fn.to_qkv.conv.weight", "mid_attn.fn.fn.to_out.0.conv.weight", "time_mlp.1.weight",
        "cond_mlp.4.bias", "final_conv.1.conv.weight", "final_conv.1.conv.bias", "mid_block1.block2.norm.weight",
        "downs.2.0.res_conv.conv.weight", "downs.0.0.mlp.1.weight", "ups.1.2.convTrans.bias", "ups.2.0.block1.proj.conv.bias"]
PICK_TINY = ["init_conv.conv.weight", "downs.1.0.res_conv.conv.weight", "downs.0.2.conv.weight", "ups.1.2.convTrans.weight",
             "ups.2.0.res_conv.conv.weight", "final_conv.1.conv.weight", "downs_attn.0.fn.fn.to_qkv.conv.weight",
             "mid_block2.block1.norm.bias", "cond_mlp.0.weight"]


def xml_record():
    h = RefXMLHandler("pion", N.XML)
    return {"xml.r_edges": np.concatenate([np.asarray(e, dtype=np.float64) for e in h.r_edges]),
            "xml.n_edges": np.array([len(e) for e in h.r_edges]), "xml.r_bins": np.array(h.r_bins), "xml.a_bins": np.array(h.a_bins),
            "xml.bin_edges": np.array(h.GetBinEdges()), "xml.relevant": np.array(h.GetRelevantLayers()),
            "xml.total": np.array(h.GetTotalNumberOfBins())}


def build(objective, time_embed, loss_type, nn_sd=None):
    cfg = N.config(objective, time_embed, LOSS_TYPE=loss_type)
    torch.manual_seed(G.SEED)
    m = G.RefCaloDiffusion(copy.deepcopy(cfg), n_steps=cfg["NSTEPS"], loss_type=loss_type)
    m.eval()
    assert m.do_embed and m.NN_embed.gc.dim_r_out == N.GRID[2] and int(m.NN_embed.gc.layer_boundaries[-1]) == N.V
    assert sum(p.numel() for p in m.model.parameters()) == N.PION_PARAMS
    if nn_sd is not None:
        m.NN_embed.load_state_dict(nn_sd)
    return m, cfg


def grads_record(tag, m, out, pick):
    unet = {k: p.grad for k, p in m.model.named_parameters()}
    keys, cks = G.checksums(unet)
    out[f"{tag}.ck_keys"], out[f"{tag}.ck_vals"] = keys, cks
    for k in pick:
        out[f"{tag}.grad.{k}"] = G.npf(unet[k])
    if getattr(m, "NN_embed", None) is not None:
        for k, p in m.NN_embed.named_parameters():
            out[f"{tag}.nn.{k}"] = G.npf(p.grad)


def f64_distance(worst, ref, g64):
    """per-tensor rel-l2 of float32 reference gradients from float64 ones (worst so far kept), and the same of all together"""
    for k in ref:
        if float(g64[k].abs().max()) > 0:
            worst[k] = max(worst.get(k, 0.0), N.rel_l2(ref[k].numpy(), g64[k].numpy()))
    keys = list(ref)
    return N.rel_l2(np.concatenate([ref[k].numpy().ravel() for k in keys]), np.concatenate([g64[k].numpy().ravel() for k in keys]))


def pion(out_dir):
    out, traj = xml_record(), {}
    m, cfg = build("hybrid_weight", "log", "l2")
    keys, cks = G.checksums(m.state_dict())
    out["ck_keys"], out["ck_vals"], out["sd_keys"] = keys, cks, np.array(list(m.state_dict().keys()))
    bound, alpha, rin = N.layout(m.NN_embed.gc)
    out["lay.bound"], out["lay.alpha"], out["lay.rin"] = np.array(bound), np.array(alpha), np.array(rin)
    gen = torch.Generator().manual_seed(G.SEED + 93)
    with torch.no_grad():
        for p in m.NN_embed.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=gen))
    nn_sd = copy.deepcopy(m.NN_embed.state_dict())
    for k, v in nn_sd.items():
        out[f"nn.{k}"] = G.npf(v)

    x = N.eighths(gen, (3, N.V), -16, 16)
    E = N.eighths(gen, (3, 1), 1, 8)
    layers = N.eighths(gen, (3, 1 + N.GRID[0]), -8, 8)
    sigma = torch.tensor(N.SIGMAS)
    data = N.eighths(gen, (3, N.V), -12, 12)
    noise = N.eighths(gen, (3, N.V), -16, 16)
    rnd = N.eighths(gen, (3,), -12, 12)
    cot = N.eighths(gen, (3, N.V), -12, 12)
    out.update(x=G.npf(x), E=G.npf(E), layers=G.npf(layers), sigma=G.npf(sigma), data=G.npf(data), noise=G.npf(noise),
               rnd_normal=G.npf(rnd), cot=G.npf(cot))

    for obj in N.OBJECTIVES:
        for te in N.TIME_EMBEDS:
            mm, _ = build(obj, te, "l2", nn_sd)
            with torch.no_grad():
                y3 = mm.denoise(x, E=E, sigma=sigma.reshape(3, 1), layers=layers)
                y1 = mm.denoise(x[:1], E=E[:1], sigma=sigma[:1].reshape(1, 1), layers=layers[:1])
            out[f"den.{obj}.{te}.b3"], out[f"den.{obj}.{te}.b1"] = G.npf(y3), G.npf(y1)
            print(f"denoise {obj} {te}: mean|y| {float(y3.abs().mean()):.4f}  rows B3 vs B1 {N.rel_l2(G.npf(y3[:1]), G.npf(y1)):.2e}")

    worst64, all64 = {}, 0.0
    for obj, lt in N.LOSS_CASES:
        mm, c = build(obj, "log", lt, nn_sd)
        mm.train()
        mm.zero_grad()
        loss = mm.compute_loss(data, E, noise=noise, layers=layers, rnd_normal=rnd)
        loss.backward()
        tag = f"loss.{obj}.{lt}"
        out[f"{tag}.loss"] = np.array(float(loss), dtype=np.float64)
        grads_record(tag, mm, out, PICK)
        sd = {k: v.detach().double().requires_grad_(True) for k, v in mm.model.state_dict().items()}
        Ws = [lay.weight.detach().double().requires_grad_(True) for lay in mm.NN_embed.encs]
        Ds = [lay.weight.detach().double().requires_grad_(True) for lay in mm.NN_embed.decs]
        sg = (rnd * mm.loss_function.P_std + mm.loss_function.P_mean).exp()
        l64 = N.oracle_loss(c, sd, Ws, Ds, N.layout(mm.NN_embed.gc), data, E, noise, sg, layers, lt, torch.float64)
        l64.backward()
        ref = {k: p.grad for k, p in mm.model.named_parameters()}
        g64 = {k: v.grad for k, v in sd.items()}
        for i in range(len(Ws)):
            ref[f"NN_embed.encs.{i}.weight"], g64[f"NN_embed.encs.{i}.weight"] = mm.NN_embed.encs[i].weight.grad, Ws[i].grad
            ref[f"NN_embed.decs.{i}.weight"], g64[f"NN_embed.decs.{i}.weight"] = mm.NN_embed.decs[i].weight.grad, Ds[i].grad
        d_all = f64_distance(worst64, ref, g64)
        all64 = max(all64, d_all)
        print(f"{tag}: loss {float(loss):.6f} (float64 restatement {float(l64):.6f}); float32 gradients from float64, all together {d_all:.2e}")
    out["f64.names"] = np.array(sorted(worst64))
    out["f64.dist"] = np.array([worst64[k] for k in sorted(worst64)])
    out["f64.all"] = np.array(all64)
    top = sorted(worst64.items(), key=lambda kv: -kv[1])[:5]
    print("float32 reference gradients vs float64 restatement, worst tensors:", [(k, f"{v:.2e}") for k, v in top])

    for obj in N.OBJECTIVES:
        mm, _ = build(obj, "log", "l2", nn_sd)
        mm.zero_grad()
        xg = x.clone().requires_grad_(True)
        y = mm.denoise(xg, E=E, sigma=sigma.reshape(3, 1), layers=layers)
        (y * cot).sum().backward()
        out[f"vjp.{obj}.dx"] = G.npf(xg.grad)
        grads_record(f"vjp.{obj}", mm, out, PICK)

    mm, c = build("hybrid_weight", "log", "l2", nn_sd)
    start = N.eighths(gen, (3, N.V), -16, 16)
    traj.update(start=G.npf(start), E=G.npf(E), layers=G.npf(layers))
    S = G.ref_sample
    with torch.no_grad():
        xf, xs, x0s = S.DDim(copy.deepcopy(c))(mm, start.clone(), E, layers, N.TRAJ_STEPS, 0, False)
    traj.update({"ddim.x": G.npf(xf), "ddim.xs": np.stack([G.npf(t) for t in xs]), "ddim.x0s": np.stack([G.npf(t) for t in x0s])})
    torch.manual_seed(779)
    traj["ddpm.noise"] = np.stack([G.npf(torch.randn(start.shape)) for _ in range(N.TRAJ_STEPS)])
    torch.manual_seed(779)  # the sampler draws torch.randn(x.shape) once per step from the global stream
    with torch.no_grad():
        xf, xs, x0s = S.DDPM(copy.deepcopy(c))(mm, start.clone(), E, layers, N.TRAJ_STEPS, 0, False)
    traj.update({"ddpm.x": G.npf(xf), "ddpm.xs": np.stack([G.npf(t) for t in xs]), "ddpm.x0s": np.stack([G.npf(t) for t in x0s])})

    grads = {k: out.pop(k) for k in list(out) if k.startswith(("loss.", "vjp."))}
    for name, d in (("narrow_pion.npz", out), ("narrow_pion_grads.npz", grads), ("narrow_pion_samplers.npz", traj)):
        path = os.path.join(out_dir, name)
        np.savez_compressed(path, **d)
        print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


def tiny(out_dir):
    cfg = N.tiny_config()
    m = G.build_ref(cfg)  # (asserts that our parameter holder reproduces the reference's initialisation for these widths)
    out = {}
    out["ck_keys"], out["ck_vals"] = G.checksums(m.state_dict())
    gen = torch.Generator().manual_seed(G.SEED + 94)
    B = 2
    x = N.eighths(gen, (B, 1, 8, 8, 8), -16, 16)
    data = N.eighths(gen, (B, 1, 8, 8, 8), -12, 12)
    noise = N.eighths(gen, (B, 1, 8, 8, 8), -16, 16)
    E = N.eighths(gen, (B, 3), 1, 8)
    layers = N.eighths(gen, (B, 9), -8, 8)
    rnd = N.eighths(gen, (B,), -12, 12)
    sigma = torch.tensor(N.SIGMAS[:B])
    out.update(x=G.npf(x), data=G.npf(data), noise=G.npf(noise), E=G.npf(E), layers=G.npf(layers), rnd_normal=G.npf(rnd),
               sigma=G.npf(sigma))
    with torch.no_grad():
        out["den.b2"] = G.npf(m.denoise(x, E=E, sigma=sigma.reshape(B, 1, 1, 1, 1), layers=layers))
    m.train()
    m.zero_grad()
    loss = m.compute_loss(data, E, noise=noise, layers=layers, rnd_normal=rnd)
    loss.backward()
    out["loss.loss"] = np.array(float(loss), dtype=np.float64)
    grads_record("loss", m, out, PICK_TINY)
    sd = {k: v.detach().double().requires_grad_(True) for k, v in m.model.state_dict().items()}
    sg = (rnd * m.loss_function.P_std + m.loss_function.P_mean).exp()
    l64 = N.grid_oracle_loss(cfg, sd, data, E, noise, sg, layers, torch.float64)
    l64.backward()
    worst = {}
    d_all = f64_distance(worst, {k: p.grad for k, p in m.model.named_parameters()}, {k: v.grad for k, v in sd.items()})
    out["f64.names"], out["f64.dist"], out["f64.all"] = np.array(sorted(worst)), np.array([worst[k] for k in sorted(worst)]), np.array(d_all)
    print(f"narrow tiny: loss {float(loss):.6f} (float64 restatement {float(l64):.6f}); float32 gradients from float64, all together "
          f"{d_all:.2e}, worst tensor {max(worst.values()):.2e}")
    path = os.path.join(out_dir, "narrow_tiny.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=G.GOLD)
    args = ap.parse_args()
    pion(args.out_dir)
    tiny(args.out_dir)
