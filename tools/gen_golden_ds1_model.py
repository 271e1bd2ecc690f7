"""Generate tests/golden/ds1_model.npz, ds1_model_grads.npz (the loss.* and vjp.* entries) and ds1_model_samplers.npz from the reference's own ``CaloDiffusion`` with an in-model ``NNConverter``
(calodiffusion/models/calodiffusion.py:86-119, 154-169): SHOWER_EMBED 'orig-NN', the Dataset-1 photon config's U-Net keys, and a
SYNTHETIC binning file, tests/golden/binning_ds1_synthetic.xml.  The real CaloChallenge binning XML is not available where the
fixtures are made; the synthetic one has what the model needs from it: five layers with alpha (1, 10, 10, 1, 1) and 8, 16, 19, 5
and 5 radial bins (368 voxels) whose edges are subsets of the 31 integer-valued Dataset-1 edges that the reference's
``create_R_Z_image`` hard-codes (utils.py:71-) -- so dim_r_out is 30, as that function asserts -- which together cover all of them;
layers 0 and 4 start above 0, layers 0, 2 and 4 end below the outermost edge, and a layer without voxels sits between them.

TEST INFRASTRUCTURE, like oracle/gen_golden.py: runs only where the reference is mounted, on the CPU, and imports it through that
script's stub-import preamble (by importing the script).  Only data is written.

    python tools/gen_golden_ds1_model.py [--out-dir DIR]      # default tests/golden

The reference model is built from a config whose BIN_FILE is the synthetic XML, after ``torch.manual_seed(SEED)``; key list and
checksums of its full state_dict are stored.  Then the NN_embed matrices get a dense O(0.1) perturbation from a second generator
(every element carries signal) and are stored.  Inputs are multiples of 1/8.  Stored (tests/ds1_model_cases.py has the cases):
  xml.*        what the reference's XMLHandler reads from the file
  ck_keys / ck_vals, nn.*   checksums of the seeded state_dict, the perturbed matrices
  den.<objective>.<time embed>.b3 / .b1     denoise at B = 3 and at B = 1 (rows [0:1])
  loss.<objective>.<loss type>.*            loss, U-Net gradient checksums and a few whole tensors, NN_embed gradients in full
  vjp.<objective>.*                         the same for sum(denoise(x) * cot), with dx
  ddim.* / ddpm.*                           4-step trajectories (xs, x0s), the start tensor and DDPM's per-step noise
  smp.<tag>.ran / .rows / .x                which further samplers run on the flat state (at B = 3, else at B = 1: rows [0:1]), and
                                            their final state
  f64.*        distance of the reference's float32 NN_embed gradients from a float64 restatement (oracle U-Net + two matmul maps)
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
import ds1_model_cases as K  # noqa: E402

# (whole tensors kept small: seven gradient records share one file)
PICK = ["init_conv.conv.weight", "downs_attn.1.fn.fn.to_qkv.conv.weight", "mid_attn.fn.fn.to_qkv.conv.weight", "time_mlp.1.weight",
        "cond_mlp.4.bias", "final_conv.1.conv.weight", "final_conv.1.conv.bias", "mid_block1.block2.norm.weight",
        "downs.1.0.res_conv.conv.weight"]


def xml_record():
    h = RefXMLHandler("photon", K.XML)
    return {"xml.r_edges": np.concatenate([np.asarray(e, dtype=np.float64) for e in h.r_edges]),
            "xml.n_edges": np.array([len(e) for e in h.r_edges]), "xml.r_bins": np.array(h.r_bins), "xml.a_bins": np.array(h.a_bins),
            "xml.bin_edges": np.array(h.GetBinEdges()), "xml.relevant": np.array(h.GetRelevantLayers()),
            "xml.n_alpha": np.array([len(a[0]) if h.r_bins[i] > 0 else 0 for i, a in enumerate(h.alphaListPerLayer)]),
            "xml.alpha0": np.asarray(h.alphaListPerLayer[1][0], dtype=np.float64), "xml.total": np.array(h.GetTotalNumberOfBins())}


def build(objective, time_embed, loss_type, nn_sd=None):
    cfg = K.config(objective, time_embed, LOSS_TYPE=loss_type)
    torch.manual_seed(G.SEED)
    m = G.RefCaloDiffusion(copy.deepcopy(cfg), n_steps=cfg["NSTEPS"], loss_type=loss_type)
    m.eval()
    assert m.do_embed and m.NN_embed.gc.dim_r_out == 30 and int(m.NN_embed.gc.layer_boundaries[-1]) == K.V
    if nn_sd is not None:
        m.NN_embed.load_state_dict(nn_sd)
    return m, cfg


def grads_record(tag, m, out):
    unet = {k: p.grad for k, p in m.model.named_parameters()}
    keys, cks = G.checksums(unet)
    out[f"{tag}.ck_keys"], out[f"{tag}.ck_vals"] = keys, cks
    for k in PICK:
        out[f"{tag}.grad.{k}"] = G.npf(unet[k])
    for k, p in m.NN_embed.named_parameters():
        out[f"{tag}.nn.{k}"] = G.npf(p.grad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=G.GOLD)
    args = ap.parse_args()
    out, traj = xml_record(), {}

    m, cfg = build("hybrid_weight", "log", "l2")
    keys, cks = G.checksums(m.state_dict())
    out["ck_keys"], out["ck_vals"], out["sd_keys"] = keys, cks, np.array(list(m.state_dict().keys()))
    gen = torch.Generator().manual_seed(G.SEED + 91)
    with torch.no_grad():
        for p in m.NN_embed.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=gen))
    nn_sd = copy.deepcopy(m.NN_embed.state_dict())
    for k, v in nn_sd.items():
        out[f"nn.{k}"] = G.npf(v)

    x = K.eighths(gen, (3, K.V), -16, 16)
    E = K.eighths(gen, (3, 1), 1, 8)
    layers = K.eighths(gen, (3, 1 + K.GRID[0]), -8, 8)
    sigma = torch.tensor(K.SIGMAS)
    data = K.eighths(gen, (3, K.V), -12, 12)
    noise = K.eighths(gen, (3, K.V), -16, 16)
    rnd = K.eighths(gen, (3,), -12, 12)
    cot = K.eighths(gen, (3, K.V), -12, 12)
    out.update(x=G.npf(x), E=G.npf(E), layers=G.npf(layers), sigma=G.npf(sigma), data=G.npf(data), noise=G.npf(noise),
               rnd_normal=G.npf(rnd), cot=G.npf(cot))

    # denoise
    for obj in K.OBJECTIVES:
        for te in K.TIME_EMBEDS:
            mm, _ = build(obj, te, "l2", nn_sd)
            with torch.no_grad():
                y3 = mm.denoise(x, E=E, sigma=sigma.reshape(3, 1), layers=layers)
                y1 = mm.denoise(x[:1], E=E[:1], sigma=sigma[:1].reshape(1, 1), layers=layers[:1])
            out[f"den.{obj}.{te}.b3"], out[f"den.{obj}.{te}.b1"] = G.npf(y3), G.npf(y1)
            print(f"denoise {obj} {te}: mean|y| {float(y3.abs().mean()):.4f}  rows B3 vs B1 {K.rel_l2(G.npf(y3[:1]), G.npf(y1)):.2e}")

    # losses and gradients; the float64 distance of the NN_embed gradients
    worst64 = {}
    for obj, lt in K.LOSS_CASES:
        mm, c = build(obj, "log", lt, nn_sd)
        mm.train()
        mm.zero_grad()
        loss = mm.compute_loss(data, E, noise=noise, layers=layers, rnd_normal=rnd)
        loss.backward()
        tag = f"loss.{obj}.{lt}"
        out[f"{tag}.loss"] = np.array(float(loss), dtype=np.float64)
        grads_record(tag, mm, out)
        # the same in float64 through the restatement
        sd = {k: v.detach().clone() for k, v in mm.model.state_dict().items()}
        Ws = [lay.weight.detach().double().requires_grad_(True) for lay in mm.NN_embed.encs]
        Ds = [lay.weight.detach().double().requires_grad_(True) for lay in mm.NN_embed.decs]
        sg = (rnd * mm.loss_function.P_std + mm.loss_function.P_mean).exp()
        l64 = K.oracle_loss(c, sd, Ws, Ds, K.layout(mm.NN_embed.gc), data, E, noise, sg, layers, lt, torch.float64)
        l64.backward()
        print(f"{tag}: loss {float(loss):.6f} (float64 restatement {float(l64):.6f})")
        for i in range(len(Ws)):
            for nm, ref, g64 in ((f"encs.{i}", mm.NN_embed.encs[i].weight.grad, Ws[i].grad), (f"decs.{i}", mm.NN_embed.decs[i].weight.grad, Ds[i].grad)):
                d = K.rel_l2(ref.numpy(), g64.numpy())
                worst64[nm] = max(worst64.get(nm, 0.0), d)
    out["f64.names"] = np.array(sorted(worst64))
    out["f64.dist"] = np.array([worst64[k] for k in sorted(worst64)])
    print("float32 reference NN_embed gradients vs float64 restatement, worst over the loss cases:",
          {k: f"{v:.2e}" for k, v in sorted(worst64.items())})

    # denoise VJP
    for obj in K.OBJECTIVES:
        mm, _ = build(obj, "log", "l2", nn_sd)
        mm.zero_grad()
        xg = x.clone().requires_grad_(True)
        y = mm.denoise(xg, E=E, sigma=sigma.reshape(3, 1), layers=layers)
        (y * cot).sum().backward()
        out[f"vjp.{obj}.dx"] = G.npf(xg.grad)
        grads_record(f"vjp.{obj}", mm, out)

    # samplers
    mm, c = build("hybrid_weight", "log", "l2", nn_sd)
    start = K.eighths(gen, (3, K.V), -16, 16)
    traj.update(start=G.npf(start), E=G.npf(E), layers=G.npf(layers))
    S = G.ref_sample
    with torch.no_grad():
        xf, xs, x0s = S.DDim(copy.deepcopy(c))(mm, start.clone(), E, layers, K.TRAJ_STEPS, 0, False)
    traj.update({"ddim.x": G.npf(xf), "ddim.xs": np.stack([G.npf(t) for t in xs]), "ddim.x0s": np.stack([G.npf(t) for t in x0s])})
    ngen_seed = 779
    torch.manual_seed(ngen_seed)
    traj["ddpm.noise"] = np.stack([G.npf(torch.randn(start.shape)) for _ in range(K.TRAJ_STEPS)])
    torch.manual_seed(ngen_seed)  # the sampler draws torch.randn(x.shape) once per step from the global stream
    with torch.no_grad():
        xf, xs, x0s = S.DDPM(copy.deepcopy(c))(mm, start.clone(), E, layers, K.TRAJ_STEPS, 0, False)
    traj.update({"ddpm.x": G.npf(xf), "ddpm.xs": np.stack([G.npf(t) for t in xs]), "ddpm.x0s": np.stack([G.npf(t) for t in x0s])})
    print(f"ddim / ddpm: xs {traj['ddim.xs'].shape} x0s {traj['ddim.x0s'].shape}")
    for tag, cls, n, over in K.OTHER_SAMPLERS:
        cc = copy.deepcopy(c)
        cc.update(over)
        ok, xf, rows = False, None, 0
        for rows in (3, 1):  # several pass sigma as (B,), which broadcasts against (B, 368) only at B = 1: then rows [0:1]
            try:
                with torch.no_grad():
                    xf, _, _ = getattr(S, cls)(cc)(mm, start[:rows].clone(), E[:rows], layers[:rows], n, 0, False)
                ok = bool(torch.isfinite(xf).all()) and tuple(xf.shape) == (rows, K.V)
                mm.loss_function.update_step(c["NSTEPS"])
                break
            except Exception as e:
                print(f"sampler {tag}: the reference fails on the flat state at B = {rows}: {type(e).__name__}: {str(e)[:100]}")
                mm.loss_function.update_step(c["NSTEPS"])
        traj[f"smp.{tag}.ran"], traj[f"smp.{tag}.rows"] = np.array(ok), np.array(rows)
        if ok:
            traj[f"smp.{tag}.x"] = G.npf(xf)
            print(f"sampler {tag}: ran at B = {rows}, mean|x| {float(xf.abs().mean()):.4f}")
        elif xf is not None:
            print(f"sampler {tag}: ran but is not usable: shape {tuple(xf.shape)}, finite {bool(torch.isfinite(xf).all())}")

    grads = {k: out.pop(k) for k in list(out) if k.startswith(("loss.", "vjp."))}
    for name, d in (("ds1_model.npz", out), ("ds1_model_grads.npz", grads), ("ds1_model_samplers.npz", traj)):
        path = os.path.join(args.out_dir, name)
        np.savez_compressed(path, **d)
        print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
