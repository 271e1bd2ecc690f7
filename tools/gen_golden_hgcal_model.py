"""Generate tests/golden/hgcal_model.npz, hgcal_model_grads.npz, hgcal_model_samplers.npz and hgcal_model_t.npz from the
reference's own ``CaloDiffusion`` with an ``HGCalConverter`` inside forward (calodiffusion/models/calodiffusion.py:86-98, 113-117)
and from its ``Embeder`` / ``Decoder`` under autograd (calodiffusion/utils/HGCal_utils.py:295-353), on SYNTHETIC geometries: the
geometry pickle of the HGCalShowers package is not available where the fixtures are made, so ``load_geom`` is replaced, inside
this tool, by a function that returns the geometry object ``tools/gen_golden_hgcal_geom.py:synthetic_geometry`` makes.

TEST INFRASTRUCTURE, like oracle/gen_golden.py: runs only where the reference is mounted, on the CPU, and imports it through that
script's stub-import preamble (by importing the script).  Only data is written.

    python tools/gen_golden_hgcal_model.py [--out-dir DIR]      # default tests/golden

Geometry "m": 8 layers onto the ``tiny`` config's (8, 8, 8) grid, max_ncell 61, ragged ncells with one layer of the centre cell
only, cells at angular bin edges (the 0.5 / 0.5 split), rings 0 .. 7.  The model: the ``tiny`` config with SHOWER_EMBED 'NN',
SHAPE_PAD [-1, 1, 8, 61], TRAINABLE_EMBED True, built after ``torch.manual_seed(SEED)``, then ``NN_embed.init()``; key list and
checksums of that state_dict are stored.  Then every element of both ``mat``s, outside the masks too, gets an O(0.1)
perturbation from a second generator.  Inputs are multiples of 1/8.  Stored (tests/hgcal_model_cases.py has the cases):
  m.*          the geometry arrays; init.* the maps and masks ``init()`` made; nn.* the perturbed maps
  sd_keys, ck_keys / ck_vals                 the seeded, initialised state_dict
  den.<objective>.<time embed>.b3 / .b1      denoise at B = 3 and at B = 1 (rows [0:1])
  loss.<objective>.<loss type>.*             loss, U-Net gradient checksums and a few whole tensors, both ``mat`` gradients: their
                                             masked entries in row-major order (the generator asserts exact zeros elsewhere)
  vjp.<objective>.*                          the same for sum(denoise(x) * cot), with dx
  ddim.* / ddpm.*                            4-step trajectories (xs, x0s), the start tensor and DDPM's per-step noise
  smp.<tag>.ran / .rows / .x                 which further samplers run on the cell-space state, and their final state
  f64.*        distance of the reference's float32 ``mat`` gradients (masked entries) from a float64 restatement
  frozen.*     trainable=False (the shipped TRAINABLE_EMBED: False; the maps are init()'s): one denoise, loss and U-Net gradients
  rn.*         ReverseNormHGCal(embed=False) of one cell-space batch
Geometry "t" (hgcal_model_t.npz, maps only): 2 layers, 4 x 26 bins, max_ncell 300, rings up to 30 -- more than 256 cells a layer.
  t.*          the geometry arrays and init()'s maps and masks; the maps in use are those plus
               ``hgcal_model_cases.hashed_perturbation`` (exact on every platform, so it is not stored)
  t.enc / t.dec                              Embeder(x) and Decoder(z), trainable=True, at batch_rows 3
  t.enc.dx / .dm, t.dec.dx / .dm             autograd's input gradient and masked ``mat`` gradient for one cotangent each
"""
from __future__ import annotations

import argparse
import copy
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from oracle import gen_golden as G  # noqa: E402  (stubs the absent modules and puts the reference on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from calodiffusion.utils import HGCal_utils as ref_hg  # noqa: E402
import gen_golden_hgcal_geom as GG  # noqa: E402
import hgcal_model_cases as K  # noqa: E402

# (whole tensors kept small: eight gradient records share one file)
PICK = ["init_conv.conv.weight", "downs_attn.1.fn.fn.to_qkv.conv.weight", "mid_attn.fn.fn.to_qkv.conv.weight", "time_mlp.1.weight",
        "cond_mlp.4.bias", "final_conv.1.conv.weight", "final_conv.1.conv.bias", "mid_block1.block2.norm.weight",
        "downs.1.0.res_conv.conv.weight"]

GEOM_M = GG.synthetic_geometry(K.LAYERS, K.GRID[1], K.NCELLS_M, K.GRID[2] - 1, seed=G.SEED + 81)
ref_hg.load_geom = lambda geom_filename: GEOM_M  # the pickle is not available: the synthetic geometry stands in for it


def build(objective, time_embed, loss_type, nn_sd=None, trainable=True):
    cfg = K.config(objective, time_embed, LOSS_TYPE=loss_type, TRAINABLE_EMBED=trainable)
    torch.manual_seed(G.SEED)
    m = G.RefCaloDiffusion(copy.deepcopy(cfg), n_steps=cfg["NSTEPS"], loss_type=loss_type)
    m.eval()
    assert m.do_embed and tuple(m.NN_embed.embeder.mat.shape) == (K.LAYERS, K.E_GRID, K.CELLS)
    if trainable:
        m.NN_embed.init()  # (a trainable converter is left un-initialised by the model, calodiffusion.py:116-117)
        if nn_sd is not None:
            m.NN_embed.load_state_dict(nn_sd)
    return m, cfg


def mat_grads(m):
    """{name: (gradient, mask)} of the two maps; exact zeros outside the masks"""
    out = {}
    for name, mod in (("embeder.mat", m.NN_embed.embeder), ("decoder.mat", m.NN_embed.decoder)):
        g, mask = mod.mat.grad, mod.mask
        assert bool((g[~mask] == 0).all()), f"{name}: the reference's gradient is not 0 outside the mask"
        out[name] = (g, mask)
    return out


def grads_record(tag, m, out, with_nn=True):
    unet = {k: p.grad for k, p in m.model.named_parameters()}
    keys, cks = G.checksums(unet)
    out[f"{tag}.ck_keys"], out[f"{tag}.ck_vals"] = keys, cks
    for k in PICK:
        out[f"{tag}.grad.{k}"] = G.npf(unet[k])
    if with_nn:
        for name, (g, mask) in mat_grads(m).items():
            out[f"{tag}.nn.{name}"] = K.masked(G.npf(g), mask.numpy())


def model_records(args):
    out, traj = {}, {}
    out.update({f"m.{k[2:]}": v for k, v in GG.geom_arrays("m", GEOM_M).items()})
    m, cfg = build("hybrid_weight", "log", "l2")
    sd = m.state_dict()
    keys, cks = G.checksums(sd)
    out["ck_keys"], out["ck_vals"], out["sd_keys"] = keys, cks, np.array(list(sd.keys()))
    emb, dcd = m.NN_embed.embeder, m.NN_embed.decoder
    out.update({"init.enc_mat": G.npf(emb.mat), "init.dec_mat": G.npf(dcd.mat), "init.enc_mask": emb.mask.numpy().copy(),
                "init.dec_mask": dcd.mask.numpy().copy()})
    n_enc, n_dec = int(emb.mask.sum()), int(dcd.mask.sum())
    print(f"state_dict NN_embed keys: {[k for k in sd if k.startswith('NN_embed')]}")
    print(f"enc: {n_enc} masked entries, {int((emb.mat != 0).sum())} non-zero; dec: {n_dec} masked, {int((dcd.mat != 0).sum())} non-zero")
    assert int(((emb.mat == 0) & emb.mask).sum()) > 0, "no masked entry with value 0"
    gen = torch.Generator().manual_seed(G.SEED + 92)
    with torch.no_grad():
        for p in (emb.mat, dcd.mat):
            p.add_(0.1 * torch.randn(p.shape, generator=gen))
    nn_sd = copy.deepcopy(m.NN_embed.state_dict())
    out["nn.embeder.mat"], out["nn.decoder.mat"] = G.npf(nn_sd["embeder.mat"]), G.npf(nn_sd["decoder.mat"])

    shp = (3,) + K.STATE
    x = K.eighths(gen, shp, -16, 16)
    E = K.eighths(gen, (3, 3), 1, 8)
    layers = K.eighths(gen, (3, 1 + K.LAYERS), -8, 8)
    sigma = torch.tensor(K.SIGMAS)
    data = K.eighths(gen, shp, -12, 12)
    noise = K.eighths(gen, shp, -16, 16)
    rnd = K.eighths(gen, (3,), -12, 12)
    cot = K.eighths(gen, shp, -12, 12)
    out.update(x=G.npf(x), E=G.npf(E), layers=G.npf(layers), sigma=G.npf(sigma), data=G.npf(data), noise=G.npf(noise),
               rnd_normal=G.npf(rnd), cot=G.npf(cot))
    sg4 = lambda s: s.reshape(-1, 1, 1, 1)  # noqa: E731

    for obj in K.OBJECTIVES:
        for te in K.TIME_EMBEDS:
            mm, _ = build(obj, te, "l2", nn_sd)
            with torch.no_grad():
                y3 = mm.denoise(x, E=E, sigma=sg4(sigma), layers=layers)
                y1 = mm.denoise(x[:1], E=E[:1], sigma=sg4(sigma[:1]), layers=layers[:1])
            assert tuple(y3.shape) == shp
            out[f"den.{obj}.{te}.b3"], out[f"den.{obj}.{te}.b1"] = G.npf(y3), G.npf(y1)
            print(f"denoise {obj} {te}: mean|y| {float(y3.abs().mean()):.4f}  rows B3 vs B1 {K.rel_l2(G.npf(y3[:1]), G.npf(y1)):.2e}")

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
        mg = mat_grads(mm)
        for name, (g, mask) in mg.items():
            zero_valued = mask & (out["init." + ("enc" if name[0] == "e" else "dec") + "_mat"] == 0)
            print(f"{tag}: {name}.grad non-zero on {int((g[mask] != 0).sum())} of {int(mask.sum())} masked entries "
                  f"({int((g[torch.as_tensor(zero_valued)] != 0).sum())} of them where init()'s value is 0)")
        # the same in float64 through the restatement
        usd = {k: v.detach().clone() for k, v in mm.model.state_dict().items()}
        We = (mm.NN_embed.embeder.mat.detach().double()).requires_grad_(True)
        Wd = (mm.NN_embed.decoder.mat.detach().double()).requires_grad_(True)
        sg = (rnd * mm.loss_function.P_std + mm.loss_function.P_mean).exp()
        l64 = K.oracle_loss(c, usd, We * mm.NN_embed.embeder.mask, Wd * mm.NN_embed.decoder.mask, data, E, noise, sg, layers, lt,
                            torch.float64)
        l64.backward()
        print(f"{tag}: loss {float(loss):.6f} (float64 restatement {float(l64):.6f})")
        for name, g64 in (("embeder.mat", We.grad), ("decoder.mat", Wd.grad)):
            g32, mask = mg[name]
            d = K.rel_l2(K.masked(g32.numpy(), mask.numpy()), K.masked(g64.numpy(), mask.numpy()))
            worst64[name] = max(worst64.get(name, 0.0), d)
    out["f64.names"] = np.array(sorted(worst64))
    out["f64.dist"] = np.array([worst64[k] for k in sorted(worst64)])
    print("float32 reference mat gradients vs float64 restatement, worst over the loss cases:",
          {k: f"{v:.2e}" for k, v in sorted(worst64.items())})

    for obj in K.OBJECTIVES:
        mm, _ = build(obj, "log", "l2", nn_sd)
        mm.zero_grad()
        xg = x.clone().requires_grad_(True)
        y = mm.denoise(xg, E=E, sigma=sg4(sigma), layers=layers)
        (y * cot).sum().backward()
        out[f"vjp.{obj}.dx"] = G.npf(xg.grad)
        grads_record(f"vjp.{obj}", mm, out)

    # frozen maps: the shipped TRAINABLE_EMBED False
    mf, _ = build("hybrid_weight", "log", "l2", trainable=False)
    assert torch.equal(mf.NN_embed.embeder.mat, torch.as_tensor(out["init.enc_mat"])) and not list(mf.NN_embed.parameters())
    with torch.no_grad():
        out["frozen.den"] = G.npf(mf.denoise(x, E=E, sigma=sg4(sigma), layers=layers))
    mf.train()
    mf.zero_grad()
    lf = mf.compute_loss(data, E, noise=noise, layers=layers, rnd_normal=rnd)
    lf.backward()
    out["frozen.loss"] = np.array(float(lf), dtype=np.float64)
    grads_record("frozen", mf, out, with_nn=False)
    print(f"frozen: loss {float(lf):.6f}")

    # samplers
    mm, c = build("hybrid_weight", "log", "l2", nn_sd)
    start = K.eighths(gen, shp, -16, 16)
    traj.update(start=G.npf(start), E=G.npf(E), layers=G.npf(layers))
    S = G.ref_sample
    with torch.no_grad():
        xf, xs, x0s = S.DDim(copy.deepcopy(c))(mm, start.clone(), E, layers, K.TRAJ_STEPS, 0, False)
    traj.update({"ddim.x": G.npf(xf), "ddim.xs": np.stack([G.npf(t) for t in xs]), "ddim.x0s": np.stack([G.npf(t) for t in x0s])})
    ngen_seed = 781
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
        for rows in (3, 1):
            try:
                with torch.no_grad():
                    xf, _, _ = getattr(S, cls)(cc)(mm, start[:rows].clone(), E[:rows], layers[:rows], n, 0, False)
                ok = bool(torch.isfinite(xf).all()) and tuple(xf.shape) == (rows,) + K.STATE
                mm.loss_function.update_step(c["NSTEPS"])
                break
            except Exception as e:
                print(f"sampler {tag}: the reference fails on the cell-space state at B = {rows}: {type(e).__name__}: {str(e)[:100]}")
                mm.loss_function.update_step(c["NSTEPS"])
        traj[f"smp.{tag}.ran"], traj[f"smp.{tag}.rows"] = np.array(ok), np.array(rows)
        if ok:
            traj[f"smp.{tag}.x"] = G.npf(xf)
            print(f"sampler {tag}: ran at B = {rows}, mean|x| {float(xf.abs().mean()):.4f}")
        elif xf is not None:
            print(f"sampler {tag}: ran but is not usable: shape {tuple(xf.shape)}, finite {bool(torch.isfinite(xf).all())}")

    # ReverseNormHGCal(embed=False) of a cell-space batch, layer mode
    vox = (torch.randn(shp, generator=gen) * 0.9 + 0.3).numpy().astype(np.float32)
    e = torch.rand((3, 3), generator=gen).numpy().astype(np.float32)
    layerE = torch.randn((3, K.LAYERS + 1), generator=gen).numpy().astype(np.float32)
    rdata, rgen = ref_hg.ReverseNormHGCal(vox.copy(), e.copy(), layerE=layerE.copy(), showerMap=cfg["SHOWERMAP"],
                                          dataset_num=cfg["DATASET_NUM"], embed=False, **K.RN)
    out.update({"rn.vox": vox, "rn.e": e, "rn.layerE": layerE, "rn.data": np.asarray(rdata, dtype=np.float32),
                "rn.gen": np.asarray(rgen, dtype=np.float32)})
    print("reverse norm:", out["rn.data"].shape, float(np.abs(out["rn.data"]).mean()))

    grads = {k: out.pop(k) for k in list(out) if k.startswith(("loss.", "vjp.", "frozen."))}
    for name, d in (("hgcal_model.npz", out), ("hgcal_model_grads.npz", grads), ("hgcal_model_samplers.npz", traj)):
        path = os.path.join(args.out_dir, name)
        np.savez_compressed(path, **d)
        print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


def maps_record(args):
    L, A, R = K.BINS_T
    geom = GG.synthetic_geometry(L, A, K.NCELLS_T, 30, seed=G.SEED + 82)
    assert int(geom.ring_map.max()) >= 23 and geom.max_ncell > 256
    enc, enc_mask, dec, dec_mask = GG.reference_maps(geom, A, R)
    out = {f"t.{k[2:]}": v for k, v in GG.geom_arrays("t", geom).items()}
    out.update({"t.bins": np.array(K.BINS_T), "t.enc_mat": G.npf(enc), "t.enc_mask": enc_mask.numpy(), "t.dec_mat": G.npf(dec),
                "t.dec_mask": dec_mask.numpy()})
    N, E = geom.max_ncell, A * R
    gen = torch.Generator().manual_seed(G.SEED + 83)
    x = K.eighths(gen, (3, 1, L, N), -16, 16)
    z = K.eighths(gen, (3, 1, L, A, R), -16, 16)
    cot_e = K.eighths(gen, (3, 1, L, A, R), -12, 12)
    cot_d = K.eighths(gen, (3, 1, L, N), -12, 12)
    out.update({"t.x": G.npf(x), "t.z": G.npf(z), "t.cot_enc": G.npf(cot_e), "t.cot_dec": G.npf(cot_d)})
    for tag, cls, mat, mask, inp, cot in (("enc", ref_hg.Embeder, enc, enc_mask, x, cot_e), ("dec", ref_hg.Decoder, dec, dec_mask, z, cot_d)):
        mod = cls(A, R, mat + torch.as_tensor(K.hashed_perturbation(tuple(mat.shape))), mask, trainable=True)
        xin = inp.clone().requires_grad_(True)
        y = mod(xin)
        (y * cot).sum().backward()
        assert bool((mod.mat.grad[~mask] == 0).all())
        out[f"t.{tag}"], out[f"t.{tag}.dx"] = G.npf(y), G.npf(xin.grad)
        out[f"t.{tag}.dm"] = K.masked(G.npf(mod.mat.grad), mask.numpy())
        print(f"t {tag}: {int(mask.sum())} masked entries, mean|y| {float(y.abs().mean()):.3f}")
    path = os.path.join(args.out_dir, "hgcal_model_t.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=G.GOLD)
    args = ap.parse_args()
    model_records(args)
    maps_record(args)


if __name__ == "__main__":
    main()
