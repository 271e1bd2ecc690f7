"""Generate tests/golden/ds1_layer.npz and hgcal_layer_inmodel.npz from the reference's own ``LayerDiffusion``
(calodiffusion/models/layerdiffusion.py) over an in-model geometry embedding: the two-stage model whose U-Net state is the flat
Dataset-0/1 shower (SHOWER_EMBED 'orig-NN') or HGCal's cell-space shower (HGCalConverter inside forward).  The three records, their
configs and geometries are those of tests/layer_inmodel_cases.py: "ph." (Dataset-1 photons, the form the reference's CI runs:
SHAPE_PAD = SHAPE_FINAL) and "pi." (the narrow pion config) in ds1_layer.npz, HGCal geometry "m" in hgcal_layer_inmodel.npz.  The
embedding matrices are the perturbed ones the existing fixtures store (ds1_model.npz, narrow_pion.npz, hgcal_model.npz).

TEST INFRASTRUCTURE, like oracle/gen_golden.py: runs only where the reference is mounted, on the CPU, and imports it through that
script's stub-import preamble (by importing the script).  Only data is written.

    python tools/gen_golden_layer_inmodel.py [--out-dir DIR]      # default tests/golden

Per record (weights from ``torch.manual_seed(SEED)``; inputs are multiples of 1/8):
  ck_keys / ck_vals, sd_keys      checksums and key order of the full state_dict (the nested 'layer_model' entry left out)
  E, start, layer_start           conditioning values, the injected start tensors of the U-Net and of the layer stage
  <te>.layers, <te>.x             ``sample(E, None, 4, 0, return_layers=True)`` with LAYER_STEPS 4, DDim on both stages, for
                                  TIME_EMBED <te> in ('log', 'sigma'): the generated layer energies and the final U-Net state
  <te>.phys, <te>.phys_e          the reference's ReverseNorm of that state with layerE = the generated layers (Dataset 0/1:
                                  orig_shape=True; HGCal: embed=False) and the incident energies it returns
  loss.<objective>.<loss type>.*  ``compute_loss`` in the layer state on (lay, lnoise, lrnd) with the noise injected: the loss,
                                  checksums of every layer-model gradient and the gradients layer_inmodel_cases.picked() names
                                  ("pi.": the first case only); the U-Net and the embedding get no gradient (asserted here)
"""
from __future__ import annotations

import argparse
import contextlib
import copy
import io
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from oracle import gen_golden as G  # noqa: E402  (stubs the absent modules and puts the reference on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from calodiffusion.models.layerdiffusion import LayerDiffusion as RefLayerDiffusion  # noqa: E402
from calodiffusion.utils import HGCal_utils as ref_hg  # noqa: E402
from calodiffusion.utils import utils as ref_utils  # noqa: E402
import gen_golden_hgcal_geom as GG  # noqa: E402
import hgcal_model_cases as KH  # noqa: E402
import layer_inmodel_cases as L  # noqa: E402

GEOM_M = GG.synthetic_geometry(KH.LAYERS, KH.GRID[1], KH.NCELLS_M, KH.GRID[2] - 1, seed=G.SEED + 81)
ref_hg.load_geom = lambda geom_filename: GEOM_M  # the pickle is not available: the synthetic geometry stands in for it


def gold(name):
    return np.load(os.path.join(G.GOLD, name + ".npz"))


def build(rec, objective="hybrid_weight", time_embed="log", loss_type="l2"):
    cfg = L.config(rec, objective, time_embed, LOSS_TYPE=loss_type)
    torch.manual_seed(G.SEED)
    m = RefLayerDiffusion(copy.deepcopy(cfg), n_steps=cfg["NSTEPS"], loss_type=loss_type)
    m.eval()
    assert m.do_embed and tuple(m._data_shape) == L.STATE[rec]
    sd = {k: v.detach().clone() for k, v in m.state_dict().items() if isinstance(v, torch.Tensor)}
    if rec == "hg":
        g = gold("hgcal_model")
        m.NN_embed.init()  # (a trainable converter is left un-initialised by the model, calodiffusion.py:116-117)
        assert np.array_equal(m.NN_embed.embeder.mask.numpy(), g["init.enc_mask"])
        with torch.no_grad():
            m.NN_embed.embeder.mat.copy_(torch.as_tensor(g["nn.embeder.mat"]))
            m.NN_embed.decoder.mat.copy_(torch.as_tensor(g["nn.decoder.mat"]))
    else:
        g = gold("ds1_model" if rec == "ph" else "narrow_pion")
        m.NN_embed.load_state_dict({k[3:]: torch.as_tensor(g[k]) for k in g.files if k.startswith("nn.")})
    return m, cfg, sd


def reverse(rec, cfg, x, E, layers):
    with contextlib.redirect_stdout(io.StringIO()):
        if rec == "hg":
            out, en = ref_hg.ReverseNormHGCal(x.copy(), E.copy(), layerE=layers.copy(), showerMap=cfg["SHOWERMAP"],
                                              dataset_num=cfg["DATASET_NUM"], embed=False, **KH.RN)
        else:
            out, en = ref_utils.ReverseNorm(x.copy(), E.copy(), hgcal=False, shape=cfg["SHAPE_FINAL"], config=cfg, emax=cfg["EMAX"],
                                            emin=cfg["EMIN"], layerE=layers.copy(), logE=cfg["logE"], binning_file=cfg["BIN_FILE"],
                                            max_deposit=cfg["MAXDEP"], showerMap=cfg["SHOWERMAP"], dataset_num=cfg["DATASET_NUM"],
                                            orig_shape=True, ecut=float(cfg["ECUT"]))
    return np.ascontiguousarray(np.asarray(out), dtype=np.float32), np.asarray(en, dtype=np.float32)


def record(rec, seed):
    out = {}
    m, cfg, sd = build(rec)
    keys, cks = G.checksums(sd)
    out["ck_keys"], out["ck_vals"], out["sd_keys"] = keys, cks, np.array(list(sd.keys()))
    assert isinstance(m.state_dict()["layer_model"], dict)
    dim, cols = L.LAYERS[rec] + 1, L.ENERGY_COLS[rec]
    assert m.layer_model.in_lay.weight.shape[1] == dim and m.layer_model.cond_mlp[0].weight.shape[1] == (3 if rec == "hg" else 1)
    gen = torch.Generator().manual_seed(seed)
    E = L.eighths(gen, (L.B, cols), 1, 7)
    start = L.eighths(gen, (L.B,) + L.STATE[rec], -16, 16)
    lstart = L.eighths(gen, (L.B, dim), -16, 16)
    lay = L.eighths(gen, (L.B, dim), -8, 8)
    lnoise = L.eighths(gen, (L.B, dim), -16, 16)
    lrnd = L.eighths(gen, (L.B,), -12, 12)
    out.update(E=G.npf(E), start=G.npf(start), layer_start=G.npf(lstart), lay=G.npf(lay), lnoise=G.npf(lnoise), lrnd=G.npf(lrnd))

    for te in L.TIME_EMBEDS:
        mm, c, _ = build(rec, time_embed=te)
        assert type(mm.layer_sampler).__name__ == "DDim" and type(mm.sampler_algorithm).__name__ == "DDim"
        draws = [start.clone(), lstart.clone()]  # sample() draws the U-Net start first, then the layer start
        mm.noise_generation = lambda shape: draws.pop(0)
        with torch.no_grad():
            res = mm.sample(E, layers=None, num_steps=L.UNET_STEPS, sample_offset=0, return_layers=True)
        assert not draws and not mm.layer_loss and mm.model is mm.base_model
        x, layers = np.asarray(res["x"], dtype=np.float32), G.npf(res["layers"])
        assert x.shape == (L.B,) + L.STATE[rec] and layers.shape == (L.B, dim) and np.isfinite(x).all()
        phys, en = reverse(rec, c, x, G.npf(E), layers)
        out[f"{te}.layers"], out[f"{te}.x"], out[f"{te}.phys"], out[f"{te}.phys_e"] = layers, x, phys.reshape(L.B, -1), en
        print(f"[{rec} {te}] layers mean|.| {np.abs(layers).mean():.4f}  x mean|.| {np.abs(x).mean():.4f}  showers sum "
              f"{phys.sum(axis=tuple(range(1, phys.ndim)))}  zeros {float((phys == 0).mean()):.3f}")

    for obj, lt in (L.LOSS_CASES if rec != "pi" else L.LOSS_CASES[:1]):
        mm, c, _ = build(rec, obj, "log", lt)
        mm.train()
        mm.zero_grad()
        mm.set_layer_state(is_layer=True)
        mm.noise_generation = lambda shape: lnoise.clone()
        loss = mm.compute_loss(None, E, None, lay, rnd_normal=lrnd)
        loss.backward()
        mm.set_layer_state(is_layer=False)
        assert all(p.grad is None for p in mm.base_model.parameters()) and all(p.grad is None for p in mm.NN_embed.parameters())
        tag = f"loss.{obj}.{lt}"
        grads = {k: p.grad for k, p in mm.layer_model.named_parameters()}
        keys, cks = G.checksums(grads)
        out[f"{tag}.loss"], out[f"{tag}.ck_keys"], out[f"{tag}.ck_vals"] = np.array(float(loss.detach()), dtype=np.float64), keys, cks
        for k, g in grads.items():
            if L.picked(k):
                out[f"{tag}.grad.{k}"] = G.npf(g)
        print(f"[{rec}] {tag}: loss {float(loss.detach()):.6f}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=G.GOLD)
    args = ap.parse_args()
    ds1 = {}
    for rec, seed in (("ph", G.SEED + 94), ("pi", G.SEED + 95)):
        ds1.update({L.PREFIX[rec] + k: v for k, v in record(rec, seed).items()})
    for name, d in (("ds1_layer.npz", ds1), ("hgcal_layer_inmodel.npz", record("hg", G.SEED + 96))):
        path = os.path.join(args.out_dir, name)
        np.savez_compressed(path, **d)
        print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
