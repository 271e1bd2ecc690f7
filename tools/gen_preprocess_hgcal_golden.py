"""Generate tests/golden/preprocess_hgcal.npz from the reference's own HGCal loader arithmetic (calodiffusion/utils/HGCal_utils.py:
``Embeder`` / ``HGCalConverter.enc`` :295-320, 636-640, ``preprocess_hgcal_shower`` :20-86 and the ``gen`` map of
``DataLoaderHGCal`` :125-162) on seeded synthetic cell energies over two SYNTHETIC geometries (``synthetic_geometry`` of
tools/gen_golden_hgcal_geom.py: no geometry pickle is needed).

TEST INFRASTRUCTURE, like oracle/gen_golden.py: runs only where the reference is mounted, and imports it through that script's
stub-import preamble (by importing the script).  Only data is written: geometry arrays, raw inputs and the reference's outputs.

    python tools/gen_preprocess_hgcal_golden.py [--out FILE]      # default tests/golden/preprocess_hgcal.npz

Geometry "g": the small one of tests/golden/hgcal_geom.npz (3 layers, 4 x 5 bins, max_ncell 37, ncells (37, 29, 1)), B = 8; the
raw array is 41 cells wide, wider than max_cells: the loader's ``[:, :, :max_cells]`` slice.  Shower 5 is all zero with e > 0
(a defined result: np.ma.divide masks its layer shares, ``.filled(0)`` follows); shower 1 has an empty layer.
Geometry "h": 28 layers, 12 x 21 bins (E = 252), max_ncell 301, ncells varying per layer, rings 0 .. 20, B = 4; shower 0 has two
empty layers (3 and 20).
Raw cell energies: about two thirds exact zeros, zero beyond each layer's ncells; the deposited fraction x SHOWERSCALE / e lies
in [0.4, 0.9]; gen_info (B, 3) uniform inside the EMIN .. EMAX box of the reference's config_HGCal.json.
Cases (key prefix ``{geometry}.{set}.{l|n}``): "g" sets 111 and 101 with 'layer-logit-norm' (l) and 'logit-norm' (n); "h" sets
111 and 101 with 'layer-logit-norm'.  Set 101 (embed_mean 0.0835, embed_std 3.1083) makes the embedded value of every empty bin
negative: the masked branch of ``logit``.  Stored per case: ``data``, ``layerE`` (layer maps), cast to float32 as the loader
casts them; per (geometry, set) ``emb``, the reference's embedded grid (for "h" only set 111's: set 101's is the same product
through the converter's affine, and the file has to stay small); per geometry ``raw``, ``gen_info`` and ``E``.

Conditioning, as tools/gen_preprocess_golden.py: the GPU test holds every (shower, layer) row to a relative bar, and a normalised
value next to zero carries the reference's own float32 rounding as an arbitrarily large relative error.  The seed of a geometry's
inputs is the first, counting up, for which the reference's results are within 1e-5 of a float64 evaluation (from the float32
quotients the reference forms) on every (shower, layer) row of layerE and of the voxels, in every case of that geometry.  The
criterion involves the reference and exact arithmetic only.  The script also prints, for each "h" case, the reference's own
layer-energy round trip: per-layer sums of ReverseNormHGCal(embed=True) of the forward result against those of the scaled raw
showers -- the figure the GPU round-trip bar is derived from.
"""
from __future__ import annotations

import argparse
import contextlib
import io
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from oracle import gen_golden as G  # noqa: E402  (stubs the absent modules and puts the reference on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gen_golden_hgcal_geom as GG  # noqa: E402  (synthetic_geometry, reference_maps)
from calodiffusion.utils import HGCal_utils as ref_hg  # noqa: E402  (the REFERENCE's module: its path comes first)
import calodiffusion.utils.consts as ref_consts  # noqa: E402

BASE_SEED = G.SEED + 110
SHOWER_SCALE = 200.0  # DataLoaderHGCal's default (:107)
EMAX, EMIN, MAXDEP = [100, 2.01, 1.572], [50, 1.99, 1.57], 1.0  # config_HGCal.json
WELL_CONDITIONED = 1e-5
H_NCELLS = [301 - (7 * l) % 53 if l else 301 for l in range(28)]
GEOMS = {
    "g": dict(layers=3, A=4, R=5, ncells=(37, 29, 1), max_ring=4, seed=G.SEED + 71, B=8, width=41,
              cases=((111, "l"), (111, "n"), (101, "l"), (101, "n"))),
    "h": dict(layers=28, A=12, R=21, ncells=H_NCELLS, max_ring=20, seed=G.SEED + 74, B=4, width=301,
              cases=((111, "l"), (101, "l"))),
}
MAPS = {"l": "layer-logit-norm", "n": "logit-norm"}


def synth_inputs(rng, tag, spec, geom):
    """(raw (B, L, width) float32 cell energies as the file stores them, gen_info (B, 3) float32)."""
    B, L, W, N = spec["B"], spec["layers"], spec["width"], geom.max_ncell
    gen_info = np.stack([rng.uniform(lo, hi, B) for lo, hi in zip(EMIN, EMAX)], axis=1).astype(np.float32)
    z = np.arange(L, dtype=np.float64)[None, :, None] + 0.5
    a, b = rng.uniform(1.5, 3.0, (B, 1, 1)), rng.uniform(0.15, 0.5, (B, 1, 1))
    v = z ** a * np.exp(-b * z) * np.exp(rng.normal(0.0, 1.0, (B, L, W)))
    v[rng.random((B, L, W)) < 0.62] = 0.0
    for l in range(L):
        v[:, l, int(round(geom.ncells[l])):] = 0.0  # the file pads a layer's row with zeros
    v[:, :, N:] = 0.0
    if tag == "h":
        v[0, 3] = 0.0
        v[0, 20] = 0.0
    else:
        v[1, 1] = 0.0
        v[5] = 0.0
    frac = rng.uniform(0.4, 0.9, (B, 1, 1))
    tot = v.sum(axis=(1, 2), keepdims=True)
    v *= frac * gen_info[:, :1].astype(np.float64).reshape(B, 1, 1) / SHOWER_SCALE / np.where(tot > 0, tot, 1.0)
    return v.astype(np.float32), gen_info


def reference_case(embeder, raw, gen_info, n_cells, dnum, smap):
    """DataLoaderHGCal(embed=True) after reading the file (:125-162); the converter's norm as init(norm=True, dnum) sets it."""
    c = ref_consts.dataset_params[dnum]
    shower = raw[:, :, :n_cells].astype(np.float32) * SHOWER_SCALE
    e = gen_info[:, 0]
    with torch.no_grad():
        out = embeder(torch.Tensor(shower))
        emb = ((out - c["embed_mean"]) / c["embed_std"]).detach().cpu().numpy()  # HGCalConverter.enc, :636-640
    with contextlib.redirect_stdout(io.StringIO()):
        data, layerE = ref_hg.preprocess_hgcal_shower(emb, e, None, smap, dataset_num=dnum, orig_shape=False, ecut=0.001,
                                                      max_deposit=MAXDEP)
    gen = (gen_info - np.array(EMIN)) / (np.array(EMAX) - np.array(EMIN))
    f32 = lambda a: None if a is None else np.ascontiguousarray(np.ma.getdata(a)).astype(np.float32)  # noqa: E731
    return emb, f32(data), f32(layerE), gen.astype(np.float32)


def float64_case(emb, e, dnum, smap):
    """The same map in float64 from the float32 quotients emb / (max_deposit e); the float32 mode rounds its constants as numpy does."""
    c = dict(ref_consts.dataset_params[dnum])
    layer = "layer" in smap
    if not layer:
        c = {k: (np.float64(np.float32(v)) if isinstance(v, float) else v) for k, v in c.items()}
    alpha, one_m = (1e-8, 1.0 - 2e-8) if layer else (np.float64(np.float32(1e-8)), np.float64(np.float32(1.0 - 2e-8)))
    q = (emb / (np.float32(MAXDEP) * e.reshape(-1, 1, 1, 1))).astype(np.float64)

    def logit(t):
        with np.errstate(all="ignore"):
            o = alpha + one_m * t
            r = o / (1.0 - o)
            lg = np.log(r)
        return np.where((r > 0) & np.isfinite(lg), lg, 0.0)

    layerE = None
    if layer:
        layers = q.sum(axis=(2, 3))
        total = layers.sum(axis=1, keepdims=True)
        with np.errstate(all="ignore"):
            share = layers / total
        lg = np.where(np.isfinite(share), logit(np.where(np.isfinite(share), share, 0.0)), 0.0)
        layerE = np.concatenate([(total - c["totalE_mean"]) / c["totalE_std"], (lg - c["layers_mean"]) / c["layers_std"]], axis=1)
    return (logit(q) - c["logit_mean"]) / c["logit_std"], layerE


def worst_row(got, want, rows):
    num = np.linalg.norm((got - want).reshape(rows + (-1,)), axis=-1)
    den = np.linalg.norm(want.reshape(rows + (-1,)), axis=-1)
    return float((num / np.maximum(den, 1e-30)).max())


class _RefConverter:
    """NN_embed for the reference's ReverseNormHGCal: HGCalConverter.dec_batches (:659-680) through the reference Decoder."""

    def __init__(self, decoder, mean, std):
        self.decoder, self.mean, self.std = decoder, mean, std

    def dec_batches(self, data, sparse_decoding=False, sparse_per_batch=False):
        with torch.no_grad():
            x = torch.as_tensor(np.asarray(data, dtype=np.float32))
            return self.decoder(x * self.std + self.mean).numpy()


def round_trip(decoder, raw, data, layerE, gen, dnum, smap):
    c = ref_consts.dataset_params[dnum]
    with contextlib.redirect_stdout(io.StringIO()):
        back, _ = ref_hg.ReverseNormHGCal(data.copy(), gen.copy(), emax=EMAX, emin=EMIN, max_deposit=MAXDEP, logE=False,
                                          layerE=layerE.copy(), showerMap=smap, dataset_num=dnum, embed=True,
                                          NN_embed=_RefConverter(decoder, c["embed_mean"], c["embed_std"]))
    want = (raw.astype(np.float32) * np.float32(SHOWER_SCALE)).astype(np.float64).sum(-1)
    got = np.asarray(back, dtype=np.float64).sum(-1)
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def make_geometry(tag, spec):
    L, A, R, B = spec["layers"], spec["A"], spec["R"], spec["B"]
    geom = GG.synthetic_geometry(L, A, spec["ncells"], spec["max_ring"], seed=spec["seed"])
    enc, enc_mask, dec, dec_mask = GG.reference_maps(geom, A, R)
    embeder, decoder = ref_hg.Embeder(A, R, enc, enc_mask), ref_hg.Decoder(A, R, dec, dec_mask)
    N = geom.max_ncell
    for seed in range(BASE_SEED, BASE_SEED + 64):
        raw, gen_info = synth_inputs(np.random.default_rng([seed, L]), tag, spec, geom)
        results, worst = {}, 0.0
        for dnum, m in spec["cases"]:
            emb, data, layerE, gen = reference_case(embeder, raw, gen_info, N, dnum, MAPS[m])
            d64, l64 = float64_case(emb, gen_info[:, 0], dnum, MAPS[m])
            w_vox = worst_row(data.astype(np.float64), d64, (B, L))
            w_lay = worst_row(layerE.astype(np.float64), l64, (B, L + 1)) if layerE is not None else 0.0
            print(f"{tag}.{dnum}.{m} seed {seed}: reference vs float64, worst row: voxels {w_vox:.2e}, layerE {w_lay:.2e}")
            worst = max(worst, w_vox, w_lay)
            results[(dnum, m)] = (emb, data, layerE, gen)
        if worst < WELL_CONDITIONED:
            break
    else:
        raise RuntimeError("no well-conditioned seed")
    zeros = float((raw[:, :, :N] == 0).mean())
    assert zeros >= 0.6 and (raw >= 0).all() and (raw[:, :, N:] == 0).all()
    print(f"{tag}: seed {seed}, {zeros:.3f} zeros, raw {raw.shape}, e {gen_info[:, 0].min():.1f}..{gen_info[:, 0].max():.1f}")
    out = dict(GG.geom_arrays(tag, geom))
    out.update({f"{tag}.bins": np.array([L, A, R]), f"{tag}.raw": raw, f"{tag}.gen_info": gen_info})
    for (dnum, m), (emb, data, layerE, gen) in results.items():
        out[f"{tag}.E"] = gen
        if tag == "g" or dnum == 111:
            out[f"{tag}.{dnum}.emb"] = emb
        out[f"{tag}.{dnum}.{m}.data"] = data
        neg = float((emb < 0).mean())
        if layerE is not None:
            out[f"{tag}.{dnum}.{m}.layerE"] = layerE
        print(f"{tag}.{dnum}.{m}: negative embedded values {neg:.3f}")
        if tag == "h":
            print(f"{tag}.{dnum}.{m}: reference layer-energy round trip rel L2 "
                  f"{round_trip(decoder, raw[:, :, :N], data, layerE, gen, dnum, MAPS[m]):.3e}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(G.GOLD, "preprocess_hgcal.npz"))
    args = ap.parse_args()
    out = {}
    for tag, spec in GEOMS.items():
        out.update(make_geometry(tag, spec))
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}  ({os.path.getsize(args.out) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
