"""Generate tests/golden/ds1_geom.npz (and ds1_geom_g1_rows.npz) from the reference's own Dataset-1 geometry classes
(calodiffusion/utils/utils.py: ``GeomConverter`` :659-784, ``NNConverter`` :576-656) on SYNTHETIC geometries: GeomConverter takes
``all_r_edges``, ``lay_r_edges``, ``alpha_out`` and ``lay_alphas`` directly and NNConverter takes a ``geomconverter``, so no
binning XML is needed.

TEST INFRASTRUCTURE, like oracle/gen_golden.py: runs only where the reference is mounted, on the CPU, and imports it through that
script's stub-import preamble (by importing the script).  Only data is written.

    python tools/gen_golden_ds1_geom.py [--out-dir DIR]      # default tests/golden

Both geometries have integer-valued radial edges, so ``torch.unique`` and ``==`` on the float edges are exact, and every matrix
entry is a ratio of small integers.

G1, photon-shaped: 5 layers, alpha (1, 10, 10, 1, 1), rin (8, 16, 19, 5, 5) -- 368 voxels as Dataset-1 photons -- on the union of
the layers' edges (29 edges between 0 and 30, dim_r_out 28).  Layers 0 and 4 start above 0 and layers 2 and 4 end below the
outermost edge, so some of their output bins get nothing.
G2, pion-shaped: 7 layers, alpha (1, 4, 4, 1, 4, 1, 4), 13 edges 0 .. 12 (dim_r_out 12); layer 1 has every edge (rin == R): its
map is the identity.
Every column of every weight matrix has its own non-empty set of output bins (the input bins of a layer do not overlap), so
every matrix has full column rank and unconvert(convert(x)) == x up to rounding in every layer of G1 and G2.

Stored per geometry (prefix "g1." / "g2."): the constructor inputs, ``weight_mats`` and their ``pinv``, the weights of an
NNConverter after a dense O(0.1) perturbation (every element carries signal), the weights of ``NNConverter(gc)`` right after
``torch.manual_seed(7)``, inputs x (B, V) >= 0 with exact zeros, g (B, 1, L, A, R) and a cotangent c (B, V), both signed, the
reference's ``enc`` / ``dec`` (perturbed weights) of them at B = 130, its ``convert`` / ``unconvert`` (fixed matrices; the same
launches, so the small batch only) at B = 3, and torch-autograd gradients:
dW and dD at B = 3 and B = 130, dx and dg at B = 3.  enc's cotangent is g, dec's is c.  THE B = 3 INPUTS ARE ROWS [0:3] OF THE
B = 130 ONES.  The reference's results at B = 3 (``enc.b3``, ``dec.b3``) are stored as well: its matrix products block by batch,
so its rows [0:3] at B = 130 can differ from them in the last bit.
Inputs and cotangents are multiples of 1/8 -- exact in float32, and they compress.

Size: the per-row arrays at B = 130 are 130 x (V + L A R) floats per stored result, which for G1 is the bulk of 0.5 MB; G1's
rows therefore live in a file of their own (ds1_geom_g1_rows.npz) and everything else in ds1_geom.npz.
"""
from __future__ import annotations

import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402  (stubs the absent modules and puts the reference on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from calodiffusion.utils import utils as ref_utils  # noqa: E402

B_SMALL, B_LARGE = 3, 130

GEOMETRIES = {
    "g1": dict(alpha_out=10, lay_alphas=[1, 10, 10, 1, 1], lay_r_edges=[
        [2, 4, 6, 9, 12, 16, 20, 25, 30],
        [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 17, 20, 23, 26, 30],
        [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 17, 19, 22, 25, 28],
        [0, 3, 8, 15, 22, 30],
        [1, 5, 11, 18, 24, 29]]),
    "g2": dict(alpha_out=4, lay_alphas=[1, 4, 4, 1, 4, 1, 4], lay_r_edges=[
        [0, 4, 8, 12],
        [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12],
        [0, 2, 4, 6, 8, 10, 12],
        [1, 3, 6, 9, 11],
        [0, 1, 2, 3, 5, 7, 9, 12],
        [0, 6, 12],
        [2, 3, 5, 8, 10, 12]]),
}


def reference_converter(spec):
    lay = [[float(e) for e in edges] for edges in spec["lay_r_edges"]]
    all_edges = torch.unique(torch.FloatTensor([e for edges in lay for e in edges]))
    gc = ref_utils.GeomConverter(all_r_edges=all_edges, lay_r_edges=lay, alpha_out=spec["alpha_out"], lay_alphas=spec["lay_alphas"])
    rin = [len(e) - 1 for e in lay]
    gc.layer_boundaries = np.concatenate([[0], np.cumsum([a * r for a, r in zip(spec["lay_alphas"], rin)])]).astype(np.int64)
    return gc, all_edges


def eighths(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).to(torch.float32) / 8.0


def one_geometry(tag, spec, seed):
    gc, all_edges = reference_converter(spec)
    L, A, R, V = gc.num_layers, int(gc.alpha_out), int(gc.dim_r_out), int(gc.layer_boundaries[-1])
    small, rows = {}, {}
    small[f"{tag}.all_r_edges"] = G.npf(all_edges)
    small[f"{tag}.lay_r_edges"] = np.concatenate([np.asarray(e, dtype=np.float32) for e in spec["lay_r_edges"]])
    small[f"{tag}.lay_n_edges"] = np.array([len(e) for e in spec["lay_r_edges"]], dtype=np.int64)
    small[f"{tag}.lay_alphas"] = np.array(spec["lay_alphas"], dtype=np.int64)
    small[f"{tag}.alpha_out"] = np.array(A, dtype=np.int64)
    small[f"{tag}.layer_boundaries"] = gc.layer_boundaries
    for i, m in enumerate(gc.weight_mats):
        assert int(torch.linalg.matrix_rank(m)) == m.shape[1], "a weight matrix without full column rank"
        small[f"{tag}.weight_mats.{i}"] = G.npf(m)
        small[f"{tag}.pinv.{i}"] = G.npf(torch.linalg.pinv(m))
    empty = [int((m.abs().sum(1) == 0).sum()) for m in gc.weight_mats]
    print(f"{tag}: L {L} A {A} R {R} V {V}; output bins without input per layer {empty}; identity layers "
          f"{[i for i, m in enumerate(gc.weight_mats) if m.shape[0] == m.shape[1]]}")

    # the seeded initialisation: pins the number and order of RNG draws
    torch.manual_seed(7)
    seeded = ref_utils.NNConverter(geomconverter=gc)
    for k, v in seeded.state_dict().items():
        small[f"{tag}.seeded.{k}"] = G.npf(v)

    # the perturbed converter
    gen = torch.Generator().manual_seed(seed)
    nn_conv = ref_utils.NNConverter(geomconverter=gc)
    with torch.no_grad():
        for p in nn_conv.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=gen))
    for k, v in nn_conv.state_dict().items():
        small[f"{tag}.nn.{k}"] = G.npf(v)

    x = eighths(gen, (B_LARGE, V), 0, 15) * (torch.rand((B_LARGE, V), generator=gen) > 0.3)
    g = eighths(gen, (B_LARGE, 1, L, A, R), -12, 12)
    c = eighths(gen, (B_LARGE, V), -12, 12)
    rows.update({f"{tag}.x": G.npf(x), f"{tag}.g": G.npf(g), f"{tag}.c": G.npf(c)})
    with torch.no_grad():
        fixed = {"convert": gc.convert(gc.reshape(x[:B_SMALL].clone())),
                 "unconvert": gc.unreshape(gc.unconvert(g[:B_SMALL, 0].clone()))}
    grads = {}
    for B in (B_SMALL, B_LARGE):
        xb, gb = x[:B].clone().requires_grad_(True), g[:B].clone().requires_grad_(True)
        nn_conv.zero_grad()
        enc, dec = nn_conv.enc(xb), nn_conv.dec(gb)
        (enc * g[:B]).sum().backward()
        (dec * c[:B]).sum().backward()
        grads[B] = dict(enc=enc.detach(), dec=dec.detach(), dx=xb.grad, dg=gb.grad,
                        dW=[lay.weight.grad.clone() for lay in nn_conv.encs], dD=[lay.weight.grad.clone() for lay in nn_conv.decs])
    lo, hi = grads[B_SMALL], grads[B_LARGE]
    rows.update({f"{tag}.enc": G.npf(hi["enc"]), f"{tag}.dec": G.npf(hi["dec"])})
    small.update({f"{tag}.convert.b3": G.npf(fixed["convert"]), f"{tag}.unconvert.b3": G.npf(fixed["unconvert"])})
    small.update({f"{tag}.enc.b3": G.npf(lo["enc"]), f"{tag}.dec.b3": G.npf(lo["dec"]), f"{tag}.dx": G.npf(lo["dx"]),
                  f"{tag}.dg": G.npf(lo["dg"])})
    for B in (B_SMALL, B_LARGE):
        for i in range(L):
            small[f"{tag}.dW.b{B}.{i}"] = G.npf(grads[B]["dW"][i])
            small[f"{tag}.dD.b{B}.{i}"] = G.npf(grads[B]["dD"][i])
    return small, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=G.GOLD)
    args = ap.parse_args()
    s1, r1 = one_geometry("g1", GEOMETRIES["g1"], G.SEED + 81)
    s2, r2 = one_geometry("g2", GEOMETRIES["g2"], G.SEED + 82)
    for name, data in (("ds1_geom.npz", {**s1, **s2, **r2}), ("ds1_geom_g1_rows.npz", r1)):
        path = os.path.join(args.out_dir, name)
        np.savez_compressed(path, **data)
        print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
