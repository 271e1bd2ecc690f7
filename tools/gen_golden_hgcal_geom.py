"""Generate tests/golden/hgcal_geom.npz from the reference's own HGCal geometry maps (calodiffusion/utils/HGCal_utils.py:
``init_map``, ``Embeder``, ``Decoder``, ``generate_sparse_mat``, ``ReverseNormHGCal``) on a SYNTHETIC geometry: the map classes
take their matrices as constructor arguments and ``init_map`` any object with four attributes, so no geometry pickle is needed.

TEST INFRASTRUCTURE, like oracle/gen_golden.py: runs only where the reference is mounted, and imports it through that script's
stub-import preamble (by importing the script).  Only data is written: the geometry arrays, inputs and the reference's outputs.

    python tools/gen_golden_hgcal_geom.py [--out FILE]      # default tests/golden/hgcal_geom.npz

Geometry "g": 3 layers, 4 angular x 5 radial bins (E = 20), max_ncell 37, ncells (37, 29, 1) -- the last layer holds the centre
cell only; seeded angles, several of them within 1e-2 of an angular bin edge (the 0.5 / 0.5 split, on both sides of the edge and
at the periodic one); rings 0 .. 4.
Geometry "w" (maps only): 2 layers, 4 x 26 bins, max_ncell 41, rings up to 30.  init_map merges the rings from 23 outwards three
to a radial bin, and a ring beyond the radial bins is an index error in the reference, so this re-binning cannot be crossed with
5 radial bins: the second geometry is there for it.

Stored for "g": init_map's output per layer, the pinv-derived decoder and its mask, Embeder(x) and Decoder(z) for 3 showers with
and without the converter's norm (set 111: embed_mean 0, embed_std 1), Decoder(z, sparse_decoding=True) for per_batch False and
True with the uniform tensor the reference drew, and ReverseNormHGCal(embed=True) through the reference Decoder in layer mode.

The sparse decode selects by u + m > 1 and by an argmax.  So that the selection does not hang on a rounding, the seed is the
first, counting up, for which over all kept entries min |u + m - 1| > 1e-6 and no column has two equal maxima; every layer with
more than one cell has a column with two or more kept entries (a layer of the centre cell alone has one entry per column).
"""
from __future__ import annotations

import argparse
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402  (stubs the absent modules and puts the reference on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from calodiffusion.utils import HGCal_utils as ref_hg  # noqa: E402
import calodiffusion.utils.consts as ref_consts  # noqa: E402

EPS = 1e-6


def synthetic_geometry(layers, A, ncells, max_ring, seed):
    """ncells, ring_map, theta_map, nlayers, max_ncell: what init_map reads."""
    rng = np.random.default_rng(seed)
    n_max = int(max(ncells))
    theta = rng.uniform(0.0, 2.0 * np.pi, size=(layers, n_max))
    edges = np.pi / A + 2.0 * np.pi / A * np.arange(A)
    for l in range(layers):  # cells at an angular bin edge: just above, just below (inside bucketize's 1e-4), and further off
        for k, (cell, off) in enumerate(((3, 3e-3), (5, -5e-5), (8, 9.9e-3), (11, 1.2e-2), (14, 4e-3), (17, -2e-2))):
            if cell < n_max:
                theta[l, cell] = edges[(k + l) % A] + off
        if n_max > 20:
            theta[l, 20] = edges[A - 1] + 2e-3  # the periodic edge
    ring = rng.integers(0, max_ring + 1, size=(layers, n_max)).astype(np.float64)
    ring[:, 1] = max_ring
    ring[:, 2] = 0
    ring[:, 0] = 0
    return types.SimpleNamespace(ncells=np.asarray(ncells, dtype=np.float64), ring_map=ring, theta_map=theta, nlayers=layers,
                                 max_ncell=n_max)


def reference_maps(geom, A, R):
    L, E, N = geom.nlayers, A * R, geom.max_ncell
    enc, enc_mask = torch.zeros((L, E, N)), torch.zeros((L, E, N), dtype=torch.bool)
    dec, dec_mask = torch.zeros((L, N, E)), torch.zeros((L, N, E), dtype=torch.bool)
    for i in range(L):  # HGCalConverter.init (HGCal_utils.py:595-634) needs the pickle for its constructor; its loop body:
        conv_map, mask = ref_hg.init_map(A, R, geom, i)
        inv = torch.linalg.pinv(conv_map)
        enc[i], enc_mask[i], dec[i], dec_mask[i] = conv_map, mask > EPS, inv, torch.abs(inv) > EPS
    return enc, enc_mask, dec, dec_mask


def geom_arrays(tag, geom):
    return {f"{tag}.ncells": geom.ncells, f"{tag}.ring_map": geom.ring_map, f"{tag}.theta_map": geom.theta_map}


class _RefDecoder:
    """NN_embed for the reference's ReverseNormHGCal: dec_batches through the reference Decoder."""

    def __init__(self, dec):
        self.dec = dec

    def dec_batches(self, data, sparse_decoding=False, sparse_per_batch=False):
        with torch.no_grad():
            return self.dec(torch.as_tensor(np.asarray(data, dtype=np.float32)), sparse_decoding=sparse_decoding,
                            sparse_per_batch=sparse_per_batch).numpy()


def sparse_case(decoder, dec, z, per_batch, seed):
    """(uniforms, output) of the reference's sparse decode for the first admissible seed >= `seed`."""
    B = z.shape[0]
    shape = (1 if per_batch else B,) + tuple(dec.shape)
    keep = (dec > EPS).expand(shape)
    while True:
        torch.manual_seed(seed)
        rand = torch.rand(shape)
        torch.manual_seed(seed)
        with torch.no_grad():
            out = decoder(z, sparse_decoding=True, sparse_per_batch=per_batch)
        r = rand * keep + dec
        margin = float((r[keep] - 1.0).abs().min())
        top2 = torch.topk(torch.where(keep, r, torch.full_like(r, -1.0)), 2, dim=-2).values
        tie = bool(((top2[..., 0, :] == top2[..., 1, :]) & (top2[..., 0, :] > 0)).any())
        if margin > EPS and not tie:
            break
        seed += 1
    # the stored uniforms ARE the reference's draw: generate_sparse_mat restated on them gives the stored output
    sel = r.scatter(-2, torch.argmax(r, dim=-2, keepdim=True), 1.0 + EPS) > 1.0
    sm = sel.to(torch.float32)
    sm = sm / sm.sum(dim=-2, keepdim=True) * keep
    again = torch.einsum("b l n e, b c l e -> b c l n", sm.repeat((B // sm.shape[0], 1, 1, 1)), z.reshape(z.shape[:3] + (-1,)))
    assert torch.equal(again, out), "the recorded uniforms do not reproduce the reference's sparse decode"
    print(f"sparse per_batch={per_batch}: seed {seed}, min |u + m - 1| = {margin:.2e}, selected {int((sm > 0).sum())} of {int(keep.sum())}")
    return rand, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(G.GOLD, "hgcal_geom.npz"))
    args = ap.parse_args()
    out = {}

    # ---- geometry "w": the ring re-binning at 23
    Aw, Rw = 4, 26
    gw = synthetic_geometry(2, Aw, (41, 33), 30, seed=G.SEED + 72)
    enc, enc_mask, dec, dec_mask = reference_maps(gw, Aw, Rw)
    assert int(gw.ring_map.max()) >= 23 and int(gw.ring_map.min()) < 23
    out.update(geom_arrays("w", gw))
    out.update({"w.bins": np.array([2, Aw, Rw]), "w.enc_mat": G.npf(enc), "w.enc_mask": enc_mask.numpy(), "w.dec_mat": G.npf(dec),
                "w.dec_mask": dec_mask.numpy()})

    # ---- geometry "g"
    L, A, R, B = 3, 4, 5, 3
    geom = synthetic_geometry(L, A, (37, 29, 1), R - 1, seed=G.SEED + 71)
    enc, enc_mask, dec, dec_mask = reference_maps(geom, A, R)
    N, E = geom.max_ncell, A * R
    split = [int(((enc[i] == 0.5).sum(0) == 2).sum()) for i in range(L)]
    print("cells split 0.5 / 0.5 per layer:", split, " enc nnz", int((enc != 0).sum()), " dec kept", int(dec_mask.sum()))
    assert split[0] >= 3 and split[1] >= 3
    for i in range(L):
        if geom.ncells[i] > 1:
            assert int((dec[i] > EPS).sum(0).max()) >= 2, "a layer without a column of two kept entries"
    out.update(geom_arrays("g", geom))
    out.update({"g.bins": np.array([L, A, R]), "g.enc_mat": G.npf(enc), "g.enc_mask": enc_mask.numpy(), "g.dec_mat": G.npf(dec),
                "g.dec_mask": dec_mask.numpy()})

    embeder, decoder = ref_hg.Embeder(A, R, enc, enc_mask), ref_hg.Decoder(A, R, dec, dec_mask)
    gen = torch.Generator().manual_seed(G.SEED + 73)
    x = torch.rand((B, 1, L, N), generator=gen) * (torch.rand((B, 1, L, N), generator=gen) > 0.3)  # cell energies, some empty
    z = torch.rand((B, 1, L, A, R), generator=gen) * 2.0 - 0.25                                    # grid values, some negative
    c = ref_consts.dataset_params[111]
    mean, std = c["embed_mean"], c["embed_std"]
    with torch.no_grad():
        out.update({"x": G.npf(x), "z": G.npf(z), "enc": G.npf(embeder(x)), "dec": G.npf(decoder(z)),
                    "norm": np.array([mean, std], dtype=np.float64),
                    "enc_norm": G.npf((embeder(x) - mean) / std),      # HGCalConverter.enc, :636-640
                    "dec_norm": G.npf(decoder(z * std + mean))})       # HGCalConverter.dec, :659-663
    for tag, per_batch, seed in (("sparse", False, 500), ("sparse_pb", True, 600)):
        rand, y = sparse_case(decoder, dec, z, per_batch, seed)
        out[f"{tag}.rand"], out[f"{tag}.out"] = G.npf(rand), G.npf(y)

    # ---- ReverseNormHGCal around the reference Decoder, layer mode, set 111
    vox = (torch.randn((B, 1, L, A, R), generator=gen) * 0.9 + 0.3).numpy().astype(np.float32)
    e = torch.rand((B, 3), generator=gen).numpy().astype(np.float32)
    layerE = torch.randn((B, L + 1), generator=gen).numpy().astype(np.float32)
    data, gen_out = ref_hg.ReverseNormHGCal(vox.copy(), e.copy(), emax=1000., emin=1., max_deposit=2, logE=True, layerE=layerE.copy(),
                                            showerMap="layer-logit-norm", dataset_num=111, embed=True, NN_embed=_RefDecoder(decoder))
    out.update({"rn.vox": vox, "rn.e": e, "rn.layerE": layerE, "rn.data": np.asarray(data, dtype=np.float32),
                "rn.gen": np.asarray(gen_out, dtype=np.float32)})
    print("reverse norm:", out["rn.data"].shape, float(np.abs(out["rn.data"]).mean()))

    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}  ({os.path.getsize(args.out) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
