"""Shared by the Dataset-1 geometry tests: the fixture (tools/gen_golden_ds1_geom.py), converters built from it, float64
restatements of the four maps and of their weight gradients, and the derived bound.

Bound: device and reference both form an fp32 sum of the same n terms, in possibly different orders, so per
element |got - ref| <= 2 n 2^-23 sum |terms|.  n counts what is summed for that element: the dot product's terms, times A where
an alpha-1 layer is summed over the angular bins, plus one where the element is divided by A."""
import numpy as np
import torch

from conftest import gold

U = 2.0 ** -23
TAGS = ("g1", "g2")
_cache = {}


def fixture(tag):
    """dict of the geometry's arrays (float64 where they enter a restatement is up to the caller)."""
    if tag not in _cache:
        g = gold("ds1_geom")
        data = {k[len(tag) + 1:]: g[k] for k in g.files if k.startswith(tag + ".")}
        if tag == "g1":
            rows = gold("ds1_geom_g1_rows")
            data.update({k[len(tag) + 1:]: rows[k] for k in rows.files})
        n = data["lay_n_edges"]
        off = np.concatenate([[0], np.cumsum(n)])
        data["edges"] = [data["lay_r_edges"][off[i]:off[i + 1]] for i in range(len(n))]
        data["L"], data["A"], data["R"] = len(n), int(data["alpha_out"]), len(data["all_r_edges"]) - 1
        data["V"] = int(data["layer_boundaries"][-1])
        _cache[tag] = data
    return _cache[tag]


def geom_converter(tag):
    from calodiffusion_amd import geom1
    f = fixture(tag)
    return geom1.GeomConverter(all_r_edges=torch.tensor(f["all_r_edges"]), lay_r_edges=[e.tolist() for e in f["edges"]],
                               alpha_out=f["A"], lay_alphas=f["lay_alphas"].tolist(), layer_boundaries=f["layer_boundaries"])


def nn_converter(tag, prefix="nn"):
    """An NNConverter holding the fixture's `prefix` weights (host parameters)."""
    from calodiffusion_amd import geom1
    f = fixture(tag)
    conv = geom1.NNConverter(geomconverter=geom_converter(tag))
    conv.load_state_dict({k[len(prefix) + 1:]: torch.tensor(v) for k, v in f.items() if k.startswith(prefix + ".")}, strict=True)
    return conv


def mats(f, prefix):
    """Per-layer matrices as float64: "weight_mats", "pinv", or the weights "nn.encs" / "nn.decs"."""
    sfx = ".weight" if prefix.startswith("nn.") else ""
    return [np.asarray(f[f"{prefix}.{i}{sfx}"], dtype=np.float64) for i in range(f["L"])]


def layers(f):
    b = f["layer_boundaries"]
    return [(i, int(b[i]), int(b[i + 1]), int(f["lay_alphas"][i])) for i in range(f["L"])]


def expand64(f, m, flat, divide, absolute=False):
    """flat (B, V) -> (value (B, 1, L, A, R), n per layer, broadcastable) with m[i] (R, rin_i): enc (divide) and, with the
    transposed decoder matrices, dec_vjp's dg (no division).  absolute: the sum of the |terms| instead."""
    fn = np.abs if absolute else (lambda v: v)
    flat = fn(np.asarray(flat, dtype=np.float64))
    B, A = flat.shape[0], f["A"]
    out, n = np.zeros((B, 1, f["L"], A, f["R"])), np.zeros(f["L"])
    for i, lo, hi, alpha in layers(f):
        o = np.einsum("rj,baj->bar", fn(m[i]), flat[:, lo:hi].reshape(B, alpha, -1))
        n[i] = m[i].shape[1]
        if alpha != A:
            o = np.repeat(o, A, axis=1)
            if divide:
                o, n[i] = o / A, n[i] + 1
        out[:, 0, i] = o
    return out, n.reshape(1, 1, -1, 1, 1)


def collapse64(f, m, grid, divide, absolute=False):
    """grid (B, 1, L, A, R) -> (value (B, V), n (V,)) with m[i] (rin_i, R): dec (no division) and, with the transposed encoder
    matrices, enc_vjp's dx (divide)."""
    fn = np.abs if absolute else (lambda v: v)
    grid = fn(np.asarray(grid, dtype=np.float64)).reshape(-1, f["L"], f["A"], f["R"])
    B, A = grid.shape[0], f["A"]
    out, n = np.zeros((B, f["V"])), np.zeros(f["V"])
    for i, lo, hi, alpha in layers(f):
        o = np.einsum("jr,bar->baj", fn(m[i]), grid[:, i])
        n[lo:hi] = f["R"]
        if alpha != A:
            o = o.sum(1, keepdims=True)
            n[lo:hi] *= A
            if divide:
                o, n[lo:hi] = o / A, n[lo:hi] + 1
        out[:, lo:hi] = o.reshape(B, -1)
    return out, n


def weight_grad64(f, flat, grid, enc, absolute=False):
    """Per layer (value, n): enc: dW_i (R, rin_i) from x = flat and gy = grid; otherwise dD_i (rin_i, R) from gx = flat, g = grid."""
    fn = np.abs if absolute else (lambda v: v)
    flat = fn(np.asarray(flat, dtype=np.float64))
    grid = fn(np.asarray(grid, dtype=np.float64)).reshape(-1, f["L"], f["A"], f["R"])
    B, A = flat.shape[0], f["A"]
    out = []
    for i, lo, hi, alpha in layers(f):
        fl, n = flat[:, lo:hi].reshape(B, alpha, -1), B * A
        if alpha == A:
            d = np.einsum("bar,baj->rj", grid[:, i], fl)
        else:
            d = np.einsum("bar,bj->rj", grid[:, i], fl[:, 0])
            if enc:
                d, n = d / A, n + 1
        out.append((d if enc else d.T, n))
    return out


def check(name, got, ref, terms, n):
    """Per element |got - ref| <= 2 n 2^-23 sum|terms|; prints and returns the worst ratio."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape == terms.shape, (name, got.shape, ref.shape, terms.shape)
    assert np.isfinite(got).all(), name
    err, bound = np.abs(got - ref), 2.0 * n * U * terms
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    print(f"{name}: worst |err| / bound = {ratio:.3f}  (max |err| {err.max():.3e})")
    assert ratio <= 1.0, (name, ratio)
    return ratio
