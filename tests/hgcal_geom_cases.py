"""Shared by test_hgcal_geom_host.py and test_gpu_hgcal_geom.py: float64 restatements of the HGCal geometry maps
(calodiffusion/utils/HGCal_utils.py: Embeder / Decoder :315-349, generate_sparse_mat :355-407) and the error bound both use."""
import types

import numpy as np

EPS = 1e-6


def geometry(g, tag):
    """The synthetic geometry object of tools/gen_golden_hgcal_geom.py from the fixture's arrays."""
    ncells = g[f"{tag}.ncells"]
    return types.SimpleNamespace(ncells=ncells, ring_map=g[f"{tag}.ring_map"], theta_map=g[f"{tag}.theta_map"], nlayers=len(ncells),
                                 max_ncell=int(ncells.max()))


def apply64(M, x):
    """y[..., l, i] = sum_j M[l, i, j] x[..., l, j] in float64"""
    return np.einsum("lij,...lj->...li", M.astype(np.float64), x.astype(np.float64))


def bound(M, x):
    """Per element 2 * nnz_row * 2^-23 * sum_j |M_ij x_j|: a recursive fp32 sum of nnz terms is within nnz * 2^-24 (products
    included: nnz * 2^-23) of the exact one, relative to the sum of magnitudes; the factor 2 covers the two fp32 results
    compared (the reference's einsum, the kernel), or the test's own rounding of a float64 result to the fp32 stored."""
    nnz = (M != 0).sum(-1)
    return 2.0 * nnz * 2.0 ** -23 * apply64(np.abs(M), np.abs(x))


def worst_ratio(got, want, bnd):
    """max |got - want| / bound; an element whose bound is 0 (an empty row) must be equal."""
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert np.all(err[bnd == 0] == 0), "an element with a zero bound differs"
    return float(np.max(err[bnd > 0] / bnd[bnd > 0])) if np.any(bnd > 0) else 0.0


def sparse_matrix(dec, rand):
    """generate_sparse_mat on recorded uniforms: dec (L, N, E), rand (b, L, N, E) -> (b, L, N, E) float64.  u + m is formed in
    fp32 as the reference does; the fixture's seed keeps every u + m more than 1e-6 from 1 and has no equal maxima."""
    keep = dec > EPS
    r = np.where(keep, rand.astype(np.float32) + dec.astype(np.float32), dec.astype(np.float32)[None])
    sel = r > 1.0
    np.put_along_axis(sel, r.argmax(-2)[..., None, :], True, axis=-2)
    sel &= keep
    return sel / np.maximum(sel.sum(-2, keepdims=True), 1).astype(np.float64)


def sparse64(sm, z):
    """sm (b, L, N, E) with b = B or 1, z (B, C, L, E) -> (B, C, L, N)"""
    sm = np.broadcast_to(sm, (z.shape[0],) + sm.shape[1:])
    return np.einsum("blne,bcle->bcln", sm, z.astype(np.float64))


def sparse_bound(dec, sm, z):
    """The same bound on the sampled matrix: nnz_row counts the kept entries (> 1e-6) of the decoder's row."""
    nnz = (dec > EPS).sum(-1)
    return 2.0 * nnz[None, None] * 2.0 ** -23 * sparse64(sm, np.abs(z))
