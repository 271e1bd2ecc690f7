"""HGCal geometry maps on the device: ``Embeder``, ``Decoder`` and ``HGCalConverter`` of the reference
(calodiffusion/utils/HGCal_utils.py:295-407, 412-486, 517-680) over the packed maps of ``cd_geom_*`` (include/calodiff.h).

The maps between HGCal's irregular cells (layers, cells) and the regular (layers, alpha, r) grid are linear with one or two
non-zeros per cell, so they are packed once (per-layer CSR, plus a column view for the sampled decode) and applied by
``cd_geom_apply`` / ``cd_geom_decode_sparse``; nothing is copied to the host.  Building a map from a geometry (``from_geometry``:
``init_map`` and ``torch.linalg.pinv``, :412-486, 595-634) is construction-time host work.

These are inference maps: no gradient flows through them, and TRAINABLE_EMBED training is not provided (``trainable=True`` only
folds ``mat * mask``, as the reference's forward does, when the map is packed).
"""
from __future__ import annotations

import ctypes as C
import pickle

import numpy as np
import torch

from . import engine
from .postprocess import HGCAL_EMBED_PARAMS

EPS = 1e-6  # the threshold of HGCalConverter.init's masks and of generate_sparse_mat (HGCal_utils.py:371, 607)


class _PackedMap:
    """Owner of one CdGeomMap handle."""

    def __init__(self, dense: torch.Tensor, want_columns: bool):
        dense = dense.detach().to(device="cuda", dtype=torch.float32).contiguous()
        self.layers, self.rows, self.cols = (int(s) for s in dense.shape)
        self._lib = engine.load_library()
        handle = C.c_void_p()
        engine._check(self._lib.cd_geom_create(dense.data_ptr(), self.layers, self.rows, self.cols, int(want_columns),
                                               C.byref(handle), engine._stream()))
        self.handle = handle

    def __del__(self):
        if getattr(self, "handle", None):
            self._lib.cd_geom_destroy(self.handle)
            self.handle = None

    def apply(self, x: torch.Tensor, scale: float, shift: float, affine_first: bool) -> torch.Tensor:
        """x (..., L, cols) -> (..., L, rows)"""
        x = engine._dev32(x, "x")
        if x.dim() < 2 or tuple(x.shape[-2:]) != (self.layers, self.cols):
            raise ValueError(f"geometry map: expected (..., {self.layers}, {self.cols}), got {tuple(x.shape)}")
        y = torch.empty(x.shape[:-1] + (self.rows,), dtype=torch.float32, device=x.device)
        if y.numel():
            engine._check(self._lib.cd_geom_apply(self.handle, x.data_ptr(), y.data_ptr(), x.numel() // (self.layers * self.cols),
                                                  float(scale), float(shift), int(affine_first), engine._stream()))
        return y

    def decode_sparse(self, x: torch.Tensor, per_batch: bool, rand, seed: int, offset: int) -> torch.Tensor:
        """x (B, C, L, cols) -> (B, C, L, rows)"""
        x = engine._dev32(x, "x")
        if x.dim() != 4 or tuple(x.shape[-2:]) != (self.layers, self.cols):
            raise ValueError(f"sparse decoding: expected (batch, channels, {self.layers}, {self.cols}), got {tuple(x.shape)}")
        B, ch = int(x.shape[0]), int(x.shape[1])
        if rand is not None:
            rand = engine._dev32(rand, "rand")
            if tuple(rand.shape) != (1 if per_batch else B, self.layers, self.rows, self.cols):
                raise ValueError(f"sparse decoding: rand must be ({1 if per_batch else B}, {self.layers}, {self.rows}, "
                                 f"{self.cols}), got {tuple(rand.shape)}")
        y = torch.empty((B, ch, self.layers, self.rows), dtype=torch.float32, device=x.device)
        if not y.numel():
            return y
        need = C.c_size_t()
        engine._check(self._lib.cd_geom_sparse_workspace_bytes(self.handle, B, C.byref(need)))
        ws = torch.empty(need.value, dtype=torch.uint8, device=x.device)
        engine._check(self._lib.cd_geom_decode_sparse(self.handle, x.data_ptr(), y.data_ptr(), B, ch, int(per_batch), engine._ptr(rand),
                                                      int(seed), int(offset), ws.data_ptr(), engine._stream()))
        return y


class _Map(torch.nn.Module):
    """Shared part of Embeder and Decoder: the reference's attributes, and the handle packed on first use (and again after
    ``set``)."""
    _want_columns = False

    def __init__(self, dim1, dim2, mat, mask, trainable=False):
        super().__init__()
        self.dim1, self.dim2 = int(dim1), int(dim2)
        self.trainable = bool(trainable)
        self.mat, self.mask = mat, mask
        self._packed = None

    def set(self, mat, mask):
        self.mat, self.mask = mat, mask
        self._packed = None

    def packed(self) -> _PackedMap:
        if self._packed is None:
            mat = self.mat * self.mask if self.trainable else self.mat
            self._packed = _PackedMap(mat, self._want_columns)
        return self._packed


class Embeder(_Map):
    """``Embeder`` (HGCal_utils.py:295-324): cells (..., L, N) -> grid (..., L, dim1, dim2) with ``mat`` (L, dim1 * dim2, N).
    Inference only: the result carries no autograd graph."""

    def forward(self, x):
        return self._embed(x, 1.0, 0.0)

    def _embed(self, x, std, mean):
        out = self.packed().apply(x, std, mean, affine_first=False)
        return out.reshape(out.shape[:-1] + (self.dim1, self.dim2))


class Decoder(_Map):
    """``Decoder`` (HGCal_utils.py:327-353): grid (..., L, dim1, dim2) -> cells (..., L, N) with ``mat`` (L, N, dim1 * dim2).
    Inference only: the result carries no autograd graph.

    ``sparse_decoding`` (``generate_sparse_mat``, :355-407) takes x (B, C, L, dim1, dim2).  Its uniforms come from the device
    Philox stream (``seed``, ``offset``): by default the decoder's own (``noise_seed``, and a running ``noise_offset`` that
    advances by the (B or 1, L, N, E) tensor a call draws); a batch shard passes ``offset`` = that of the global call + first
    shower * L * N * E.  ``rand`` (B or 1, L, N, E) replaces the draw (parity with a recorded ``torch.rand``)."""
    _want_columns = True

    def __init__(self, dim1, dim2, mat, mask, trainable=False):
        super().__init__(dim1, dim2, mat, mask, trainable)
        self.noise_seed, self.noise_offset = 1234, 0

    def forward(self, x, sparse_decoding=False, sparse_per_batch=False, *, rand=None, seed=None, offset=None):
        return self._decode(x, 1.0, 0.0, sparse_decoding, sparse_per_batch, rand, seed, offset)

    def _decode(self, x, std, mean, sparse_decoding, sparse_per_batch, rand=None, seed=None, offset=None):
        if tuple(x.shape[-2:]) != (self.dim1, self.dim2):
            raise ValueError(f"Decoder: expected (..., layers, {self.dim1}, {self.dim2}), got {tuple(x.shape)}")
        x = x.reshape(x.shape[:-2] + (self.dim1 * self.dim2,))
        pm = self.packed()
        if not sparse_decoding:
            return pm.apply(x, std, mean, affine_first=True)
        if std != 1.0 or mean != 0.0:  # (every shipped HGCal constant set has embed_mean 0, embed_std 1)
            x = engine._dev32(x, "x") * std + mean
        if rand is None and seed is None and offset is None:
            seed, offset = self.noise_seed, self.noise_offset
            self.noise_offset += (1 if sparse_per_batch else int(x.shape[0])) * pm.layers * pm.rows * pm.cols
        return pm.decode_sparse(x, bool(sparse_per_batch), rand, seed if seed is not None else self.noise_seed, offset or 0)


def init_map(num_alpha_bins, num_r_bins, geom, ilay):
    """The geometric encoding matrix of layer ``ilay`` and the mask of its trainable neighbourhood, both (alpha * r, max_ncell):
    ``init_map`` of the reference (HGCal_utils.py:412-486), quirks included.  A cell goes to the (alpha, r) bin of its angle and
    (re-binned) ring; within 1e-2 of the lower edge of its angular bin it is split 0.5 / 0.5 with the bin below; cell 0, the
    centre, is shared by every angular bin of the first ring."""
    A, R, n_in = int(num_alpha_bins), int(num_r_bins), int(geom.max_ncell)
    ncells = int(round(geom.ncells[ilay]))
    weight, mask = torch.zeros((A, R, n_in)), torch.zeros((A, R, n_in))
    # rings from 23 outwards are merged three to a radial bin
    inner, max_ring, outer_step = 23, 100, 3
    r_binning = np.arange(0, max_ring, 1)
    r_binning[inner:] = (r_binning[inner:] - inner) // outer_step + inner
    # angular bin edges, shifted by half a bin so that a bin is centred on angle 0; phi is periodic: the last bin is the first
    step = 2.0 * np.pi / A
    edges = torch.arange(0, 2.0 * np.pi + step, step)
    edges += np.pi / A
    alphas = torch.tensor(geom.theta_map[ilay][:n_in])
    a_bins = torch.bucketize(alphas + 1e-4, edges, right=True)
    a_bins[a_bins == A] = 0
    below = torch.abs(alphas - edges[a_bins - 1])
    at_edge = (below < 1e-2) | (torch.abs(below - 2.0 * np.pi) < 1e-2)
    weight[:, 0, 0] = 1.0 / A
    mask[:, 0, 0] = 1.0
    for i in range(1, ncells):
        a = int(a_bins[i]) % A
        r = int(r_binning[int(round(geom.ring_map[ilay, i]))])
        am = (a - 1) % A
        if at_edge[i]:
            weight[a, r, i] = weight[am, r, i] = 0.5
            mask[a, r, i] = mask[am, r, i] = 1.0
            if r > 0:
                mask[a, r - 1, i] = mask[am, r - 1, i] = 1.0
            if r < R - 1:
                mask[a, r + 1, i] = 1.0
                mask[am, (r - 1) % R, i] = 1.0  # (the reference marks r - 1 here, not r + 1: kept, the masks must agree)
        else:
            weight[a, r, i] = 1.0
            mask[a, r, i] = mask[am, r, i] = mask[(a + 1) % A, r, i] = 1.0
            if r > 0:
                mask[a, r - 1, i] = 1.0
            if r < R - 1:
                mask[a, r + 1, i] = 1.0
    return weight.reshape((A * R, n_in)), mask.reshape((A * R, n_in))


class _RenamedGeoUnpickler(pickle.Unpickler):
    """Geometry pickles name their class as the top-level module ``HGCalGeo``; it lives in the HGCalShowers package."""

    def find_class(self, module, name):
        return super().find_class("HGCalShowers.HGCalGeo" if module == "HGCalGeo" else module, name)


def load_geom(geom_filename):
    """The pickled HGCalGeo of a binning file, with ``theta_map`` and ``max_ncell`` added (HGCal_utils.py:489-514)."""
    try:
        import HGCalShowers.HGCalGeo  # noqa: F401  (the pickle holds an instance of its class)
    except ImportError as err:
        raise ImportError(f"loading the geometry file {geom_filename!r} needs the HGCalShowers package (its HGCalGeo class is "
                          "what the file pickles), which is not importable; build the converter with "
                          "HGCalConverter.from_geometry / from_matrices instead") from err
    with open(geom_filename, "rb") as fh:
        geom = _RenamedGeoUnpickler(fh).load()
    geom.theta_map = np.arctan2(geom.xmap, geom.ymap) % (2.0 * np.pi)
    geom.max_ncell = int(round(np.amax(geom.ncells)))
    return geom


class HGCalConverter(torch.nn.Module):
    """``HGCalConverter`` (HGCal_utils.py:517-680) with the maps on the device: ``enc`` / ``dec`` take and return device
    tensors, ``enc_batches`` / ``dec_batches`` numpy, as the reference's.  Inference only (see the module docstring).

    Built as the reference is -- ``HGCalConverter(bins=, geom_file=)`` then ``init(norm=, dataset_num=)`` -- or without the
    pickle by ``from_geometry``, ``from_matrices`` or ``from_reference``."""

    def __init__(self, bins=None, geom_file=None, hidden_size=32, device=None, trainable=False, geom=None):
        super().__init__()
        self.device, self.trainable = device, bool(trainable)
        self.geom = load_geom(geom_file) if geom is None and geom_file else geom
        if self.geom is not None and not hasattr(self.geom, "theta_map"):
            self.geom.theta_map = np.arctan2(self.geom.xmap, self.geom.ymap) % (2.0 * np.pi)
        self.bins = bins
        self.num_layers, self.num_alpha_bins, self.num_r_bins = (int(b) for b in bins[-3:])
        self.norm, self.embed_mean, self.embed_std = False, 0.0, 1.0
        E = self.num_alpha_bins * self.num_r_bins
        N = int(self.geom.max_ncell) if self.geom is not None else 1
        self._set_maps(torch.zeros((self.num_layers, E, N)), torch.zeros((self.num_layers, N, E)), None, None)

    def _set_maps(self, enc_mat, dec_mat, enc_mask, dec_mask):
        L, E = self.num_layers, self.num_alpha_bins * self.num_r_bins
        if enc_mat.dim() != 3 or enc_mat.shape[:2] != (L, E) or tuple(dec_mat.shape) != (L, enc_mat.shape[2], E):
            raise ValueError(f"HGCalConverter: enc_mat must be ({L}, {E}, cells) and dec_mat ({L}, cells, {E}); got "
                             f"{tuple(enc_mat.shape)} and {tuple(dec_mat.shape)}")
        self.enc_mat, self.dec_mat = enc_mat, dec_mat
        self.enc_mask = torch.abs(enc_mat) > EPS if enc_mask is None else enc_mask
        self.dec_mask = torch.abs(dec_mat) > EPS if dec_mask is None else dec_mask
        self.embeder = Embeder(self.num_alpha_bins, self.num_r_bins, self.enc_mat, self.enc_mask, trainable=self.trainable)
        self.decoder = Decoder(self.num_alpha_bins, self.num_r_bins, self.dec_mat, self.dec_mask, trainable=self.trainable)

    @classmethod
    def from_matrices(cls, bins, enc_mat, dec_mat, enc_mask=None, dec_mask=None):
        """A converter over given maps: enc_mat (L, alpha * r, cells), dec_mat (L, cells, alpha * r); the masks (used by a
        trainable converter only) default to |mat| > 1e-6."""
        conv = cls(bins=bins)
        as_t = lambda a: None if a is None else torch.as_tensor(a)  # noqa: E731
        conv._set_maps(as_t(enc_mat).to(torch.float32), as_t(dec_mat).to(torch.float32), as_t(enc_mask), as_t(dec_mask))
        return conv

    @classmethod
    def from_reference(cls, obj, bins=None):
        """A converter with the maps and normalisation of an initialised reference ``HGCalConverter`` (or anything with
        ``enc_mat``, ``dec_mat``, ``norm``, ``embed_mean`` and ``embed_std``; ``bins`` if the object has none)."""
        conv = cls.from_matrices(bins if bins is not None else obj.bins, obj.enc_mat.detach(), obj.dec_mat.detach(),
                                 getattr(obj, "enc_mask", None), getattr(obj, "dec_mask", None))
        conv.norm, conv.embed_mean, conv.embed_std = bool(obj.norm), float(obj.embed_mean), float(obj.embed_std)
        return conv

    @classmethod
    def from_geometry(cls, geom, bins, norm=False, dataset_num=101):
        """A converter initialised from a geometry object: ``ncells``, ``ring_map``, ``theta_map`` (or ``xmap`` / ``ymap``),
        ``nlayers`` and ``max_ncell``."""
        conv = cls(bins=bins, geom=geom)
        conv.init(norm=norm, dataset_num=dataset_num)
        return conv

    def init(self, noise_scale=0.0, norm=False, dataset_num=101):
        """``HGCalConverter.init`` (HGCal_utils.py:595-634): the geometric encoding of every layer and its pseudo-inverse."""
        if noise_scale > 0.0:
            raise NotImplementedError("HGCalConverter.init(noise_scale > 0) perturbs the maps for TRAINABLE_EMBED training, "
                                      "which is not provided")
        if self.geom is None:
            raise ValueError("HGCalConverter.init needs a geometry (geom_file= or geom=)")
        E, N = self.num_alpha_bins * self.num_r_bins, int(self.geom.max_ncell)
        enc_mat, dec_mat = torch.zeros((self.num_layers, E, N)), torch.zeros((self.num_layers, N, E))
        enc_mask, dec_mask = torch.zeros((self.num_layers, E, N), dtype=torch.bool), torch.zeros((self.num_layers, N, E), dtype=torch.bool)
        for i in range(self.geom.nlayers):
            conv_map, mask = init_map(self.num_alpha_bins, self.num_r_bins, self.geom, i)
            inv = torch.linalg.pinv(conv_map)
            enc_mat[i], enc_mask[i] = conv_map, mask > EPS
            dec_mat[i], dec_mask[i] = inv, torch.abs(inv) > EPS
        self._set_maps(enc_mat, dec_mat, enc_mask, dec_mask)
        if norm:
            if dataset_num not in HGCAL_EMBED_PARAMS:
                raise KeyError(f"no embed_mean / embed_std for dataset_num {dataset_num!r}")
            self.norm = True
            self.embed_mean, self.embed_std = HGCAL_EMBED_PARAMS[dataset_num]

    def _affine(self):
        return (self.embed_std, self.embed_mean) if self.norm else (1.0, 0.0)

    def enc(self, x):
        return self.embeder._embed(x, *self._affine())

    def dec(self, x, sparse_decoding=False, sparse_per_batch=False, **draw):
        """``draw``: the ``rand`` / ``seed`` / ``offset`` keywords of ``Decoder.forward``."""
        return self.decoder._decode(x, *self._affine(), sparse_decoding, sparse_per_batch, **draw)

    def enc_batches(self, x, batch_size=256):
        x = torch.as_tensor(x)
        out = [self.enc(x[i:i + batch_size].cuda()).cpu().numpy() for i in range(0, x.shape[0], batch_size)]
        return np.concatenate(out) if out else None

    def dec_batches(self, x, batch_size=128, sparse_decoding=False, sparse_per_batch=False):
        x = torch.as_tensor(x)
        out = [self.dec(x[i:i + batch_size].cuda(), sparse_decoding=sparse_decoding, sparse_per_batch=sparse_per_batch).cpu().numpy()
               for i in range(0, x.shape[0], batch_size)]
        return np.concatenate(out) if out else None

    def forward(self, x):
        return self.dec(self.enc(x))
