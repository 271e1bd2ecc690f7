"""HGCal geometry maps on the device: ``Embeder``, ``Decoder`` and ``HGCalConverter`` of the reference
(calodiffusion/utils/HGCal_utils.py:295-407, 412-486, 517-680) over the packed maps of ``cd_geom_*`` (include/calodiff.h).

The maps between HGCal's irregular cells (layers, cells) and the regular (layers, alpha, r) grid are linear with one or two
non-zeros per cell, so they are packed once (per-layer CSR, a transposed view for the gradients, and a column view for the
sampled decode) and applied by ``cd_geom_apply`` / ``cd_geom_decode_sparse``; nothing is copied to the host.  Building a map
from a geometry (``from_geometry``: ``init_map`` and ``torch.linalg.pinv``, :412-486, 595-634) is construction-time host work.

``forward``, ``enc`` and ``dec`` are differentiable (``cd_geom_apply_vjp``) when grad is enabled and the input or a trainable
``mat`` requires one; any other call is the plain product without a graph.  A trainable converter (``trainable=True``, the
configs' TRAINABLE_EMBED) holds its two maps as ``nn.Parameter``s trained through ``mat * mask``, as the reference's forward
does: the packed pattern is then the boolean ``mask`` -- a masked entry whose value is 0 still takes gradient, the gradient
outside the mask is exactly 0, and parameter values outside the mask never enter a product -- and the packed values are
gathered again from the live parameter whenever it changed.  Inside a model (``CaloDiffusion`` with HGCAL and no 'pre-embed')
the maps run within the denoise-based device calls (``cd_plan_set_geom``).  Not provided: ``init(noise_scale > 0)``.
"""
from __future__ import annotations

import ctypes as C
import pickle

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .abi import Handle, _check, _dev32, _nbytes, _ptr, _stream, _upload, load_library
from .postprocess import HGCAL_EMBED_PARAMS

EPS = 1e-6  # the threshold of HGCalConverter.init's masks and of generate_sparse_mat (HGCal_utils.py:371, 607)
_GEOM_COLUMNS, _GEOM_TRANSPOSED = 1, 2  # CD_GEOM_* of include/calodiff.h


def map_entries(mat, mask=None):
    """The sparse entries of a dense map (L, rows, cols), host or device tensor: per-layer CSR (row_ptr (L * rows + 1,) int32,
    col_idx, val) over the pattern ``mask != 0`` -- or ``mat != 0`` without one -- columns ascending within a row: the arrays
    ``cd_geom_create_ex`` packs on the device, formed on the host a layer at a time (the generator file's exporter; needs no GPU)."""
    mat = torch.as_tensor(mat).detach()
    L, rows, _ = (int(v) for v in mat.shape)
    if mask is not None and tuple(torch.as_tensor(mask).shape) != tuple(mat.shape):
        raise ValueError(f"geometry map: mask {tuple(torch.as_tensor(mask).shape)} must have the map's shape {tuple(mat.shape)}")
    counts, cols, vals = np.zeros(L * rows + 1, dtype=np.int64), [], []
    for l in range(L):
        m = mat[l].to("cpu", torch.float32)
        pat = (m != 0) if mask is None else (torch.as_tensor(mask)[l].to("cpu") != 0)
        r, c = torch.nonzero(pat, as_tuple=True)  # row-major: rows ascending, columns ascending within a row
        counts[1 + l * rows: 1 + (l + 1) * rows] = np.bincount(r.numpy(), minlength=rows)
        cols.append(c.numpy().astype(np.int32))
        vals.append(m[r, c].numpy())
    row_ptr = np.cumsum(counts)
    if row_ptr[-1] >= 2 ** 31:
        raise ValueError("geometry map: 2^31 or more entries")
    return row_ptr.astype(np.int32), np.concatenate(cols), np.concatenate(vals).astype(np.float32)


class _PackedMap(Handle):
    """Owner of one CdGeomMap handle.  ``mask``: the pattern of a trainable map (``dense`` then holds the values, read at the
    masked entries only; see ``refresh``); without one the pattern is ``dense != 0``."""

    def __init__(self, dense: torch.Tensor, want_columns: bool, mask=None):
        dense = _upload(dense, torch.float32, "dense")
        self.layers, self.rows, self.cols = (int(s) for s in dense.shape)
        self._lib = load_library()
        super().__init__(self._lib.cd_geom_destroy)
        pattern = None
        if mask is not None:
            pattern = _upload(torch.as_tensor(mask) != 0, torch.float32, "mask")
            if pattern.shape != dense.shape:
                raise ValueError(f"geometry map: mask {tuple(pattern.shape)} must have the map's shape {tuple(dense.shape)}")
        flags = _GEOM_TRANSPOSED | (_GEOM_COLUMNS if want_columns else 0)
        _check(self._lib.cd_geom_create_ex(dense.data_ptr(), _ptr(pattern), self.layers, self.rows, self.cols, flags,
                                           C.byref(self.handle), _stream()))

    @classmethod
    def from_entries(cls, row_ptr, col_idx, val, layers: int, rows: int, cols: int, want_columns: bool = False,
                     want_transposed: bool = True):
        """The same handle from the map's sparse entries (``map_entries``), without the dense tensor: ``cd_geom_create_csr``."""
        self = cls.__new__(cls)
        self.layers, self.rows, self.cols = int(layers), int(rows), int(cols)
        self._lib = load_library()
        Handle.__init__(self, self._lib.cd_geom_destroy)
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
        col_idx, val = np.ascontiguousarray(col_idx, dtype=np.int32), np.ascontiguousarray(val, dtype=np.float32)
        if row_ptr.shape != (self.layers * self.rows + 1,) or col_idx.shape != val.shape or col_idx.ndim != 1:
            raise ValueError(f"geometry map: row_ptr must hold layers * rows + 1 = {self.layers * self.rows + 1} entries and col_idx / "
                             "val one per entry")
        if col_idx.size < max(int(row_ptr[-1]), 0):
            raise ValueError(f"geometry map: row_ptr ends at {int(row_ptr[-1])}, {col_idx.size} entries given")
        flags = (_GEOM_TRANSPOSED if want_transposed else 0) | (_GEOM_COLUMNS if want_columns else 0)
        _check(self._lib.cd_geom_create_csr(row_ptr.ctypes.data, col_idx.ctypes.data, val.ctypes.data, self.layers, self.rows,
                                            self.cols, flags, C.byref(self.handle), _stream()))
        return self

    def refresh(self, dense: torch.Tensor):
        """the packed values again from ``dense`` (a trainable map's live parameter)"""
        dense = _upload(dense, torch.float32, "dense")
        if tuple(dense.shape) != (self.layers, self.rows, self.cols):
            raise ValueError(f"geometry map: expected ({self.layers}, {self.rows}, {self.cols}), got {tuple(dense.shape)}")
        _check(self._lib.cd_geom_refresh(self.handle, dense.data_ptr(), _stream()))
        self._held = dense  # (a converted copy must outlive the launch)

    def apply(self, x: torch.Tensor, scale: float, shift: float, affine_first: bool) -> torch.Tensor:
        """x (..., L, cols) -> (..., L, rows)"""
        x = _dev32(x, "x")
        if x.dim() < 2 or tuple(x.shape[-2:]) != (self.layers, self.cols):
            raise ValueError(f"geometry map: expected (..., {self.layers}, {self.cols}), got {tuple(x.shape)}")
        y = torch.empty(x.shape[:-1] + (self.rows,), dtype=torch.float32, device=x.device)
        if y.numel():
            _check(self._lib.cd_geom_apply(self.handle, x.data_ptr(), y.data_ptr(), x.numel() // (self.layers * self.cols),
                                           float(scale), float(shift), int(affine_first), _stream()))
        return y

    def apply_vjp(self, x, gy, scale: float, shift: float, affine_first: bool, want_dx: bool, want_dm: bool):
        """The gradients of ``apply`` for the cotangent gy (..., L, rows): (dx like x or None, dm (L, rows, cols) dense or None)"""
        x, gy = _dev32(x, "x"), _dev32(gy, "gy")
        if tuple(x.shape[-2:]) != (self.layers, self.cols) or gy.shape != x.shape[:-1] + (self.rows,):
            raise ValueError(f"geometry map gradient: x {tuple(x.shape)} and gy {tuple(gy.shape)} do not fit "
                             f"({self.layers}, {self.rows}, {self.cols})")
        dx = torch.empty_like(x) if want_dx else None
        dm = torch.empty((self.layers, self.rows, self.cols), dtype=torch.float32, device=x.device) if want_dm else None
        n = x.numel() // (self.layers * self.cols)
        if n == 0:
            return dx, (dm.zero_() if want_dm else None)
        if want_dx or want_dm:
            _check(self._lib.cd_geom_apply_vjp(self.handle, x.data_ptr(), gy.data_ptr(), _ptr(dx), _ptr(dm), n,
                                               float(scale), float(shift), int(affine_first), _stream()))
        return dx, dm

    def decode_sparse(self, x: torch.Tensor, per_batch: bool, rand, seed: int, offset: int) -> torch.Tensor:
        """x (B, C, L, cols) -> (B, C, L, rows)"""
        x = _dev32(x, "x")
        if x.dim() != 4 or tuple(x.shape[-2:]) != (self.layers, self.cols):
            raise ValueError(f"sparse decoding: expected (batch, channels, {self.layers}, {self.cols}), got {tuple(x.shape)}")
        B, ch = int(x.shape[0]), int(x.shape[1])
        if rand is not None:
            rand = _dev32(rand, "rand")
            if tuple(rand.shape) != (1 if per_batch else B, self.layers, self.rows, self.cols):
                raise ValueError(f"sparse decoding: rand must be ({1 if per_batch else B}, {self.layers}, {self.rows}, "
                                 f"{self.cols}), got {tuple(rand.shape)}")
        y = torch.empty((B, ch, self.layers, self.rows), dtype=torch.float32, device=x.device)
        if not y.numel():
            return y
        ws = torch.empty(_nbytes(self._lib.cd_geom_sparse_workspace_bytes, self.handle, B), dtype=torch.uint8, device=x.device)
        _check(self._lib.cd_geom_decode_sparse(self.handle, x.data_ptr(), y.data_ptr(), B, ch, int(per_batch), _ptr(rand),
                                               int(seed), int(offset), ws.data_ptr(), _stream()))
        return y


class _Apply(torch.autograd.Function):
    """``_PackedMap.apply`` with a backward: one cd_geom_apply_vjp call gives the input its gradient and, for a trainable map,
    ``mat`` its dense one (zero outside the mask).  ``mat`` is an argument only so that autograd routes that gradient."""

    @staticmethod
    def forward(ctx, x, mat, pm, scale, shift, affine_first):
        ctx.pm, ctx.affine = pm, (scale, shift, affine_first)
        ctx.mat_version = None if mat is None else mat._version
        ctx.mat = mat
        ctx.save_for_backward(x)
        return pm.apply(x.detach(), scale, shift, affine_first)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        if ctx.mat is not None and ctx.mat._version != ctx.mat_version:
            raise RuntimeError("geometry map: the trainable matrix was modified in place between forward and backward")
        dx, dm = ctx.pm.apply_vjp(x, gy.contiguous(), *ctx.affine, want_dx=ctx.needs_input_grad[0],
                                  want_dm=ctx.mat is not None and ctx.needs_input_grad[1])
        if dm is not None and dm.device != ctx.mat.device:
            dm = dm.to(ctx.mat.device)
        return dx, dm, None, None, None, None


class _Map(torch.nn.Module):
    """Shared part of Embeder and Decoder: the reference's attributes, and the handle packed on first use (and again after
    ``set``).  ``trainable``: ``mat`` is an ``nn.Parameter`` (one passed in is kept as it is), the handle is packed over ``mask`` and its
    values follow the parameter (its version and pointer are looked at on every use)."""
    _want_columns = False

    def __init__(self, dim1, dim2, mat, mask, trainable=False):
        super().__init__()
        self.dim1, self.dim2 = int(dim1), int(dim2)
        self.trainable = bool(trainable)
        if self.trainable and not isinstance(mat, torch.nn.Parameter):
            # (a map built on its own from a plain tensor stays frozen until its owner asks: HGCalConverter(trainable=True) does,
            # a direct caller says ``mat.requires_grad_()`` -- the result of a call then carries a graph, as the reference's)
            mat = torch.nn.Parameter(torch.as_tensor(mat).to(torch.float32), requires_grad=False)
        self.mat = mat
        self.mask = mask
        self._packed = self._values = self._sampled = None

    def set(self, mat, mask):
        """New values and mask.  A trainable map's Parameter object survives: it is filled in place."""
        if self.trainable:
            with torch.no_grad():
                self.mat.copy_(torch.as_tensor(mat))
        else:
            self.mat = mat
        self.mask = mask
        self._packed = self._values = self._sampled = None

    def _state(self):
        return (self.mat._version, self.mat.data_ptr())

    def packed(self) -> _PackedMap:
        if not self.trainable:
            if self._packed is None:
                self._packed = _PackedMap(self.mat, self._want_columns)
            return self._packed
        if self._packed is None:
            self._packed = _PackedMap(self.mat, False, mask=self.mask)
            self._values = self._state()
        elif self._values != self._state():
            self._packed.refresh(self.mat)
            self._values = self._state()
        return self._packed

    def _apply_map(self, x, scale, shift, affine_first):
        pm = self.packed()
        mat = self.mat if self.trainable and self.mat.requires_grad else None
        if torch.is_grad_enabled() and (mat is not None or (isinstance(x, torch.Tensor) and x.requires_grad)):
            return _Apply.apply(_dev32(x, "x"), mat, pm, scale, shift, affine_first)
        return pm.apply(x, scale, shift, affine_first)


class Embeder(_Map):
    """``Embeder`` (HGCal_utils.py:295-324): cells (..., L, N) -> grid (..., L, dim1, dim2) with ``mat`` (L, dim1 * dim2, N)."""

    def forward(self, x):
        return self._embed(x, 1.0, 0.0)

    def _embed(self, x, std, mean):
        out = self._apply_map(x, std, mean, affine_first=False)
        return out.reshape(out.shape[:-1] + (self.dim1, self.dim2))


class Decoder(_Map):
    """``Decoder`` (HGCal_utils.py:327-353): grid (..., L, dim1, dim2) -> cells (..., L, N) with ``mat`` (L, N, dim1 * dim2).

    ``sparse_decoding`` (``generate_sparse_mat``, :355-407) takes x (B, C, L, dim1, dim2) and carries no autograd graph.  Its
    uniforms come from the device Philox stream (``seed``, ``offset``): by default the decoder's own (``noise_seed``, and a running
    ``noise_offset`` that advances by the (B or 1, L, N, E) tensor a call draws); a batch shard passes ``offset`` = that of the
    global call + first shower * L * N * E.  ``rand`` (B or 1, L, N, E) replaces the draw (parity with a recorded
    ``torch.rand``)."""
    _want_columns = True

    def __init__(self, dim1, dim2, mat, mask, trainable=False):
        super().__init__(dim1, dim2, mat, mask, trainable)
        self.noise_seed, self.noise_offset = 1234, 0

    def forward(self, x, sparse_decoding=False, sparse_per_batch=False, *, rand=None, seed=None, offset=None):
        return self._decode(x, 1.0, 0.0, sparse_decoding, sparse_per_batch, rand, seed, offset)

    def _sampled_map(self) -> _PackedMap:
        """the map with its column view: a trainable map's is packed from ``mat * mask`` as it stands (the view holds values)"""
        if not self.trainable:
            return self.packed()
        if self._sampled is None or self._sampled[0] != self._state():
            mask = torch.as_tensor(self.mask).to(self.mat.device)
            self._sampled = (self._state(), _PackedMap(self.mat.detach() * mask, True))
        return self._sampled[1]

    def _decode(self, x, std, mean, sparse_decoding, sparse_per_batch, rand=None, seed=None, offset=None):
        if tuple(x.shape[-2:]) != (self.dim1, self.dim2):
            raise ValueError(f"Decoder: expected (..., layers, {self.dim1}, {self.dim2}), got {tuple(x.shape)}")
        x = x.reshape(x.shape[:-2] + (self.dim1 * self.dim2,))
        if not sparse_decoding:
            return self._apply_map(x, std, mean, affine_first=True)
        pm = self._sampled_map()
        if std != 1.0 or mean != 0.0:  # (every shipped HGCal constant set has embed_mean 0, embed_std 1)
            x = _dev32(x, "x") * std + mean
        if rand is None and seed is None and offset is None:
            seed, offset = self.noise_seed, self.noise_offset
            self.noise_offset += (1 if sparse_per_batch else int(x.shape[0])) * pm.layers * pm.rows * pm.cols
        return pm.decode_sparse(x.detach(), bool(sparse_per_batch), rand, seed if seed is not None else self.noise_seed, offset or 0)


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
    tensors, ``enc_batches`` / ``dec_batches`` numpy, as the reference's; both are differentiable (see the module docstring).

    Built as the reference is -- ``HGCalConverter(bins=, geom_file=)`` then ``init(norm=, dataset_num=)`` -- or without the
    pickle by ``from_geometry``, ``from_matrices`` or ``from_reference``.  ``trainable=True``: ``embeder.mat`` and
    ``decoder.mat`` are Parameters (state_dict keys ``embeder.mat``, ``decoder.mat``, ``nets.0.mat``, ``nets.1.mat``, the
    reference's), zero with empty masks until ``init()`` or a checkpoint fills them in place."""

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
        L = self.num_layers
        self._set_maps(torch.zeros((L, E, N)), torch.zeros((L, N, E)), torch.zeros((L, E, N), dtype=torch.bool),
                       torch.zeros((L, N, E), dtype=torch.bool))

    # the reference's four tensors live in the two map modules (a trainable converter's enc_mat / dec_mat: the Parameters' data)
    enc_mat = property(lambda self: self.embeder.mat.detach() if self.trainable else self.embeder.mat)
    dec_mat = property(lambda self: self.decoder.mat.detach() if self.trainable else self.decoder.mat)
    enc_mask = property(lambda self: self.embeder.mask)
    dec_mask = property(lambda self: self.decoder.mask)

    def _set_maps(self, enc_mat, dec_mat, enc_mask, dec_mask):
        L, E = self.num_layers, self.num_alpha_bins * self.num_r_bins
        if enc_mat.dim() != 3 or enc_mat.shape[:2] != (L, E) or tuple(dec_mat.shape) != (L, enc_mat.shape[2], E):
            raise ValueError(f"HGCalConverter: enc_mat must be ({L}, {E}, cells) and dec_mat ({L}, cells, {E}); got "
                             f"{tuple(enc_mat.shape)} and {tuple(dec_mat.shape)}")
        enc_mask = torch.abs(enc_mat) > EPS if enc_mask is None else enc_mask
        dec_mask = torch.abs(dec_mat) > EPS if dec_mask is None else dec_mask
        if tuple(enc_mask.shape) != tuple(enc_mat.shape) or tuple(dec_mask.shape) != tuple(dec_mat.shape):
            raise ValueError(f"HGCalConverter: the masks must have the maps' shapes; got {tuple(enc_mask.shape)} and "
                             f"{tuple(dec_mask.shape)}")
        have = getattr(self, "embeder", None)
        if self.trainable and have is not None and have.mat.shape == enc_mat.shape:  # in place: the Parameter objects survive
            self.embeder.set(enc_mat, enc_mask)
            self.decoder.set(dec_mat, dec_mask)
            return
        self.embeder = Embeder(self.num_alpha_bins, self.num_r_bins, enc_mat, enc_mask, trainable=self.trainable)
        self.decoder = Decoder(self.num_alpha_bins, self.num_r_bins, dec_mat, dec_mask, trainable=self.trainable)
        self.nets = torch.nn.ModuleList([self.embeder, self.decoder])
        if self.trainable:
            self.embeder.mat.requires_grad_(True)
            self.decoder.mat.requires_grad_(True)

    @classmethod
    def from_matrices(cls, bins, enc_mat, dec_mat, enc_mask=None, dec_mask=None, trainable=False):
        """A converter over given maps: enc_mat (L, alpha * r, cells), dec_mat (L, cells, alpha * r); the masks (used by a
        trainable converter only) default to |mat| > 1e-6."""
        conv = cls(bins=bins, trainable=trainable)
        as_t = lambda a: None if a is None else torch.as_tensor(a)  # noqa: E731
        conv._set_maps(as_t(enc_mat).to(torch.float32), as_t(dec_mat).to(torch.float32), as_t(enc_mask), as_t(dec_mask))
        return conv

    @classmethod
    def from_reference(cls, obj, bins=None):
        """A converter with the maps and normalisation of an initialised reference ``HGCalConverter`` (or anything with
        ``enc_mat``, ``dec_mat``, ``norm``, ``embed_mean`` and ``embed_std``; ``bins`` if the object has none)."""
        conv = cls.from_matrices(bins if bins is not None else obj.bins, obj.enc_mat.detach(), obj.dec_mat.detach(),
                                 getattr(obj, "enc_mask", None), getattr(obj, "dec_mask", None),
                                 trainable=bool(getattr(obj, "trainable", False)))
        conv.norm, conv.embed_mean, conv.embed_std = bool(obj.norm), float(obj.embed_mean), float(obj.embed_std)
        return conv

    @classmethod
    def from_geometry(cls, geom, bins, norm=False, dataset_num=101, trainable=False):
        """A converter initialised from a geometry object: ``ncells``, ``ring_map``, ``theta_map`` (or ``xmap`` / ``ymap``),
        ``nlayers`` and ``max_ncell``."""
        conv = cls(bins=bins, geom=geom, trainable=trainable)
        conv.init(norm=norm, dataset_num=dataset_num)
        return conv

    def init(self, noise_scale=0.0, norm=False, dataset_num=101):
        """``HGCalConverter.init`` (HGCal_utils.py:595-634): the geometric encoding of every layer and its pseudo-inverse.  A
        trainable converter's Parameters are filled in place."""
        if noise_scale > 0.0:
            raise NotImplementedError("HGCalConverter.init(noise_scale > 0) perturbs the initial maps of TRAINABLE_EMBED training "
                                      "with torch.randn draws; that form of init is not provided")
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
