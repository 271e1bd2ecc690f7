"""Dataset-1 geometry maps on the device: ``GeomConverter`` and ``NNConverter`` of the reference
(calodiffusion/utils/utils.py:659-784, 576-656) over ``cd_radial_*`` (include/calodiff.h, "Dataset-1 radial maps").

CaloChallenge Dataset 1 has an irregular voxel layout: every layer has its own radial edges and 1 or ``alpha_out`` angular bins.
``GeomConverter`` maps a layer's radial bins onto the union of all radial edges in proportion to r^2 area (and back by the
pseudo-inverse); ``NNConverter`` holds the same maps as trainable ``nn.Linear(bias=False)`` weights, which the model applies
inside ``forward``.  Here the matrices are built on the host exactly as the reference builds them, and every product -- for the
whole batch and all layers -- is one launch; the trainable form is differentiable with respect to its input and its weights
(``cd_radial_enc_vjp`` / ``cd_radial_dec_vjp``), once.

Difference to the reference: results stay on the device (the reference allocates ``enc``'s and ``convert``'s outputs on the CPU).
Inputs that are numpy arrays or host tensors are moved to the device.  There is no torch fallback: without a GPU or the built
library every product raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from .abi import Handle, _check, _ptr, _stream, _upload, load_library, require_gpu

# the on-chip limits of cd_radial_create (include/calodiff.h)
MAX_LAYERS, MAX_WEIGHT_FLOATS, MAX_ROW_FLOATS = 64, 8192, 6144


class _RadialMap(Handle):
    """Owner of one CdRadialMap handle; the four launches on raw device tensors."""

    def __init__(self, bound, alpha, rin, alpha_out, r_out):
        self._lib = load_library()
        require_gpu()
        super().__init__(self._lib.cd_radial_destroy)
        L = len(alpha)
        self.L, self.A, self.R, self.V = L, int(alpha_out), int(r_out), int(bound[-1])
        self.wtotal = self.R * int(sum(rin))
        i32 = lambda v: (C.c_int32 * len(v))(*[int(a) for a in v])  # noqa: E731
        _check(self._lib.cd_radial_create(L, i32(bound), i32(alpha), i32(rin), self.A, self.R, C.byref(self.handle),
                                          _stream()))

    def _flat(self, x, name):
        if x.dim() != 2 or x.shape[1] != self.V:
            raise ValueError(f"{name}: expected (batch, {self.V}) voxels, got {tuple(x.shape)}")
        return x

    def _grid(self, g, name):
        if g.dim() not in (4, 5) or g.numel() != g.shape[0] * self.L * self.A * self.R or \
                tuple(g.shape[-3:]) != (self.L, self.A, self.R):
            raise ValueError(f"{name}: expected (batch, 1, {self.L}, {self.A}, {self.R}), got {tuple(g.shape)}")
        return g

    def _weights(self, w, name):
        if w.numel() != self.wtotal:
            raise ValueError(f"{name}: the concatenated matrices hold {self.wtotal} values, got {w.numel()}")
        return w

    def enc(self, w, x):
        self._flat(x, "enc"), self._weights(w, "enc")
        y = torch.empty((x.shape[0], 1, self.L, self.A, self.R), dtype=torch.float32, device=x.device)
        if y.numel():
            _check(self._lib.cd_radial_enc(self.handle, w.data_ptr(), x.data_ptr(), y.data_ptr(), x.shape[0], _stream()))
        return y

    def dec(self, d, g):
        self._grid(g, "dec"), self._weights(d, "dec")
        x = torch.empty((g.shape[0], self.V), dtype=torch.float32, device=g.device)
        if x.numel():
            _check(self._lib.cd_radial_dec(self.handle, d.data_ptr(), g.data_ptr(), x.data_ptr(), g.shape[0], _stream()))
        return x

    def enc_vjp(self, w, x, gy, want_dw):
        self._flat(x, "enc_vjp"), self._grid(gy, "enc_vjp"), self._weights(w, "enc_vjp")
        dx = torch.empty_like(x)
        dw = (torch.empty_like(w) if x.shape[0] else torch.zeros_like(w)) if want_dw else None
        if x.shape[0]:
            _check(self._lib.cd_radial_enc_vjp(self.handle, w.data_ptr(), x.data_ptr(), gy.data_ptr(), dx.data_ptr(),
                                               _ptr(dw), x.shape[0], _stream()))
        return dx, dw

    def dec_vjp(self, d, g, gx, want_dd):
        self._grid(g, "dec_vjp"), self._flat(gx, "dec_vjp"), self._weights(d, "dec_vjp")
        dg = torch.empty_like(g)
        dd = (torch.empty_like(d) if g.shape[0] else torch.zeros_like(d)) if want_dd else None
        if g.shape[0]:
            _check(self._lib.cd_radial_dec_vjp(self.handle, d.data_ptr(), g.data_ptr(), gx.data_ptr(), dg.data_ptr(),
                                               _ptr(dd), g.shape[0], _stream()))
        return dg, dd


class GeomConverter:
    """``GeomConverter`` (utils.py:659-784): the fixed area-weighted maps of an irregular cylindrical geometry.

    Built from ``bins`` -- any object with ``GetBinEdges()``, ``GetRelevantLayers()``, ``r_edges`` and ``alphaListPerLayer``, such
    as the reference's ``XMLHandler`` -- or from explicit edges: ``all_r_edges`` (the sorted union), ``lay_r_edges`` (per layer),
    ``alpha_out`` and ``lay_alphas``; then ``layer_boundaries`` (offsets of the layers in the flat shower, which the reference
    leaves empty on this path) is given here or set before the first product.

    ``reshape`` / ``unreshape`` / ``convert`` / ``unconvert`` keep the reference's contracts; ``convert_flat`` and
    ``unconvert_flat`` are the fused forms, one launch each, and the list forms go through them."""

    def __init__(self, bins=None, all_r_edges=None, lay_r_edges=None, alpha_out=1, lay_alphas=None, layer_boundaries=None):
        self.layer_boundaries = [] if layer_boundaries is None else np.asarray(layer_boundaries, dtype=np.int64)
        self.bins = None
        if bins is not None:
            self.layer_boundaries = np.unique(bins.GetBinEdges())
            lay_alphas = [len(bins.alphaListPerLayer[idx][0]) for idx, edges in enumerate(bins.r_edges) if len(edges) > 1]
            alpha_out = np.amax(lay_alphas)
            lay_r_edges = [bins.r_edges[lay] for lay in bins.GetRelevantLayers()]
            all_r_edges = torch.unique(torch.FloatTensor([e for edges in lay_r_edges for e in edges]))
        if all_r_edges is None or lay_r_edges is None:
            raise ValueError("GeomConverter needs bins, or all_r_edges and lay_r_edges")
        self.all_r_edges = torch.as_tensor(all_r_edges, dtype=torch.float32)
        self.lay_r_edges = lay_r_edges
        self.alpha_out = alpha_out
        self.lay_alphas = lay_alphas
        self.num_layers = len(lay_r_edges)
        self.all_r_areas = self.all_r_edges[1:] ** 2 - self.all_r_edges[:-1] ** 2
        self.dim_r_out = len(self.all_r_edges) - 1
        self.weight_mats = []
        for ilay, edges in enumerate(lay_r_edges):
            edges = torch.as_tensor(edges, dtype=torch.float32)
            dim_in = len(edges) - 1
            nn.Linear(dim_in, self.dim_r_out, bias=False)  # the reference builds (and drops) one per layer: same RNG draws
            mat = torch.zeros((self.dim_r_out, dim_in))
            at = [torch.nonzero(self.all_r_edges == e) for e in edges]
            if any(len(hit) == 0 for hit in at):
                raise ValueError(f"lay_r_edges[{ilay}] has an edge that is not in all_r_edges")
            at = [int(hit[0][0]) for hit in at]
            for ir in range(dim_in):  # input bin ir is split over the output bins it covers, in proportion to their r^2 area
                lo, hi = at[ir], at[ir + 1]
                mat[lo:hi, ir] = self.all_r_areas[lo:hi] / (edges[ir + 1] ** 2 - edges[ir] ** 2)
            self.weight_mats.append(mat)
        self.pinv_mats = [torch.linalg.pinv(m) for m in self.weight_mats]
        self._map = self._map_key = self._fixed = None

    # ---- layout ------------------------------------------------------------------------------------------------------
    def descriptor(self):
        """(bound, alpha, rin) as lists of int, validated: what ``cd_radial_create`` takes."""
        L, A = self.num_layers, int(self.alpha_out)
        alpha = [A] * L if self.lay_alphas is None else [int(a) for a in self.lay_alphas]
        rin = [len(e) - 1 for e in self.lay_r_edges]
        bound = [int(b) for b in self.layer_boundaries]
        if len(alpha) != L:
            raise ValueError(f"lay_alphas has {len(alpha)} entries for {L} layers")
        for i, a in enumerate(alpha):
            if a != 1 and a != A:
                raise ValueError(f"lay_alphas[{i}] is {a}: a layer has 1 or alpha_out = {A} angular bins")
        if len(bound) != L + 1:
            raise ValueError(f"layer_boundaries must hold {L + 1} offsets (pass layer_boundaries= or set it), got {len(bound)}")
        if bound[0] != 0 or any(hi <= lo for lo, hi in zip(bound, bound[1:])):
            raise ValueError(f"layer_boundaries must start at 0 and increase strictly, got {bound}")
        for i in range(L):
            if bound[i + 1] - bound[i] != alpha[i] * rin[i]:
                raise ValueError(f"layer_boundaries: layer {i} spans {bound[i + 1] - bound[i]} voxels, but lay_alphas[{i}] * radial "
                                 f"bins = {alpha[i]} * {rin[i]}")
        if L > MAX_LAYERS or self.dim_r_out * sum(rin) > MAX_WEIGHT_FLOATS or max(bound[-1], L * A * self.dim_r_out) > MAX_ROW_FLOATS:
            raise ValueError(f"geometry beyond the on-chip limits of cd_radial_create: layers <= {MAX_LAYERS}, dim_r_out * sum of "
                             f"radial bins <= {MAX_WEIGHT_FLOATS}, voxels and layers * alpha_out * dim_r_out <= {MAX_ROW_FLOATS}")
        return bound, alpha, rin

    def radial_map(self) -> _RadialMap:
        """The device handle of the current layout (rebuilt when the layout attributes change)."""
        bound, alpha, rin = self.descriptor()
        key = (tuple(bound), tuple(alpha), tuple(rin), int(self.alpha_out), int(self.dim_r_out))
        if self._map_key != key:
            self._map, self._map_key = _RadialMap(bound, alpha, rin, self.alpha_out, self.dim_r_out), key
        return self._map

    def reshape(self, raw_shower):
        """flat (N, V) -> per layer (N, alpha_i, rin_i)"""
        b = self.layer_boundaries
        return [raw_shower[:, b[i]:b[i + 1]].reshape(raw_shower.shape[0], int(self.lay_alphas[i]), -1) for i in range(len(b) - 1)]

    def unreshape(self, raw_shower):
        """per layer (N, alpha_i, rin_i) -> flat (N, V)"""
        return torch.cat([torch.as_tensor(lay).reshape(lay.shape[0], -1) for lay in raw_shower], dim=1)

    # ---- products ----------------------------------------------------------------------------------------------------
    def _fixed_weights(self):
        if self._fixed is None:
            self._fixed = tuple(torch.cat([m.reshape(-1) for m in mats]).to(device="cuda", dtype=torch.float32)
                                for mats in (self.weight_mats, self.pinv_mats))
        return self._fixed

    def convert_flat(self, x):
        """flat showers (N, V) -> (N, L, alpha_out, dim_r_out): ``convert(reshape(x))`` in one launch."""
        rm = self.radial_map()
        return rm.enc(self._fixed_weights()[0], _upload(x, torch.float32, "convert_flat", need_gpu=True))[:, 0]

    def unconvert_flat(self, d):
        """(N, L, alpha_out, dim_r_out) (or with the channel axis) -> flat showers (N, V): ``unreshape(unconvert(d))`` in one launch."""
        rm = self.radial_map()
        return rm.dec(self._fixed_weights()[1], _upload(d, torch.float32, "unconvert_flat", need_gpu=True))

    def convert(self, d):
        return self.convert_flat(self.unreshape([torch.as_tensor(lay, dtype=torch.float32) for lay in d]))

    def unconvert(self, d):
        return self.reshape(self.unconvert_flat(d))


class _RadialFunction(torch.autograd.Function):
    """enc (``is_enc``) or dec of an NNConverter: one launch forward, one backward (input gradient, and the weight gradients when
    a weight requires one)."""

    @staticmethod
    def forward(ctx, x, rmap, is_enc, *weights):
        w = torch.cat([p.detach().reshape(-1) for p in weights]).to(device=x.device, dtype=torch.float32)
        ctx.rmap, ctx.is_enc, ctx.shapes = rmap, is_enc, [p.shape for p in weights]
        ctx.save_for_backward(x, w)
        return rmap.enc(w, x) if is_enc else rmap.dec(w, x)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        x, w = ctx.saved_tensors
        want_w = any(ctx.needs_input_grad[3:])
        grad = grad.to(torch.float32).contiguous()
        dx, dw = (ctx.rmap.enc_vjp if ctx.is_enc else ctx.rmap.dec_vjp)(w, x, grad, want_w)
        dws = [None] * (len(ctx.needs_input_grad) - 3)
        if want_w:
            parts = torch.split(dw, [shape.numel() for shape in ctx.shapes])
            dws = [part.reshape(shape) if need else None for part, shape, need in zip(parts, ctx.shapes, ctx.needs_input_grad[3:])]
        return (dx, None, None, *dws)


class NNConverter(nn.Module):
    """``NNConverter`` (utils.py:576-656): the maps of a ``GeomConverter`` as trainable ``nn.Linear(bias=False)`` weights,
    ``encs[i].weight`` (dim_r_out, rin_i) and ``decs[i].weight`` (rin_i, dim_r_out), initialised as the reference initialises them
    (same values under the same ``torch.manual_seed``; a reference checkpoint's ``NN_embed.*`` entries load).

    ``enc``: flat showers (N, V) -> (N, 1, L, alpha_out, dim_r_out); ``dec`` the way back; ``forward`` is ``enc``.  Both are
    differentiable once with respect to the input and the weights; results are device tensors."""

    def __init__(self, geomconverter=None, bins=None, hidden_size=32):
        super().__init__()
        self.gc = GeomConverter(bins) if geomconverter is None else geomconverter
        self.encs, self.decs = nn.ModuleList([]), nn.ModuleList([])
        eps = 1e-5
        for mat in self.gc.weight_mats:  # RNG draws in the reference's order: Linear, noise, Linear, noise
            dim_out, dim_in = mat.shape
            lay = nn.Linear(dim_in, dim_out, bias=False)
            lay.weight.data = mat + eps * torch.randn_like(mat)
            self.encs.append(lay)
            inv_lay = nn.Linear(dim_out, dim_in, bias=False)
            inv = torch.linalg.pinv(mat)
            inv_lay.weight.data = inv + eps * torch.randn_like(inv)
            self.decs.append(inv_lay)

    def _apply_map(self, x, is_enc, layers):
        rmap = self.gc.radial_map()
        x = torch.as_tensor(x)
        if not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous():
            if not torch.cuda.is_available():
                raise RuntimeError("NNConverter: calodiffusion_amd computes on the GPU only and torch.cuda.is_available() is False")
            x = x.to(device="cuda", dtype=torch.float32).contiguous()  # (differentiable: a gradient flows back to a host input)
        return _RadialFunction.apply(x, rmap, is_enc, *[lay.weight for lay in layers])

    def enc(self, x):
        return self._apply_map(x, True, self.encs)

    def dec(self, x):
        return self._apply_map(x, False, self.decs)

    def forward(self, x):
        return self.enc(x)
