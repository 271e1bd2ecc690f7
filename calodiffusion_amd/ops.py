"""The primitive ops of the HIP library one at a time (``cd_op_*``): what the parity tests and the tools call; no library code
goes through ``Ops``.  ``ode_step`` and ``ema_step`` wrap the two stateless calls of consistency distillation (``distill.py``)."""
from __future__ import annotations

import ctypes as C
from typing import Dict

import numpy as np
import torch

from .abi import WorkspaceCache, _P, _check, _dev32, _i32x3, _ptr, _stream, load_library, require_gpu


def axpy_sigma(data, noise, sigma):
    """data + sigma[b] * noise from the launch the training step forms its network input with (cd_op_axpy_sigma): the same bits."""
    lib = load_library()
    require_gpu()
    data, noise, sigma = _dev32(data, "data"), _dev32(noise, "noise"), _dev32(sigma, "sigma").reshape(-1)
    B = data.shape[0]
    if noise.shape != data.shape or sigma.numel() != B or data.numel() == 0:
        raise ValueError(f"axpy_sigma: noise {tuple(noise.shape)} must have data's shape {tuple(data.shape)} and sigma B elements")
    out = torch.empty_like(data)
    _check(lib.cd_op_axpy_sigma(data.data_ptr(), noise.data_ptr(), sigma.data_ptr(), out.data_ptr(), B, data.numel() // B, _stream()))
    return out


def ode_step(x_hi, d_hi, sigma_hi, sigma_lo, x_e=None, d_e=None, out=None):
    """One probability-flow ODE step from sigma_hi to sigma_lo, a noise level per sample (cd_ode_step): the Euler x_lo from
    (x_hi, D_hi), or with (x_e, D_e) -- the Euler x_lo and the denoiser's output there -- the Heun x_lo.  ``out`` may be ``x_e``
    (in place); a fresh tensor otherwise.  The first axis is the batch, the rest of a sample is one row of any length."""
    lib = load_library()
    require_gpu()
    if (x_e is None) != (d_e is None):
        raise ValueError("ode_step: x_e and d_e come together (Heun) or not at all (Euler)")
    xs = [x_hi, d_hi] + ([x_e, d_e] if x_e is not None else []) + ([out] if out is not None else [])
    for v in xs:
        if not (isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and v.shape == x_hi.shape):
            raise ValueError("ode_step: contiguous float32 device tensors of one shape")
    B = x_hi.shape[0]
    sigma_hi, sigma_lo = _dev32(sigma_hi, "sigma_hi").reshape(-1), _dev32(sigma_lo, "sigma_lo").reshape(-1)
    if sigma_hi.numel() != B or sigma_lo.numel() != B or B == 0 or x_hi.numel() == 0:
        raise ValueError(f"ode_step: one sigma_hi and one sigma_lo per sample of x_hi {tuple(x_hi.shape)}")
    if out is None:
        out = torch.empty_like(x_hi)
    _check(lib.cd_ode_step(x_hi.data_ptr(), d_hi.data_ptr(), _ptr(x_e), _ptr(d_e), sigma_hi.data_ptr(), sigma_lo.data_ptr(),
                           out.data_ptr(), B, x_hi.numel() // B, _stream()))
    return out


def ema_step(dst, src, mu: float):
    """dst[i] <- mu dst[i] + (1 - mu) src[i] over two lists of tensors in ceil(n / 48) launches (cd_ema_step); mu in [0, 1).
    The tensors of ``dst`` are written through raw pointers: their versions are bumped, as FusedAdam does."""
    lib = load_library()
    require_gpu()
    dst, src = list(dst), list(src)
    if not 0.0 <= float(mu) < 1.0:
        raise ValueError(f"ema_step: mu must lie in [0, 1), not {mu}")
    if len(dst) != len(src):
        raise ValueError("ema_step: as many source tensors as destinations")
    for d, s in zip(dst, src):
        for v in (d, s):
            if not (isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32 and v.is_contiguous()):
                raise ValueError("ema_step: contiguous float32 device tensors")
        if d.shape != s.shape:
            raise ValueError(f"ema_step: destination {tuple(d.shape)} and source {tuple(s.shape)} differ in shape")
    n = len(dst)
    if n == 0:
        return
    arr = lambda xs: (C.c_void_p * n)(*[x.data_ptr() for x in xs])  # noqa: E731
    numel = (C.c_int64 * n)(*[d.numel() for d in dst])
    _check(lib.cd_ema_step(n, arr(dst), arr(src), numel, float(mu), _stream()))
    torch.autograd.graph.increment_version(dst)


class Ops:
    """Thin wrappers over the cd_op_* entry points.  Activations are channels-last (B, D, H, W, C)."""

    def __init__(self):
        self.lib = load_library()
        require_gpu()
        self._ws = WorkspaceCache()  # kinds "scratch" and "bwd", both grown on demand

    def scratch(self, batch, channels, voxels):
        return self._ws.get("scratch", (), "cuda", self.lib.cd_op_scratch_bytes(batch, channels, voxels))

    def to_channels_last(self, x):
        x = _dev32(x, "x")
        B, Cc = x.shape[:2]
        vox = int(np.prod(x.shape[2:]))
        y = torch.empty((B,) + tuple(x.shape[2:]) + (Cc,), dtype=torch.float32, device=x.device)
        _check(self.lib.cd_op_to_channels_last(x.data_ptr(), y.data_ptr(), B, Cc, vox, _stream()))
        return y

    def to_ncdhw(self, y):
        y = _dev32(y, "y")
        B, Cc = y.shape[0], y.shape[-1]
        vox = int(np.prod(y.shape[1:-1]))
        x = torch.empty((B, Cc) + tuple(y.shape[1:-1]), dtype=torch.float32, device=y.device)
        _check(self.lib.cd_op_to_ncdhw(y.data_ptr(), x.data_ptr(), B, Cc, vox, _stream()))
        return x

    def cyl_conv(self, x_cl, w, bias, stride=(1, 1, 1), x1_cl=None):
        x_cl, w = _dev32(x_cl, "x"), _dev32(w, "w")
        B, D, H, W, c0 = x_cl.shape
        c1 = 0 if x1_cl is None else x1_cl.shape[-1]
        cout = w.shape[0]
        k = tuple(w.shape[2:])
        if k == (1, 1, 1):
            od = (D, H, W)
        else:
            od = ((D + 2 - k[0]) // stride[0] + 1, (H + 2 - k[1]) // stride[1] + 1, (W + 2 - k[2]) // stride[2] + 1)
        y = torch.empty((B,) + od + (cout,), dtype=torch.float32, device=x_cl.device)
        sc = self.scratch(B, max(c0 + c1, cout), D * H * W)
        _check(self.lib.cd_op_cyl_conv(x_cl.data_ptr(), c0, _ptr(x1_cl), c1, w.data_ptr(), _ptr(bias), y.data_ptr(), B, cout,
                                       _i32x3((D, H, W)), _i32x3(k), _i32x3(stride), sc.data_ptr(), _stream()))
        return y

    def zslide_conv_chunked(self, x_cl, w, bias, chunks=0):
        """3x3x3 conv through the z-slide kernel with every sample dealt in `chunks` chunks (0: the launcher's choice).  Returns
        (y, stats): stats [B][cout][2] = the kernel's channel partials {sum, sum of squares} of y, added up in fp64."""
        x_cl, w = _dev32(x_cl, "x"), _dev32(w, "w")
        B, D, H, W, cin = x_cl.shape
        cout = w.shape[0]
        y = torch.empty((B, D, H, W, cout), dtype=torch.float32, device=x_cl.device)
        cap = (D * H * W + 31) // 32
        part = torch.zeros((B, cap, cout, 2), dtype=torch.float32, device=x_cl.device)
        units = C.c_int()
        sc = self.scratch(B, max(cin, cout), D * H * W)
        _check(self.lib.cd_op_zslide_conv(x_cl.data_ptr(), cin, w.data_ptr(), _ptr(bias), y.data_ptr(), part.data_ptr(), C.byref(units),
                                          B, cout, _i32x3((D, H, W)), int(chunks), sc.data_ptr(), _stream()))
        u = units.value  # (the partials are packed [B][units][cout][2] at the front of the buffer)
        return y, part.view(-1)[:B * u * cout * 2].view(B, u, cout, 2).double().sum(1)

    def cyl_conv_transpose(self, x_cl, w, bias, kernel_z, stride_z, out_pad):
        x_cl, w = _dev32(x_cl, "x"), _dev32(w, "w")
        B, D, H, W, c = x_cl.shape
        od = ((D - 1) * stride_z - 2 + kernel_z, 2 * H + out_pad[1], 2 * W + out_pad[2])
        y = torch.empty((B,) + od + (c,), dtype=torch.float32, device=x_cl.device)
        sc = self.scratch(B, c, int(np.prod(od)))
        _check(self.lib.cd_op_cyl_conv_transpose(x_cl.data_ptr(), w.data_ptr(), _ptr(bias), y.data_ptr(), B, c,
                                                 _i32x3((D, H, W)), kernel_z, stride_z, _i32x3(out_pad), sc.data_ptr(),
                                                 _stream()))
        return y

    def init_conv(self, x_ncdhw, w, bias):
        x, w = _dev32(x_ncdhw, "x"), _dev32(w, "w")
        B, cin, D, H, W = x.shape
        cout = w.shape[0]
        y = torch.empty((B, D, H, W, cout), dtype=torch.float32, device=x.device)
        sc = self.scratch(B, cout, D * H * W)
        _check(self.lib.cd_op_init_conv(x.data_ptr(), w.data_ptr(), _ptr(bias), y.data_ptr(), B, cin, cout, _i32x3((D, H, W)),
                                        sc.data_ptr(), _stream()))
        return y

    def init_pair_conv(self, x, w0, b0, w1, b1, profiles=None, scale=None, slabs=0, y=None, part=None):
        """The init conv followed by a 32 -> 32 3x3x3 conv as the one composed 5x5x5 launch.  x: (B, D, H, W), the data channel;
        w0 (32, cin, 3, 3, 3) with cin = 1 + coordinate channels; profiles = (r_w, z_d, phi_h, use_rz, use_phi) or None; scale:
        (B,) per-sample multiplier of x or None.  y (B, D, H, W, 32) and part (>= B * D * 64 floats) may be the caller's own
        (guard-band tests).  Returns (y, stats, units), stats as zslide_conv_chunked's."""
        x, w0, w1 = _dev32(x, "x"), _dev32(w0, "w0"), _dev32(w1, "w1")
        B, D, H, W = x.shape
        cin = w0.shape[1]
        if y is None:
            y = torch.empty((B, D, H, W, 32), dtype=torch.float32, device=x.device)
        if part is None:
            part = torch.zeros((B * D * 64,), dtype=torch.float32, device=x.device)
        r_w, z_d, phi_h, use_rz, use_phi = profiles if profiles is not None else (None, None, None, 0, 0)
        units = C.c_int()
        sc = self.scratch(B, 32, D * H * W)
        _check(self.lib.cd_op_init_pair_conv(x.data_ptr(), w0.data_ptr(), _ptr(b0), w1.data_ptr(), _ptr(b1), cin, _ptr(r_w), _ptr(z_d),
                                             _ptr(phi_h), int(use_rz), int(use_phi), _ptr(scale), y.data_ptr(), part.data_ptr(),
                                             C.byref(units), B, _i32x3((D, H, W)), int(slabs), sc.data_ptr(), _stream()))
        u = units.value
        return y, part.view(-1)[:B * u * 64].view(B, u, 32, 2).double().sum(1), u

    def group_norm(self, x_cl, gamma, beta, groups, silu=False, add_bc=None, residual=None):
        x = _dev32(x_cl, "x")
        B, Cc = x.shape[0], x.shape[-1]
        vox = int(np.prod(x.shape[1:-1]))
        y = torch.empty_like(x)
        sc = self.scratch(B, Cc, vox)
        _check(self.lib.cd_op_group_norm(x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), B, Cc, vox, groups,
                                         int(silu), _ptr(add_bc), _ptr(residual), sc.data_ptr(), _stream()))
        return y

    def _bws(self, nbytes=1 << 30):
        return self._ws.get("bwd", (), "cuda", nbytes)

    def conv_backward(self, x_cl, w, dy_cl, stride=(1, 1, 1), x1_cl=None, need_dx=True, bias=True):
        """Gradients (dx, dw, db) of cyl_conv; channels-last activations, torch-layout weights."""
        x, w, dy = _dev32(x_cl, "x"), _dev32(w, "w"), _dev32(dy_cl, "dy")
        B, D, H, W, c0 = x.shape
        c1 = 0 if x1_cl is None else x1_cl.shape[-1]
        cout, k = w.shape[0], tuple(w.shape[2:])
        dx = torch.empty((B, D, H, W, c0 + c1), dtype=torch.float32, device=x.device) if need_dx else None
        dw = torch.empty_like(w)
        db = torch.empty((cout,), dtype=torch.float32, device=x.device) if bias else None
        ws = self._bws()
        _check(self.lib.cd_op_conv_backward(x.data_ptr(), c0, _ptr(x1_cl), c1, w.data_ptr(), dy.data_ptr(), _ptr(dx), dw.data_ptr(),
                                            _ptr(db), B, cout, _i32x3((D, H, W)), _i32x3(k), _i32x3(stride), ws.data_ptr(),
                                            ws.numel(), _stream()))
        return dx, dw, db

    def conv_transpose_backward(self, x_cl, w, dy_cl, kernel_z, stride_z, out_pad):
        x, w, dy = _dev32(x_cl, "x"), _dev32(w, "w"), _dev32(dy_cl, "dy")
        B, D, H, W, c = x.shape
        dx, dw = torch.empty_like(x), torch.empty_like(w)
        db = torch.empty((c,), dtype=torch.float32, device=x.device)
        ws = self._bws()
        _check(self.lib.cd_op_conv_transpose_backward(x.data_ptr(), w.data_ptr(), dy.data_ptr(), dx.data_ptr(), dw.data_ptr(),
                                                      db.data_ptr(), B, c, _i32x3((D, H, W)), kernel_z, stride_z, _i32x3(out_pad),
                                                      ws.data_ptr(), ws.numel(), _stream()))
        return dx, dw, db

    def group_norm_backward(self, x_cl, gamma, beta, dy_cl, groups, silu=False, want_dadd=False):
        x, dy = _dev32(x_cl, "x"), _dev32(dy_cl, "dy")
        B, Cc = x.shape[0], x.shape[-1]
        vox = int(np.prod(x.shape[1:-1]))
        dx, dg, db = torch.empty_like(x), torch.empty_like(gamma), torch.empty_like(beta)
        dadd = torch.empty((B, Cc), dtype=torch.float32, device=x.device) if want_dadd else None
        ws = self._bws()
        _check(self.lib.cd_op_group_norm_backward(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), dy.data_ptr(), dx.data_ptr(),
                                                  dg.data_ptr(), db.data_ptr(), _ptr(dadd), B, Cc, vox, groups, int(silu),
                                                  ws.data_ptr(), ws.numel(), _stream()))
        return dx, dg, db, dadd

    _RES_KEYS = ("block1.proj.conv.weight", "block1.proj.conv.bias", "block1.norm.weight", "block1.norm.bias",
                 "block2.proj.conv.weight", "block2.proj.conv.bias", "block2.norm.weight", "block2.norm.bias",
                 "mlp.1.weight", "mlp.1.bias", "res_conv.conv.weight", "res_conv.conv.bias")

    def resnet_block(self, x_cl, sd: Dict[str, torch.Tensor], cond=None, groups=8, x1_cl=None):
        """ResnetBlock on channels-last input; ``sd`` uses the reference's key names (models.py:172-200)."""
        x = _dev32(x_cl, "x")
        B, D, H, W, c0 = x.shape
        c1 = 0 if x1_cl is None else x1_cl.shape[-1]
        cout = sd["block1.proj.conv.weight"].shape[0]
        ptrs = (_P * 12)(*[(sd[k].data_ptr() if k in sd else None) for k in self._RES_KEYS])
        y = torch.empty((B, D, H, W, cout), dtype=torch.float32, device=x.device)
        nbytes = self.lib.cd_op_scratch_bytes(B, max(c0 + c1, cout), D * H * W) + 4 * B * D * H * W * cout * 4 * 4
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        _check(self.lib.cd_op_resnet_block(x.data_ptr(), c0, _ptr(x1_cl), c1, ptrs, _ptr(cond), y.data_ptr(), B, cout,
                                           _i32x3((D, H, W)), groups, ws.data_ptr(), ws.numel(), _stream()))
        return y

    _ATTN_KEYS = ("fn.norm.weight", "fn.norm.bias", "fn.fn.to_qkv.conv.weight", "fn.fn.to_out.0.conv.weight",
                  "fn.fn.to_out.0.conv.bias", "fn.fn.to_out.1.weight", "fn.fn.to_out.1.bias")

    def linear_attention(self, x_cl, sd: Dict[str, torch.Tensor]):
        """Residual(PreNorm(LinearAttention)) on channels-last input (models.py:281-329)."""
        x = _dev32(x_cl, "x")
        B, D, H, W, c = x.shape
        ptrs = (_P * 7)(*[sd[k].data_ptr() for k in self._ATTN_KEYS])
        y = torch.empty_like(x)
        nbytes = self.lib.cd_op_scratch_bytes(B, 96, D * H * W) + 4 * B * D * H * W * 96 * 4
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        _check(self.lib.cd_op_linear_attention(x.data_ptr(), ptrs, y.data_ptr(), B, c, _i32x3((D, H, W)), ws.data_ptr(),
                                               ws.numel(), _stream()))
        return y
