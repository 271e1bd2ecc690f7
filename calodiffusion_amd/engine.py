"""The engines: the objects that own a plan of the HIP library and call it (``UnetEngine``, ``LayerMlpEngine``).  The ctypes
binding they stand on is ``abi.py``, the primitive-op wrappers are ``ops.py``; both are re-imported here by name, so
``engine.<name>`` keeps reaching everything it always did.

PyTorch is used here for device memory, streams and parameter storage only.  There is no fallback of
any kind: if the library is missing, or no gfx950 GPU is visible, every compute entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from .abi import (CD_ABI_VERSION, CD_MAX_SIZES, EXPORTED_SYMBOLS, LIB_PATH, LOSS_TYPES, OBJECTIVES, SOP_DENOISE, SOP_DENOISE_PS,
                  SOP_LINCOMB, SOP_LINDIV, SOP_RANDN, SOP_RECORD, TIME_KINDS, CdClassifierDesc, CdGeneratorRun, CdHlfDesc,
                  CdLayerMlpDesc, CdSamplerOp, CdShowerStatsDesc, CdStep, CdUnetDesc, Handle, WorkspaceCache, _P, _SIGNATURES, _check,
                  _check_built_from_these_sources, _dev32, _i32x3, _nbytes, _ptr, _stream, get_conv_precision, load_library,
                  profile_begin, profile_end, randn, require_gpu, set_conv_precision)
from .hgcal import HGCalConverter
from .ops import Ops


def _sigma_b(sigma, B: int) -> torch.Tensor:
    """sigma as a flat fp32 device tensor; a single value stands for the whole batch."""
    sigma = _dev32(sigma, "sigma").reshape(-1)
    if sigma.numel() == 1 and B > 1:
        sigma = sigma.expand(B).contiguous()
    return sigma


def _pack_ops(program) -> np.ndarray:
    """program.ops as int32 rows in CdSamplerOp's field order (kind, dst, nsrc, src[6], col)."""
    ops = np.zeros((len(program.ops), C.sizeof(CdSamplerOp) // 4), dtype=np.int32)
    for row, (kind, dst, src, col) in zip(ops, program.ops):
        row[0], row[1], row[2], row[9] = kind, dst, len(src), col
        row[3:3 + len(src)] = src
    return ops


def _trajectories(start, n_steps: int, want_xs: bool, want_x0s: bool, zeroed: bool):
    """The (n_steps,) + start.shape trajectory tensors a sampler entry point fills, None where not wanted."""
    new = torch.zeros if zeroed else torch.empty
    shape = (n_steps,) + tuple(start.shape)
    return tuple(new(shape, dtype=torch.float32, device=start.device) if want else None for want in (want_xs, want_x0s))


def _program_io(start, program, n_steps: int, step_noise, debug: bool, what: str):
    """What both sampler_run methods derive from a program: the trajectories its RECORD ops fill (``debug`` only; zeroed, a
    program need not record every step) and the checked step_noise."""
    recorded = {d for k, d, _, _ in program.ops if k == SOP_RECORD}
    xs, x0s = _trajectories(start, n_steps, debug and 0 in recorded, debug and 1 in recorded, zeroed=True)
    if step_noise is not None:
        step_noise = _dev32(step_noise, "step_noise")
        assert step_noise.numel() == program.n_randn * start.numel(), f"step_noise: one {what} tensor per RANDN op executed"
    return xs, x0s, step_noise


def unet_desc(unet, rz_input=False, phi_input=False, time_kind="raw", objective="hybrid", sigma_data=1.0, coords=None) -> CdUnetDesc:
    """The CdUnetDesc of a CondUnet under its ``_engine_opts`` (``coords`` is not part of it).  Needs no GPU."""
    d = CdUnetDesc()
    d.struct_size = C.sizeof(CdUnetDesc)
    d.grid = _i32x3(unet.grid)
    d.in_channels = unet.channels
    d.n_sizes = len(unet.layer_sizes)
    for i, v in enumerate(unet.layer_sizes):
        d.layer_sizes[i] = int(v)
    d.groups = unet.groups
    d.block_attn = int(bool(unet.block_attn))
    d.mid_attn = int(unet.mid_attn is not False)
    d.compress_z = int(bool(unet.compress_Z))
    d.cond_size, d.cond_dim = unet.cond_size, unet.cond_dim
    d.rz_input, d.phi_input = int(bool(rz_input)), int(bool(phi_input))
    d.time_embed_kind = TIME_KINDS[time_kind]
    d.objective = OBJECTIVES[objective]
    d.sigma_data = float(sigma_data)
    d.time_sin, d.cond_sin = int(bool(getattr(unet, "time_embed", False))), int(bool(getattr(unet, "cond_embed", False)))
    return d


def layer_mlp_desc(resnet, time_kind="raw", objective="hybrid", sigma_data=1.0) -> CdLayerMlpDesc:
    """The CdLayerMlpDesc of a ResNet layer model under its ``_engine_opts``.  Needs no GPU."""
    d = CdLayerMlpDesc()
    d.struct_size = C.sizeof(CdLayerMlpDesc)
    d.dim_in, d.hidden, d.cond_emb, d.cond_size = resnet.dim_in, resnet.hidden_dim, resnet.cond_emb_dim, resnet.cond_size
    d.n_res = len(resnet.hidden_layers)
    d.time_embed_kind, d.objective, d.sigma_data = TIME_KINDS[time_kind], OBJECTIVES[objective], float(sigma_data)
    return d


class UnetEngine(Handle):
    """One HIP plan bound to one CondUnet parameter set on one device; the plan is freed with the engine (``abi.Handle``)."""
    plan = property(lambda self: self.handle)

    def __init__(self, unet, rz_input=False, phi_input=False, time_kind="raw", objective="hybrid", sigma_data=1.0,
                 coords=None):
        self.lib = load_library()
        self.device_name = require_gpu()
        self.unet = unet
        d = self.desc = unet_desc(unet, rz_input, phi_input, time_kind, objective, sigma_data)
        self.grid = tuple(unet.grid)
        self.voxels = int(np.prod(self.grid))
        super().__init__(self.lib.cd_plan_destroy)
        _check(self.lib.cd_plan_create(C.byref(d), C.byref(self.handle)))
        self._weights_version = None
        self._weight_order = None  # [(state_dict name, tensor)] in the plan's order
        self._weight_ids = None
        self._held_weights = []
        self._ws = WorkspaceCache()  # kinds "net", "sampler", "train", "vjp", "bns"; every key starts with _ws_key(batch)
        self._grad_layout = None
        self.range_fallbacks = 0
        self.embedding = None  # set_embedding: the NNConverter / HGCalConverter whose enc / dec run inside the denoise-based calls
        self._rmap = self._enc_flat = self._dec_flat = self._gmaps = self._embed_version = None
        self.state_shape = (1,) + self.grid  # per-sample state of those calls
        self.device = next(unet.parameters()).device
        if self.device.type != "cuda":
            raise RuntimeError("move the model to the GPU first (model.to('cuda')): calodiffusion_amd has no CPU path")
        if coords is not None:
            r, z, phi = (np.ascontiguousarray(a, dtype=np.float32) for a in coords)
            assert len(r) == self.grid[2] and len(z) == self.grid[0] and len(phi) == self.grid[1]
            _check(self.lib.cd_plan_set_coords(self.plan, r.ctypes.data, z.ctypes.data, phi.ctypes.data, _stream()))
        self.sync_weights(force=True)

    @classmethod
    def for_unet(cls, unet):
        opts = getattr(unet, "_engine_opts", {})
        return cls(unet, **opts)

    # ------------------------------------------------------------------ weights
    def _version(self):
        ps = list(self.unet.parameters())
        return tuple(p._version for p in ps) + tuple(p.data_ptr() for p in ps) + (tuple(id(p) for p in ps),)

    def _plan_weights(self):
        """[(state_dict name, numel)] of the plan's weight tensors, in the plan's order."""
        n = C.c_int()
        _check(self.lib.cd_plan_num_weights(self.plan, C.byref(n)))
        buf = C.create_string_buffer(256)
        numel = C.c_int64()
        out = []
        for i in range(n.value):
            _check(self.lib.cd_plan_weight_name(self.plan, i, buf, 256, C.byref(numel)))
            out.append((buf.value.decode(), numel.value))
        return out

    # ------------------------------------------------------------------ flat-state embedding
    def set_embedding(self, nn_embed):
        """Bind a geometry embedding (None: unbind) to the plan: the state of denoise, the samplers, the loss, train_step and
        denoise_vjp becomes the flat shower.  A ``geom1.NNConverter`` (cd_plan_set_radial): state (B, V); the per-layer
        ``encs[i].weight`` / ``decs[i].weight`` are gathered into two device buffers the plan reads in place.  An
        ``hgcal.HGCalConverter`` (cd_plan_set_geom): state (B, 1, layers, cells); the plan reads the converter's two packed maps,
        whose values follow a trainable converter's parameters.  Either is refreshed whenever a weight changed (sync_weights)."""
        self._grad_layout = None
        self._ws.clear()
        self._embed_version = None
        self._rmap = self._enc_flat = self._dec_flat = self._gmaps = None
        if nn_embed is None:
            _check(self.lib.cd_plan_set_radial(self.plan, None, None, None, 0, _stream()))  # (clears either kind)
            self.embedding, self.state_shape = None, (1,) + self.grid
            return
        if isinstance(nn_embed, HGCalConverter):
            have = (nn_embed.num_layers, nn_embed.num_alpha_bins, nn_embed.num_r_bins)
            if have != self.grid:
                raise ValueError(f"the embedding maps onto the grid {have}, the U-Net runs on {self.grid}")
            if nn_embed.norm:
                raise ValueError("an in-model HGCalConverter has no norm (the reference calls init(norm=pre_embed), "
                                 "calodiffusion.py:117): bind a converter initialised with norm=False")
            self.embedding, self.state_shape = nn_embed, (1, have[0], int(nn_embed.embeder.mat.shape[-1]))
        else:
            rmap = nn_embed.gc.radial_map()
            if (rmap.L, rmap.A, rmap.R) != self.grid:
                raise ValueError(f"the embedding maps onto the grid {(rmap.L, rmap.A, rmap.R)}, the U-Net runs on {self.grid}")
            self._rmap = rmap  # (the plan reads the handle: kept alive here)
            self._enc_flat = torch.empty(rmap.wtotal, dtype=torch.float32, device=self.device)
            self._dec_flat = torch.empty(rmap.wtotal, dtype=torch.float32, device=self.device)
            self.embedding, self.state_shape = nn_embed, (rmap.V,)
        self._sync_embedding()

    def _check_state(self, x, name, what="x"):
        """The per-sample state is the grid, or with an embedding the flat shower: a tensor of the other form would be read and
        written with the wrong size on the device."""
        if tuple(x.shape[1:]) != self.state_shape:
            raise ValueError(f"{name}: {what} has shape {tuple(x.shape)}, expected (B,) + {self.state_shape}")

    def _embed_is_geom(self) -> bool:
        return self.embedding is not None and self._rmap is None

    def _embed_params(self):
        """[(name in grad_layout, parameter)] of the bound embedding, in the order of its ``parameters()``"""
        if self._embed_is_geom():
            return [(f"NN_embed.{k}", p) for k, p in self.embedding.named_parameters()]
        return ([(f"NN_embed.encs.{i}", lay.weight) for i, lay in enumerate(self.embedding.encs)] +
                [(f"NN_embed.decs.{i}", lay.weight) for i, lay in enumerate(self.embedding.decs)])

    def embedding_trains(self) -> bool:
        return self.embedding is not None and any(p.requires_grad for _, p in self._embed_params())

    def _sync_embedding(self):
        if self._embed_is_geom():
            # packed(): packs on first use, gathers the values again when a trainable parameter changed (one launch); the plan
            # reads the handles in place, so only a new handle or a change of the gradient flag is a call
            enc, dec = self.embedding.embeder.packed(), self.embedding.decoder.packed()
            ver = (enc.handle.value, dec.handle.value, self.embedding_trains())
            if ver != self._embed_version:
                _check(self.lib.cd_plan_set_geom(self.plan, enc.handle, dec.handle, int(ver[-1]), _stream()))
                self._gmaps = (enc, dec)  # (kept alive here)
                self._grad_layout = None  # (frozen maps have no gradient slots)
                self._ws.drop("train", "vjp")
                self._embed_version = ver
            return
        ps = [p for _, p in self._embed_params()]
        ver = tuple(p._version for p in ps) + tuple(p.data_ptr() for p in ps) + (self.embedding_trains(),)
        if ver == self._embed_version:
            return
        n = len(self.embedding.encs)
        torch.cat([p.detach().reshape(-1).to(device=self.device, dtype=torch.float32) for p in ps[:n]], out=self._enc_flat)
        torch.cat([p.detach().reshape(-1).to(device=self.device, dtype=torch.float32) for p in ps[n:]], out=self._dec_flat)
        # (the plan reads the two buffers in place: only a first binding or a change of the gradient flag is a call, which
        # synchronises and drops the cached step graphs)
        if self._embed_version is None or self._embed_version[-1] != ver[-1]:
            _check(self.lib.cd_plan_set_radial(self.plan, self._rmap.handle, self._enc_flat.data_ptr(), self._dec_flat.data_ptr(),
                                               int(ver[-1]), _stream()))
        self._embed_version = ver

    def sync_weights(self, force=False):
        """(Re-)pack the parameters into the plan's arena; cheap no-op when nothing changed.  All tensors go in ONE C-ABI call
        (cd_plan_set_weights: two launches); the plan's tensor order and the Parameter objects behind it are looked up once (and
        again whenever a Parameter object of the module is replaced)."""
        if self.embedding is not None:
            self._sync_embedding()
        ver = self._version()
        if not force and ver == self._weights_version:
            return
        ids = ver[-1]
        if self._weight_order is None or self._weight_ids != ids:
            sd = self.unet.state_dict(keep_vars=True)
            order = []
            for name, numel in self._plan_weights():
                if name not in sd:
                    raise RuntimeError(f"state_dict has no tensor named {name!r}")
                if sd[name].numel() != numel:
                    raise RuntimeError(f"{name}: {sd[name].numel()} elements, HIP plan expects {numel}")
                order.append((name, sd[name]))
            missing = set(sd) - {name for name, _ in order}
            if missing:
                raise RuntimeError(f"HIP plan does not consume these state_dict tensors: {sorted(missing)[:5]} ...")
            self._weight_order, self._weight_ids = order, ids
        tensors = [_dev32(t.detach(), name) for name, t in self._weight_order]
        ptrs = (_P * len(tensors))(*[t.data_ptr() for t in tensors])
        _check(self.lib.cd_plan_set_weights(self.plan, len(tensors), ptrs, _stream()))
        self._held_weights = tensors  # (conversions made by _dev32 must outlive the launches)
        self._weights_version = ver

    # launch-sequence switches the library reads per call (tests and A/B runs flip them inside one process): a workspace sized
    # under one setting is not valid under another, so they are part of every cache key.  (The arithmetic mode is not: the
    # library sizes for the largest of its three modes.)
    _WS_SWITCHES = ("CD_NO_DEEP_LEVEL", "CD_NO_PW_CLOSE", "CD_NO_FUSED_ATTN", "CD_NO_GNDEFER", "CD_ATTN_COMBINE_LAUNCH", "CD_PW_F32",
                    "CD_NO_ATTN_MOMENTS", "CD_ATTN_MOM_MIN", "CD_NO_DEEP_SIDE_CONV")

    def _ws_key(self, batch: int):
        return (int(batch),) + tuple(os.environ.get(k) for k in self._WS_SWITCHES)

    def workspace(self, batch: int) -> torch.Tensor:
        return self._ws.get("net", self._ws_key(batch), self.device,
                            lambda: _nbytes(self.lib.cd_plan_workspace_bytes, self.plan, batch))

    # ------------------------------------------------------------------ compute
    def unet_forward(self, x, cond, time):
        x, cond, time = _dev32(x, "x"), _dev32(cond, "cond"), _dev32(time, "time")
        B = x.shape[0]
        if tuple(x.shape[1:]) != (self.unet.channels,) + self.grid:
            raise ValueError(f"x has shape {tuple(x.shape)}, expected (B, {self.unet.channels}, {self.grid})")
        if self.desc.cond_sin:  # sinusoidal cond embedding: one scalar per sample (models.py:132-144 broadcasts a (B,) tensor)
            if cond.numel() != B:
                raise ValueError("cond_embed='sin' takes cond of shape (B,)")
        elif cond.shape != (B, self.unet.cond_size):
            raise ValueError("cond must be (B, cond_size)")
        if time.numel() != B:
            raise ValueError("time must be (B,)")
        self.sync_weights()
        ws = self.workspace(B)
        out = torch.empty((B, 1) + self.grid, dtype=torch.float32, device=x.device)
        _check(self.lib.cd_unet_forward(self.plan, B, x.data_ptr(), cond.data_ptr(), time.data_ptr(), out.data_ptr(),
                                        ws.data_ptr(), ws.numel(), _stream()))
        return out

    # denoise() recovers from an fp16-range overflow by itself (cd_denoise_safe: one stream synchronisation per call to read the
    # flag, then a full-range re-run if it was raised) so that samplers calling the model back from Python never die
    # mid-trajectory; set False for the asynchronous, graph-capturable cd_denoise, whose overflow only shows in check_status().
    safe_denoise = True

    def denoise(self, x, sigma, cond):
        x, cond = _dev32(x, "x"), _dev32(cond, "cond")
        B = x.shape[0]
        sigma = _sigma_b(sigma, B)
        if tuple(x.shape[1:]) != self.state_shape or sigma.numel() != B or cond.shape != (B, self.unet.cond_size):
            raise ValueError(f"denoise shapes: x {tuple(x.shape)} (expected (B,) + {self.state_shape}), sigma {tuple(sigma.shape)}, "
                             f"cond {tuple(cond.shape)}")
        self.sync_weights()
        ws = self.workspace(B)
        out = torch.empty_like(x)
        if self.safe_denoise:
            fell = C.c_int(0)
            _check(self.lib.cd_denoise_safe(self.plan, B, x.data_ptr(), sigma.data_ptr(), cond.data_ptr(), out.data_ptr(),
                                            ws.data_ptr(), ws.numel(), C.byref(fell), _stream()))
            if fell.value:
                self.range_fallbacks += 1
        else:
            _check(self.lib.cd_denoise(self.plan, B, x.data_ptr(), sigma.data_ptr(), cond.data_ptr(), out.data_ptr(),
                                       ws.data_ptr(), ws.numel(), _stream()))
        return out

    def ddim_sample(self, start, cond, steps: np.ndarray, step_noise=None, seed=0, offset=0, debug=False, use_graph=True,
                    out=None, noise_stride=0):
        """steps: float32 array (n_steps, 4) = (sigma, sigma_prev*[t>0], ddim_sigma, denom).  noise_stride: Philox stream
        distance between the noise tensors of consecutive steps (0 = this batch's own size; a batch shard passes the global
        tensor size so that the union of the shards is the single-GPU result)."""
        start, cond = _dev32(start, "start"), _dev32(cond, "cond")
        B = start.shape[0]
        self._check_state(start, "ddim_sample", "start")
        steps = np.ascontiguousarray(steps, dtype=np.float32)
        n_steps = steps.shape[0]
        assert steps.shape == (n_steps, 4)
        self.sync_weights()
        ws = self.workspace(B)
        x_out = torch.empty_like(start) if out is None else out
        xs, x0s = _trajectories(start, n_steps, debug, debug, zeroed=False)
        if step_noise is not None:
            step_noise = _dev32(step_noise, "step_noise")
            assert step_noise.shape[0] == n_steps and step_noise[0].numel() == start.numel()
        _check(self.lib.cd_ddim_sample(self.plan, B, start.data_ptr(), cond.data_ptr(),
                                       steps.ctypes.data_as(C.POINTER(CdStep)), n_steps, _ptr(step_noise), int(seed),
                                       int(offset), int(noise_stride), x_out.data_ptr(), _ptr(xs), _ptr(x0s),
                                       int(bool(use_graph)), ws.data_ptr(), ws.numel(), _stream()))
        self.check_status()
        return x_out, xs, x0s

    def sampler_run(self, start, cond, program, step_noise=None, seed=0, offset=0, noise_stride=0, debug=False, use_graph=True):
        """Run a sampler step program (calodiffusion_amd.sample.Program) on the device loop (cd_sampler_run).
        Returns (x, xs, x0s); the trajectories (n_steps, B, 1, D, H, W) only when ``debug`` and the program records them."""
        start, cond = _dev32(start, "start"), _dev32(cond, "cond")
        B = start.shape[0]
        self._check_state(start, "sampler_run", "start")
        coefs = np.ascontiguousarray(program.coefs, dtype=np.float32)
        n_steps, n_coef = coefs.shape
        ops = _pack_ops(program)
        op_begin = None
        if program.op_begin is not None:
            assert len(program.op_begin) == n_steps + 1
            op_begin = (C.c_int32 * (n_steps + 1))(*program.op_begin)
        self.sync_weights()
        # (the size follows the program as well as the batch: kept while it is large enough)
        ws = self._ws.get("sampler", self._ws_key(B), self.device,
                          _nbytes(self.lib.cd_plan_sampler_workspace_bytes, self.plan, B, program.n_bufs, n_steps, n_coef))
        x_out = torch.empty_like(start)
        xs, x0s, step_noise = _program_io(start, program, n_steps, step_noise, debug, "(B,1,D,H,W)")
        _check(self.lib.cd_sampler_run(self.plan, B, start.data_ptr(), float(program.start_scale), cond.data_ptr(), program.n_bufs,
                                       n_steps, ops.ctypes.data_as(C.POINTER(CdSamplerOp)), len(program.ops), op_begin,
                                       coefs.ctypes.data, n_coef, _ptr(step_noise), int(seed), int(offset), int(noise_stride),
                                       x_out.data_ptr(), _ptr(xs), _ptr(x0s), int(bool(use_graph)), ws.data_ptr(), ws.numel(), _stream()))
        self.check_status()
        return x_out, xs, x0s

    def check_status(self):
        """Raise if a compute call since the last check left the fp16 range of the f16x2 convolution path (synchronises).
        The sampler entry points recover by themselves (bf16x3 re-run of the trajectory): that only sets ``range_fallbacks``."""
        flags = C.c_int(0)
        _check(self.lib.cd_plan_status(self.plan, C.byref(flags), _stream()))
        if flags.value & 2:
            self.range_fallbacks += 1
        if flags.value & 1:
            raise FloatingPointError("calodiff: an activation exceeded the fp16 range of the f16x2 convolution kernels "
                                     "(outputs contain inf/NaN); set CD_CONV_PRECISION=bf16x3 for the full fp32 range")

    # ------------------------------------------------------------------ training
    def grad_layout(self):
        """{state_dict name: (offset, numel)} into the flat gradient buffer, and its total length."""
        if self._grad_layout is None:
            off, total = C.c_int64(), C.c_int64()
            weights = self._plan_weights()
            lay = {}
            for i, (name, numel) in enumerate(weights):
                _check(self.lib.cd_plan_grad_layout(self.plan, i, C.byref(off), C.byref(total)))
                lay[name] = (off.value, numel)
            # the embedding's two blocks follow the U-Net's (cd_plan_set_radial; cd_plan_set_geom when its maps train)
            if self.embedding is not None and (not self._embed_is_geom() or self.embedding_trains()):
                sizes = ((self._rmap.wtotal,) * 2 if not self._embed_is_geom() else
                         (self.embedding.embeder.mat.numel(), self.embedding.decoder.mat.numel()))
                for k, name in enumerate(("NN_embed.encs", "NN_embed.decs")):
                    _check(self.lib.cd_plan_grad_layout(self.plan, len(weights) + k, C.byref(off), C.byref(total)))
                    lay[name] = (off.value, sizes[k])
            self._grad_layout = (lay, total.value)
        return self._grad_layout

    def train_workspace(self, batch: int) -> torch.Tensor:
        return self._ws.get("train", self._ws_key(batch), self.device,
                            lambda: _nbytes(self.lib.cd_plan_train_workspace_bytes, self.plan, batch))

    def _loss_io(self, data, noise, sigma, cond, name):
        """The checked arguments of train_step and loss_hybrid, and the batch size."""
        data, noise, cond = _dev32(data, "data"), _dev32(noise, "noise"), _dev32(cond, "cond")
        sigma = _dev32(sigma, "sigma").reshape(-1)
        B = data.shape[0]
        self._check_state(data, name, "data")
        if noise.shape != data.shape or sigma.numel() != B:
            raise ValueError(f"{name}: noise {tuple(noise.shape)} must have data's shape and sigma {tuple(sigma.shape)} B elements")
        return data, noise, sigma, cond, B

    def train_step(self, data, noise, sigma, cond, loss_type="l2"):
        """hybrid_weight loss (LOSS_TYPE l2 / l1 / mse / huber) and the gradient of every parameter (flat fp32 buffer, see
        grad_layout)."""
        data, noise, sigma, cond, B = self._loss_io(data, noise, sigma, cond, "train_step")
        self.sync_weights()
        ws = self.train_workspace(B)
        _, total = self.grad_layout()
        flat = torch.empty(total, dtype=torch.float32, device=data.device)
        loss = torch.empty((), dtype=torch.float64, device=data.device)
        _check(self.lib.cd_train_step(self.plan, B, data.data_ptr(), noise.data_ptr(), sigma.data_ptr(), cond.data_ptr(),
                                      LOSS_TYPES[loss_type], loss.data_ptr(), flat.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        return loss, flat

    def train_step_target(self, data, noise, sigma, cond, target, loss_type="mse"):
        """train_step against a given target (cd_train_step_target: consistency distillation): the loss compares
        denoise(data + sigma noise) with ``target`` (a constant of data's shape), residual out - target and weight 1 for every
        objective; LOSS_TYPE mse / l1 / huber.  Returns (loss, flat gradient) as train_step does, from the same workspace."""
        if loss_type == "l2":
            raise ValueError("train_step_target: the weighted 'l2' loss has no meaning against a given target, use 'mse'")
        data, noise, sigma, cond, B = self._loss_io(data, noise, sigma, cond, "train_step_target")
        target = _dev32(target, "target")
        if target.shape != data.shape:
            raise ValueError(f"train_step_target: target {tuple(target.shape)} must have data's shape {tuple(data.shape)}")
        self.sync_weights()
        ws = self.train_workspace(B)
        _, total = self.grad_layout()
        flat = torch.empty(total, dtype=torch.float32, device=data.device)
        loss = torch.empty((), dtype=torch.float64, device=data.device)
        _check(self.lib.cd_train_step_target(self.plan, B, data.data_ptr(), noise.data_ptr(), sigma.data_ptr(), cond.data_ptr(),
                                             target.data_ptr(), LOSS_TYPES[loss_type], loss.data_ptr(), flat.data_ptr(),
                                             ws.data_ptr(), ws.numel(), _stream()))
        return loss, flat

    def vjp_workspace(self, batch: int, with_param_grads: bool) -> torch.Tensor:
        """Workspace of cd_denoise_vjp."""
        mode = bool(with_param_grads)
        return self._ws.get("vjp", self._ws_key(batch) + (mode,), self.device,
                            lambda: _nbytes(self.lib.cd_plan_vjp_workspace_bytes, self.plan, batch, int(mode)))

    def denoise_vjp(self, x, sigma, cond, gy, param_grads: bool):
        """Vector-Jacobian product of denoise (cd_denoise_vjp): dx = dL/dx for gy = dL/dD, and with ``param_grads`` the
        gradient of every parameter as a flat fp32 buffer (see grad_layout), else None.  sigma and cond are constants."""
        x, cond, gy = _dev32(x, "x"), _dev32(cond, "cond"), _dev32(gy, "gy")
        B = x.shape[0]
        sigma = _sigma_b(sigma, B)
        if (tuple(x.shape[1:]) != self.state_shape or gy.shape != x.shape or sigma.numel() != B
                or cond.shape != (B, self.unet.cond_size)):
            raise ValueError(f"denoise_vjp shapes: x {tuple(x.shape)}, gy {tuple(gy.shape)}, sigma {tuple(sigma.shape)}, "
                             f"cond {tuple(cond.shape)}")
        self.sync_weights()
        ws = self.vjp_workspace(B, param_grads)
        dx = torch.empty_like(x)
        flat = None
        if param_grads:
            _, total = self.grad_layout()
            flat = torch.empty(total, dtype=torch.float32, device=x.device)
        _check(self.lib.cd_denoise_vjp(self.plan, B, x.data_ptr(), sigma.data_ptr(), cond.data_ptr(), gy.data_ptr(), dx.data_ptr(),
                                       _ptr(flat), ws.data_ptr(), ws.numel(), _stream()))
        return dx, flat

    def bns_workspace(self, batch: int, n_steps: int) -> torch.Tensor:
        """Workspace of cd_bns_theta_grad."""
        return self._ws.get("bns", self._ws_key(batch) + (int(n_steps),), self.device,
                            lambda: _nbytes(self.lib.cd_plan_bns_workspace_bytes, self.plan, batch, n_steps))

    def bns_theta_grad(self, data, cond, theta, sigma):
        """BespokeNonStationary training loss and its gradient with respect to theta (cd_bns_theta_grad): the chain
        x_0 = data, x_{i+1} = x_i a_i + denoise(x_i, sigma_i) b_i, loss = mean(20 log10(max(data, -1) / sqrt(mse(data, x_N)))).
        theta (2, N); sigma (N, B).  Returns (loss: 0-d fp64 tensor, dtheta: (2, N) fp32), both on the device."""
        data, cond = _dev32(data, "data"), _dev32(cond, "cond")
        theta, sigma = _dev32(theta.detach(), "theta"), _dev32(sigma, "sigma")
        B = data.shape[0]
        N = theta.shape[1] if theta.dim() == 2 else -1
        if (tuple(data.shape[1:]) != (1,) + self.grid or theta.shape != (2, N) or tuple(sigma.shape) != (N, B)
                or cond.shape != (B, self.unet.cond_size)):
            raise ValueError(f"bns_theta_grad shapes: data {tuple(data.shape)}, theta {tuple(theta.shape)}, sigma {tuple(sigma.shape)}, "
                             f"cond {tuple(cond.shape)}")
        self.sync_weights()
        ws = self.bns_workspace(B, N)
        loss = torch.empty((), dtype=torch.float64, device=data.device)
        dtheta = torch.empty((2, N), dtype=torch.float32, device=data.device)
        _check(self.lib.cd_bns_theta_grad(self.plan, B, N, data.data_ptr(), cond.data_ptr(), theta.data_ptr(), sigma.data_ptr(),
                                          loss.data_ptr(), dtheta.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        return loss, dtheta

    def param_grads(self, flat):
        """Views of the flat gradient buffer, one per parameter of the bound CondUnet, in .parameters() order; with an embedding,
        its ``encs[i].weight`` and then its ``decs[i].weight`` follow (the order of ``NNConverter.parameters()``), or a trainable
        ``HGCalConverter``'s ``embeder.mat`` and ``decoder.mat`` (None for both while neither requires a gradient: no slots)."""
        lay, _ = self.grad_layout()
        out = []
        for name, p in self.unet.named_parameters():
            off, numel = lay[name]
            out.append(flat[off:off + numel].view(p.shape))
        if self._embed_is_geom():  # the two dense maps of a trainable HGCalConverter; a frozen one has no parameters
            for name, mod in (("NN_embed.encs", self.embedding.embeder), ("NN_embed.decs", self.embedding.decoder)):
                if mod.trainable:
                    out.append(flat[lay[name][0]:lay[name][0] + lay[name][1]].view(mod.mat.shape) if name in lay else None)
        elif self.embedding is not None:
            for name, layers in (("NN_embed.encs", self.embedding.encs), ("NN_embed.decs", self.embedding.decs)):
                off = lay[name][0]
                for layer in layers:
                    out.append(flat[off:off + layer.weight.numel()].view(layer.weight.shape))
                    off += layer.weight.numel()
        return out

    def loss_hybrid(self, data, noise, sigma, cond, loss_type="l2"):
        data, noise, sigma, cond, B = self._loss_io(data, noise, sigma, cond, "loss_hybrid")
        self.sync_weights()
        ws = self.workspace(B)
        out = torch.empty((), dtype=torch.float64, device=data.device)
        _check(self.lib.cd_loss_hybrid(self.plan, B, data.data_ptr(), noise.data_ptr(), sigma.data_ptr(), cond.data_ptr(),
                                       LOSS_TYPES[loss_type], out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        return out

    def loss_hybrid_l2(self, data, noise, sigma, cond):
        return self.loss_hybrid(data, noise, sigma, cond, "l2")


class LayerMlpEngine:
    """The layer-energy MLP of LayerDiffusion on the HIP library (cd_layer_forward / cd_layer_denoise / cd_layer_sample /
    cd_layer_sampler_run; cd_layer_train_step_loss / cd_layer_loss / cd_layer_denoise_vjp).
    Stateless on the library side: the parameters are read in place from the torch storage."""

    def __init__(self, resnet, time_kind="raw", objective="hybrid", sigma_data=1.0):
        self.lib = load_library()
        self.device_name = require_gpu()
        self.net = resnet
        self.desc = layer_mlp_desc(resnet, time_kind, objective, sigma_data)
        self.dim = resnet.dim_in
        self.device = next(resnet.parameters()).device
        self._ws = WorkspaceCache()  # kinds "train" and "vjp"
        self._keep = []

    def _weights(self):
        ps = [_dev32(p.detach(), k) for k, p in self.net.state_dict().items()]
        if len(ps) != 2 * (8 + 3 * self.desc.n_res):
            raise RuntimeError("unexpected layer-model state_dict")
        for p in ps:
            if p.data_ptr() % 16:
                raise RuntimeError("layer-model parameters must be 16-byte aligned")
        self._keep = ps
        return (C.c_void_p * len(ps))(*[p.data_ptr() for p in ps]), len(ps)

    def _io(self, x, cond):
        x, cond = _dev32(x, "x"), _dev32(cond, "cond")
        B = x.shape[0]
        if x.shape != (B, self.dim) or cond.shape != (B, self.desc.cond_size):
            raise ValueError(f"layer model shapes: x {tuple(x.shape)} (expected (B, {self.dim})), cond {tuple(cond.shape)} "
                             f"(expected (B, {self.desc.cond_size}))")
        return x, cond, B

    def forward(self, x, cond, time):
        x, cond, B = self._io(x, cond)
        time = _dev32(time, "time").reshape(-1)
        if time.numel() != B:
            raise ValueError("time must be (B,)")
        w, n = self._weights()
        out = torch.empty_like(x)
        _check(self.lib.cd_layer_forward(C.byref(self.desc), w, n, B, x.data_ptr(), cond.data_ptr(), time.data_ptr(),
                                         out.data_ptr(), _stream()))
        return out

    def denoise(self, x, sigma, cond):
        x, cond, B = self._io(x, cond)
        sigma = _sigma_b(sigma, B)
        if sigma.numel() != B:
            raise ValueError("sigma must be (B,)")
        w, n = self._weights()
        out = torch.empty_like(x)
        _check(self.lib.cd_layer_denoise(C.byref(self.desc), w, n, B, x.data_ptr(), sigma.data_ptr(), cond.data_ptr(),
                                         out.data_ptr(), _stream()))
        return out

    # ------------------------------------------------------------------ training (same contract as UnetEngine's)
    def grad_layout(self):
        """{state_dict name: (offset, numel)} into the flat gradient buffer (state_dict order), and its total length."""
        lay, off = {}, 0
        for k, p in self.net.state_dict().items():
            lay[k] = (off, p.numel())
            off += p.numel()
        return lay, off

    def train_workspace(self, batch: int) -> torch.Tensor:
        """Workspace of cd_layer_train_step_loss / cd_layer_loss."""
        return self._ws.get("train", (int(batch),), self.device,
                            lambda: _nbytes(self.lib.cd_layer_train_workspace_bytes, C.byref(self.desc), batch))

    def _loss_io(self, data, noise, sigma, cond):
        data, cond, B = self._io(data, cond)
        noise = _dev32(noise, "noise")
        sigma = _dev32(sigma, "sigma").reshape(-1)
        if noise.shape != data.shape or sigma.numel() != B:
            raise ValueError("noise must have the shape of data and sigma must be (B,)")
        return data, noise, sigma, cond, B

    def train_step(self, data, noise, sigma, cond, loss_type="l2"):
        """The loss of the engine's objective (hybrid / noise_pred / mean_pred; LOSS_TYPE l2 / l1 / mse / huber) and the gradient
        of every parameter of the layer model (cd_layer_train_step_loss)."""
        data, noise, sigma, cond, B = self._loss_io(data, noise, sigma, cond)
        w, n = self._weights()
        ws = self.train_workspace(B)
        _, total = self.grad_layout()
        flat = torch.empty(total, dtype=torch.float32, device=data.device)
        loss = torch.empty((), dtype=torch.float64, device=data.device)
        _check(self.lib.cd_layer_train_step_loss(C.byref(self.desc), w, n, B, data.data_ptr(), noise.data_ptr(), sigma.data_ptr(),
                                                 cond.data_ptr(), LOSS_TYPES[loss_type], loss.data_ptr(), flat.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), _stream()))
        return loss, flat

    def loss(self, data, noise, sigma, cond, loss_type="l2"):
        """The same loss without any gradient work (cd_layer_loss): a 0-d fp64 tensor, bitwise train_step's value."""
        data, noise, sigma, cond, B = self._loss_io(data, noise, sigma, cond)
        w, n = self._weights()
        ws = self.train_workspace(B)
        loss = torch.empty((), dtype=torch.float64, device=data.device)
        _check(self.lib.cd_layer_loss(C.byref(self.desc), w, n, B, data.data_ptr(), noise.data_ptr(), sigma.data_ptr(),
                                      cond.data_ptr(), LOSS_TYPES[loss_type], loss.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        return loss

    def vjp_workspace(self, batch: int, with_param_grads: bool) -> torch.Tensor:
        """Workspace of cd_layer_denoise_vjp."""
        mode = bool(with_param_grads)
        return self._ws.get("vjp", (int(batch), mode), self.device,
                            lambda: _nbytes(self.lib.cd_layer_vjp_workspace_bytes, C.byref(self.desc), batch, int(mode)))

    def denoise_vjp(self, x, sigma, cond, gy, param_grads: bool):
        """Vector-Jacobian product of denoise (cd_layer_denoise_vjp): dx = dL/dx for gy = dL/dD, and with ``param_grads`` the
        gradient of every parameter as a flat fp32 buffer (see grad_layout), else None.  sigma and cond are constants."""
        x, cond, B = self._io(x, cond)
        gy = _dev32(gy, "gy")
        sigma = _sigma_b(sigma, B)
        if gy.shape != x.shape or sigma.numel() != B:
            raise ValueError(f"denoise_vjp shapes: x {tuple(x.shape)}, gy {tuple(gy.shape)}, sigma {tuple(sigma.shape)}")
        w, n = self._weights()
        ws = self.vjp_workspace(B, param_grads)
        dx = torch.empty_like(x)
        flat = None
        if param_grads:
            _, total = self.grad_layout()
            flat = torch.empty(total, dtype=torch.float32, device=x.device)
        _check(self.lib.cd_layer_denoise_vjp(C.byref(self.desc), w, n, B, x.data_ptr(), sigma.data_ptr(), cond.data_ptr(),
                                             gy.data_ptr(), dx.data_ptr(), _ptr(flat), ws.data_ptr(), ws.numel(), _stream()))
        return dx, flat

    def param_grads(self, flat):
        """Views of the flat gradient buffer, one per parameter of the bound ResNet, in .parameters() order."""
        lay, _ = self.grad_layout()
        names = {id(p): k for k, p in self.net.named_parameters()}
        return [flat[lay[names[id(p)]][0]: lay[names[id(p)]][0] + p.numel()].view_as(p) for p in self.net.parameters()]

    def loss_hybrid(self, data, noise, sigma, cond, loss_type="l2"):
        return self.loss(data, noise, sigma, cond, loss_type).to(torch.float32)

    def loss_hybrid_l2(self, data, noise, sigma, cond):
        return self.loss_hybrid(data, noise, sigma, cond, "l2")

    def sampler_run(self, start, cond, program, step_noise=None, seed=0, offset=0, noise_stride=0, debug=False, use_graph=True):
        """Same contract as UnetEngine.sampler_run on (B, dim) vectors (cd_layer_sampler_run): the whole program is one launch
        (use_graph is irrelevant).  The k-th RANDN op executed takes the Philox stream elements offset + k * stride + row * dim
        + i, stride = noise_stride or B * dim, so batch shards are slices of one global stream; step_noise: one (B, dim) tensor
        per RANDN op executed instead.  Returns (x, xs, x0s); the trajectories (n_steps, B, dim) only when ``debug`` and the
        program records them."""
        start, cond, B = self._io(start, cond)
        coefs = np.ascontiguousarray(program.coefs, dtype=np.float32)
        n_steps, n_coef = coefs.shape
        ops_dev = torch.from_numpy(_pack_ops(program)).to(start.device)
        coefs_dev = torch.from_numpy(coefs).to(start.device)
        op_begin = None
        if program.op_begin is not None:
            assert len(program.op_begin) == n_steps + 1
            op_begin = torch.tensor(program.op_begin, dtype=torch.int32, device=start.device)
        x_out = torch.empty_like(start)
        xs, x0s, step_noise = _program_io(start, program, n_steps, step_noise, debug, "(B, dim)")
        w, n = self._weights()
        _check(self.lib.cd_layer_sampler_run(C.byref(self.desc), w, n, B, start.data_ptr(), float(program.start_scale),
                                             cond.data_ptr(), program.n_bufs, n_steps, ops_dev.data_ptr(), len(program.ops),
                                             _ptr(op_begin), coefs_dev.data_ptr(), n_coef, _ptr(step_noise), int(seed), int(offset),
                                             int(noise_stride), x_out.data_ptr(), _ptr(xs), _ptr(x0s), _stream()))
        return x_out, xs, x0s

    def ddim_sample(self, start, cond, steps: np.ndarray, step_noise=None, seed=0, offset=0, debug=False, use_graph=True,
                    out=None, noise_stride=0):
        """Same contract as UnetEngine.ddim_sample; the whole trajectory is one launch (use_graph is irrelevant; the noise of
        a stochastic sampler is drawn as one (n_steps, B, dim) block, so batch shards are not slices of a global stream)."""
        start, cond, B = self._io(start, cond)
        steps = np.ascontiguousarray(steps, dtype=np.float32)
        n_steps = steps.shape[0]
        assert steps.shape == (n_steps, 4)
        table = torch.from_numpy(steps).to(start.device)
        if step_noise is None and float(np.abs(steps[:, 2]).max()) > 0:
            step_noise = randn((n_steps, B, self.dim), start.device, seed, offset)
        if step_noise is not None:
            step_noise = _dev32(step_noise, "step_noise")
            assert step_noise.numel() == n_steps * start.numel()
        x_out = torch.empty_like(start) if out is None else out
        xs, x0s = _trajectories(start, n_steps, debug, debug, zeroed=False)
        w, n = self._weights()
        _check(self.lib.cd_layer_sample(C.byref(self.desc), w, n, B, start.data_ptr(), cond.data_ptr(), table.data_ptr(),
                                        n_steps, _ptr(step_noise), x_out.data_ptr(), _ptr(xs), _ptr(x0s), _stream()))
        return x_out, xs, x0s
