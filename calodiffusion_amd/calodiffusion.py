"""CaloDiffusion: the EDM-preconditioned cylindrical U-Net denoiser (mirror of reference
calodiffusion/models/calodiffusion.py:9-173) running on the HIP engine."""
from __future__ import annotations

from typing import Union

import torch

from . import utils
from .diffusion import Diffusion
from .unet import CondUnet, unet_kwargs_from_config


class CaloDiffusion(Diffusion):
    def __init__(self, config: Union[str, dict], n_steps: int = 400, loss_type: str = "l2"):
        super().__init__(config, n_steps, loss_type)
        config = self.config
        self.pre_embed = "pre-embed" in config.get("SHOWER_EMBED", "")
        self.hgcal = config.get("HGCAL", False)
        self.fully_connected = "FCN" in config.get("SHOWER_EMBED", "")
        self.time_embed = config.get("TIME_EMBED", "sin")
        self.dataset_num = config.get("DATASET_NUM", 2)
        self.training_objective = config.get("TRAINING_OBJ", "noise_pred")
        self.layer_cond = "layer" in config.get("SHOWERMAP", "")
        if self.fully_connected:
            raise NotImplementedError("the FCN/ResNet layer model is outside the HIP hot path (SURVEY.md 8f rank 3)")
        if self.hgcal and not self.pre_embed:
            # HGCalConverter inside forward (calodiffusion.py:86-98, 113-117): the state is the cell-space shower
            pad, grid = list(config["SHAPE_PAD"]), [int(v) for v in config["SHAPE_FINAL"][2:]]
            if len(pad) != 4 or int(pad[1]) != 1 or int(pad[2]) != grid[0]:
                raise NotImplementedError(f"HGCal's in-model embedding (HGCalConverter inside forward) acts on the cell-space shower: "
                                          f"SHAPE_PAD must be [-1, 1, {grid[0]}, cells], not {pad}; a dataset that is already on "
                                          "the grid uses the pre-embedded form of the config (SHOWER_EMBED '...-pre-embed')")
        if self.time_embed not in ("log", "sigma"):
            raise KeyError(self.time_embed)  # the reference's do_time_embed raises the same way (calodiffusion.py:148-152)
        self.model = self.init_model()
        self.NN_embed = self.init_embedding_model()  # (after init_model: the RNG draws come in the reference's order)
        self.do_embed = self.NN_embed is not None and not self.pre_embed

    # ------------------------------------------------------------------ construction / weights
    def init_model(self):
        cfg = self.config
        unet = CondUnet(**unet_kwargs_from_config(cfg))
        objective = type(self.loss_function).__name__
        if "noise_pred" in objective:
            obj = "noise_pred"
        elif "mean_pred" in objective:
            obj = "mean_pred"
        elif "hybrid" in objective:
            obj = "hybrid"
        else:
            raise ValueError("??? Training obj %s" % objective)
        unet._engine_opts = dict(
            rz_input=cfg.get("R_Z_INPUT", False), phi_input=cfg.get("PHI_INPUT", False), time_kind=self.time_embed,
            objective=obj, sigma_data=self.loss_function.sigma_data,
            coords=utils.coordinate_profiles(self.dataset_num, cfg["SHAPE_FINAL"][2:]))
        return unet.to(self.device)

    def init_embedding_model(self):
        """calodiffusion.py:100-119.  The non-HGCal 'NN' case: an ``NNConverter`` over the binning file.  HGCal without
        'pre-embed': an ``HGCalConverter`` over the geometry file, initialised without norm -- or, with TRAINABLE_EMBED, left as
        the reference leaves it (:116-117): zero maps and empty masks, for ``init()`` or a checkpoint to fill.  Without the file
        at hand, ``config['NN_EMBED']`` may hold an already built converter of the kind (taken as it is: no RNG draws)."""
        cfg = self.config
        if self.pre_embed or ("NN" not in cfg.get("SHOWER_EMBED", "") and not self.hgcal):
            return None
        grid = tuple(int(v) for v in cfg["SHAPE_FINAL"][2:])
        nn_embed = cfg.get("NN_EMBED")
        if self.hgcal:
            from .hgcal import HGCalConverter
            if nn_embed is None:
                trainable = bool(cfg.get("TRAINABLE_EMBED", False))
                nn_embed = HGCalConverter(bins=cfg["SHAPE_FINAL"], geom_file=cfg["BIN_FILE"], device=self.device, trainable=trainable)
                if not trainable:
                    nn_embed.init(norm=self.pre_embed, dataset_num=self.dataset_num)
            elif not isinstance(nn_embed, HGCalConverter):
                raise TypeError("config['NN_EMBED'] takes a calodiffusion_amd.hgcal.HGCalConverter on an HGCAL config")
            have = (nn_embed.num_layers, nn_embed.num_alpha_bins, nn_embed.num_r_bins)
            if have != grid:
                raise ValueError(f"the geometry embedding maps onto (layers, alpha, r) = {have}, but SHAPE_FINAL gives the U-Net "
                                 f"the grid {grid}")
            cells = int(nn_embed.embeder.mat.shape[-1])
            if [int(v) for v in cfg["SHAPE_PAD"][1:]] != [1, grid[0], cells]:
                raise ValueError(f"the geometry embedding has {cells} cells a layer: SHAPE_PAD must be [-1, 1, {grid[0]}, {cells}], "
                                 f"not {list(cfg['SHAPE_PAD'])}")
            if nn_embed.norm:
                raise ValueError("an in-model HGCalConverter is initialised without norm (calodiffusion.py:117)")
            return nn_embed.to(self.device)
        from .geom1 import NNConverter
        if nn_embed is None:
            from .xml_handler import XMLHandler
            bins = XMLHandler("photon" if cfg.get("DATASET_NUM", 2) == 1 else "pion", cfg["BIN_FILE"])
            nn_embed = NNConverter(bins=bins)
        elif not isinstance(nn_embed, NNConverter):
            raise TypeError("config['NN_EMBED'] takes a calodiffusion_amd.geom1.NNConverter")
        gc = nn_embed.gc
        have = (int(gc.num_layers), int(gc.alpha_out), int(gc.dim_r_out))
        if have != grid:
            raise ValueError(f"the geometry embedding maps onto (layers, alpha_out, dim_r_out) = {have}, but SHAPE_FINAL gives the "
                             f"U-Net the grid {grid}")
        gc.descriptor()  # refuses a layout the device maps cannot hold, now rather than at the first denoise
        if int(gc.layer_boundaries[-1]) != int(self._data_shape[-1]):
            raise ValueError(f"the geometry embedding has {int(gc.layer_boundaries[-1])} voxels, SHAPE_ORIG says {self._data_shape[-1]}")
        return nn_embed.to(self.device)

    def load_state_dict(self, state_dict, strict=True):
        """Prefix-tolerant loading, as the reference (calodiffusion.py:31-37)."""
        base = list(state_dict.keys())[10].split(".")[0]
        if base != "model":
            state_dict = {k.removeprefix(f"{base}."): v for k, v in state_dict.items() if k.split(".")[0] == base}
        return super().load_state_dict(state_dict, strict)

    def engine(self):
        eng = self.model.engine()
        if self.do_embed and eng.embedding is not self.NN_embed:
            eng.set_embedding(self.NN_embed)  # (a fresh engine after .to(): bound again)
        return eng

    def _params(self):
        """The parameters the device calls hand gradients to, in ``engine().param_grads`` order."""
        return list(self.model.parameters()) + (list(self.NN_embed.parameters()) if self.do_embed else [])

    def to(self, *a, **k):
        out = super().to(*a, **k)
        self.device = next(self.parameters()).device
        return out

    # ------------------------------------------------------------------ hot path
    def noise_generation(self, shape):
        return super().noise_generation(shape)

    def cond_tensor(self, E, layers):
        """cat(E, layers) when the config conditions on layer energies (calodiffusion.py:89-90)."""
        if self.layer_cond and layers is not None:
            E = torch.cat([E, layers], dim=1)
        return E.to(torch.float32).contiguous()

    def forward(self, x, E, time, layers, controls=None):
        """calodiffusion.py:86-98: x is the already c_in-scaled input; returns the raw network output F."""
        if controls is not None:
            raise NotImplementedError("ControlNet is dead code in the reference")
        if self.do_embed:
            x = self.NN_embed.enc(x.to(torch.float32))
        rz_phi = self.add_RZPhi(x).float()
        out = self.model(rz_phi, cond=self.cond_tensor(E, layers), time=time.float())
        return self.NN_embed.dec(out) if self.do_embed else out

    def add_RZPhi(self, x):
        """calodiffusion.py:121-142 (only used by the generic `forward`; `denoise` synthesises the channels in-kernel)."""
        cats = [x]
        shape = (x.shape[0], 1) + tuple(x.shape[2:])
        r, z, phi = utils.coordinate_profiles(self.dataset_num, x.shape[2:])
        if self.config.get("R_Z_INPUT", False):
            cats.append(torch.from_numpy(r).to(x.device).view(1, 1, 1, 1, -1).expand(shape))
            cats.append(torch.from_numpy(z).to(x.device).view(1, 1, -1, 1, 1).expand(shape))
        if self.config.get("PHI_INPUT", False):
            cats.append(torch.from_numpy(phi).to(x.device).view(1, 1, 1, -1, 1).expand(shape))
        return torch.cat(cats, dim=1) if len(cats) > 1 else x

    def do_time_embed(self, sigma=None):
        embed = {"sigma": lambda s: s / (1 + s ** 2).sqrt(), "log": lambda s: 0.5 * torch.log(s)}
        return embed[self.time_embed](sigma)

    def denoise(self, x, E=None, sigma=None, layers=None, controls=None):
        """EDM-preconditioned denoiser (calodiffusion.py:154-169): one C-ABI call.  With a geometry embedding (``do_embed``) x is
        the flat shower -- (B, V) for Dataset 1, the cells (B, 1, layers, cells) for HGCal -- : enc and dec run inside the call, and the embedding's weights take gradients as the U-Net's do.

        Differentiable when ``torch.is_grad_enabled()`` and ``x.requires_grad``: backward then gives x its gradient and, if a
        parameter requires grad, every parameter too (cd_denoise_vjp recomputes the forward on the device).  Any other call is
        the plain call without a graph; a caller who wants only the parameter gradients sets ``x.requires_grad_()``.  sigma, E
        and layers are constants of the graph: one that requires grad raises NotImplementedError.  Gradients stay local to
        the process (no data-parallel all-reduce), as plain torch autograd gives them."""
        if controls is not None:
            raise NotImplementedError("ControlNet is dead code in the reference")
        if torch.is_grad_enabled() and isinstance(x, torch.Tensor) and x.requires_grad:
            for name, t in (("sigma", sigma), ("E", E), ("layers", layers)):
                if isinstance(t, torch.Tensor) and t.requires_grad:
                    raise NotImplementedError(f"denoise: no gradient with respect to {name}; pass {name}.detach()")
            params = self._params()
            return _Denoise.apply(self.engine(), x, sigma.reshape(-1), self.cond_tensor(E, layers), *params)
        return self.engine().denoise(x, sigma.reshape(-1), self.cond_tensor(E, layers))

    def __call__(self, x, **kwargs):
        return self.denoise(x, **kwargs)


class _Denoise(torch.autograd.Function):
    """denoise with a backward: the forward is the plain engine call (same bits), the backward is one cd_denoise_vjp call that
    recomputes the taped forward from the saved x, sigma and cond."""

    @staticmethod
    def forward(ctx, engine, x, sigma, cond, *params):
        out = engine.denoise(x.detach(), sigma.detach(), cond.detach())
        ctx.save_for_backward(x, sigma, cond)
        ctx.engine, ctx.params = engine, params
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, sigma, cond = ctx.saved_tensors
        want = any(p.requires_grad for p in ctx.params)
        dx, flat = ctx.engine.denoise_vjp(x, sigma, cond, gy.contiguous(), param_grads=want)
        if want:
            # the parameters' gradients handed over as in _TrainStep.backward (loss.py): a view of the flat buffer on the first
            # assignment, added to an existing gradient otherwise
            for p, g in zip(ctx.params, ctx.engine.param_grads(flat)):
                if not p.requires_grad:
                    continue
                if p.grad is None:
                    p.grad = g
                else:
                    p.grad = p.grad + g if p.grad.requires_grad else p.grad.add_(g)
        return (None, dx if ctx.needs_input_grad[1] else None, None, None) + (None,) * len(ctx.params)
