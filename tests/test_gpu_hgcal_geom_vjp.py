"""GPU (MI355X): the differentiable HGCal geometry maps -- ``cd_geom_create_ex`` over a mask, ``cd_geom_refresh`` and
``cd_geom_apply_vjp`` behind ``hgcal.Embeder`` / ``Decoder`` / ``HGCalConverter(trainable=True)`` -- on three synthetic
geometries: "g" (tests/golden/hgcal_geom.npz), "m" and "t" (tools/gen_golden_hgcal_model.py; "t" has 300 cells a layer, so the
lane-per-column gather crosses a workgroup).  The reference's autograd is the fixture's for "t" (``Embeder`` / ``Decoder`` of the
reference under ``backward()``) and a float64 restatement of the same einsum through ``mat * mask`` for all three.

Bounds: TOL_OP 1e-5 per call, TOL_GRAD 5e-6 for gradients, TOL_ROW 2e-6 for batch independence (helpers.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import gold, rel_l2
from helpers import TOL_GRAD, TOL_OP, TOL_ROW, t
import hgcal_model_cases as K

pytestmark = pytest.mark.gpu

TAGS = ("g", "m", "t")


def _maps(tag, perturbed=True):
    """(A, R, enc, enc_mask, dec, dec_mask) as CPU tensors; perturbed: every element moved, outside the masks too"""
    if tag == "m":
        g = gold("hgcal_model")
        A, R = K.GRID[1:]
        maps = [g["nn.embeder.mat" if perturbed else "init.enc_mat"], g["init.enc_mask"],
                g["nn.decoder.mat" if perturbed else "init.dec_mat"], g["init.dec_mask"]]
    else:
        g = gold("hgcal_geom" if tag == "g" else "hgcal_model_t")
        A, R = (int(b) for b in g[f"{tag}.bins"][1:])
        maps = [g[f"{tag}.enc_mat"], g[f"{tag}.enc_mask"], g[f"{tag}.dec_mat"], g[f"{tag}.dec_mask"]]
        if perturbed:
            maps[0] = maps[0] + K.hashed_perturbation(maps[0].shape)
            maps[2] = maps[2] + K.hashed_perturbation(maps[2].shape)
    return (A, R) + tuple(t(m) for m in maps)


def _modules(tag, trainable=True, perturbed=True):
    from calodiffusion_amd import hgcal
    A, R, enc, enc_mask, dec, dec_mask = _maps(tag, perturbed)
    mods = hgcal.Embeder(A, R, enc.clone(), enc_mask, trainable).cuda(), hgcal.Decoder(A, R, dec.clone(), dec_mask, trainable).cuda()
    for mod in mods:
        if trainable:
            assert isinstance(mod.mat, torch.nn.Parameter)
            mod.mat.requires_grad_(True)  # (a map built on its own is frozen until asked; HGCalConverter asks)
    return mods


def _inputs(tag, B=3, seed=7):
    A, R, enc, *_ = _maps(tag)
    L, E, N = enc.shape
    gen = torch.Generator().manual_seed(seed)
    return (K.eighths(gen, (B, 1, L, N), -16, 16), K.eighths(gen, (B, 1, L, A, R), -16, 16),
            K.eighths(gen, (B, 1, L, A, R), -12, 12), K.eighths(gen, (B, 1, L, N), -12, 12))


def _autograd64(mat, mask, x, cot, enc):
    """(y, dx, dmat) of the reference's forward through mat * mask, in float64 on the CPU"""
    M, xx = mat.double().requires_grad_(True), x.double().requires_grad_(True)
    y = (K.enc_einsum if enc else K.dec_einsum)(M * mask, xx.reshape(xx.shape[:3] + (-1,)))
    (y * cot.double().reshape(y.shape)).sum().backward()
    return y.detach(), xx.grad, M.grad


def _run(mod, x, cot):
    """(y, dx, dmat) through the module under autograd"""
    mod.zero_grad()
    xg = x.cuda().requires_grad_(True)
    y = mod(xg)
    (y * cot.cuda()).sum().backward()
    return y.detach(), xg.grad, None if not mod.trainable else mod.mat.grad


@pytest.mark.parametrize("tag", TAGS)
def test_frozen_forward_is_todays_cd_geom_apply_bit_for_bit(tag):
    from calodiffusion_amd import engine
    lib = engine.load_library()
    emb, dcd = _modules(tag, trainable=False)
    x, z, _, _ = _inputs(tag)
    for mod, inp, first in ((emb, x, 0), (dcd, z, 1)):
        dense = mod.mat.cuda().contiguous()
        L, rows, cols = dense.shape
        handle = C.c_void_p()
        engine._check(lib.cd_geom_create(dense.data_ptr(), L, rows, cols, 0, C.byref(handle), engine._stream()))
        xin = inp.cuda().reshape(3, 1, L, cols).contiguous()
        want = torch.empty((3, 1, L, rows), device="cuda")
        engine._check(lib.cd_geom_apply(handle, xin.data_ptr(), want.data_ptr(), 3, 1.0, 0.0, first, engine._stream()))
        with torch.no_grad():
            got = mod(inp.cuda())
        y_grad, _, _ = _run(mod, inp, torch.ones(got.shape))  # the differentiable call: the same forward launch
        torch.cuda.synchronize()
        lib.cd_geom_destroy(handle)
        assert torch.equal(got.reshape(want.shape), want) and torch.equal(y_grad, got)


@pytest.mark.parametrize("tag", TAGS)
def test_gradients_against_autograd_through_mat_times_mask(tag):
    """dx, dmat (dense; exact zeros outside the mask) and the forward of a trainable map, against the float64 restatement and,
    for "t", against what the reference's modules returned"""
    emb, dcd = _modules(tag)
    A, R, enc, enc_mask, dec, dec_mask = _maps(tag)
    x, z, cot_e, cot_d = _inputs(tag)
    if tag == "t":
        g = gold("hgcal_model_t")
        x, z, cot_e, cot_d = t(g["t.x"]), t(g["t.z"]), t(g["t.cot_enc"]), t(g["t.cot_dec"])
    for name, mod, mat, mask, inp, cot in (("enc", emb, enc, enc_mask, x, cot_e), ("dec", dcd, dec, dec_mask, z, cot_d)):
        y, dx, dm = _run(mod, inp, cot)
        y64, dx64, dm64 = _autograd64(mat, mask, inp, cot, name == "enc")
        errs = {"y": rel_l2(y.cpu().numpy().reshape(y64.shape), y64.numpy()), "dx": rel_l2(dx.cpu().numpy(), dx64.numpy()),
                "dm": rel_l2(dm.cpu().numpy(), dm64.numpy())}
        if tag == "t":
            errs["y ref"] = rel_l2(y.cpu().numpy(), g[f"t.{name}"])
            errs["dx ref"] = rel_l2(dx.cpu().numpy(), g[f"t.{name}.dx"])
            errs["dm ref"] = rel_l2(K.masked(dm.cpu().numpy(), mask.numpy()), g[f"t.{name}.dm"])
        print(f"[{tag} {name}] " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert dm.shape == mat.shape and bool((dm.cpu()[~mask] == 0).all())
        assert errs["y"] < TOL_OP and errs.get("y ref", 0.0) < TOL_OP
        assert max(v for k, v in errs.items() if k[0] == "d") < TOL_GRAD
        # a second pass is the same bits
        y2, dx2, dm2 = _run(mod, inp, cot)
        assert torch.equal(y, y2) and torch.equal(dx, dx2) and torch.equal(dm, dm2)


@pytest.mark.parametrize("tag", ("g", "m"))
def test_masked_entries_at_zero_take_gradient_and_values_outside_the_mask_never_enter(tag):
    emb, _ = _modules(tag, perturbed=False)  # init()'s maps: most masked entries are 0
    A, R, enc, enc_mask, *_ = _maps(tag, perturbed=False)
    x, _, cot, _ = _inputs(tag)
    x = x.abs() + 0.125  # (every cell carries signal)
    y, dx, dm = _run(emb, x, cot.abs() + 0.125)
    zero_valued = enc_mask & (enc == 0)
    live = torch.zeros_like(enc_mask)
    ncells = gold("hgcal_model" if tag == "m" else "hgcal_geom")[f"{tag}.ncells"]
    for l, n in enumerate(ncells):
        live[l, :, :int(n)] = True
    assert int(zero_valued.sum()) > 0 and bool((dm.cpu()[zero_valued & live] != 0).all()) and bool((dm.cpu()[~enc_mask] == 0).all())
    # move every value outside the mask: nothing changes, to the bit (the refresh gathers the masked entries only)
    with torch.no_grad():
        emb.mat.add_((~enc_mask).to(torch.float32).cuda() * 3.0)
    y2, dx2, dm2 = _run(emb, x, cot.abs() + 0.125)
    assert torch.equal(y, y2) and torch.equal(dx, dx2) and torch.equal(dm, dm2)
    # ... and a masked value does reach the next call through the refresh
    with torch.no_grad():
        emb.mat.add_(enc_mask.to(torch.float32).cuda() * 0.5)
    y3, _, _ = _run(emb, x, cot.abs() + 0.125)
    want = K.enc_einsum((emb.mat.detach().cpu() * enc_mask).double(), x.double()).reshape(y3.shape)
    assert not torch.equal(y3, y) and rel_l2(y3.cpu().numpy(), want.numpy()) < TOL_OP


@pytest.mark.parametrize("tag", ("m", "t"))
def test_rows_do_not_depend_on_the_batch(tag):
    emb, dcd = _modules(tag)
    x, z, cot_e, cot_d = _inputs(tag)
    xb, zb, cb_e, cb_d = _inputs(tag, B=130, seed=8)
    for name, mod, inp, cot, big, big_cot in (("enc", emb, x, cot_e, xb, cb_e), ("dec", dcd, z, cot_d, zb, cb_d)):
        y3, dx3, _ = _run(mod, inp, cot)
        yb, dxb, _ = _run(mod, torch.cat([inp, big[3:]]), torch.cat([cot, big_cot[3:]]))
        ey, ex = rel_l2(yb[:3].cpu().numpy(), y3.cpu().numpy()), rel_l2(dxb[:3].cpu().numpy(), dx3.cpu().numpy())
        print(f"[{tag} {name}] rows [0:3] of 130 against 3: y {ey:.2e} dx {ex:.2e}")
        assert ey < TOL_ROW and ex < TOL_ROW


def test_uninitialised_trainable_converter_gives_zeros():
    from calodiffusion_amd import hgcal
    from hgcal_geom_cases import geometry
    conv = hgcal.HGCalConverter(bins=[-1, 1] + list(K.GRID), geom=geometry(gold("hgcal_model"), "m"), trainable=True).cuda()
    x, z, cot_e, cot_d = _inputs("m")
    for mod, inp, cot in ((conv.embeder, x, cot_e), (conv.decoder, z, cot_d)):
        y, dx, dm = _run(mod, inp, cot)
        assert not y.any() and not dx.any() and not dm.any() and dm.shape == mod.mat.shape
    conv.init()  # in place: the next call sees the maps
    with torch.no_grad():
        y = conv.enc(x.cuda())
    want = K.enc_einsum(t(gold("hgcal_model")["init.enc_mat"]).double(), x.double())
    assert rel_l2(y.cpu().numpy().reshape(want.shape), want.numpy()) < TOL_OP


def test_converter_norm_rides_in_the_gradients():
    """enc's 1 / std on the output and dec's std on the input (HGCal_utils.py:636-640, 659-663), set 101"""
    from calodiffusion_amd import hgcal
    A, R, enc, enc_mask, dec, dec_mask = _maps("m")
    conv = hgcal.HGCalConverter.from_matrices([-1, 1] + list(K.GRID), enc, dec, enc_mask, dec_mask, trainable=True).cuda()
    conv.norm, (conv.embed_mean, conv.embed_std) = True, hgcal.HGCAL_EMBED_PARAMS[101]
    mean, std = conv.embed_mean, conv.embed_std
    x, z, cot_e, cot_d = _inputs("m")
    conv.zero_grad()
    xg, zg = x.cuda().requires_grad_(True), z.cuda().requires_grad_(True)
    (conv.enc(xg) * cot_e.cuda()).sum().backward()
    (conv.dec(zg) * cot_d.cuda()).sum().backward()
    M, D = enc.double().requires_grad_(True), dec.double().requires_grad_(True)
    x64, z64 = x.double().requires_grad_(True), z.double().requires_grad_(True)
    ((K.enc_einsum(M * enc_mask, x64) - mean) / std * cot_e.double().reshape(3, 1, K.LAYERS, -1)).sum().backward()
    (K.dec_einsum(D * dec_mask, z64.reshape(3, 1, K.LAYERS, -1) * std + mean) * cot_d.double()).sum().backward()
    errs = [rel_l2(a.cpu().numpy(), b.numpy()) for a, b in ((xg.grad, x64.grad), (zg.grad, z64.grad), (conv.embeder.mat.grad, M.grad),
                                                            (conv.decoder.mat.grad, D.grad))]
    print("norm: dx enc, dx dec, dmat enc, dmat dec:", [f"{e:.2e}" for e in errs])
    assert max(errs) < TOL_GRAD
