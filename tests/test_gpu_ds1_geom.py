"""GPU (MI355X): the Dataset-1 geometry maps on the device -- cd_radial_enc / dec / enc_vjp / dec_vjp through
calodiffusion_amd/geom1.py -- against the reference's GeomConverter / NNConverter outputs and torch-autograd gradients on two
synthetic geometries (fixture: tools/gen_golden_ds1_geom.py; G1 photon-shaped, G2 pion-shaped), per element at the derived bound
of ds1_geom_cases, at B = 1, 3 and 130.  The B = 3 inputs are rows [0:3] of the B = 130 ones.  Where the fixture holds the
reference at B = 3 only (the fixed matrices, dx, dg), the other batch sizes are held against the float64 restatement as well."""
import ctypes as C

import numpy as np
import pytest
import torch

from ds1_geom_cases import TAGS, check, collapse64, expand64, fixture, geom_converter, mats, nn_converter, weight_grad64

pytestmark = pytest.mark.gpu

BATCHES = (1, 3, 130)
_conv = {}


def _nn(tag):
    if tag not in _conv:
        _conv[tag] = nn_converter(tag).cuda()
    return _conv[tag]


def _cat(layers):
    return torch.cat([lay.weight.detach().reshape(-1) for lay in layers])


def _ref_rows(f, name, B):
    """The reference's rows for batch B: stored at B = 3 and B = 130; B = 1 is the first row of the B = 3 result."""
    return f[name][:B] if B == 130 else f[name + ".b3"][:B]


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("tag", TAGS)
def test_forward_matches_the_reference(tag, B):
    f, conv = fixture(tag), _nn(tag)
    x, g = f["x"][:B], f["g"][:B]
    enc, dec = conv.enc(x), conv.dec(torch.tensor(g).cuda())  # numpy and device inputs
    assert enc.is_cuda and dec.is_cuda and enc.shape == (B, 1, f["L"], f["A"], f["R"]) and dec.shape == (B, f["V"])
    W, D = mats(f, "nn.encs"), mats(f, "nn.decs")
    check(f"{tag} B={B} enc", enc.detach().cpu().numpy(), _ref_rows(f, "enc", B), *expand64(f, W, x, True, absolute=True))
    check(f"{tag} B={B} dec", dec.detach().cpu().numpy(), _ref_rows(f, "dec", B), *collapse64(f, D, g, False, absolute=True))
    assert torch.equal(conv(x), enc)  # forward is enc

    gc = conv.gc
    Wf, Df = mats(f, "weight_mats"), mats(f, "pinv")
    cv, ucv = gc.convert_flat(x), gc.unconvert_flat(g)
    assert cv.shape == (B, f["L"], f["A"], f["R"]) and ucv.shape == (B, f["V"])
    t_cv, n_cv = expand64(f, Wf, x, True, absolute=True)
    t_ucv, n_ucv = collapse64(f, Df, g, False, absolute=True)
    check(f"{tag} B={B} convert_flat vs float64", cv.detach().cpu().numpy()[:, None], expand64(f, Wf, x, True)[0], t_cv, n_cv)
    check(f"{tag} B={B} unconvert_flat vs float64", ucv.detach().cpu().numpy(), collapse64(f, Df, g, False)[0], t_ucv, n_ucv)
    if B <= 3:
        check(f"{tag} B={B} convert_flat", cv.detach().cpu().numpy(), f["convert.b3"][:B], t_cv[:, 0], n_cv[:, 0])
        check(f"{tag} B={B} unconvert_flat", ucv.detach().cpu().numpy(), f["unconvert.b3"][:B], t_ucv, n_ucv)
    # an output bin that no input bin of its layer covers is exactly 0
    empty = np.stack([np.abs(m).sum(1) == 0 for m in Wf])  # (L, R)
    assert empty.any() and (cv.detach().cpu().numpy()[:, empty[:, None, :].repeat(f["A"], 1)] == 0.0).all()
    # the list forms are the flat ones
    xt = torch.tensor(x)
    assert torch.equal(gc.convert(gc.reshape(xt)), cv)
    assert torch.equal(gc.unreshape(gc.unconvert(g[:, 0])), ucv)
    assert [tuple(p.shape) for p in gc.unconvert(g)] == [tuple(p.shape) for p in gc.reshape(xt)]


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("tag", TAGS)
def test_gradients_match_autograd_of_the_reference(tag, B):
    """dx, dW (cotangent g) and dg, dD (cotangent c) through .backward() against the stored torch-autograd values of the
    reference: dx, dg stored at B = 3 (n = R, rin_i: no batch in it), dW, dD at B = 3 and 130 (n = B A); every batch size also
    against the float64 restatement."""
    f, conv = fixture(tag), _nn(tag)
    conv.zero_grad(set_to_none=True)
    x = torch.tensor(f["x"][:B]).cuda().requires_grad_(True)
    g = torch.tensor(f["g"][:B]).cuda().requires_grad_(True)
    c = torch.tensor(f["c"][:B]).cuda()
    conv.enc(x).backward(g.detach())
    conv.dec(g).backward(c)
    W, D = mats(f, "nn.encs"), mats(f, "nn.decs")
    xn, gn, cn = f["x"][:B], f["g"][:B], f["c"][:B]
    t_dx, n_dx = collapse64(f, [m.T for m in W], gn, True, absolute=True)
    t_dg, n_dg = expand64(f, [m.T for m in D], cn, False, absolute=True)
    dx, dg = x.grad.detach().cpu().numpy(), g.grad.detach().cpu().numpy()
    check(f"{tag} B={B} dx vs float64", dx, collapse64(f, [m.T for m in W], gn, True)[0], t_dx, n_dx)
    check(f"{tag} B={B} dg vs float64", dg, expand64(f, [m.T for m in D], cn, False)[0], t_dg, n_dg)
    k = min(B, 3)
    check(f"{tag} B={B} dx", dx[:k], f["dx"][:k], t_dx[:k], n_dx)
    check(f"{tag} B={B} dg", dg[:k], f["dg"][:k], t_dg[:k], n_dg)
    for name, layers_, enc, flat, grid in (("dW", conv.encs, True, xn, gn), ("dD", conv.decs, False, cn, gn)):
        val, tot = weight_grad64(f, flat, grid, enc), weight_grad64(f, flat, grid, enc, absolute=True)
        for i, lay in enumerate(layers_):
            got = lay.weight.grad.detach().cpu().numpy()
            check(f"{tag} B={B} {name}[{i}] vs float64", got, val[i][0], tot[i][0], tot[i][1])
            if B != 1:
                check(f"{tag} B={B} {name}[{i}]", got, f[f"{name}.b{B}.{i}"], tot[i][0], tot[i][1])


@pytest.mark.parametrize("tag", TAGS)
def test_autograd_end_to_end_equals_the_vjp_entry_points(tag):
    """loss = (dec(stub(enc(x))) * c).sum(): x.grad and every parameter's .grad are set, finite and bitwise what the two VJP entry
    points give by hand; with the parameters frozen x.grad is bitwise the same and no parameter gets a gradient."""
    f, conv = fixture(tag), _nn(tag)
    B = 130
    stub = lambda y: torch.tanh(y) * 1.5 + 0.25 * y  # noqa: E731
    c = torch.tensor(f["c"][:B]).cuda()
    conv.zero_grad(set_to_none=True)
    x = torch.tensor(f["x"][:B]).cuda().requires_grad_(True)
    (conv.dec(stub(conv.enc(x))) * c).sum().backward()
    params = list(conv.parameters())
    assert x.grad is not None and all(p.grad is not None and torch.isfinite(p.grad).all() for p in params)
    assert torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0

    rmap, w, d = conv.gc.radial_map(), _cat(conv.encs), _cat(conv.decs)
    xd = x.detach()
    y = rmap.enc(w, xd).requires_grad_(True)
    h = stub(y)
    dg, dd = rmap.dec_vjp(d, h.detach().contiguous(), c, True)
    h.backward(dg)
    dx, dw = rmap.enc_vjp(w, xd, y.grad.contiguous(), True)
    assert torch.equal(x.grad, dx)
    assert torch.equal(_cat_grads(conv.encs), dw) and torch.equal(_cat_grads(conv.decs), dd)
    # input gradient only: a null weight-gradient pointer
    dx_only, none = rmap.enc_vjp(w, xd, y.grad.contiguous(), False)
    assert none is None and torch.equal(dx_only, dx)

    first = x.grad.clone()
    conv.zero_grad(set_to_none=True)
    try:
        conv.requires_grad_(False)
        x2 = xd.clone().requires_grad_(True)
        (conv.dec(stub(conv.enc(x2))) * c).sum().backward()
        assert torch.equal(x2.grad, first) and all(p.grad is None for p in params)
        with torch.no_grad():
            assert not conv.dec(stub(conv.enc(xd))).requires_grad
    finally:
        conv.requires_grad_(True)


def _cat_grads(layers):
    return torch.cat([lay.weight.grad.reshape(-1) for lay in layers])


@pytest.mark.parametrize("tag", TAGS)
def test_rows_do_not_depend_on_the_batch_and_calls_repeat(tag):
    f, conv = fixture(tag), _nn(tag)
    rmap, w, d = conv.gc.radial_map(), _cat(conv.encs), _cat(conv.decs)
    x, g, c = (torch.tensor(f[k]).cuda() for k in ("x", "g", "c"))
    runs = {"enc": lambda n: (rmap.enc(w, x[:n]),), "dec": lambda n: (rmap.dec(d, g[:n]),),
            "enc_vjp": lambda n: rmap.enc_vjp(w, x[:n], g[:n], True), "dec_vjp": lambda n: rmap.dec_vjp(d, g[:n], c[:n], True)}
    for name, run in runs.items():
        big, again, small, one = run(130), run(130), run(3), run(1)
        assert all(torch.equal(a, b) for a, b in zip(big, again)), name  # weight gradients included
        assert torch.equal(big[0][:3], small[0]) and torch.equal(big[0][:1], one[0]), name
        assert all(torch.equal(a, b) for a, b in zip(small, run(3))), name


@pytest.mark.parametrize("tag", TAGS)
def test_round_trip_through_the_fixed_matrices(tag):
    """unconvert_flat(convert_flat(x)) against the float64 chain pinv (W x) of the same stored matrices, within the bound of the
    two chained products: the first product's error, at most its own bound e1 per grid value, passes through |pinv|, and the
    second adds its bound on the values it sums.  That chain is x itself -- every layer map of G1 and G2 has full column rank
    (tools/gen_golden_ds1_geom.py), so pinv(W) W = I -- up to the float32 pinv: 1e-6 of its largest element per entry, the bound
    tests/test_ds1_geom_host.py holds it to, times the |grid values| a voxel sums."""
    f, gc = fixture(tag), geom_converter(tag)
    x = f["x"]
    Wf, Df = mats(f, "weight_mats"), mats(f, "pinv")
    back = gc.unconvert_flat(gc.convert_flat(x)).detach().cpu().numpy()
    y64, n1 = expand64(f, Wf, x, True)
    e1 = 2.0 * n1 * 2.0 ** -23 * expand64(f, Wf, x, True, absolute=True)[0]
    chain = collapse64(f, Df, y64, False)[0]
    carried = collapse64(f, Df, e1, False, absolute=True)[0]
    t2, n2 = collapse64(f, Df, np.abs(y64) + e1, False, absolute=True)
    err, bound = np.abs(back - chain), carried + 2.0 * n2 * 2.0 ** -23 * t2
    print(f"{tag}: round trip worst |err| / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}, max |err| {err.max():.2e}")
    assert (err <= bound).all()
    slack = collapse64(f, [1e-6 * np.abs(m).max() * np.ones_like(m) for m in Df], y64, False, absolute=True)[0]
    assert (np.abs(chain - x) <= slack).all()


def test_c_side_refusals():
    """Invalid descriptors and B = 0: CD_EINVAL with a message, from argument checks that launch nothing."""
    from calodiffusion_amd import engine
    lib = engine.load_library()
    engine.require_gpu()
    i32 = lambda *v: (C.c_int32 * len(v))(*v)  # noqa: E731
    out = C.c_void_p()
    good = dict(L=2, bound=i32(0, 2, 32), alpha=i32(1, 10), rin=i32(2, 3), A=10, R=3)
    bad = {"strictly increasing": dict(bound=i32(0, 32, 2)), "must equal alpha": dict(bound=i32(0, 2, 31)),
           "alpha must be 1 or alpha_out": dict(bound=i32(0, 6, 36), alpha=i32(3, 10)), "must be positive": dict(R=0),
           "layers, alpha_out and r_out must be positive": dict(L=0), "rin must be positive": dict(rin=i32(2, 0)),
           "not be null": dict(rin=None), "bound[0] must be 0": dict(bound=i32(1, 3, 33)),
           "8192 floats": dict(L=1, bound=i32(0, 300), alpha=i32(1), rin=i32(300), A=1, R=30)}
    for needle, change in bad.items():
        a = {**good, **change}
        rc = lib.cd_radial_create(a["L"], a["bound"], a["alpha"], a["rin"], a["A"], a["R"], C.byref(out), engine._stream())
        assert rc == -1 and needle in lib.cd_last_error().decode() and not out.value, (needle, rc, lib.cd_last_error())
    engine._check(lib.cd_radial_create(*good.values(), C.byref(out), engine._stream()))
    try:
        w, x, y = (torch.ones(n, device="cuda") for n in (15, 32, 60))
        s = engine._stream()
        calls = {"cd_radial_enc": lambda b, p: lib.cd_radial_enc(out, p, x.data_ptr(), y.data_ptr(), b, s),
                 "cd_radial_dec": lambda b, p: lib.cd_radial_dec(out, p, y.data_ptr(), x.data_ptr(), b, s),
                 "cd_radial_enc_vjp": lambda b, p: lib.cd_radial_enc_vjp(out, p, x.data_ptr(), y.data_ptr(), x.data_ptr(), None, b, s),
                 "cd_radial_dec_vjp": lambda b, p: lib.cd_radial_dec_vjp(out, p, y.data_ptr(), x.data_ptr(), y.data_ptr(), None, b, s)}
        for name, call in calls.items():
            for b, p, needle in ((0, w.data_ptr(), "batch must be positive"), (-2, w.data_ptr(), "batch must be positive"),
                                 (1, None, "must not be null")):
                assert call(b, p) == -1 and name in lib.cd_last_error().decode() and needle in lib.cd_last_error().decode(), name
        torch.cuda.synchronize()
        assert bool((x == 1).all()) and bool((y == 1).all())  # nothing ran
    finally:
        lib.cd_radial_destroy(out)
    with pytest.raises(ValueError, match="alpha must be 1 or alpha_out"):
        from calodiffusion_amd import geom1
        geom1._RadialMap([0, 6, 36], [3, 10], [2, 3], 10, 3)
