"""GPU (MI355X): Dataset-0/1 pre-processing on the device in both directions (cd_preprocess_ds1 / cd_reverse_norm_ds1 under
preprocess.PreprocessDS1 / preprocess_shower, postprocess.ReverseNormCaloChall and generate(geometry=)) against the reference's own
preprocess_shower / DataLoaderCaloChall / ReverseNormCaloChall outputs (tests/golden/ds1_preprocess.npz,
tools/gen_golden_ds1_preprocess.py) on the two synthetic binning files.

Bars: those tests/test_gpu_preprocess.py and test_reverse_norm_on_device hold the same reference functions to -- rel L2 1e-5 per
tensor, 3e-5 per (shower, layer) row and per layerE element, zero pattern on > 99.9 % of the voxels, the round trip within twice
the reference's own (the fixture's rt.<tag>).  Everything called the same computation in two forms is compared bitwise."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import gold
import ds1_preprocess_cases as P
from ds1_preprocess_cases import rel_l2, worst_row

pytestmark = pytest.mark.gpu


def _raw(tag):
    g = gold("ds1_preprocess")
    return g[f"{tag}.showers"], g[f"{tag}.incident_energies"]


def _pre(tag, **over):
    from calodiffusion_amd.preprocess import PreprocessDS1
    return PreprocessDS1(P.config(tag, **over), P.geometry(tag))


def _reverse(tag, voxels, e01, layerE, **over):
    from calodiffusion_amd.postprocess import ReverseNorm
    cfg = P.config(tag)
    dnum, orig, smap = P.CASES[tag]
    kw = dict(emax=cfg["EMAX"], emin=cfg["EMIN"], max_deposit=cfg["MAXDEP"], logE=cfg["logE"], layerE=layerE, showerMap=smap,
              dataset_num=dnum, orig_shape=orig, ecut=float(cfg["ECUT"]), geometry=P.geometry(tag))
    kw.update(over)
    return ReverseNorm(voxels, e01, **kw)


@pytest.mark.parametrize("logE", [True, False])
@pytest.mark.parametrize("tag", P.TAGS)
def test_forward_matches_the_reference(tag, logE):
    """preprocess_shower (reference signature, numpy in / numpy out, the geometry read from the binning file) and PreprocessDS1
    (device tensors) against the reference.  Every shower and every element is compared."""
    from calodiffusion_amd.preprocess import preprocess_shower
    g, cfg = gold("ds1_preprocess"), P.config(tag, logE=logE)
    dnum, orig, smap = P.CASES[tag]
    V, (L, A, R), _ = P.SHAPES[tag[:2]]
    raw, e = _raw(tag)
    want, want_l = g[f"{tag}.data"], (g[f"{tag}.layerE"] if "layer" in smap else None)
    want_E = g[f"{tag}.E"] if logE else g[f"{tag}.E_lin"]

    got, got_l = preprocess_shower(raw * P.SCALE, e * P.SCALE, None, P.XML[tag[:2]], smap, dataset_num=dnum, orig_shape=orig,
                                   ecut=cfg["ECUT"], max_deposit=cfg["MAXDEP"])
    assert got.shape == want.shape and got.dtype == np.float32 and np.isfinite(got).all()
    e_all, e_row = rel_l2(got, want), worst_row(got, want, P.segments(tag))
    print(f"[{tag} logE={logE}] voxels: rel L2 {e_all:.3e}, worst (shower, layer) row {e_row:.3e}")
    assert e_all < 1e-5 and e_row < 3e-5
    if want_l is None:
        assert got_l is None
    else:
        assert got_l.shape == want_l.shape == (P.B, L + 1) and got_l.dtype == np.float32 and np.isfinite(got_l).all()
        l_all = rel_l2(got_l, want_l)
        l_el = float((np.abs(got_l.astype(np.float64) - want_l) / np.abs(want_l)).max())
        print(f"[{tag} logE={logE}] layerE: rel L2 {l_all:.3e}, worst element {l_el:.3e}")
        assert l_all < 1e-5 and l_el < 3e-5

    E, layers, data = _pre(tag, logE=logE)(raw, e)
    assert E.is_cuda and data.is_cuda and E.shape == (P.B, 1) and E.dtype == data.dtype == torch.float32
    assert data.shape == ((P.B, V) if orig else (P.B, 1, L, A, R))
    err_E = rel_l2(E.cpu().numpy(), want_E)
    print(f"[{tag} logE={logE}] E: rel L2 {err_E:.3e}")
    assert err_E < 1e-5
    # the loader's scaling happens inside the same call: the same float32 products, so the same bits
    assert np.array_equal(data.cpu().numpy().reshape(P.B, -1), got)
    assert (layers is None and got_l is None) or np.array_equal(layers.cpu().numpy(), got_l)


@pytest.mark.parametrize("tag", P.TAGS)
def test_reverse_matches_the_reference(tag):
    """ReverseNormCaloChall on the fixture's normalised inputs: test_reverse_norm_on_device's bars."""
    g = gold("ds1_preprocess")
    smap = P.CASES[tag][2]
    lE = g[f"{tag}.rev.layerE"] if "layer" in smap else None
    want, want_en = g[f"{tag}.rev.out"], g[f"{tag}.rev.energy"]
    for geo in (dict(), dict(geometry=None, binning_file=P.XML[tag[:2]])):
        got, energy = _reverse(tag, g[f"{tag}.rev.voxels"], g[f"{tag}.rev.e"], lE, **geo)
        assert got.shape == want.shape and got.dtype == np.float32 and np.isfinite(got).all()
        err, same = rel_l2(got, want), float(((got == 0) == (want == 0)).mean())
        print(f"[{tag}] reverse: rel L2 {err:.3e}, zero pattern agrees on {same:.6f} ({float((want == 0).mean()):.3f} zeros)")
        assert err < 1e-5 and same > 0.999
        assert np.array_equal(np.asarray(energy, dtype=np.float32), want_en)
    if "layer" in smap:
        assert (got >= 0).all()


@pytest.mark.parametrize("tag", P.TAGS)
def test_round_trip(tag):
    """ReverseNorm(PreprocessDS1(raw)) against raw x scale.  The map is not exactly invertible (logit's alpha, ECUT, the
    pseudo-inverse of the grid form), so the bar is the reference's own round trip on the same inputs (rt.<tag>) times 2 for
    fp32 reordering."""
    g = gold("ds1_preprocess")
    raw, e = _raw(tag)
    E, layers, data = _pre(tag)(raw, e)
    back, energy = _reverse(tag, data.cpu().numpy(), E.cpu().numpy(), None if layers is None else layers.cpu().numpy())
    want, ref_rt = raw * P.SCALE, float(g[f"rt.{tag}"])
    err, same = rel_l2(back, want), float(((back == 0) == (want == 0)).mean())
    print(f"[{tag}] round trip: rel L2 {err:.3e} (reference's own {ref_rt:.3e}), zero pattern agrees on {same:.6f}")
    assert back.shape == want.shape
    assert err < 2 * ref_rt
    assert same >= 0.999
    assert rel_l2(np.reshape(energy, (-1, 1)), e * P.SCALE) < 1e-5


def _consts32(c):
    return (C.c_float * 6)(c["logit_mean"], c["logit_std"], c["totalE_mean"], c["totalE_std"], c["layers_mean"], c["layers_std"])


def test_grid_form_is_the_composition_of_the_existing_calls():
    """Forward: cd_radial_enc of the scaled showers into a temporary, then cd_preprocess on dims (L, A, R) -- two launches.
    Reverse: cd_reverse_norm_staged(stage 1), cd_radial_dec, cd_reverse_norm_staged(stage 2) on the flat row -- three.  Bitwise."""
    from calodiffusion_amd import engine
    from calodiffusion_amd.postprocess import DATASET1_PARAMS
    tag = "ph.grid.plain"
    g, cfg, gc = gold("ds1_preprocess"), P.config(tag), P.geometry(tag)
    V, (L, A, R), _ = P.SHAPES["ph"]
    lib, rm, c = engine.load_library(), gc.radial_map(), DATASET1_PARAMS[1]
    conv_w, unconv_w = gc._fixed_weights()
    raw, e = _raw(tag)
    E, layers, data = _pre(tag)(raw, e)
    assert layers is None

    x = torch.from_numpy(raw).cuda() * float(P.SCALE)
    en = (torch.from_numpy(e).cuda() * float(P.SCALE)).reshape(-1).contiguous()
    tmp = rm.enc(conv_w, x)
    out, e_out = torch.empty_like(tmp), torch.empty((P.B, 1), device="cuda")
    status = torch.empty((1,), dtype=torch.int32, device="cuda")
    engine._check(lib.cd_preprocess(tmp.data_ptr(), en.data_ptr(), out.data_ptr(), None, e_out.data_ptr(), status.data_ptr(), P.B,
                                    (C.c_int32 * 3)(L, A, R), _consts32(c), float(cfg["MAXDEP"]), float(cfg["EMIN"]),
                                    float(cfg["EMAX"]), 1, 1.0, engine._stream()))
    assert int(status.item()) == 0
    assert torch.equal(out, data) and torch.equal(e_out, E)

    vox, e01 = torch.from_numpy(g[f"{tag}.rev.voxels"]).cuda(), g[f"{tag}.rev.e"]
    got, energy = _reverse(tag, vox, e01, None)
    en = torch.from_numpy(np.ascontiguousarray(np.asarray(energy, dtype=np.float32).reshape(-1))).cuda()

    def staged(v, energies, dims, stage):
        o = torch.empty((P.B, int(np.prod(dims))), dtype=torch.float32, device="cuda")
        engine._check(lib.cd_reverse_norm_staged(v.data_ptr(), engine._ptr(energies), None, o.data_ptr(), P.B, (C.c_int32 * 3)(*dims),
                                                 _consts32(c), float(cfg["MAXDEP"]), float(cfg["ECUT"]), 1e-6, 1e-6, stage,
                                                 engine._stream()))
        return o
    s1 = staged(vox, None, (L * A * R, 1, 1), 1)
    flat = rm.dec(unconv_w, s1.reshape(P.B, 1, L, A, R))
    want = staged(flat, en, (1, 1, V), 2)
    assert np.array_equal(want.cpu().numpy(), got)
    assert (got < 0).sum() == 0 and (got == 0).any()   # ECUT removes the negatives; they are not clamped before the scaling


@pytest.mark.parametrize("tag", P.TAGS)
def test_rows_do_not_depend_on_the_batch_or_the_input_kind(tag):
    """Halves processed separately, a single shower, and the first rows of a 130-shower call (more showers than one pass of
    some grids, an odd count) are bitwise the rows of the 8-shower call; numpy and device-tensor input give equal bits.  Both
    directions."""
    g = gold("ds1_preprocess")
    raw, e = _raw(tag)
    pre = _pre(tag)
    whole = pre(raw, e)
    lo, hi, one = pre(raw[:4], e[:4]), pre(raw[4:], e[4:]), pre(raw[:1], e[:1])
    dev = pre(torch.from_numpy(raw).cuda(), torch.from_numpy(e).cuda())
    big = pre(np.tile(raw, (17, 1))[:130], np.tile(e, (17, 1))[:130])
    for w, a, b, o, d, m in zip(whole, lo, hi, one, dev, big):
        if w is None:
            assert a is None and b is None and o is None and d is None and m is None
            continue
        assert torch.equal(torch.cat([a, b]), w) and torch.equal(o, w[:1]) and torch.equal(d, w) and torch.equal(m[:8], w)
        assert torch.equal(m[128:130], w[:2])
    smap = P.CASES[tag][2]
    vox, e01 = g[f"{tag}.rev.voxels"], g[f"{tag}.rev.e"]
    lE = g[f"{tag}.rev.layerE"] if "layer" in smap else None
    cut = lambda a, s: None if a is None else a[s]  # noqa: E731
    tile = lambda a: None if a is None else np.tile(a, (17,) + (1,) * (a.ndim - 1))[:130]  # noqa: E731
    back = _reverse(tag, vox, e01, lE)[0]
    parts = [_reverse(tag, vox[s], e01[s], cut(lE, s))[0] for s in (slice(0, 4), slice(4, 8))]
    assert np.array_equal(np.concatenate(parts), back)
    assert np.array_equal(_reverse(tag, vox[:1], e01[:1], cut(lE, slice(0, 1)))[0], back[:1])
    assert np.array_equal(_reverse(tag, tile(vox), tile(e01), tile(lE))[0][:8], back)
    assert np.array_equal(_reverse(tag, torch.from_numpy(vox).cuda(), e01, lE)[0], back)


@pytest.mark.parametrize("tag", P.TAGS)
def test_a_shower_without_energy_raises(tag):
    """A wholly empty shower, or a zero incident energy, raises ValueError naming the row; the next clean call works, and the
    empty layer of shower 0 is ordinary data."""
    from calodiffusion_amd.preprocess import preprocess_shower
    dnum, orig, smap = P.CASES[tag]
    raw, e = _raw(tag)
    pre = _pre(tag)
    empty = raw.copy()
    empty[5] = 0.0
    with pytest.raises(ValueError, match="shower 5 "):
        pre(empty, e)
    with pytest.raises(ValueError, match="shower 5 "):
        preprocess_shower(empty * P.SCALE, e * P.SCALE, None, P.XML[tag[:2]], smap, dataset_num=dnum, orig_shape=orig, max_deposit=3.1)
    no_e = e.copy()
    no_e[2] = 0.0
    with pytest.raises(ValueError, match="shower 2 "):
        pre(raw, no_e)
    E, layers, data = pre(raw, e)   # the flag is per call
    assert torch.isfinite(data).all() and torch.isfinite(E).all() and (layers is None or torch.isfinite(layers).all())
    _, _, bound = P.SHAPES[tag[:2]]
    assert not raw[0, bound[1]:bound[2]].any()
    if orig:   # the empty layer: every voxel is logit(0), and its share too
        assert len(torch.unique(data[0, bound[1]:bound[2]])) == 1
        assert layers is None or (float(layers[0, 2]) < float(layers[0, 1:].max()) and float(layers[0, 2]) == float(layers[0, 1:].min()))


def test_generate_ends_in_physical_showers():
    """generate(geometry=NN_embed) on the Dataset-1 model: physical (N, V) showers, bitwise ReverseNormCaloChall applied by hand
    to the normalised-space output of the same noise.  (The 4-step samples of this untrained model reach |x| ~ 120: float32
    exp overflows on them, and reverse_logit saturates at 1 where the reference's exp / (1 + exp) would be NaN.)"""
    from ds1_model_cases import inputs as _inputs, model as _model
    import ds1_model_cases as K
    from calodiffusion_amd.postprocess import ReverseNormCaloChall
    m = _model()
    _, E, layers = _inputs("x", "E", "layers")
    loader = [(E.cpu(), layers.cpu(), None), (E[:2].cpu(), layers[:2].cpu(), None)]
    offset = m.noise_offset
    gen, en = m.generate(loader, 4, geometry=m.NN_embed)
    assert gen.shape == (5, K.V) and en.shape == (5, 1) and gen.dtype == np.float32
    assert np.isfinite(gen).all() and (gen >= 0).all() and (gen > 0).any()
    m.noise_offset = offset
    norm, e01 = m.generate(loader, 4, reverse_norm=False)
    cfg = m.config
    lE = np.concatenate([layers.cpu().numpy(), layers[:2].cpu().numpy()])
    want, energy = ReverseNormCaloChall(norm, e01, emax=cfg["EMAX"], emin=cfg["EMIN"], max_deposit=cfg["MAXDEP"], logE=cfg["logE"],
                                        layerE=lE, showerMap=cfg["SHOWERMAP"], dataset_num=1, orig_shape=True, ecut=float(cfg["ECUT"]),
                                        geometry=m.NN_embed.gc)
    assert np.array_equal(gen, want) and np.array_equal(en, np.reshape(energy, (5, 1)))
    with pytest.raises(TypeError, match="GeomConverter"):
        m.generate(loader, 4, geometry=object())


def test_one_training_step_from_raw_data():
    """compute_loss on PreprocessDS1(raw) equals compute_loss on the reference-pre-processed tensors of the fixture (same noise,
    same sigma draw) within the relative 1e-5 tests/test_gpu_train.py holds the loss to; backward reaches every parameter, the
    geometry embedding's matrices included."""
    from ds1_model_cases import model as _model
    from calodiffusion_amd.preprocess import PreprocessDS1
    tag = "ph.flat.layer"
    g = gold("ds1_preprocess")
    m = _model(fresh=True)
    m.train()
    raw, e = _raw(tag)
    E, layers, data = PreprocessDS1(m.config, m.NN_embed)(raw, e)
    gen = torch.Generator().manual_seed(11)
    noise, rnd = torch.randn(data.shape, generator=gen).cuda(), torch.randn((P.B,), generator=gen).cuda()
    want_in = [torch.from_numpy(g[f"{tag}.{k}"]).cuda() for k in ("data", "E", "layerE")]
    got = m.compute_loss(data, E, noise=noise, layers=layers, rnd_normal=rnd)
    want = m.compute_loss(want_in[0], want_in[1], noise=noise, layers=want_in[2], rnd_normal=rnd)
    assert got.requires_grad and got.dim() == 0
    got.backward()
    named = dict(m.named_parameters())
    assert any(k.startswith("NN_embed.encs") for k in named) and any(k.startswith("NN_embed.decs") for k in named)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in named.values())
    assert all(float(named[k].grad.abs().max()) > 0 for k in named if k.startswith("NN_embed"))
    print(f"loss from raw data {float(got):.8f}, from the reference's tensors {float(want):.8f}")
    assert np.isfinite(float(want)) and abs(float(got) - float(want)) <= 1e-5 * abs(float(want))


def test_bad_shapes_are_refused_before_the_launch():
    pre = _pre("ph.flat.layer")
    with pytest.raises(ValueError, match="voxels"):
        pre(np.ones((2, 367), dtype=np.float32), np.ones((2,), dtype=np.float32))
    with pytest.raises(ValueError, match="incident energies"):
        pre(np.ones((2, 368), dtype=np.float32), np.ones((3,), dtype=np.float32))
    with pytest.raises(ValueError, match="no showers"):
        pre(np.ones((0, 368), dtype=np.float32), np.ones((0,), dtype=np.float32))
    ones = np.ones((2, 1), dtype=np.float32)
    with pytest.raises(ValueError, match="368 values"):
        _reverse("ph.flat.layer", np.zeros((2, 1500), dtype=np.float32), ones, np.zeros((2, 6), dtype=np.float32))
    with pytest.raises(ValueError, match="1500 values"):
        _reverse("ph.grid.plain", np.zeros((2, 368), dtype=np.float32), ones, None)
    with pytest.raises(ValueError, match="layerE"):
        _reverse("ph.flat.layer", np.zeros((2, 368), dtype=np.float32), ones, np.zeros((2, 5), dtype=np.float32))
    with pytest.raises(ValueError, match="incident energies"):
        _reverse("ph.flat.plain", np.zeros((2, 368), dtype=np.float32), np.ones((3, 1), dtype=np.float32), None)
