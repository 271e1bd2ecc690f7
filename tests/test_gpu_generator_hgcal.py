"""GPU (MI355X): HGCal generator files (format version 2) -- cd_geom_create_csr against cd_geom_create_ex, and
cd_generator_run_ex against the Python path it restates, ``model.generate(loader, steps[, geometry=conv])`` from
``model.noise_offset = 0`` (held to the reference's outputs by test_gpu_hgcal_geom.py and test_gpu_hgcal_model.py).  Every
comparison is bitwise: showers, layer energies, the sampler's Philox offset and the decoder's.

The models are the tiny pre-embedded config (form 0) and hgcal_model_cases' in-model config (form 1) over geometry "m", with three
energy columns whose EMAX / EMIN differ.  ``generate()`` squeezes the decoded showers, so a Python-path loader holds two showers or
more in all; batches of one are the second batch of a loader."""
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import gold
import generator_hgcal_cases as H
import hgcal_model_cases as K

pytestmark = pytest.mark.gpu


def bits_equal(a, b):
    """the same float32 bits everywhere (stricter than np.array_equal: NaN payloads and the sign of zero count)"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def same(a, b):
    return bits_equal(a.cpu().numpy(), b.cpu().numpy())


# ---------------------------------------------------------------------- cd_geom_create_csr against cd_geom_create_ex
def _maps(geometry, which, masked):
    """(dense values, mask or None) of one map: geometry "m" (8 layers, 61 cells, one layer with the centre cell only) or "t"
    (300 / 271 cells: more than one 256-thread block); masked: a trainable map's pattern, which keeps zeros"""
    if geometry == "m":
        conv = H.converter(trainable=masked)
        m = conv.embeder if which == "enc" else conv.decoder
        return m.mat.detach().clone(), (torch.as_tensor(m.mask) if masked else None)
    g = gold("hgcal_model_t")
    mat, mask = torch.tensor(g[f"t.{which}_mat"]), torch.tensor(g[f"t.{which}_mask"])
    if masked:
        mat = mat + torch.tensor(K.hashed_perturbation(tuple(mat.shape))) * mask
        mat.reshape(-1)[torch.nonzero(mask.reshape(-1)).reshape(-1)[::7]] = 0.0
    return mat, (mask if masked else None)


@pytest.mark.parametrize("geometry", ["m", "t"])
@pytest.mark.parametrize("which", ["enc", "dec"])
@pytest.mark.parametrize("masked", [False, True], ids=["frozen", "masked"])
def test_create_csr_equals_create_ex(geometry, which, masked):
    from calodiffusion_amd.hgcal import _PackedMap, map_entries
    mat, mask = _maps(geometry, which, masked)
    L, rows, cols = (int(v) for v in mat.shape)
    ptr, col, val = map_entries(mat, mask)
    if masked:
        assert (val == 0).any()
    want = _PackedMap(mat, not masked, mask=mask)  # (cd_geom_create_ex builds no column view over a mask)
    got = _PackedMap.from_entries(ptr, col, val, L, rows, cols, want_columns=True)
    gen = torch.Generator().manual_seed(7)
    x = torch.randn((3, 2, L, cols), generator=gen).cuda()
    gy = torch.randn((3, 2, L, rows), generator=gen).cuda()
    for scale, shift, first in ((1.0, 0.0, False), (3.1083, 0.0835, True), (3.1083, 0.0835, False)):
        assert same(got.apply(x, scale, shift, first), want.apply(x, scale, shift, first))
        dx_g, dm_g = got.apply_vjp(x, gy, scale, shift, first, True, True)
        dx_w, dm_w = want.apply_vjp(x, gy, scale, shift, first, True, True)
        assert same(dx_g, dx_w) and same(dm_g, dm_w)  # the transposed view with t_pos; ent_row
    if masked:
        want = _PackedMap(mat * mask, True)  # the sampled decode's map of a trainable decoder (Decoder._sampled_map)
    for per_batch in (False, True):
        a = got.decode_sparse(x.abs(), per_batch, None, 1234, 77)
        b = want.decode_sparse(x.abs(), per_batch, None, 1234, 77)
        assert same(a, b) and float(a.abs().sum()) > 0
    want.refresh(mat * 2)  # ent_row again: the values gathered from a dense tensor
    got.refresh(mat * 2)
    assert same(got.apply(x, 1.0, 0.0, False), want.apply(x, 1.0, 0.0, False))


def test_create_csr_refuses_every_violated_invariant():
    """CD_EINVAL with a message, checked on the host: nothing is uploaded (free memory unchanged) or launched"""
    from calodiffusion_amd.hgcal import _PackedMap, map_entries
    mat, _ = _maps("m", "dec", False)
    L, rows, cols = (int(v) for v in mat.shape)
    ptr, col, val = map_entries(mat)
    line = int(np.flatnonzero(np.diff(ptr)[1:] >= 2)[0]) + 1
    p = int(ptr[line])

    def changed(arr, at, value):
        out = arr.copy()
        out[at] = value
        return out

    swapped = col.copy()
    swapped[p], swapped[p + 1] = col[p + 1], col[p]
    bad = [("row_ptr\\[0\\]", changed(ptr, 0, 1), col, val), ("non-decreasing", changed(ptr, line, ptr[line + 1] + 1), col, val),
           ("non-decreasing", changed(ptr, line + 1, -1), col, val), ("outside", ptr, changed(col, p, cols), val),
           ("outside", ptr, changed(col, p, -1), val), ("strictly ascending", ptr, swapped, val),
           ("strictly ascending", ptr, changed(col, p, col[p + 1]), val), ("not finite", ptr, col, changed(val, p, np.nan)),
           ("not finite", ptr, col, changed(val, 0, np.inf))]
    _PackedMap.from_entries(ptr, col, val, L, rows, cols, want_columns=True)  # (the good arrays pass)
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0]
    for word, a, b, c in bad:
        with pytest.raises(ValueError, match=word):
            _PackedMap.from_entries(a, b, c, L, rows, cols, want_columns=True)
    with pytest.raises(ValueError, match="ends at"):
        _PackedMap.from_entries(changed(ptr, L * rows, len(col) + 1), col, val, L, rows, cols)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free


# ---------------------------------------------------------------------- the run against generate()
def loader_of(m, sizes, seed):
    """(E (b, 3), layers, None) batches: layers only where the model takes them from its caller"""
    from calodiffusion_amd.layerdiffusion import LayerDiffusion
    g = torch.Generator().manual_seed(seed)
    out = []
    for b in sizes:
        E = torch.rand((b, 3), generator=g)
        given = not isinstance(m, LayerDiffusion)
        out.append((E, torch.randn((b, K.LAYERS + 1), generator=g) if given else torch.zeros((b, 0)), None))
    return out


def python_path(m, loader, steps, conv=None, **decode):
    """(showers (n, L * N), layer energies per batch, final offset, the decoder's final offset) of model.generate from offset 0"""
    from calodiffusion_amd.layerdiffusion import LayerDiffusion
    layers = []
    if isinstance(m, LayerDiffusion):
        inner = m.sample_layers
        m.sample_layers = lambda *a, **k: (layers.append(inner(*a, **k)), layers[-1])[1]  # what generate() conditions on
    m.noise_offset = 0
    if conv is not None:
        conv.decoder.noise_offset = 0
    try:
        showers, _ = m.generate(loader, steps, geometry=conv, **decode)
    finally:
        m.__dict__.pop("sample_layers", None)
    if not layers:
        layers = [lay for _, lay, _ in loader]
    n = sum(E.shape[0] for E, _, _ in loader)
    return showers.reshape(n, -1), [lay.cpu().numpy() for lay in layers], m.noise_offset, conv.decoder.noise_offset if conv else 0


def c_path(gen, m, loader, **decode):
    from calodiffusion_amd.layerdiffusion import LayerDiffusion
    showers, layers, off, doff = [], [], 0, 0
    for E, lay, _ in loader:
        given = None if isinstance(m, LayerDiffusion) else lay.cuda()
        s, lout, off, doff = gen.run(E.cuda(), layers=given, seed=m.noise_seed, offset=off, decode_seed=1234, decode_offset=doff, **decode)
        showers.append(s.cpu().numpy())
        layers.append(lout.cpu().numpy())
    return np.concatenate(showers), layers, off, doff


def compare(gen, m, loader, steps, conv=None, **decode):
    want, want_layers, want_off, want_doff = python_path(m, loader, steps, conv, **decode)
    got, got_layers, got_off, got_doff = c_path(gen, m, loader, **decode)
    assert want.shape == (sum(E.shape[0] for E, _, _ in loader), gen.info["voxels"]) and np.isfinite(want).all() and want.max() > 0
    assert bits_equal(got, want)
    for a, b in zip(got_layers, want_layers):
        assert bits_equal(a, b)
    assert got_off == want_off and got_doff == want_doff
    return want


@pytest.fixture(scope="module")
def given_layers():
    """form 0, CaloDiffusion with given layers, DDPM (the tiny config's stochastic sampler), 3 steps"""
    from calodiffusion_amd.generator import Generator, export_generator
    m, conv = H.pre_embedded(False), H.converter(norm=True)
    return m, conv, Generator(export_generator(m, 3, geometry=conv))


@pytest.fixture(scope="module")
def two_stage():
    """form 0, LayerDiffusion: DDim layer stage of 6 steps, a step-program sampler (DPMPP2M) on the U-Net, 4 steps"""
    from calodiffusion_amd.generator import Generator, export_generator
    m, conv = H.pre_embedded(True, LAYER_STEPS=6, SAMPLER="DPMPP2M"), H.converter(norm=True)
    return m, conv, Generator(export_generator(m, 4, geometry=conv))


def test_form0_given_layers(given_layers):
    m, conv, gen = given_layers
    assert gen.info == dict(voxels=K.LAYERS * K.CELLS, layers=8, energy_columns=3, has_layer_stage=0, takes_layers=1, sample_steps=3,
                            layer_steps=0, format_version=2)
    loader = loader_of(m, (3, 2), 11)
    plain = compare(gen, m, loader, 3, conv)
    sampled = compare(gen, m, loader, 3, conv, sparse_decoding=True)
    assert conv.decoder.noise_offset == 5 * K.LAYERS * K.CELLS * K.E_GRID and not bits_equal(plain, sampled)
    compare(gen, m, loader[:1], 3, conv, sparse_decoding=True, sparse_per_batch=True)
    assert conv.decoder.noise_offset == K.LAYERS * K.CELLS * K.E_GRID


def test_form0_layerdiffusion(two_stage):
    m, conv, gen = two_stage
    assert gen.info["has_layer_stage"] == 1 and gen.info["layer_steps"] == 6
    loader = loader_of(m, (2, 1), 12)
    compare(gen, m, loader, 4, conv)
    compare(gen, m, loader, 4, conv, sparse_decoding=True)
    compare(gen, m, loader_of(m, (3,), 13), 4, conv, sparse_decoding=True, sparse_per_batch=True)


def test_form0_without_a_norm_samples_the_decoder_unscaled():
    """embed_mean 0, embed_std 1: the plain product, and no scaling launch before the sampled decode"""
    from calodiffusion_amd.generator import Generator, export_generator
    m, conv = H.pre_embedded(False, SAMPLER="DDim"), H.converter()
    gen = Generator(export_generator(m, 2, geometry=conv))
    loader = loader_of(m, (2,), 14)
    compare(gen, m, loader, 2, conv)
    compare(gen, m, loader, 2, conv, sparse_decoding=True)


@pytest.mark.parametrize("trainable", [False, True], ids=["frozen", "trainable"])
@pytest.mark.parametrize("sampler,steps", [("DDPM", 3), ("DPMPP2M", 4)])
def test_form1(trainable, sampler, steps):
    from calodiffusion_amd.generator import Generator, export_generator
    m = H.in_model(trainable, SAMPLER=sampler)
    gen = Generator(export_generator(m, steps))
    assert gen.info["voxels"] == K.LAYERS * K.CELLS and gen.info["energy_columns"] == 3
    compare(gen, m, loader_of(m, (3, 2) if sampler == "DDPM" else (2, 1), 15), steps)


# ---------------------------------------------------------------------- shards, the energy map, memory, refusals
def test_shards_are_slices_of_one_global_batch(two_stage):
    """each shard is bitwise the Python path's under set_noise_shard at the same batch; the layer energies (one workgroup per
    sample) are rows of the whole batch's"""
    m, conv, gen = two_stage
    E = loader_of(m, (4,), 16)[0][0]
    _, lay, _, _ = gen.run(E.cuda(), seed=m.noise_seed, offset=7)
    lays = []
    for first in (0, 2):
        s, lay_s, _, _ = gen.run(E[first:first + 2].cuda(), seed=m.noise_seed, offset=7, shard=(first, 4))
        m.set_noise_shard(first, 4)
        try:
            m.noise_offset = 7
            want, _ = m.generate([(E[first:first + 2], torch.zeros((2, 0)), None)], 4, geometry=conv)
        finally:
            m.set_noise_shard(0, 0)
        assert bits_equal(s.cpu().numpy(), want.reshape(2, -1)), first
        lays.append(lay_s)
    assert same(torch.cat(lays), lay)


def test_physical_energies_map_as_preprocess_hgcal_maps_them(two_stage):
    """energy_is_normalised = 0 on physical (B, 3) gen-info: the conditioning is PreprocessHGCal's E of the same values, bit for
    bit, in every column -- one ulp more on any column of E changes the layer energies"""
    from calodiffusion_amd.preprocess import PreprocessHGCal
    m, conv, gen = two_stage
    g = torch.Generator().manual_seed(8)
    lo, hi = torch.tensor(H.EMIN, dtype=torch.float32), torch.tensor(H.EMAX, dtype=torch.float32)
    phys = (lo + (hi - lo) * torch.rand((3, 3), generator=g)).cuda()
    cells = torch.rand((3, K.LAYERS, K.CELLS), generator=g).cuda()
    E, _, _ = PreprocessHGCal(m.config, conv, shower_scale=1.0)(cells, phys)
    a, lay_a, off_a, _ = gen.run(phys, seed=m.noise_seed, offset=0, normalised=False)
    b, lay_b, off_b, _ = gen.run(E, seed=m.noise_seed, offset=0, normalised=True)
    assert same(a, b) and same(lay_a, lay_b) and off_a == off_b
    for col in range(3):
        E1 = E.clone()
        E1[:, col] = torch.nextafter(E[:, col], E[:, col] + 1)
        assert not same(lay_a, gen.run(E1, seed=m.noise_seed, offset=0)[1]), col


def test_run_allocates_nothing(given_layers):
    m, conv, gen = given_layers
    E, lay, _ = loader_of(m, (3,), 17)[0]
    E, lay = E.cuda(), lay.cuda()
    ws = gen.workspace(3)
    for decode in (dict(), dict(sparse_decoding=True)):
        out = gen.run(E, layers=lay, seed=m.noise_seed, workspace=ws, **decode)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        for _ in range(2):
            out = gen.run(E, layers=lay, seed=m.noise_seed, workspace=ws, **decode)
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free0
        assert np.isfinite(out[0].cpu().numpy()).all()


def test_run_refusals_launch_nothing(two_stage):
    from calodiffusion_amd.generator import Generator, export_generator
    m, conv, gen = two_stage
    E = loader_of(m, (2,), 18)[0][0].cuda()
    ws = torch.zeros(gen.workspace_bytes(2), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="workspace too small"):
        gen.run(E, workspace=ws[:-1])
    with pytest.raises(ValueError, match="generates its layer energies itself"):
        gen.run(E, layers=torch.zeros((2, K.LAYERS + 1), device="cuda"), workspace=ws)
    with pytest.raises(ValueError, match=r"E must have shape \(batch, 3\)"):
        gen.run(E[:, :2], workspace=ws)
    torch.cuda.synchronize()
    assert not ws.any()  # nothing was launched: the first launch of a run writes the start tensor there
    inside = Generator(export_generator(H.in_model(False), 2))
    ws1 = torch.zeros(inside.workspace_bytes(2), dtype=torch.uint8, device="cuda")
    lay = torch.zeros((2, K.LAYERS + 1), device="cuda")
    with pytest.raises(ValueError, match="sparse_mode != 0 needs a file whose decoder has a column view"):
        inside.run(E, layers=lay, sparse_decoding=True, workspace=ws1)
    torch.cuda.synchronize()
    assert not ws1.any()


# ---------------------------------------------------------------------- from C
def write_python_reference(out_dir):
    """the form-0 two-stage file, a file of 3 + 2 rows of three energies, and the showers model.generate gives for them: plain,
    and sampled per shower"""
    from calodiffusion_amd.generator import export_generator
    m, conv = H.pre_embedded(True, LAYER_STEPS=6, SAMPLER="DPMPP2M"), H.converter(norm=True)
    loader = loader_of(m, (3, 2), 11)
    export_generator(m, 4, path=os.path.join(out_dir, "hgcal.cdgen"), geometry=conv)
    torch.cat([E for E, _, _ in loader]).numpy().astype("<f4").tofile(os.path.join(out_dir, "e.f32"))
    for name, decode in (("plain", dict()), ("sampled", dict(sparse_decoding=True))):
        showers, _, offset, _ = python_path(m, loader, 4, conv, **decode)
        showers.astype("<f4").tofile(os.path.join(out_dir, f"want_{name}.f32"))
    print(f"next offset {offset}")


def test_c_example_writes_the_python_showers(tmp_path):
    """tools/cd_generate_example.c as a fresh process on three energy columns, plain and sampled per shower: bytewise the Python
    path's showers, both sides with the convolution timer off (CD_NO_AUTOTUNE), the Python path as a fresh process of its own
    (this module as a script)."""
    import sys
    from calodiffusion_amd import build as b
    assert os.path.exists(b.EXAMPLE), f"{b.EXAMPLE} was not built (calodiffusion_amd.build compiles tools/cd_generate_example.c)"
    env = dict(os.environ, CD_NO_AUTOTUNE="1")
    ref = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), str(tmp_path)], env=env,
                         capture_output=True, text=True)
    assert ref.returncode == 0, (ref.returncode, ref.stdout[-2000:], ref.stderr[-2000:])
    for name, sparse in (("plain", []), ("sampled", ["0", "1"])):
        r = subprocess.run(["timeout", "-k", "10", "120", b.EXAMPLE, str(tmp_path / "hgcal.cdgen"), str(tmp_path / "e.f32"),
                            str(tmp_path / "out.f32"), "3", "1234", "0"] + sparse, env=env, capture_output=True, text=True)
        assert r.returncode == 0, (name, r.returncode, r.stdout, r.stderr)
        want = (tmp_path / f"want_{name}.f32").read_bytes()
        assert len(want) == 5 * K.LAYERS * K.CELLS * 4 and (tmp_path / "out.f32").read_bytes() == want, name
        assert r.stdout.split("next offset")[1].strip() == ref.stdout.split("next offset")[1].strip()


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    write_python_reference(sys.argv[1])
