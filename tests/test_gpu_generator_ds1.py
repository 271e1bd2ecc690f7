"""GPU (MI355X): Dataset-0/1 generator files (format version 3) and the two-stage in-model HGCal file -- cd_generator_run[_ex]
against the Python path it restates, ``model.generate(loader, steps[, geometry=])`` from ``model.noise_offset = 0`` (held to the
reference's outputs by test_gpu_layer_inmodel.py, test_gpu_ds1_model.py and test_gpu_ds1_preprocess.py).  The launches are the
same, so every comparison is bitwise: showers, layer energies and the Philox offset the model is left at.

The incident energies of the Dataset-0/1 loaders are drawn where this host's numpy float32 power is the correctly rounded one
(generator_ds1_cases.energies; test_gpu_generator.py has the reasons)."""
import os
import subprocess

import numpy as np
import pytest
import torch

import ds1_model_cases as K1
import generator_ds1_cases as H
import layer_inmodel_cases as L
import narrow_cases as KN

pytestmark = pytest.mark.gpu

STEPS = H.STEPS


def bits_equal(a, b):
    """the same float32 bits everywhere (stricter than np.array_equal: NaN payloads and the sign of zero count)"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def loader_of(m, sizes, seed):
    """(E, layers, None) batches: layers only where the model takes them from its caller"""
    from calodiffusion_amd.layerdiffusion import LayerDiffusion
    cols = 3 if m.hgcal else 1
    g = torch.Generator().manual_seed(seed)
    E = torch.rand((sum(sizes), cols), generator=g) if m.hgcal else H.energies(sum(sizes), seed)
    given = m.layer_cond and not isinstance(m, LayerDiffusion)
    out, lo = [], 0
    for b in sizes:
        out.append((E[lo:lo + b], torch.randn((b, m.config["SHAPE_FINAL"][2] + 1), generator=g) if given else torch.zeros((b, 0)), None))
        lo += b
    return out


def python_path(m, loader, steps, geometry, sample_offset=0, offset=0):
    """(showers (n, V), layer energies per batch or None, final offset) of model.generate from `offset`"""
    from calodiffusion_amd.layerdiffusion import LayerDiffusion
    layers = []
    if isinstance(m, LayerDiffusion):
        inner = m.sample_layers
        m.sample_layers = lambda *a, **k: (layers.append(inner(*a, **k)), layers[-1])[1]  # what generate() conditions on
    m.noise_offset = offset
    try:
        showers, _ = m.generate(loader, steps, sample_offset=sample_offset, geometry=geometry)
    finally:
        m.__dict__.pop("sample_layers", None)
    if not layers and m.layer_cond:
        layers = [lay for _, lay, _ in loader]
    return np.reshape(showers, (showers.shape[0], -1)), [lay.cpu().numpy() for lay in layers] or None, m.noise_offset


def c_path(gen, m, loader, offset=0):
    """the same loader through cd_generator_run_ex, chaining next_offset"""
    from calodiffusion_amd.layerdiffusion import LayerDiffusion
    showers, layers, off = [], [], offset
    for E, lay, _ in loader:
        given = lay.cuda() if m.layer_cond and not isinstance(m, LayerDiffusion) else None
        s, lout, off = gen.run(E.cuda(), layers=given, seed=m.noise_seed, offset=off)[:3]
        showers.append(s.cpu().numpy())
        if lout is not None:
            layers.append(lout.cpu().numpy())
    return np.concatenate(showers), layers or None, off


def geometries(m, gc=None):
    """(generate()'s geometry=, export_generator()'s geometry=)"""
    if m.hgcal:
        return None, None
    return (m.NN_embed, None) if m.do_embed else (gc, gc)


def compare(m, sizes, steps, gc=None, sample_offset=0, seed=11):
    from calodiffusion_amd.generator import Generator, export_generator
    gen_geo, exp_geo = geometries(m, gc)
    loader = loader_of(m, sizes, seed)
    gen = Generator(export_generator(m, steps, sample_offset=sample_offset, geometry=exp_geo))
    want, want_layers, want_off = python_path(m, loader, steps, gen_geo, sample_offset)
    got, got_layers, got_off = c_path(gen, m, loader)
    assert want.shape == (sum(sizes), gen.info["voxels"]) and np.isfinite(want).all() and want.max() > 0
    assert bits_equal(got, want)
    assert (got_layers is None) == (want_layers is None)
    for a, b in zip(got_layers or [], want_layers or []):
        assert bits_equal(a, b)
    assert got_off == want_off
    return gen, loader, want


@pytest.fixture(scope="module")
def photon_two_stage():
    """the form the reference's CI runs: LayerDiffusion over 'orig-NN', DDim on both stages; two consecutive batches (3 + 2)
    continue one Philox stream"""
    m = H.two_stage("ph")
    gen, loader, want = compare(m, (3, 2), STEPS)
    return m, gen, loader, want


def test_photon_two_stage_two_batches(photon_two_stage):
    m, gen, loader, want = photon_two_stage
    assert gen.info == dict(voxels=K1.V, layers=5, energy_columns=1, has_layer_stage=1, takes_layers=1, sample_steps=STEPS,
                            layer_steps=L.LAYER_STEPS, format_version=3)
    assert gen.geometry == dict(geometry="radial", form=1, state_shape=(K1.V,))
    assert (want >= 0).all()
    # the second batch alone from the offset the first one ends at: the stream is one
    first = c_path(gen, m, loader[:1])
    second = c_path(gen, m, loader[1:], offset=first[2])
    assert bits_equal(second[0], want[3:]) and not bits_equal(c_path(gen, m, loader[1:])[0], want[3:])


def test_photon_given_layers():
    gen, _, _ = compare(H.photon_given(), (2, 1), STEPS)
    assert gen.info["has_layer_stage"] == 0 and gen.info["takes_layers"] == 1 and gen.info["format_version"] == 3


def test_pion_two_stage_narrow_widths():
    """[16, 16, 16, 32] in the file: the plan widens inside cd_generator_create"""
    gen, _, _ = compare(H.two_stage("pi"), (2,), STEPS)
    assert gen.info["voxels"] == KN.V and gen.info["layers"] == 7 and gen.geometry["state_shape"] == (KN.V,)


def test_form_0_on_the_converted_grid():
    m, gc = H.on_the_grid()
    gen, _, want = compare(m, (2, 1), STEPS, gc=gc)
    assert gen.geometry == dict(geometry="radial", form=0, state_shape=(1,) + K1.GRID)
    assert gen.info["voxels"] == K1.V and gen.info["takes_layers"] == 0


def test_hgcal_in_model_two_stage():
    gen, _, _ = compare(H.two_stage("hg"), (2, 2), STEPS)
    assert gen.info["format_version"] == 2 and gen.info["has_layer_stage"] == 1 and gen.info["energy_columns"] == 3
    assert gen.geometry == dict(geometry="hgcal", form=1, state_shape=L.STATE["hg"])


def test_a_step_program_sampler_on_the_flat_state():
    compare(H.photon_given(SAMPLER="DPMPP2M"), (2, 1), 5)


def test_step_noise_and_a_sample_offset():
    """per-step device noise on both stages of the flat state, from the stream position and stride"""
    compare(H.two_stage("ph", SAMPLER="DDPM", LAYER_SAMPLER="DDPM"), (2, 2), 4)
    compare(H.two_stage("ph"), (2,), 5, sample_offset=2)


def test_the_generator_of_a_regular_grid_reports_no_geometry():
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    from calodiffusion_amd.configs import load_config
    from calodiffusion_amd.generator import Generator, export_generator
    cfg = dict(load_config("dataset3"), LAYER_SIZE_UNET=[16, 16, 16, 16])
    torch.manual_seed(1234)
    gen = Generator(export_generator(CaloDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"]), 2))
    assert gen.geometry == dict(geometry=None, form=-1, state_shape=(1, 45, 50, 18))


# ---------------------------------------------------------------------- sharding, the energy map, memory, refusals
# Every shard draws its rows of the SAME global noise tensors, so B = 4 as 2 + 2 is the single run of 4, bitwise: showers and layer
# energies.  (On the 5 x 10 x 30 grid the U-Net's kernels tile a batch of 2 and a batch of 4 alike; on Dataset 2's larger grid they do
# not, which is why tests/test_gpu_generator.py holds its shards to a tolerance.)  Each shard is also bitwise the Python path's under
# the same set_noise_shard.


def test_shards_are_slices_of_one_global_batch(photon_two_stage):
    m, gen, _, _ = photon_two_stage
    E = H.energies(4, 5)
    whole, lay, off = gen.run(E.cuda(), seed=m.noise_seed, offset=7)
    parts, lays = [], []
    for first in (0, 2):
        s, lay_s, _ = gen.run(E[first:first + 2].cuda(), seed=m.noise_seed, offset=7, shard=(first, 4))
        m.set_noise_shard(first, 4)
        try:
            want, _, _ = python_path(m, [(E[first:first + 2], torch.zeros((2, 0)), None)], STEPS, m.NN_embed, offset=7)
        finally:
            m.set_noise_shard(0, 0)
        assert bits_equal(s.cpu().numpy(), want), first
        parts.append(s)
        lays.append(lay_s)
    assert bits_equal(torch.cat(parts).cpu().numpy(), whole.cpu().numpy())
    assert bits_equal(torch.cat(lays).cpu().numpy(), lay.cpu().numpy())
    # and the Python path: the two shards under set_noise_shard are its single run of the four
    single, _, _ = python_path(m, [(E, torch.zeros((4, 0)), None)], STEPS, m.NN_embed, offset=7)
    assert bits_equal(whole.cpu().numpy(), single)


def test_physical_energies_map_as_preprocess_maps_them(photon_two_stage):
    """energy_is_normalised = 0: the conditioning is PreprocessDS1's e_out of the same energies, bit for bit -- fed back as
    normalised input it gives the same showers and layer energies, which any other bit of e would change"""
    from calodiffusion_amd.preprocess import PreprocessDS1
    m, gen, _, _ = photon_two_stage
    g = torch.Generator().manual_seed(8)
    phys = (0.3 + 4000.0 * torch.rand((3,), generator=g)).cuda()
    showers = torch.rand((3, K1.V), generator=g).cuda()
    E, _, _ = PreprocessDS1(m.config, m.NN_embed.gc, shower_scale=1.0)(showers, phys)
    a, lay_a, off_a = gen.run(phys, seed=m.noise_seed, offset=0, normalised=False)
    b, lay_b, off_b = gen.run(E, seed=m.noise_seed, offset=0, normalised=True)
    assert bits_equal(a.cpu().numpy(), b.cpu().numpy()) and bits_equal(lay_a.cpu().numpy(), lay_b.cpu().numpy()) and off_a == off_b
    assert not bits_equal(lay_a.cpu().numpy(), gen.run(torch.nextafter(E, E + 1), seed=m.noise_seed, offset=0)[1].cpu().numpy())


def test_run_allocates_nothing(photon_two_stage):
    m, gen, loader, _ = photon_two_stage
    E = loader[0][0].cuda()
    ws = gen.workspace(E.shape[0])
    out = gen.run(E, seed=m.noise_seed, workspace=ws)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(2):
        out = gen.run(E, seed=m.noise_seed, workspace=ws)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
    assert np.isfinite(out[0].cpu().numpy()).all()


def test_run_refusals_launch_nothing(photon_two_stage):
    from calodiffusion_amd import engine
    from calodiffusion_amd.generator import Generator
    m, gen, loader, _ = photon_two_stage
    E = loader[0][0].cuda()
    B = E.shape[0]
    ws = torch.zeros(gen.workspace_bytes(B), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="workspace too small"):
        gen.run(E, workspace=ws[:-1])
    with pytest.raises(ValueError, match="sparse_mode != 0 needs a file whose decoder has a column view"):
        gen.run(E, workspace=ws, sparse_decoding=True)
    with pytest.raises(ValueError, match="generates its layer energies itself"):
        gen.run(E, layers=torch.zeros((B, 6), device="cuda"), workspace=ws)
    with pytest.raises(ValueError, match="global_batch"):
        gen.run(E, shard=(2, 4), workspace=ws)
    showers = torch.zeros((B, K1.V), device="cuda")
    for energy, out, work in ((None, showers.data_ptr(), ws.data_ptr()), (E.data_ptr(), None, ws.data_ptr()), (E.data_ptr(), showers.data_ptr(), None)):
        code = gen.lib.cd_generator_run(gen.handle, B, energy, 1, None, 1234, 0, 0, B, out, None, None, work, ws.numel(), engine._stream())
        assert code == -1  # CD_EINVAL
    torch.cuda.synchronize()
    assert not ws.any() and not showers.any()  # nothing was launched: the first launch of a run writes the start tensor there
    # a corrupted layout is refused on the host, and nothing is uploaded for it
    from calodiffusion_amd.generator import export_generator
    words = {"alpha outside {1, A}": "1 or alpha_out", "span mismatch: rin one more": "alpha \\* rin", "matrix entry NaN": "not finite",
             "wtotal 8193": "8192"}
    bad = {label: blob for label, blob in H.corruptions(export_generator(m, STEPS)) if label in words}
    assert len(bad) == len(words)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for label, word in words.items():
        with pytest.raises(ValueError, match=word):
            Generator(bad[label])
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0


# ---------------------------------------------------------------------- from C
def write_python_reference(out_dir):
    """the two-stage photon model's generator file, a file of 3 + 2 energies and the showers model.generate gives for them"""
    from calodiffusion_amd.generator import export_generator
    m = H.two_stage("ph")
    loader = loader_of(m, (3, 2), 11)
    export_generator(m, STEPS, path=os.path.join(out_dir, "photon.cdgen"))
    torch.cat([E for E, _, _ in loader]).numpy().astype("<f4").tofile(os.path.join(out_dir, "e.f32"))
    showers, _, offset = python_path(m, loader, STEPS, m.NN_embed)
    showers.astype("<f4").tofile(os.path.join(out_dir, "want.f32"))
    print(f"next offset {offset}")


def test_c_example_writes_the_python_showers(tmp_path):
    """tools/cd_generate_example.c as a fresh process on a photon file: raw fp32 showers out, bytewise the Python path's.  Both
    processes run with the tiling timer off (CD_NO_AUTOTUNE), as tests/test_gpu_generator.py explains; the Python path is this
    module as a script."""
    import sys
    from calodiffusion_amd import build as b
    assert os.path.exists(b.EXAMPLE), f"{b.EXAMPLE} was not built (calodiffusion_amd.build compiles tools/cd_generate_example.c)"
    env = dict(os.environ, CD_NO_AUTOTUNE="1")
    ref = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), str(tmp_path)], env=env,
                         capture_output=True, text=True)
    assert ref.returncode == 0, (ref.returncode, ref.stdout[-2000:], ref.stderr[-2000:])
    r = subprocess.run(["timeout", "-k", "10", "120", b.EXAMPLE, str(tmp_path / "photon.cdgen"), str(tmp_path / "e.f32"),
                        str(tmp_path / "out.f32"), "3", "1234", "0"], env=env, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    want = (tmp_path / "want.f32").read_bytes()
    assert len(want) == 5 * K1.V * 4 and (tmp_path / "out.f32").read_bytes() == want
    assert "format version 3: Dataset-0/1 radial maps, form 1 (the converter inside the model), state (368)" in r.stdout
    assert r.stdout.split("next offset")[1].strip() == ref.stdout.split("next offset")[1].strip()


if __name__ == "__main__":
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    write_python_reference(sys.argv[1])
