"""GPU (MI355X): cd_generator_run against the Python path it restates.  The oracle is ``model.generate(loader, steps)`` from
``model.noise_offset = 0`` with the device reverse norm -- the existing, reference-pinned path -- and the comparison is bitwise, on
showers, on the layer energies and on the Philox offset the model is left at.

One thing of the oracle is not the library's: ``ReverseNormCaloChall`` forms the incident energies ``emin * (emax / emin) ** e`` with
numpy's float32 power on the host, whose last bit depends on the host's vector math library (on an AVX-512 host about a fifth of
all e differ from the correctly rounded value); cd_generator_run forms the correctly rounded power on the device.  The tests draw
their e among the values on which this host's numpy returns the correctly rounded power, so that what is compared is the
generator and not the host's libm."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NARROW = dict(LAYER_SIZE_UNET=[16, 16, 16, 16])


def bits_equal(a, b):
    """the same float32 bits everywhere (stricter than np.array_equal: NaN payloads and the sign of zero count)"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def energies(n, seed, emax=1000.0, emin=1.0):
    """n conditioning values e in [0, 1) on which numpy's float32 power is the correctly rounded one (see the module docstring)"""
    rng = np.random.default_rng(seed)
    keep = []
    while len(keep) < n:
        e = rng.random(4 * n, dtype=np.float32)
        host = (emax / emin) ** e
        exact = np.array([math.pow(float(np.float32(emax / emin)), float(v)) for v in e]).astype(np.float32)
        keep += [v for v, ok in zip(e, host == exact) if ok]
    return torch.tensor(np.array(keep[:n], dtype=np.float32)).reshape(n, 1)


def build(two_stage, name, **over):
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    from calodiffusion_amd.configs import load_config
    from calodiffusion_amd.layerdiffusion import LayerDiffusion
    cfg = dict(load_config(name))
    cfg.update(over)
    torch.manual_seed(1234)
    return (LayerDiffusion if two_stage else CaloDiffusion)(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"])


def loader_of(m, sizes, seed):
    """(E, layers, None) batches: layers only where the model takes them from its caller"""
    from calodiffusion_amd.layerdiffusion import LayerDiffusion
    E = energies(sum(sizes), seed)
    want_layers = m.layer_cond and not isinstance(m, LayerDiffusion)
    g = torch.Generator().manual_seed(seed)
    out, lo = [], 0
    for b in sizes:
        layers = torch.randn((b, m.config["SHAPE_FINAL"][2] + 1), generator=g) if want_layers else torch.zeros((b, 0))
        out.append((E[lo:lo + b], layers, None))
        lo += b
    return out


def python_path(m, loader, steps, sample_offset=0):
    """(showers, layer energies per batch or None, final offset) of model.generate from offset 0"""
    from calodiffusion_amd.layerdiffusion import LayerDiffusion
    layers = []
    if isinstance(m, LayerDiffusion):
        inner = m.sample_layers
        m.sample_layers = lambda *a, **k: (layers.append(inner(*a, **k)), layers[-1])[1]  # what generate() conditions on
    m.noise_offset = 0
    try:
        showers, _ = m.generate(loader, steps, sample_offset=sample_offset)
    finally:
        m.__dict__.pop("sample_layers", None)
    if not layers and m.layer_cond:
        layers = [lay for _, lay, _ in loader]
    return showers, [lay.cpu().numpy() for lay in layers] or None, m.noise_offset


def c_path(gen, m, loader):
    """the same loader through cd_generator_run, chaining next_offset"""
    from calodiffusion_amd.layerdiffusion import LayerDiffusion
    showers, layers, off = [], [], 0
    for E, lay, _ in loader:
        given = lay.cuda() if m.layer_cond and not isinstance(m, LayerDiffusion) else None
        s, lout, off = gen.run(E.cuda(), layers=given, seed=m.noise_seed, offset=off)
        showers.append(s.cpu().numpy())
        if lout is not None:
            layers.append(lout.cpu().numpy())
    return np.concatenate(showers), layers or None, off


def compare(m, sizes, steps, sample_offset=0, seed=11):
    from calodiffusion_amd.generator import Generator, export_generator
    loader = loader_of(m, sizes, seed)
    gen = Generator(export_generator(m, steps, sample_offset=sample_offset))
    want, want_layers, want_off = python_path(m, loader, steps, sample_offset)
    got, got_layers, got_off = c_path(gen, m, loader)
    assert want.shape == (sum(sizes), gen.info["voxels"])
    assert bits_equal(got, want)
    assert (got_layers is None) == (want_layers is None)
    for a, b in zip(got_layers or [], want_layers or []):
        assert bits_equal(a, b)
    assert got_off == want_off
    return gen, loader, want


# ---------------------------------------------------------------------- the shipped two-stage model, and what hangs off it
@pytest.fixture(scope="module")
def ds2_two_stage():
    """dataset2 LayerDiffusion, DDim on both stages, 3 steps, LAYER_STEPS 12; a loader of 3 + 2 showers"""
    m = build(True, "dataset2", LAYER_STEPS=12)
    gen, loader, want = compare(m, (3, 2), 3)
    return m, gen, loader, want


def test_dataset2_layerdiffusion_two_batches(ds2_two_stage):
    m, gen, loader, want = ds2_two_stage
    assert gen.info == dict(voxels=6480, layers=45, energy_columns=1, has_layer_stage=1, takes_layers=1, sample_steps=3, layer_steps=12,
                            format_version=1)
    assert np.isfinite(want).all() and (want >= 0).all() and want.max() > 0


def test_dataset2_calodiffusion_given_layers():
    compare(build(False, "dataset2"), (2,), 3)


def test_dataset3_calodiffusion_batch_1_no_layers():
    gen, _, _ = compare(build(False, "dataset3"), (1,), 2)
    assert gen.info["takes_layers"] == 0 and gen.info["layers"] == 45 and gen.info["voxels"] == 40500


def test_ddpm_on_both_stages():
    """per-step device noise: the U-Net's from the stream position and stride, the layer stage's as one block"""
    compare(build(True, "dataset2", LAYER_STEPS=12, SAMPLER="DDPM", LAYER_SAMPLER="DDPM", **NARROW), (2, 2), 4)


@pytest.mark.parametrize("name,opts,steps", [("Heun", {}, 4), ("DPMPP2M", {}, 5), ("DPMPPSDE", {"ETA": 1.0}, 3)])
def test_program_samplers(name, opts, steps):
    """one step program per family (cd_sampler_run): EDM, DPM-Solver++ multistep, the stochastic DPM-Solver++ with its RANDN ops"""
    compare(build(False, "dataset3", SAMPLER=name, SAMPLER_OPTIONS=opts, **NARROW), (2, 1), steps)


def test_layer_sampler_program():
    """a LAYER_SAMPLER that runs on cd_layer_sampler_run, with noise draws of its own"""
    compare(build(True, "dataset2", LAYER_STEPS=12, LAYER_SAMPLER="DPMPPSDE", SAMPLER_OPTIONS={"ETA": 1.0}, **NARROW), (2, 2), 3)


def test_sample_offset_2():
    compare(build(True, "dataset2", LAYER_STEPS=12, **NARROW), (2,), 5, sample_offset=2)


# ---------------------------------------------------------------------- sharding, the energy map, memory, refusals
# What set_noise_shard promises, and to what: every shard draws its rows of the SAME global noise tensors -- exactly -- while the
# U-Net's kernels tile a batch of 2 and a batch of 4 differently, so the fp32 summation order of their statistics differs
# (tests/test_gpu_distributed.py holds the Python path's shards to 2e-6 relative L2 of the single-process result in normalised
# space for that reason).  Hence: each shard is BITWISE the Python path's under the same set_noise_shard at the same batch; the
# layer energies (one workgroup per sample, nothing depends on the batch) are bitwise rows of the whole batch's; and the
# physical showers of the shards agree with the whole batch to SHARD_TOL relative L2.  The inverse map is
# s = E maxdep fac sigmoid(std v + mean): |d ln s / dv| <= std for the voxel and as much again through its layer's factor,
# so 2e-6 in v, concentrated up to ten-fold on the bright voxels that carry the L2 norm, is at most 2 * 1.9123 * 10 * 2e-6 = 8e-5.
# Rows drawn at a wrong stream position are independent showers: a relative L2 distance of order 1.
SHARD_TOL = 1e-4


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def shards_against_whole(m, gen, steps, offset, seed):
    E = energies(4, seed)
    whole, lay, off = gen.run(E.cuda(), seed=m.noise_seed, offset=offset)
    parts, lays = [], []
    for first in (0, 2):
        s, lay_s, _ = gen.run(E[first:first + 2].cuda(), seed=m.noise_seed, offset=offset, shard=(first, 4))
        m.set_noise_shard(first, 4)
        try:
            m.noise_offset = offset
            want, _ = m.generate([(E[first:first + 2], torch.zeros((2, 0)), None)], steps)
        finally:
            m.set_noise_shard(0, 0)
        assert bits_equal(s.cpu().numpy(), want), first
        parts.append(s)
        lays.append(lay_s)
    err = rel_l2(torch.cat(parts).cpu().numpy(), whole.cpu().numpy())
    print(f"shards against the whole batch: relative L2 {err:.3e} (bound {SHARD_TOL:g})")
    assert err < SHARD_TOL
    if lay is not None:
        assert bits_equal(torch.cat(lays).cpu().numpy(), lay.cpu().numpy())
    return off


def test_shards_are_slices_of_one_global_batch(ds2_two_stage):
    m, gen, _, _ = ds2_two_stage
    shards_against_whole(m, gen, 3, 7, 5)


def test_shards_with_step_noise():
    """a stochastic sampler: the shards draw their rows of every global noise tensor"""
    from calodiffusion_amd.generator import Generator, export_generator
    m = build(False, "dataset3", SAMPLER="DDPM", **NARROW)
    off = shards_against_whole(m, Generator(export_generator(m, 3)), 3, 0, 6)
    assert off == 4 * 40500 * (1 + 3)


def test_physical_energies_map_as_preprocess_maps_them(ds2_two_stage):
    """energy_is_normalised = 0: the conditioning is Preprocess's E of the same energies, bit for bit -- fed back as normalised
    input it gives the same showers and layer energies, which any other bit of e would change -- and a second physical call too."""
    from calodiffusion_amd.preprocess import Preprocess
    m, gen, _, _ = ds2_two_stage
    g = torch.Generator().manual_seed(8)
    phys = (1.0 + 990.0 * torch.rand((3,), generator=g)).cuda()
    showers = torch.rand((3, 6480), generator=g).cuda()
    E, _, _ = Preprocess(m.config, shower_scale=1.0)(showers, phys)
    a, lay_a, off_a = gen.run(phys, seed=m.noise_seed, offset=0, normalised=False)
    b, lay_b, off_b = gen.run(E, seed=m.noise_seed, offset=0, normalised=True)
    assert bits_equal(a.cpu().numpy(), b.cpu().numpy()) and bits_equal(lay_a.cpu().numpy(), lay_b.cpu().numpy()) and off_a == off_b
    assert not bits_equal(lay_a.cpu().numpy(), gen.run(torch.nextafter(E, E + 1), seed=m.noise_seed, offset=0)[1].cpu().numpy())


def test_run_allocates_nothing(ds2_two_stage):
    m, gen, loader, _ = ds2_two_stage
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


def test_run_refusals_launch_nothing(ds2_two_stage):
    from calodiffusion_amd.generator import Generator, export_generator
    m, gen, loader, _ = ds2_two_stage
    E = loader[0][0].cuda()
    B = E.shape[0]
    ws = torch.zeros(gen.workspace_bytes(B), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="workspace too small"):
        gen.run(E, workspace=ws[:-1])
    with pytest.raises(ValueError, match="generates its layer energies itself"):
        gen.run(E, layers=torch.zeros((B, 46), device="cuda"), workspace=ws)
    with pytest.raises(ValueError, match="global_batch"):
        gen.run(E, shard=(2, 4), workspace=ws)
    torch.cuda.synchronize()
    assert not ws.any()  # nothing was launched: the first launch of a run writes the start tensor there
    given = Generator(export_generator(build(False, "dataset2", **NARROW), 2))
    with pytest.raises(ValueError, match="`layers` .* is required"):
        given.run(E)
    none = Generator(export_generator(build(False, "dataset3", **NARROW), 2))
    with pytest.raises(ValueError, match="takes no layer energies"):
        none.run(E, layers=torch.zeros((B, 46), device="cuda"))
    with pytest.raises(ValueError, match="wrong magic"):
        Generator(b"x" * 4096)


# ---------------------------------------------------------------------- from C
def write_python_reference(out_dir):
    """the dataset2 two-stage model's generator file, a file of 3 + 2 energies and the showers model.generate gives for them"""
    from calodiffusion_amd.generator import export_generator
    m = build(True, "dataset2", LAYER_STEPS=12)
    loader = loader_of(m, (3, 2), 11)
    export_generator(m, 3, path=os.path.join(out_dir, "ds2.cdgen"))
    torch.cat([E for E, _, _ in loader]).numpy().astype("<f4").tofile(os.path.join(out_dir, "e.f32"))
    showers, _, offset = python_path(m, loader, 3)
    showers.astype("<f4").tofile(os.path.join(out_dir, "want.f32"))
    print(f"next offset {offset}")


def test_c_example_writes_the_python_showers(tmp_path):
    """tools/cd_generate_example.c as a fresh process: a generator file and a file of energies in, raw fp32 showers out, bytewise
    the Python path's.  The convolutions' tilings are picked by a timer once per process and geometry, and two tilings differ in
    the last bits (the summation order of the channel statistics), so showers are reproducible to the bit across PROCESSES only
    with the timer off (CD_NO_AUTOTUNE: the top-ranked tiling): the Python path runs as a fresh process of its own under the
    same setting, this module as a script."""
    import sys
    from calodiffusion_amd import build as b
    if not os.path.exists(b.EXAMPLE):
        pytest.skip(f"{b.EXAMPLE} was not built (calodiffusion_amd.build compiles tools/cd_generate_example.c with gcc)")
    env = dict(os.environ, CD_NO_AUTOTUNE="1")
    ref = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), str(tmp_path)], env=env,
                         capture_output=True, text=True)
    assert ref.returncode == 0, (ref.returncode, ref.stdout[-2000:], ref.stderr[-2000:])
    r = subprocess.run(["timeout", "-k", "10", "120", b.EXAMPLE, str(tmp_path / "ds2.cdgen"), str(tmp_path / "e.f32"),
                        str(tmp_path / "out.f32"), "3", "1234", "0"], env=env, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    want = (tmp_path / "want.f32").read_bytes()
    assert len(want) == 5 * 6480 * 4 and (tmp_path / "out.f32").read_bytes() == want
    assert r.stdout.split("next offset")[1].strip() == ref.stdout.split("next offset")[1].strip()


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    write_python_reference(sys.argv[1])
