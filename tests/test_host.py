"""CPU: host logic, the C-ABI library's export table, and the loud failure without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, gold, rel_l2
from helpers import seeded_unet, t, verify_checksums
from sampler_oracles import (SDE_CASES, OracleBackedModel, check_sampler_case, dpm_adaptive_on_oracle, interpret_program,
                             sde_oracle_run)
from oracle import torch_oracle as O
from calodiffusion_amd import engine, schedule, utils
from calodiffusion_amd.calodiffusion import CaloDiffusion
from calodiffusion_amd.configs import load_config


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "calodiff.h")).read()
    declared = set(re.findall(r"\b(cd_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    lib = ctypes.CDLL(engine.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/calodiff.h but not exported"
    assert declared == set(engine.EXPORTED_SYMBOLS)
    engine.load_library()  # binds argtypes for all of them


def test_step_table_matches_reference_loop_scalars():
    """ddim_step_table == the scalars DDim.__call__ gathers per iteration (pinned through the oracle's tables,
    themselves bit-identical to the reference's: test_oracle_golden.test_schedules_bitwise)."""
    for n, eta, off in ((400, 0.0, 0), (50, 1.0, 0), (10, 0.0, 3), (2, 1.0, 0)):
        tab = schedule.ddim_step_table(n, eta, off)
        tb = O.ddim_tables(n)
        ts = list(range(n - 1, -1, -1))[off:]
        assert tab.shape == (len(ts), 4)
        for i, tt in enumerate(ts):
            a, ap = tb.alphas_cumprod[tt], tb.alphas_cumprod_prev[tt]
            denom = tb.sqrt_alphas_cumprod[max(tt - 1, 0)]
            sigma = tb.sqrt_one_minus_alphas_cumprod[tt] / tb.sqrt_alphas_cumprod[tt]
            ds = eta * (((1 - ap) / (1 - a)) * (1 - a / ap)) ** 0.5
            sp = (1.0 - ap - ds ** 2).sqrt() / denom * (1.0 if tt > 0 else 0.0)
            want = np.array([float(sigma), float(sp), float(ds), float(denom)], dtype=np.float32)
            assert np.array_equal(tab[i], want), (n, eta, tt)
    # N = 400: sigma spans 2.57e4 .. 1.06e-2
    tab = schedule.ddim_step_table(400, 0.0)
    assert abs(tab[0, 0] / 2.57e4 - 1) < 0.01 and abs(tab[-1, 0] / 1.06e-2 - 1) < 0.01 and tab[-1, 1] == 0.0


def test_coordinate_profiles_match_reference_images():
    r, z, phi = utils.coordinate_profiles(2, (45, 16, 9))
    ro, zo, po = O.rz_phi_profiles(2, (45, 16, 9))
    assert np.array_equal(r, ro.numpy()) and np.array_equal(z, zo.numpy()) and np.array_equal(phi, po.numpy())
    assert r[-1] == 1.0 and z[0] == 0.0 and abs(z[-1] - 44 / 45) < 1e-7 and phi[0] == 0.0 and phi[-1] == 1.0
    with pytest.raises(ValueError):
        utils.coordinate_profiles(2, (45, 16, 10))


@pytest.mark.parametrize("name", ["dataset2", "dataset3", "hgcal", "tiny"])
def test_parameter_container_reproduces_reference_init(name):
    g = gold(f"model_{name}")
    verify_checksums(seeded_unet(name, int(g["seed"])).state_dict(), g)


def test_calodiffusion_surface_and_state_dict_roundtrip(tmp_path):
    m = CaloDiffusion("dataset2", n_steps=400, loss_type="l2")
    assert type(m.sampler_algorithm).__name__ == "DDim" and type(m.loss_function).__name__ == "hybrid_weight"
    assert m.loss_function.sigma_data == 1.0 and m._data_shape == [1, 45, 16, 9] and m.nsteps == 400
    sd = m.state_dict()
    assert all(k.startswith("model.") for k in sd) and sum(v.numel() for v in sd.values()) == 2212785
    # checkpoints written with a wrapper prefix load, as in the reference (calodiffusion.py:31-37)
    wrapped = {"module." + k: v.clone() for k, v in sd.items()}
    path = tmp_path / "ckpt.pth"
    torch.save({"model_state_dict": wrapped}, path)
    m2 = CaloDiffusion("dataset2", n_steps=400, loss_type="l2")
    m2.load_state_dict(torch.load(path)["model_state_dict"])
    for k in sd:
        assert torch.equal(sd[k], m2.state_dict()[k])
    with pytest.raises(ValueError):
        cfg = dict(load_config("dataset2"))
        cfg["SAMPLER"] = "NoSuchSampler"
        CaloDiffusion(cfg)


def test_unsupported_configurations_fail_at_construction():
    cfg = dict(load_config("dataset2"))
    cfg["TIME_EMBED"] = "sin"
    with pytest.raises((KeyError, NotImplementedError)):
        CaloDiffusion(cfg)
    cfg = dict(load_config("dataset2"))
    cfg["CYLINDRICAL"] = False
    with pytest.raises(NotImplementedError):
        CaloDiffusion(cfg)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_compute_fails_loudly_without_gpu():
    m = CaloDiffusion("tiny", 50, "l2")
    with pytest.raises(RuntimeError, match="no CPU fallback|GPU"):
        m.denoise(torch.zeros(1, 1, 8, 8, 8), E=torch.zeros(1, 3), sigma=torch.ones(1), layers=torch.zeros(1, 9))
    with pytest.raises(RuntimeError):
        m.sample(torch.zeros(1, 3), torch.zeros(1, 9), num_steps=2)


def test_shard_batch_partitions():
    for n, w in ((64, 8), (10, 4), (3, 8), (128, 2)):
        seen = []
        for r in range(w):
            s = utils.shard_batch(n, w, r)
            seen += list(range(n))[s]
        assert seen == list(range(n))


def test_loss_sigma_draw_matches_oracle_formula():
    m = CaloDiffusion("dataset2", 400, "l2")
    rnd = torch.tensor([0.3, -1.1, 2.0])
    s = m.loss_function.draw_sigma(torch.zeros(3, 1, 2, 2, 2), rnd_normal=rnd)
    assert torch.equal(s, (rnd * 1.2 + (-1.2)).exp())
    m3 = CaloDiffusion("dataset3", 400, "l2")
    tt = torch.tensor([0, 137, 399])
    s3 = m3.loss_function.draw_sigma(torch.zeros(3, 1, 2, 2, 2), time=tt)
    tb = O.ddim_tables(400)
    assert torch.equal(s3, tb.sqrt_one_minus_alphas_cumprod[tt] / tb.sqrt_alphas_cumprod[tt])


def test_layerdiffusion_surface_and_checkpoints(tmp_path):
    """LayerDiffusion mirrors reference models/layerdiffusion.py: layer model + base U-Net, state switching, the nested
    'layer_model' state_dict entry, loading the layer model from config['layer_model'] and the base model from a
    'base_model.' / 'model.' prefixed checkpoint; and no CPU fallback."""
    from calodiffusion_amd.layerdiffusion import LayerDiffusion
    cfg = dict(load_config("dataset2"))
    m = LayerDiffusion(dict(cfg), n_steps=400, loss_type="l2")
    assert m.layer_steps == 400 and type(m.layer_sampler).__name__ == "DDim" and m.model is m.base_model
    lsd = m.layer_model.state_dict()
    assert list(lsd)[:2] == ["time_mlp.1.weight", "time_mlp.1.bias"] and "hidden_layers.3.dense2.0.bias" in lsd
    assert lsd["in_lay.weight"].shape == (256, 46) and sum(v.numel() for v in lsd.values()) == 694958
    m.set_layer_state(True)
    assert m.model is m.layer_model and m.layer_loss
    m.set_layer_state(False)
    sd = m.state_dict()
    assert set(sd["layer_model"]) == set(lsd) and any(k.startswith("base_model.") for k in sd)
    torch.save({"model_state_dict": {"layer_model." + k: v + 1 for k, v in lsd.items()}}, tmp_path / "layer.pth")
    cfg["layer_model"] = str(tmp_path / "layer.pth")
    m2 = LayerDiffusion(dict(cfg), n_steps=400, loss_type="l2")
    base = {k: v.clone() for k, v in sd.items() if k.startswith("base_model.")}
    m2.load_state_dict(base)
    assert torch.equal(m2.layer_model.state_dict()["out_lay.bias"], lsd["out_lay.bias"] + 1)
    for k, v in m.base_model.state_dict().items():
        assert torch.equal(m2.base_model.state_dict()[k], v)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback|GPU"):
            m.sample_layers(torch.zeros(2, 1), start=torch.zeros(2, 46))
        assert not m.layer_loss  # the state is restored on failure


def test_sampler_programs_reproduce_the_reference_trajectories():
    """Every step program of calodiffusion_amd.sample (EDM Euler+churn / Heun / DPM2 / LMS / Restart, DPM / DPM++2S / DPM++2M,
    Consistency), interpreted on the CPU with the oracle as denoiser, against trajectories of the reference's own sampler
    classes (tests/golden/samplers_tiny.npz)."""
    import copy
    from sampler_cases import CASES, options, replay_noise
    g = gold("samplers_tiny")
    base = load_config("tiny")
    om = O.OracleModel(base, seeded_unet("tiny").state_dict())
    for tag, (name, over, _, off, rows) in CASES.items():
        cfg = copy.deepcopy(base)
        cfg.update(over)
        cfg["SAMPLER"] = name
        if options(g, tag):
            cfg["SAMPLER_OPTIONS"] = options(g, tag)
        m = CaloDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"])
        smp = m.sampler_algorithm
        assert type(smp).__name__ == name
        n = int(g[f"{tag}.n"])
        prog = smp.build(m, n, off).finalize()
        if name == "DPM":
            # the step table as the host that made the goldens computes it (torch's vectorised cos / exp / log / expm1 differ in the
            # last bit between CPUs, and dpm_2 amplifies a 4e-7 change of a coefficient to 1.5e-4): this host's must agree to
            # rounding; the run below uses the recorded one (tests/golden/dpm_tables.npz)
            gt = gold("dpm_tables")
            assert np.allclose(prog.coefs, gt[f"{tag}.coefs"], rtol=2e-5, atol=0), tag
            prog.coefs, prog.start_scale = gt[f"{tag}.coefs"].copy(), float(gt[f"{tag}.start_scale"])
        start, E, layers = t(g["start"])[:rows], t(g["E"])[:rows], t(g["layers"])[:rows]
        noise = replay_noise(g, tag, start.shape)
        if prog.n_randn:
            assert prog.n_randn == len(noise), (tag, prog.n_randn, len(noise))
        den = lambda x, s: om.denoise(x, E, s.float().expand(rows), layers)  # noqa: E731
        with torch.no_grad():
            x, xs, x0s = interpret_program(prog, den, start, noise if prog.n_randn else [])
        if name == "Restart":
            xs, x0s = None, [x0s[i] for i in smp._main_steps]
        if name in ("LMS", "DPM", "DPMPP2S", "DPMPP2M"):
            xs = x0s = None
        if name == "Consistency":
            x0s = None
        check_sampler_case(tag, g, x, xs, x0s, 2e-5)
        if name == "DPM":
            # DPM-Solver-fast cancels terms of order sigma_max against each other (dpm_2: ONE second-order step from sigma = 142
            # to 1 amplifies the rounding of its intermediate state 12x), so its program is emitted in the reference's own
            # operation order (LINDIV ops): on the recorded step table the interpreted program reproduces the reference's fp32
            # result (bit for bit on the host that made the goldens; elsewhere the oracle's convolutions differ by ~5e-7 per call)
            assert rel_l2(np.asarray(x), g[f"{tag}.x"]) <= 2e-5, tag
        # uniform programs replay one captured step graph; nested / order-changing ones run their steps eagerly
        if tag in ("euler_noisy", "heun", "heun_noisy", "dpm2", "lms", "dpmpp2m", "dpmpp2s", "restart_default"):
            assert prog.op_begin is None, tag
        if tag in ("restart_int", "restart_noisy", "dpm_7", "dpm_6", "consistency", "dpmpp2s_eta"):
            assert prog.op_begin is not None, tag


def test_generate_never_returns_normalised_showers_silently():
    m = CaloDiffusion("tiny", 50, "l2")
    gen_, en = np.zeros((2, 1, 8, 8, 8), np.float32), np.zeros((2, 3), np.float32)
    with pytest.raises(ValueError, match="inverse pre-processing"):
        m._to_physical(gen_, en, None, None)
    out, e = m._to_physical(gen_, en, None, False)
    assert out is gen_ and e.shape == (2, 3)
    out, _ = m._to_physical(gen_, en, None, lambda a, b, c, d: (a + 1, b))
    assert float(out.mean()) == 1.0


def test_noise_shard_bookkeeping():
    """set_noise_shard: offsets / strides of a rank's rows of the global Philox tensors (no GPU needed for the arithmetic)."""
    m = CaloDiffusion("tiny", 50, "l2")
    start = torch.zeros(2, 1, 8, 8, 8)
    assert m.step_noise_stream(start) == (0, 1024)
    m.set_noise_shard(4, 6)
    m.noise_offset = 100
    assert m._shard_geometry(start.shape) == (512, 2048, 3072)
    assert m.step_noise_stream(start) == (100 + 2048, 3072)
    with pytest.raises(ValueError):
        m._shard_geometry((3, 1, 8, 8, 8))


def test_reference_module_paths_resolve_to_this_package():
    """`calodiffusion.models.*` / `calodiffusion.utils.utils` (the reference's import paths) are aliases of calodiffusion_amd."""
    import calodiffusion.models.calodiffusion as m_cd
    import calodiffusion.models.diffusion as m_d
    import calodiffusion.models.layerdiffusion as m_ld
    import calodiffusion.models.loss as m_l
    import calodiffusion.models.models as m_m
    import calodiffusion.models.sample as m_s
    import calodiffusion.utils.utils as m_u
    import calodiffusion_amd as A
    from calodiffusion_amd import calodiffusion as a_cd, diffusion as a_d, layerdiffusion as a_ld, loss as a_l, sample as a_s, unet as a_u

    assert m_d.Diffusion is a_d.Diffusion and m_cd.CaloDiffusion is a_cd.CaloDiffusion and m_ld.LayerDiffusion is a_ld.LayerDiffusion
    assert m_s.DDim is a_s.DDim and m_s.DPMPP2M is a_s.DPMPP2M and m_l.hybrid_weight is a_l.hybrid_weight
    assert m_m.CondUnet is a_u.CondUnet
    assert m_u.load_attr("sampler", "Heun") is a_s.Heun and callable(m_u.ReverseNorm)
    assert A is not None


def test_dpm_adaptive_host_loop():
    """The host-decision sampler on the oracle: step count = the t-range over H_INIT (the reference's controller never changes
    the step), 3 / 2 model evaluations per step at order 3 / 2, a halved step lands within the error estimate's scale of the
    full one, and a rejected step raises instead of looping forever."""
    import math
    _, x3, calls3, steps3 = dpm_adaptive_on_oracle({"ORDER": 3}, 8)
    m = OracleBackedModel(load_config("tiny"))
    from calodiffusion_amd import sample
    sig = sample.DPMAdaptive(load_config("tiny")).setup_sigmas(m, 8)
    span = float(torch.log(sig[0] / sig[-1]))
    assert steps3 == math.ceil((span - 1e-5) / 0.05) and calls3 == 3 * steps3 and torch.isfinite(x3).all()
    _, x3h, _, steps3h = dpm_adaptive_on_oracle({"ORDER": 3, "H_INIT": 0.1}, 8)
    assert steps3h == math.ceil((span - 1e-5) / 0.1) and rel_l2(x3h.numpy(), x3.numpy()) < 5e-3
    _, x2, calls2, steps2 = dpm_adaptive_on_oracle({"ORDER": 2}, 8)
    assert calls2 == 2 * steps2 and rel_l2(x2.numpy(), x3.numpy()) < 2e-2
    with pytest.raises(RuntimeError, match="rejected"):
        dpm_adaptive_on_oracle({"ORDER": 2, "H_INIT": 3.0, "R_TOL": 1e-6, "A_TOL": 1e-8}, 8)
    with pytest.raises(ValueError):
        dpm_adaptive_on_oracle({"ORDER": 4}, 8)


@pytest.mark.parametrize("name,opts", SDE_CASES)
def test_sde_sampler_programs_equal_the_restated_loops(name, opts):
    """DPMPPSDE / DPMPP2MSDE / DPMPP3MSDE (models/sample.py:347-574) as step programs, interpreted on the CPU with the oracle as
    denoiser, against the reference's loops restated on the oracle with the SAME unit normals (the reference's torchsde Brownian
    tree is not installed: there is no reference trajectory; parity unpinned, see sample._BrownianSDE).  ETA = 0 draws nothing
    and is a uniform program; DPMPPSDE draws two normals per step and mixes them as the Brownian path implies."""
    import copy
    from oracle import samplers_oracle as SO
    base = load_config("tiny")
    om = O.OracleModel(base, seeded_unet("tiny").state_dict())
    cfg = copy.deepcopy(base)
    cfg["SAMPLER"] = name
    cfg["SAMPLER_OPTIONS"] = dict(opts)
    m = CaloDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"])
    smp = m.sampler_algorithm
    assert type(smp).__name__ == name
    n, rows = 7, 2
    prog = smp.build(m, n, 0).finalize()
    sig = SO.model_sigmas(m.loss_function, n)
    m.loss_function.update_step(m.nsteps)
    gen = torch.Generator().manual_seed(41)
    start = torch.randn((rows, 1, 8, 8, 8), generator=gen)
    E, layers = torch.rand((rows, 3), generator=gen), torch.randn((rows, 9), generator=gen)
    per_step = {"DPMPPSDE": 2, "DPMPP2MSDE": 1, "DPMPP3MSDE": 1}[name] if opts.get("ETA") else 0
    assert prog.n_randn == per_step * (n - 1)
    if not opts.get("ETA") and name == "DPMPPSDE":
        assert prog.op_begin is None  # nothing drawn, same ops every step: one captured step graph
    noise = [torch.randn(start.shape, generator=gen) for _ in range(prog.n_randn)]
    den = lambda x, s: om.denoise(x, E, torch.as_tensor(s).float().expand(rows), layers)  # noqa: E731
    with torch.no_grad():
        got, _, _ = interpret_program(prog, den, start, noise)
        want = sde_oracle_run(name, opts, den, start, sig, noise)
    err = rel_l2(got.numpy(), want.numpy())
    assert err < 2e-5, (name, opts, err)
    if opts.get("ETA"):
        # the noise matters: another set of normals moves the end point by far more than the bound above
        with torch.no_grad():
            other, _, _ = interpret_program(prog, den, start, [torch.randn(start.shape, generator=gen) for _ in range(prog.n_randn)])
        assert rel_l2(other.numpy(), want.numpy()) > 1e-2
