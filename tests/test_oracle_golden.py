"""CPU: the oracle (oracle/torch_oracle.py) against the golden vectors generated from the reference itself."""
import numpy as np
import pytest
import torch

from conftest import gold, rel_l2
from helpers import d1grid_kwargs, per_layer_worst, seeded_unet, t, verify_checksums
from sampler_oracles import check_sampler_case
from oracle import torch_oracle as O
from calodiffusion_amd.configs import load_config

TOL = 2e-6  # fp32 reorder noise floor of one denoise call is 5.5e-7


def test_cyl_conv_known_answer():
    """The reference's only known-answer fixture for this path: calodiffusion/tests/test_cyl_conv.py."""
    g = gold("cyl_known_answer")
    x = t(g["x"])
    w = torch.ones(1, 1, 1, 3, 3)
    y = O.cyl_conv3d(x, w, None, padding=(0, 1, 1))
    assert np.array_equal(y.numpy(), g["cyl"])
    # hand-computed: every phi row sees three identical rows [1,2,3] -> 3*(l+c+r) with zero padding in r
    assert np.array_equal(g["cyl"][0, 0, 0], np.array([[9.0, 18.0, 15.0]] * 4, dtype=np.float32))
    # plain zero padding differs on the two phi edge rows
    assert np.array_equal(g["plain"][0, 0, 0, 0], np.array([6.0, 12.0, 10.0], dtype=np.float32))


def test_schedules_bitwise():
    g = gold("schedules")
    for n in (2, 10, 50, 200, 400):
        assert np.array_equal(O.cosine_beta_schedule(n).numpy(), g[f"betas_{n}"])
        assert np.array_equal(O.ddim_tables(n).alphas_cumprod.numpy(), g[f"alphas_cumprod_{n}"])


def test_conv_primitives():
    g = gold("primitives_conv")
    tags = sorted({k.split(".")[0] for k in g.files})
    for tag in tags:
        x, w = t(g[f"{tag}.x"]), t(g[f"{tag}.w"])
        b = t(g[f"{tag}.b"]) if f"{tag}.b" in g.files else None
        if tag.startswith("c3"):
            y = O.cyl_conv3d(x, w, b, padding=(1, 1, 1))
        elif tag.startswith("c1"):
            y = O.cyl_conv3d(x, w, b)
        elif tag.startswith("down"):
            zs = 2 if int(g[f"{tag}.cz"]) else 1
            y = O.cyl_conv3d(x, w, b, stride=(zs, 2, 2), padding=(1, 1, 1))
        else:
            zs = 2 if int(g[f"{tag}.cz"]) else 1
            e = g[f"{tag}.extra"]
            y = O.cyl_conv_transpose3d(x, w, b, (zs, 2, 2), (0, int(e[1]), int(e[2])))
        assert y.shape == g[f"{tag}.y"].shape, tag
        assert rel_l2(y.numpy(), g[f"{tag}.y"]) < TOL, tag


def _sub(g, tag):
    pre = f"{tag}.sd."
    return {k[len(pre):]: t(g[k]) for k in g.files if k.startswith(pre)}


def test_block_primitives():
    g = gold("primitives_blocks")
    for tag in ("res_32_32", "res_32_64", "res_128_32", "res_nocond"):
        sd = {"blk." + k: v for k, v in _sub(g, tag).items()}
        cond = t(g[f"{tag}.cond"]) if f"{tag}.cond" in g.files else None
        y = O.resnet_block(sd, "blk", t(g[f"{tag}.x"]), cond, 8, True)
        assert rel_l2(y.numpy(), g[f"{tag}.y"]) < TOL, tag
    for tag in ("attn_32", "attn_64", "attn_96"):
        sd = {"a." + k: v for k, v in _sub(g, tag).items()}
        y = O.attn_residual(sd, "a", t(g[f"{tag}.x"]), True)
        assert rel_l2(y.numpy(), g[f"{tag}.y"]) < TOL, tag


@pytest.mark.parametrize("name", ["dataset2", "dataset3", "hgcal", "tiny"])
def test_denoise_models(name):
    g = gold(f"model_{name}")
    cfg = load_config(name)
    net = seeded_unet(name, int(g["seed"]))
    verify_checksums(net.state_dict(), g)
    m = O.OracleModel(cfg, net.state_dict())
    x, E = t(g["x"]), t(g["E"])
    layers = t(g["layers"]) if "layers" in g.files else None
    with torch.no_grad():
        for i in range(3):
            s = float(g[f"sigma_{i}"])
            sig = torch.full((x.shape[0],), s)
            y = m.denoise(x * float(np.sqrt(1.0 + s * s)), E, sig, layers)
            assert rel_l2(y.numpy(), g[f"denoise_{i}"]) < TOL, (name, i)


def test_unet_d1_grid():
    g = gold("unet_d1grid")
    net = seeded_unet(d1grid_kwargs(), int(g["seed"]))
    verify_checksums(net.state_dict(), g)
    spec = O.UnetSpec(layer_sizes=[32, 32, 64, 96], channels=4, cond_size=7, data_shape=(5, 10, 30))
    assert spec.up_kernel_z == [3, 3] and spec.up_out_pad == [(0, 1, 1), (0, 0, 0)]
    with torch.no_grad():
        y = O.cond_unet_forward(net.state_dict(), spec, t(g["x"]), t(g["cond"]), t(g["time"]))
    assert rel_l2(y.numpy(), g["y"]) < TOL


def test_reverse_norm():
    """Inverse pre-processing (utils.ReverseNormCaloChall): numpy restatement against the reference's outputs."""
    from calodiffusion_amd.postprocess import DATASET_PARAMS
    g = gold("reverse_norm")
    for tag, dnum in (("d2", 2), ("d3", 3)):
        layerE = g[f"{tag}.layerE"] if f"{tag}.layerE" in g.files else None
        data, energy = O.reverse_norm_calochall(g[f"{tag}.vox"], g[f"{tag}.e"], layerE, DATASET_PARAMS[dnum], ecut=0.0000151)
        assert np.array_equal(np.asarray(energy, dtype=np.float32), g[f"{tag}.energy"])
        assert rel_l2(np.asarray(data, dtype=np.float32), g[f"{tag}.data"]) < 2e-6, tag
        assert ((np.asarray(data) == 0) == (g[f"{tag}.data"] == 0)).mean() > 0.9999  # same voxels under the read-out threshold


def test_reverse_norm_hgcal():
    """utils.ReverseNormHGCal: numpy restatement against the reference's outputs (stand-in decoder: (phi, r) flattened to cells)."""
    from calodiffusion_amd.postprocess import DATASET_PARAMS
    g = gold("reverse_norm_hgcal")
    dec = lambda d: np.squeeze(d, axis=1).reshape(d.shape[0], d.shape[2], -1)  # noqa: E731
    data, gen = O.reverse_norm_hgcal(g["vox"], g["e"], g["layerE"], DATASET_PARAMS[111], decode=dec)
    assert np.allclose(np.asarray(gen, dtype=np.float32), g["layer.gen"], rtol=1e-6) and data.shape == g["layer.data"].shape
    assert rel_l2(np.asarray(data, dtype=np.float32), g["layer.data"]) < 2e-6
    data, gen = O.reverse_norm_hgcal(g["vox"], g["e"], None, DATASET_PARAMS[120], decode=dec)
    assert data.shape == g["plain.data"].shape and rel_l2(np.asarray(data, dtype=np.float32), g["plain.data"]) < 2e-6
    # dataset 121, layer mode: many layer energies sit near reverse_logit's alpha, where 1e-8 and 1e-6 give different showers
    data, gen = O.reverse_norm_hgcal(g["vox"], g["e"], g["layerE"], DATASET_PARAMS[121], decode=dec)
    assert rel_l2(np.asarray(data, dtype=np.float32), g["layer121.data"]) < 2e-6
    assert per_layer_worst(np.asarray(data, dtype=np.float32), g["layer121.data"]) < 1e-5


def test_edm_euler_trajectories():
    """EDM Euler sampler (reference models/sample.py:577-727, 771-789): the Karras time steps bit for bit, the oracle's loop
    against the reference's trajectories, and the host step table that maps it onto the device sampler loop."""
    from calodiffusion_amd import schedule
    g = gold("euler_dataset2")
    for n in (5, 18):
        assert np.array_equal(schedule.edm_time_steps(n).numpy(), g[f"tsteps_{n}"])
        tab = schedule.edm_euler_step_table(n)
        assert tab.shape == (n, 4) and np.array_equal(tab[:, 0], g[f"tsteps_{n}"][:-1]) and np.array_equal(tab[:, 1], g[f"tsteps_{n}"][1:])
        assert tab[-1, 1] == 0.0 and not tab[:, 2].any() and (tab[:, 3] == 1).all()
    cfg = load_config("dataset2")
    m = O.OracleModel(cfg, seeded_unet("dataset2").state_dict())
    start, E, layers = t(g["start"]), t(g["E"]), t(g["layers"])
    x, xs, x0s = m.edm_euler_sample(start, E, layers, 5, keep=True)
    assert rel_l2(x.numpy(), g["euler_5"]) < 1e-5
    assert rel_l2(torch.stack(x0s).numpy(), g["euler_5_x0s"]) < 1e-5
    x, _, _ = m.edm_euler_sample(start, E, layers, 18, sample_offset=2)
    assert rel_l2(x.numpy(), g["euler_18_off2"]) < 1e-5


def test_ddim_trajectories():
    g = gold("ddim_dataset2")
    cfg = load_config("dataset2")
    m = O.OracleModel(cfg, seeded_unet("dataset2").state_dict())
    start, E, layers = t(g["start"]), t(g["E"]), t(g["layers"])
    for n in (2, 10):
        x, xs, x0s = m.ddim_sample(start, E, layers, n, keep=True)
        assert rel_l2(x.numpy(), g[f"ddim_{n}"]) < 1e-5, n
        if n == 10:
            assert rel_l2(torch.stack(xs).numpy(), g["ddim_10_xs"]) < 1e-5
            assert rel_l2(torch.stack(x0s).numpy(), g["ddim_10_x0s"]) < 1e-5
    x, _, _ = m.ddim_sample(start, E, layers, 10, sample_offset=3)
    assert rel_l2(x.numpy(), g["ddim_10_off3"]) < 1e-5


def test_ddpm_tiny_with_seeded_noise():
    g = gold("ddpm_tiny")
    cfg = load_config("tiny")
    m = O.OracleModel(cfg, seeded_unet("tiny").state_dict())
    start, E, layers = t(g["start"]), t(g["E"]), t(g["layers"])
    torch.manual_seed(int(g["noise_seed"]))
    noise = [torch.randn(start.shape) for _ in range(50)]
    x, xs, x0s = m.ddim_sample(start, E, layers, 50, eta=1.0, step_noise=noise, keep=True)
    assert rel_l2(xs[10].numpy(), g["x_step10"]) < 1e-5
    assert rel_l2(x0s[10].numpy(), g["x0_step10"]) < 1e-5
    assert rel_l2(x.numpy(), g["ddpm_50"]) < 1e-4


def test_loss_values():
    g = gold("loss_dataset2")
    m = O.OracleModel(load_config("dataset2"), seeded_unet("dataset2").state_dict())
    with torch.no_grad():
        loss = m.hybrid_l2_loss(t(g["data"]), t(g["E"]), t(g["noise"]), t(g["layers"]), rnd_normal=t(g["rnd_normal"]))
    assert abs(float(loss) - float(g["loss"])) <= 2e-6 * abs(float(g["loss"]))
    g = gold("loss_dataset3")
    m = O.OracleModel(load_config("dataset3"), seeded_unet("dataset3").state_dict())
    with torch.no_grad():
        loss = m.hybrid_l2_loss(t(g["data"]), t(g["E"]), t(g["noise"]), None, time=torch.from_numpy(g["time"]))
    assert abs(float(loss) - float(g["loss"])) <= 2e-6 * abs(float(g["loss"]))


def test_work_accounting_matches_survey():
    """Algorithmic FLOPs per sample-step reproduce SURVEY.md section 8d (5.44 G D2, 30.3 G D3, 6.47 G HGCal)."""
    for name, want in (("dataset2", 5.44e9), ("dataset3", 30.3e9), ("hgcal", 6.47e9)):
        w = O.algorithmic_work(O.spec_from_config(load_config(name)))
        assert abs(w["flops"]["total"] - want) / want < 0.02, (name, w["flops"]["total"])


def test_layer_model_against_reference():
    """LayerDiffusion's layer stage (reference models/layerdiffusion.py:109-132, models/models.py:373-457): the oracle's ResNet
    MLP, its EDM denoiser and the DDim / Euler trajectories over (B, D+1) vectors against the reference's outputs; the
    parameter containers reproduce the reference's seeded initialisation (layer model first, then the U-Net)."""
    from helpers import seeded_layer_models
    g = gold("layer_dataset2")
    layer, unet = seeded_layer_models("dataset2")
    verify_checksums(layer.state_dict(), g)
    verify_checksums(unet.state_dict(), {"ck_keys": g["unet_ck_keys"], "ck_vals": g["unet_ck_vals"]})
    cfg = load_config("dataset2")
    m = O.OracleLayerModel(cfg, layer.state_dict())
    x, E, tm, start = t(g["x"]), t(g["E"]), t(g["time"]), t(g["start"])
    with torch.no_grad():
        assert rel_l2(O.resnet_mlp_forward(m.sd, x, E, tm).numpy(), g["forward"]) < TOL
        for i in range(3):
            s = float(g[f"sigma_{i}"])
            y = m.denoise(x * float(np.sqrt(0.25 + s * s)), E, torch.full((3,), s), None)
            assert rel_l2(y.numpy(), g[f"denoise_{i}"]) < TOL, i
        for n in (12, 400):
            y, _, _ = m.ddim_sample(start, E, None, n)
            assert rel_l2(y.numpy(), g[f"layers_{n}"]) < 1e-5, n
        y, _, _ = m.ddim_sample(start, E, None, 12, sample_offset=2)
        assert rel_l2(y.numpy(), g["layers_12_off2"]) < 1e-5
        y, _, _ = m.edm_euler_sample(start, E, None, 12)
        assert rel_l2(y.numpy(), g["layers_euler_12"]) < 1e-5
        # two-stage sample: the generated layer energies condition the U-Net sampler
        assert rel_l2(m.ddim_sample(start, E, None, 12)[0].numpy(), g["sample_3_layers"]) < 1e-5
        u = O.OracleModel(cfg, unet.state_dict())
        xs, _, _ = u.ddim_sample(t(g["shower_start"]), E, t(g["sample_3_layers"]), 3)
        assert rel_l2(xs.numpy(), g["sample_3_x"]) < 1e-5


def test_layer_model_loss_matches_reference():
    """The oracle's layer-state loss against the reference's LayerDiffusion.compute_loss (golden made with a fixed noise draw)."""
    from helpers import seeded_layer_models
    g = gold("layer_dataset2")
    if "loss" not in g.files:
        pytest.skip("golden without the layer loss")
    layer, _ = seeded_layer_models("dataset2")
    m = O.OracleLayerModel(load_config("dataset2"), layer.state_dict())
    with torch.no_grad():
        loss = m.hybrid_l2_loss(t(g["loss_layers"]), t(g["E"]), t(g["loss_noise"]), rnd_normal=t(g["loss_rnd"]))
    assert abs(float(loss) - float(g["loss"])) < 2e-6 * abs(float(g["loss"]))


def test_unet_sinusoidal_embeddings():
    """CondUnet(time_embed / cond_embed = True) (reference models.py:132-144, 578-601), called directly as the reference's own
    denoise path cannot (do_time_embed raises KeyError for 'sin'): parameter container and oracle forward."""
    g = gold("unet_sinusoidal")
    for tag, over in (("both", dict(time_embed=True, cond_embed=True, cond_size=1)),
                      ("time", dict(time_embed=True, cond_embed=False, cond_size=10)),
                      ("cond", dict(time_embed=False, cond_embed=True, cond_size=1))):
        kw = dict(out_dim=1, layer_sizes=[32, 32, 64, 32], channels=4, cond_dim=128, resnet_block_groups=8, mid_attn=True,
                  block_attn=True, compress_Z=True, cylindrical=True, data_shape=[1, 4, 8, 8, 8])
        kw.update(over)
        net = seeded_unet(kw, int(g["seed"]))
        verify_checksums(net.state_dict(), {"ck_keys": g[f"{tag}.ck_keys"], "ck_vals": g[f"{tag}.ck_vals"]})
        spec = O.UnetSpec(layer_sizes=[32, 32, 64, 32], channels=4, cond_size=kw["cond_size"], data_shape=(8, 8, 8),
                          time_sin=kw["time_embed"], cond_sin=kw["cond_embed"])
        with torch.no_grad():
            y = O.cond_unet_forward(net.state_dict(), spec, t(g[f"{tag}.x"]), t(g[f"{tag}.cond"]), t(g[f"{tag}.time"]))
        assert rel_l2(y.numpy(), g[f"{tag}.y"]) < TOL, tag


def oracle_sampler(tag, g, m, start, E, layers, noise):
    """One case of sampler_cases.CASES on the oracle (oracle/samplers_oracle.py) -> (x, xs, x0s)."""
    from oracle import samplers_oracle as S
    from sampler_cases import CASES, options
    name, over, _, off, rows = CASES[tag]
    n = int(g[f"{tag}.n"])
    B = start.shape[0]
    den = lambda x, s: m.denoise(x, E, torch.as_tensor(s, dtype=torch.float32).expand(B), layers)  # noqa: E731
    it = iter(noise)
    noisy = bool(over.get("NOISY_SAMPLE", False))
    opts = options(g, tag) or {}
    if name in ("Euler", "Heun", "DPM2"):
        return S.edm_loop(name.lower(), den, start, n, it, noisy=noisy, sample_offset=off)
    if name == "LMS":
        return S.lms(den, start, n, order=opts.get("ORDER", 4)), None, None
    if name == "Restart":
        rl = opts.get("RESTART_LIST", {"0": 0, "1": 0})  # the default table has string keys: never matched
        x, x0s = S.restart(den, start, n, it, rl, noisy=noisy)
        return x, None, x0s
    sig = S.model_sigmas(O.ddim_tables(n), n)
    if name == "DPMPP2M":
        return S.dpmpp2m(den, start, sig), None, None
    if name == "DPMPP2S":
        return S.dpmpp2s(den, start, sig, it, eta=opts.get("ETA", 0.0)), None, None
    if name == "DPM":
        return S.dpm_fast(den, start, sig, n), None, None
    if name == "Consistency":
        x, xs, x0 = S.consistency(den, start, O.ddim_tables(over["CONSIS_NSTEPS"]), over["CONSIS_NSTEPS"], n, it)
        return x, xs, None
    raise KeyError(name)


def test_other_samplers_against_reference_trajectories():
    """oracle/samplers_oracle.py (EDM Euler+churn / Heun / DPM2 / LMS / Restart, DPM / DPM++2S / DPM++2M, Consistency) against
    trajectories of the reference's own sampler classes on the tiny config, with the reference's noise draws replayed."""
    from sampler_cases import CASES, replay_noise
    g = gold("samplers_tiny")
    cfg = load_config("tiny")
    m = O.OracleModel(cfg, seeded_unet("tiny").state_dict())
    for tag, (_, _, _, _, rows) in CASES.items():
        start, E, layers = t(g["start"])[:rows], t(g["E"])[:rows], t(g["layers"])[:rows]
        noise = replay_noise(g, tag, start.shape)
        with torch.no_grad():
            x, xs, x0s = oracle_sampler(tag, g, m, start, E, layers, noise)
        check_sampler_case(tag, g, x, xs, x0s, 2e-5)


def denoise_error_amplification(tag, eps=1e-6, seed=0):
    """How much one sampler case amplifies an error of the denoiser: the oracle's trajectory with every denoise output
    perturbed by `eps` relative L2 (white noise), against the unperturbed one -> (relative L2 of the final tensor) / eps."""
    from sampler_cases import CASES, replay_noise
    g = gold("samplers_tiny")
    m = O.OracleModel(load_config("tiny"), seeded_unet("tiny").state_dict())
    rows = CASES[tag][4]
    start, E, layers = t(g["start"])[:rows], t(g["E"])[:rows], t(g["layers"])[:rows]
    gen = torch.Generator().manual_seed(seed)

    class Perturbed:
        def denoise(self, x, E_, sig, layers_):
            y = m.denoise(x, E_, sig, layers_)
            n = torch.randn(y.shape, generator=gen)
            return y + eps * y.norm() / n.norm() * n

    with torch.no_grad():
        clean = oracle_sampler(tag, g, m, start, E, layers, replay_noise(g, tag, start.shape))[0]
        dirty = oracle_sampler(tag, g, Perturbed(), start, E, layers, replay_noise(g, tag, start.shape))[0]
    return rel_l2(np.asarray(dirty), np.asarray(clean)) / eps


def test_dpm2_case_amplifies_denoiser_error():
    """The `dpm_2` case (DPM-Solver-fast, TWO model evaluations from sigma = 142 to 1) cancels terms of order sigma_max: a
    white-noise denoiser error of 1e-6 comes out ~10x larger (measured: 9.8x), where the seven-evaluation case passes it on at
    ~2x.  tests/test_gpu_round2.py prints this number next to the device's own denoise error for the case."""
    a2, a7 = denoise_error_amplification("dpm_2"), denoise_error_amplification("dpm_7")
    print(f"denoise-error amplification: dpm_2 {a2:.1f}x, dpm_7 {a7:.1f}x")
    assert 5.0 < a2 < 20.0, a2
    assert a7 < a2 / 3, (a2, a7)


def test_reference_gradients():
    """torch autograd through the oracle against .grad of the reference's own compute_loss(...).backward()
    (models/loss.py:163-179, train/train_diffusion.py:52-63): whole tensors and checksums of every parameter's gradient."""
    for name in ("dataset2", "dataset3", "hgcal"):
        g = gold(f"grads_{name}")
        gl = g if name == "hgcal" else gold(f"loss_{name}")  # (the HGCal fixture of round 3 carries its own inputs)
        cfg = load_config(name)
        sd = {k: v.detach().clone().requires_grad_(True) for k, v in seeded_unet(name).state_dict().items()}
        m = O.OracleModel(cfg, sd)
        kw = dict(rnd_normal=t(gl["rnd_normal"])) if name != "dataset3" else dict(time=torch.from_numpy(gl["time"]))
        layers = t(gl["layers"]) if "layers" in gl.files else None
        loss = m.hybrid_l2_loss(t(gl["data"]), t(gl["E"]), t(gl["noise"]), layers, **kw)
        loss.backward()
        assert abs(float(loss) - float(g["loss"])) <= 2e-6 * abs(float(g["loss"]))
        for k in g.files:
            if k.startswith("grad."):
                assert rel_l2(m.sd[k[5:]].grad.numpy(), g[k]) < 2e-5, (name, k)
        for k, (s1, s2) in zip(g["ck_keys"], g["ck_vals"]):
            gr = m.sd[str(k)].grad.double()
            assert abs(float((gr * gr).sum()) - s2) <= 1e-4 * max(s2, 1e-30), (name, k)


def test_loss_types_against_the_reference():
    """LOSS_TYPE l1 / mse / huber / l2 under hybrid_weight (models/loss.py:97-116, 163-179): loss value and .grad of the reference's
    own compute_loss(...).backward() on the tiny config (fixture: oracle/gen_golden.py grads3).  The huber case has residuals on
    both sides of its knee."""
    g = gold("losstypes_tiny")
    cfg = load_config("tiny")
    assert 0.5 < float(g["huber.frac_abs_d_below_1"]) < 0.999
    for lt in ("l1", "mse", "huber", "l2"):
        sd = {k: v.detach().clone().requires_grad_(True) for k, v in seeded_unet("tiny").state_dict().items()}
        m = O.OracleModel(cfg, sd)
        loss = m.hybrid_l2_loss(t(g["data"]), t(g["E"]), t(g["noise"]), t(g["layers"]), rnd_normal=t(g["rnd_normal"]), loss_type=lt)
        loss.backward()
        assert abs(float(loss) - float(g[f"{lt}.loss"])) <= 2e-6 * abs(float(g[f"{lt}.loss"])), lt
        for k in g.files:
            if k.startswith(f"{lt}.grad."):
                assert rel_l2(m.sd[k[len(lt) + 6:]].grad.numpy(), g[k]) < 2e-5, (lt, k)
        for k, (s1, s2) in zip(g[f"{lt}.ck_keys"], g[f"{lt}.ck_vals"]):
            gr = m.sd[str(k)].grad.double()
            assert abs(float((gr * gr).sum()) - s2) <= 1e-4 * max(s2, 1e-30), (lt, k)


def test_dataset3_and_hgcal_trajectories():
    """Dataset-3 DDIM (10 steps) and the first half of the HGCal 200-step DDPM trajectory with the reference's seeded noise."""
    g = gold("ddim_dataset3")
    m = O.OracleModel(load_config("dataset3"), seeded_unet("dataset3").state_dict())
    x, _, _ = m.ddim_sample(t(g["start"]), t(g["E"]), None, 10)
    assert rel_l2(x.numpy(), g["ddim_10"]) < 1e-5
    g = gold("ddpm_hgcal")
    m = O.OracleModel(load_config("hgcal"), seeded_unet("hgcal").state_dict())
    start = t(g["start"])
    torch.manual_seed(int(g["noise_seed"]))
    noise = [torch.randn(start.shape) for _ in range(101)]
    _, xs, x0s = m.ddim_sample(start, t(g["E"]), t(g["layers"]), 200, eta=1.0, step_noise=noise, keep=True, stop_after=101)
    assert rel_l2(xs[100].numpy(), g["x_step100"]) < 1e-5 and rel_l2(x0s[100].numpy(), g["x0_step100"]) < 1e-5


def test_objectives_against_the_reference():
    """TRAINING_OBJ noise_pred / mean_pred (calodiffusion.py:161-165, models/loss.py:181-210) on the tiny config: the oracle's
    denoise, loss value and gradients against the reference's own (fixture: oracle/gen_golden.py objectives); minsnr cannot be
    constructed by the reference (recorded in the fixture) nor here, with the same TypeError."""
    import copy
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    g = gold("objectives_tiny")
    base = load_config("tiny")
    data, E, noise, layers, rnd = (t(g[k]) for k in ("data", "E", "noise", "layers", "rnd_normal"))
    for obj in ("noise_pred", "mean_pred"):
        cfg = copy.deepcopy(base)
        cfg["TRAINING_OBJ"] = obj
        with torch.no_grad():
            m = O.OracleModel(cfg, seeded_unet("tiny").state_dict())
            for i, sg in enumerate(g["sigmas"]):
                xin = data * float(np.sqrt(1.0 + float(sg) ** 2))
                got = m.denoise(xin, E, torch.full((4,), float(sg)), layers)
                assert rel_l2(got.numpy(), g[f"{obj}.denoise_{i}"]) < TOL, (obj, i)
            assert rel_l2(m.ddim_sample(data, E, layers, 6)[0].numpy(), g[f"{obj}.ddim_6"]) < 1e-5, obj
        for lt in ("l2", "huber"):
            sd = {k: v.detach().clone().requires_grad_(True) for k, v in seeded_unet("tiny").state_dict().items()}
            m = O.OracleModel(cfg, sd)
            loss = m.hybrid_l2_loss(data, E, noise, layers, rnd_normal=rnd, loss_type=lt)
            loss.backward()
            want = float(g[f"{obj}.{lt}.loss"])
            assert abs(float(loss) - want) <= 2e-6 * abs(want), (obj, lt)
            pre = f"{obj}.{lt}.grad."
            for k in g.files:
                if k.startswith(pre):
                    assert rel_l2(m.sd[k[len(pre):]].grad.numpy(), g[k]) < 2e-5, k
            for k, (s1, s2) in zip(g[f"{obj}.{lt}.ck_keys"], g[f"{obj}.{lt}.ck_vals"]):
                gr = m.sd[str(k)].grad.double()
                assert abs(float((gr * gr).sum()) - s2) <= 1e-4 * max(s2, 1e-30), (obj, lt, k)
    assert int(g["minsnr.constructs"]) == 0
    cfg = copy.deepcopy(base)
    cfg["TRAINING_OBJ"] = "minsnr"
    with pytest.raises(TypeError, match="positional arguments"):
        CaloDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"])
    with pytest.raises(NotImplementedError, match="Loss type"):  # Loss._loss raises at construction (models/loss.py:113-114)
        CaloDiffusion(base, n_steps=50, loss_type="l3")
