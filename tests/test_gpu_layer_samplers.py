"""GPU (MI355X): every step-program sampler of calodiffusion_amd/sample.py on LayerDiffusion's layer stage, through
cd_layer_sampler_run (one launch per trajectory), against the CPU oracle's sampler loops (oracle/samplers_oracle.py) run over
OracleLayerModel.denoise with the same unit normals; its noise stream, its element-wise arithmetic, the two-stage sample, the
unchanged DDim / DDPM / Euler path and the host-side program checks."""
import copy
import itertools

import numpy as np
import pytest
import torch

from conftest import gold, rel_l2
from helpers import TOL_TRAJ
from oracle import torch_oracle as O

pytestmark = pytest.mark.gpu

DIM = 46  # dataset2: SHAPE_FINAL[2] + 1


def _model(**extra):
    from calodiffusion_amd.configs import load_config
    from calodiffusion_amd.layerdiffusion import LayerDiffusion
    cfg = load_config("dataset2")
    cfg["LAYER_STEPS"] = 6
    cfg.update(extra)
    torch.manual_seed(1234)
    return LayerDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"])


def _sampler(m, name, over=None, opts=None):
    from calodiffusion_amd import utils
    cfg = copy.deepcopy(m.config)
    cfg.update(over or {})
    if opts:
        cfg["SAMPLER_OPTIONS"] = dict(opts)
    smp = utils.load_attr("sampler", name)(cfg)
    assert type(smp).__name__ == name
    return smp


def _inputs(B, seed):
    gen = torch.Generator().manual_seed(seed)
    start = torch.randn((B, DIM), generator=gen)
    E = torch.rand((B, 1), generator=gen) + 0.5
    return start, E, gen


def _run_layer(m, smp, start, E, n, off, debug=True):
    m.set_layer_state(is_layer=True)
    try:
        return smp(m, start.cuda(), E.cuda(), None, n, off, debug)
    finally:
        m.set_layer_state(is_layer=False)


def _oracle(name, over, opts, om, start, E, n, off, noise):
    """The oracle loop of one sampler on the layer model; (B, dim) vectors viewed as (B, 1, 1, 1, dim) for the loops.
    -> (x, xs, x0s) as (B, dim) tensors / lists (None where the loop keeps no trajectory)."""
    from oracle import samplers_oracle as S
    B = start.shape[0]
    v5 = lambda a: a.reshape(B, 1, 1, 1, DIM)  # noqa: E731
    den = lambda x, s: v5(om.denoise(x.reshape(B, DIM), E, torch.as_tensor(s, dtype=torch.float32).expand(B)))  # noqa: E731
    # normals in draw order; a loop that draws where the program does not multiplies the draw by zero
    it = itertools.chain((v5(z) for z in noise), itertools.repeat(torch.zeros(B, 1, 1, 1, DIM)))
    noisy = bool(over.get("NOISY_SAMPLE", False))
    opts = opts or {}
    x5, xs, x0s = start.reshape(B, 1, 1, 1, DIM), None, None
    if name in ("Euler", "Heun", "DPM2"):
        x, xs, x0s = S.edm_loop(name.lower(), den, x5, n, it, noisy=noisy, sample_offset=off)
    elif name == "LMS":
        x = S.lms(den, x5, n, order=opts.get("ORDER", 4), sample_offset=off)
    elif name == "Restart":
        x, x0s = S.restart(den, x5, n, it, opts.get("RESTART_LIST", {"0": 0, "1": 0}), noisy=noisy)
    elif name == "Consistency":
        x, xs, x0 = S.consistency(den, x5, O.ddim_tables(over["CONSIS_NSTEPS"]), over["CONSIS_NSTEPS"], n, it)
        x0s = [x0]
    else:
        sig = S.model_sigmas(O.ddim_tables(n), n)
        eta, s_noise = opts.get("ETA", 0.0), opts.get("S_NOISE", 1.0)
        if name == "DPMPP2M":
            x = S.dpmpp2m(den, x5, sig)
        elif name == "DPMPP2S":
            x = S.dpmpp2s(den, x5, sig, it, eta=eta)
        elif name == "DPM":
            x = S.dpm_fast(den, x5, sig, n)
        elif name == "DPMPPSDE":
            x = S.dpmpp_sde(den, x5, sig, it, eta, s_noise, opts.get("R", 0.5))
        elif name == "DPMPP2MSDE":
            x = S.dpmpp_2m_sde(den, x5, sig, it, eta, s_noise, opts.get("SOLVER", "heun"))
        elif name == "DPMPP3MSDE":
            x = S.dpmpp_3m_sde(den, x5, sig, it, eta, s_noise)
        else:
            raise KeyError(name)
    flat = lambda seq: None if seq is None else [a.reshape(B, DIM) for a in seq]  # noqa: E731
    return x.reshape(B, DIM), flat(xs), flat(x0s)


def _close(got, want, tol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    fin = np.isfinite(want)
    if not fin.all():  # Heun / DPM2 divide by t_next = 0 on their last step, like the reference: not finite here either
        assert not np.isfinite(got).all(), what
        return
    err = rel_l2(got, want)
    assert err < tol, (what, err)


def _parity_cases():
    from sampler_cases import CASES
    cases = [(tag, name, over, opts, off) for tag, (name, over, opts, off, _) in CASES.items()]
    for name, solver in (("DPMPPSDE", None), ("DPMPP2MSDE", "heun"), ("DPMPP2MSDE", "midpoint"), ("DPMPP3MSDE", None)):
        opts = {"ETA": 1.0} if solver is None else {"ETA": 1.0, "SOLVER": solver}
        cases.append((f"{name.lower()}{'_' + solver if solver else ''}_eta1", name, {}, opts, 0))
    return cases


_CASES = _parity_cases()


@pytest.fixture(scope="module")
def hybrid_model():
    return _model()


@pytest.mark.parametrize("case", _CASES, ids=[c[0] for c in _CASES])
def test_program_samplers_match_the_oracle_loops(case, hybrid_model):
    """Final x and the recorded trajectories of every program sampler on the layer stage (B = 3) against the oracle loop with
    the same injected normals."""
    from sampler_cases import options
    tag, name, over, opts, off = case
    g = gold("samplers_tiny")
    if opts in ("restart_int", "restart_noisy"):
        opts = options(g, tag)
    n = int(g[f"{tag}.n"]) if f"{tag}.n" in g.files else 7
    _check_case(hybrid_model, name, over, opts, off, n, seed=11)


def test_program_sampler_on_a_noise_pred_model():
    m = _model(TRAINING_OBJ="noise_pred")
    assert m.layer_model._engine_opts["objective"] == "noise_pred"
    _check_case(m, "Heun", {"NOISY_SAMPLE": True}, None, 0, 6, seed=12)
    _check_case(m, "DPMPP2M", {}, None, 0, 6, seed=13)


def _check_case(m, name, over, opts, off, n, seed):
    smp = _sampler(m, name, over, opts)
    start, E, gen = _inputs(3, seed)
    n_randn = smp.build(m, n, off).finalize().n_randn
    m.loss_function.update_step(m.nsteps)  # (DPM.setup_sigmas re-tabulates the model's schedule)
    noise = [torch.randn((3, DIM), generator=gen) for _ in range(n_randn)]
    smp.step_noise = torch.stack(noise).cuda() if n_randn else None
    x, xs, x0s = _run_layer(m, smp, start, E, n, off)
    m.loss_function.update_step(m.nsteps)
    assert smp.ran_program and smp.noise_tensors_drawn == n_randn
    om = O.OracleLayerModel(m.config, {k: v.detach().cpu() for k, v in m.layer_model.state_dict().items()})
    with torch.no_grad():
        wx, wxs, wx0s = _oracle(name, over, opts, om, start, E, n, off, noise)
    _close(x.cpu(), wx, TOL_TRAJ, (name, "x"))
    if name == "Consistency":
        wx0s, x0s = wx0s[-1], x0s
        _close(x0s.cpu(), wx0s, TOL_TRAJ, (name, "x0"))
        wx0s = None
    for what, got, want in (("xs", xs, wxs), ("x0s", x0s, wx0s)):
        if want is None or not smp.returns_trajectories:
            continue
        assert len(got) == len(want), (name, what, len(got), len(want))
        _close(torch.stack(list(got)).cpu(), torch.stack(want), TOL_TRAJ, (name, what))


def _euler_noisy(m):
    """EDM Euler with churn: a program sampler that draws one normal tensor per step and ends finite."""
    return _sampler(m, "Euler", {"NOISY_SAMPLE": True})


def test_device_noise_is_the_documented_philox_slice(hybrid_model):
    """step_noise=None draws tensor k of a program at Philox elements offset + k * B * dim + b * dim + i: bitwise the run fed
    the tensors cd_randn draws there."""
    from calodiffusion_amd import engine
    m = hybrid_model
    smp = _euler_noisy(m)
    start, E, _ = _inputs(4, 21)
    prog = smp.build(m, 5, 0).finalize()
    assert prog.n_randn > 0
    eng = m.layer_model.engine()
    seed, offset = 77, 1000
    a, _, _ = eng.sampler_run(start.cuda(), E.cuda(), prog, seed=seed, offset=offset)
    per = start.numel()
    fed = torch.stack([engine.randn((4, DIM), "cuda", seed, offset + k * per) for k in range(prog.n_randn)])
    b, _, _ = eng.sampler_run(start.cuda(), E.cuda(), prog, step_noise=fed)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    c, _, _ = eng.sampler_run(start.cuda(), E.cuda(), prog, seed=seed, offset=offset + 1)
    assert not torch.equal(a, c)


def test_batch_shards_concatenate_to_the_whole_batch(hybrid_model):
    """Rows [0, 2) and [2, 5) of a 5-row batch, each drawing its rows of the global stream (set_noise_shard), concatenate to the
    5-row run bit for bit, and every run advances the stream by the same global amount."""
    m = hybrid_model
    m.layer_sampler = _euler_noisy(m)
    _, E, _ = _inputs(5, 22)
    E = E.cuda()
    outs, offsets = [], []
    for lo, hi, shard in ((0, 5, None), (0, 2, (0, 5)), (2, 5, (2, 5))):
        m.noise_offset = 0
        m.set_noise_shard(*(shard or (0, 0)))
        outs.append(m.sample_layers(E[lo:hi], sample_offset=0))
        offsets.append(m.noise_offset)
    m.set_noise_shard(0, 0)
    n_randn = m.layer_sampler.noise_tensors_drawn
    assert n_randn > 0 and m.layer_sampler.ran_program
    assert offsets == [5 * DIM * (1 + n_randn)] * 3
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(torch.cat(outs[1:]), outs[0])


def test_elementwise_ops_round_as_torch():
    """RANDN / LINCOMB / LINDIV / RECORD without DENOISE: LINDIV bitwise the chain of torch fp32 element-wise ops, LINCOMB (one
    fused multiply-add) within 1 ulp of the sum of its terms' magnitudes."""
    from calodiffusion_amd import engine
    from calodiffusion_amd.sample import Program
    m = _model()
    eng = m.layer_model.engine()
    rng = np.random.default_rng(5)
    n_steps, B = 4, 3
    coef = lambda: float(np.float32(rng.uniform(0.3, 1.7)) * (1 if rng.random() < 0.7 else -1))  # noqa: E731
    prog = Program(4, float(np.float32(1.25)))
    for _ in range(n_steps):
        st = prog.step()
        st.randn(1)
        st.lin(2, [(0, coef()), (1, coef())])
        st.record(1, 2)
        st.lin_div(0, [(0, coef()), (1, coef()), (2, coef())], coef())  # dst is a source
        st.record(0, 0)
    prog.finalize()
    assert prog.op_begin is None  # the same ops every step, their coefficients per step
    start = torch.randn((B, DIM), generator=torch.Generator().manual_seed(6)).cuda()
    E = torch.full((B, 1), 1.0, device="cuda")
    seed, offset = 3, 500
    x, xs, x0s = eng.sampler_run(start, E, prog, seed=seed, offset=offset, debug=True)
    c = prog.coefs
    xt = start * np.float32(prog.start_scale)
    worst = 0.0
    for i in range(n_steps):
        nz = engine.randn((B, DIM), "cuda", seed, offset + i * B * DIM)
        row = [float(v) for v in c[i]]
        t0, t1 = row[0] * xt, row[1] * nz
        want2 = t0 + t1
        bound = torch.from_numpy(np.spacing((t0.abs() + t1.abs()).cpu().numpy().astype(np.float32)))
        gap = (x0s[i] - want2).abs().cpu()
        worst = max(worst, float((gap / bound).max()))
        assert bool((gap <= bound).all()), (i, float((gap / bound).max()))
        got2 = x0s[i]  # the device's own buffer 2 feeds the LINDIV check
        acc = row[2] * xt
        acc = acc + row[3] * nz
        acc = acc + row[4] * got2
        xt = acc / torch.full_like(acc, row[5])  # (a tensor divisor: torch multiplies by the reciprocal of a scalar one)
        assert torch.equal(xs[i], xt), i
    assert torch.equal(x, xt)
    print(f"LINCOMB: worst gap {worst:.3f} ulp of the terms' magnitude sum")


# (Heun is not among them: like the reference, its last step divides by t_next = 0 and the layer energies it ends with are not
# finite -- see sample.Heun; its one-launch trajectory is checked below and its parity above)
E2E_SAMPLERS = [("Euler", {"NOISY_SAMPLE": True}), ("LMS", {}), ("Restart", {}), ("DPMPP2M", {}), ("DPMPP2MSDE", {"ETA": 1.0})]


@pytest.mark.parametrize("name,opts", E2E_SAMPLERS, ids=[n for n, _ in E2E_SAMPLERS])
def test_two_stage_sample_with_a_program_layer_sampler(name, opts):
    """LayerDiffusion.sample(return_layers=True) with LAYER_SAMPLER = a program sampler: layers and showers come back, and the
    stream offset accounts for the layer start, every tensor the layer program drew, the shower start and its steps."""
    over = {"LAYER_SAMPLER": name}
    if opts.get("NOISY_SAMPLE"):
        over["NOISY_SAMPLE"] = True
    elif opts:
        over["SAMPLER_OPTIONS"] = dict(opts)
    m = _model(**over)
    assert type(m.layer_sampler).__name__ == name
    B, n_shower = 2, 3
    E = (torch.rand((B, 1), generator=torch.Generator().manual_seed(30)) + 0.5).cuda()
    m.noise_offset = 0
    out = m.sample(E, num_steps=n_shower, sample_offset=0, return_layers=True)
    layers, x = out["layers"].cpu().numpy(), out["x"]
    assert layers.shape == (B, DIM) and x.shape[0] == B
    drawn = m.layer_sampler.noise_tensors_drawn
    assert m.layer_sampler.ran_program
    if name in ("DPMPP2MSDE", "Euler"):
        assert drawn > 0
    vox = int(np.prod(x.shape[1:]))
    assert m.noise_offset == B * DIM * (1 + drawn) + B * vox * (1 + n_shower)
    assert np.isfinite(layers).all() and np.isfinite(x).all()


@pytest.mark.parametrize("name", ["DDim", "DDPM", "Euler"])
def test_table_samplers_still_ride_cd_layer_sample(name):
    """DDim / DDPM / Euler without churn: one layer_mlp launch (cd_layer_sample), no layer_program, bitwise a direct
    engine.ddim_sample, and the stream advanced as before."""
    from calodiffusion_amd import engine, schedule
    m = _model(LAYER_SAMPLER=name)
    start, E, _ = _inputs(3, 40)
    start, E = start.cuda(), E.cuda()
    m.noise_offset = 123
    engine.profile_begin()
    y = m.sample_layers(E, sample_offset=0, start=start)
    prof = engine.profile_end()
    # (DDPM draws its (n_steps, B, dim) noise block with cd_randn first, as before)
    assert set(prof) == ({"layer_mlp", "randn"} if name == "DDPM" else {"layer_mlp"}), prof
    assert prof["layer_mlp"]["launches"] == 1, prof
    assert not m.layer_sampler.ran_program
    assert m.noise_offset == 123 + start.numel() * m.layer_steps
    n = m.layer_steps
    if name == "Euler":
        smp = m.layer_sampler
        table = schedule.edm_euler_step_table(n, 0, sigma_min=smp.sigma_min, sigma_max=smp.sigma_max, rho=smp.rho)
    else:
        table = schedule.ddim_step_table(n, 1.0 if name == "DDPM" else 0.0, 0)
    want, _, _ = m.layer_model.engine().ddim_sample(start, E, table, seed=m.noise_seed, offset=123)
    assert torch.equal(y, want)


def test_one_heun_trajectory_is_one_launch(hybrid_model):
    from calodiffusion_amd import engine
    m = hybrid_model
    m.layer_sampler = _sampler(m, "Heun")
    start, E, _ = _inputs(3, 50)
    engine.profile_begin()
    y = m.sample_layers(E.cuda(), sample_offset=0, start=start.cuda())
    prof = engine.profile_end()
    assert set(prof) == {"layer_program"} and prof["layer_program"]["launches"] == 1, prof
    assert y.shape == (3, DIM)


class _Prog:
    """A hand-made program object with the attributes engine.sampler_run reads."""

    def __init__(self, ops, n_bufs=4, n_steps=2, n_coef=3, op_begin=None):
        self.ops, self.op_begin, self.n_bufs, self.start_scale, self.n_randn = ops, op_begin, n_bufs, 1.0, 0
        self.coefs = np.ones((n_steps, n_coef), dtype=np.float32)


def test_bad_programs_are_refused_before_any_launch():
    from calodiffusion_amd import engine
    from calodiffusion_amd.engine import SOP_DENOISE, SOP_LINCOMB, SOP_LINDIV, SOP_RECORD
    m = _model()
    eng = m.layer_model.engine()
    start, E, _ = _inputs(2, 60)
    start, E = start.cuda(), E.cuda()
    good = [(SOP_DENOISE, 1, (0,), 0), (SOP_LINCOMB, 0, (0, 1), 1)]
    bad = {
        "dst buffer": [(SOP_LINCOMB, 4, (0, 1), 0)],
        "src buffer": [(SOP_LINCOMB, 0, (0, 4), 0)],
        "negative buffer": [(SOP_DENOISE, 1, (-1,), 0)],
        "record src": [(SOP_RECORD, 0, (9,), 0)],
        "lincomb column": [(SOP_LINCOMB, 0, (0, 1), 2)],
        "lindiv column": [(SOP_LINDIV, 0, (0, 1), 1)],
        "denoise column": [(SOP_DENOISE, 1, (0,), 3)],
        "nsrc 0": [(SOP_LINCOMB, 0, (), 0)],
        "nsrc 7": [(SOP_LINCOMB, 0, (0, 1, 2, 3, 0, 1, 2), 0)],
        "unknown kind": [(9, 0, (0,), 0)],
    }
    engine.profile_begin()
    x, _, _ = eng.sampler_run(start, E, _Prog(good))  # the good program runs
    for what, ops in bad.items():
        with pytest.raises(ValueError):
            eng.sampler_run(start, E, _Prog(ops))
        print(what, "refused")
    with pytest.raises(ValueError, match="op_begin"):
        eng.sampler_run(start, E, _Prog(good + good, op_begin=[0, 3, 2]))
    with pytest.raises(ValueError, match="op_begin"):
        eng.sampler_run(start, E, _Prog(good + good, op_begin=[0, 2, 3]))
    prof = engine.profile_end()
    assert prof["layer_program"]["launches"] == 1 and set(prof) == {"layer_program"}, prof
    assert torch.isfinite(x).all()


def test_unet_engine_refuses_the_same_bad_programs_with_the_same_messages():
    """cd_sampler_run and cd_layer_sampler_run check a program with one function: on the tiny U-Net every bad program of the test
    above is refused before anything is enqueued, in the words the layer model refuses it with."""
    from calodiffusion_amd import engine
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    from calodiffusion_amd.configs import load_config
    from calodiffusion_amd.engine import SOP_DENOISE, SOP_LINCOMB, SOP_LINDIV, SOP_RECORD
    cfg = copy.deepcopy(load_config("tiny"))
    torch.manual_seed(1234)
    um = CaloDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type=cfg["LOSS_TYPE"])
    ueng = um.engine()
    gen = torch.Generator().manual_seed(61)
    ucond = torch.rand((2, ueng.unet.cond_size), generator=gen).cuda()
    ustart = torch.randn((2,) + tuple(ueng.state_shape), generator=gen).cuda()
    leng = _model().layer_model.engine()
    lstart, lE, _ = _inputs(2, 60)
    lstart, lE = lstart.cuda(), lE.cuda()
    good = [(SOP_DENOISE, 1, (0,), 0), (SOP_LINCOMB, 0, (0, 1), 1)]
    bad = {
        "dst buffer": _Prog([(SOP_LINCOMB, 4, (0, 1), 0)]),
        "src buffer": _Prog([(SOP_LINCOMB, 0, (0, 4), 0)]),
        "negative buffer": _Prog([(SOP_DENOISE, 1, (-1,), 0)]),
        "record src": _Prog([(SOP_RECORD, 0, (9,), 0)]),
        "lincomb column": _Prog([(SOP_LINCOMB, 0, (0, 1), 2)]),
        "lindiv column": _Prog([(SOP_LINDIV, 0, (0, 1), 1)]),
        "denoise column": _Prog([(SOP_DENOISE, 1, (0,), 3)]),
        "nsrc 0": _Prog([(SOP_LINCOMB, 0, (), 0)]),
        "nsrc 7": _Prog([(SOP_LINCOMB, 0, (0, 1, 2, 3, 0, 1, 2), 0)]),
        "unknown kind": _Prog([(9, 0, (0,), 0)]),
        "op_begin decreasing": _Prog(good + good, op_begin=[0, 3, 2]),
        "op_begin short of n_ops": _Prog(good + good, op_begin=[0, 2, 3]),
    }
    x, _, _ = ueng.sampler_run(ustart, ucond, _Prog(good))  # the good program runs
    assert torch.isfinite(x).all()
    engine.profile_begin()
    for what, prog in bad.items():
        with pytest.raises(ValueError) as from_unet:
            ueng.sampler_run(ustart, ucond, prog)
        with pytest.raises(ValueError) as from_layer:
            leng.sampler_run(lstart, lE, prog)
        print(what, "refused:", from_unet.value)
        assert str(from_unet.value) == str(from_layer.value), what
        if what.startswith("op_begin"):
            assert "op_begin" in str(from_unet.value)
    prof = engine.profile_end()
    assert prof == {}, prof
