"""GPU (MI355X): the sampler loops on the device -- DDIM with its embeddings computed a chunk of steps ahead, DPMAdaptive's host
loop, the SDE variants through cd_sampler_run -- against the reference's golden trajectory or the same loop on the CPU oracle,
at north_star's 1e-4 per trajectory."""
import numpy as np
import pytest
import torch

from conftest import gold, rel_l2
from helpers import seeded_model, t
from sampler_oracles import SDE_CASES, dpm_adaptive_on_oracle, sde_oracle_run

pytestmark = pytest.mark.gpu


def test_ddim_with_chunked_embeddings_matches_the_reference_over_chunk_boundaries():
    """The sampler loop computes its embeddings 16 steps ahead in one launch and updates x inside the head kernel: 50 steps cross
    three chunk boundaries and end on a partial chunk; against the reference's DDIM trajectory (golden) in graph and eager mode,
    with trajectories recorded (debug) and without."""
    g = gold("ddim_dataset2")
    start, E, layers = t(g["start"]).cuda(), t(g["E"]).cuda(), t(g["layers"]).cuda()
    outs = []
    for use_graph in (True, False):
        m = seeded_model("dataset2")
        assert type(m.sampler_algorithm).__name__ == "DDim"
        m.sampler_algorithm.use_graph = use_graph
        x = m.sample(E, layers, num_steps=50, start=start)
        assert rel_l2(x, g["ddim_50"]) < 1e-4
        outs.append(x)
    assert np.array_equal(outs[0], outs[1])
    xd, xs, x0s = m.sample(E, layers, num_steps=50, start=start, debug=True)
    assert np.array_equal(xd, outs[0]) and len(xs) == 50 and len(x0s) == 50


def test_dpm_adaptive_on_the_device_equals_the_same_loop_on_the_oracle():
    """DPMAdaptive (host loop, one cd_denoise_safe call per model evaluation): the device against the CPU oracle running the
    identical loop -- the reference's own class raises for every input (see the class docstring), so the oracle is the pin."""
    opts = {"ORDER": 3, "H_INIT": 0.25, "R_TOL": 0.5}  # (large steps: ~30 of them, each three oracle evaluations on the CPU)
    (start, E, layers), want, calls, steps = dpm_adaptive_on_oracle(opts, 8)
    m = seeded_model("tiny", {"SAMPLER": "DPMAdaptive", "SAMPLER_OPTIONS": opts})
    assert type(m.sampler_algorithm).__name__ == "DPMAdaptive"
    got = m.sample(E.cuda(), layers.cuda(), num_steps=8, start=start.cuda())
    smp = m.sampler_algorithm
    err = rel_l2(got, want.numpy())
    print(f"DPMAdaptive: {smp.steps_taken} steps, {smp.denoise_calls} denoise calls; device vs oracle loop rel L2 {err:.2e}")
    assert (smp.steps_taken, smp.denoise_calls) == (steps, calls) and err < 1e-4


@pytest.mark.parametrize("name,opts", SDE_CASES)
def test_sde_samplers_on_the_device_equal_the_restated_loops(name, opts):
    """DPMPPSDE / DPMPP2MSDE / DPMPP3MSDE (models/sample.py:347-574) through cd_sampler_run with the unit normals injected, against
    the reference's loops restated on the CPU oracle with the same normals (torchsde is absent: parity unpinned, there is no
    reference trajectory for these classes); and, drawing from the device Philox stream, two runs differ while ETA = 0 is
    deterministic."""
    from oracle import samplers_oracle as SO
    from oracle import torch_oracle as O
    m = seeded_model("tiny", {"SAMPLER": name, "SAMPLER_OPTIONS": dict(opts)})
    smp = m.sampler_algorithm
    assert type(smp).__name__ == name
    n, rows = 7, 2
    gen = torch.Generator().manual_seed(43)
    start = torch.randn((rows, 1, 8, 8, 8), generator=gen)
    E, layers = torch.rand((rows, 3), generator=gen), torch.randn((rows, 9), generator=gen)
    prog = smp.build(m, n, 0).finalize()
    sig = SO.model_sigmas(m.loss_function, n)
    m.loss_function.update_step(m.nsteps)
    noise = [torch.randn(start.shape, generator=gen) for _ in range(prog.n_randn)]
    om = O.OracleModel(m.config, {k[6:]: v.detach().cpu() for k, v in m.state_dict().items()})
    den = lambda x, s: om.denoise(x, E, torch.as_tensor(s).float().expand(rows), layers)  # noqa: E731
    with torch.no_grad():
        want = sde_oracle_run(name, opts, den, start, sig, noise)
    if prog.n_randn:
        smp.step_noise = torch.stack(noise).cuda()
    got = m.sample(E.cuda(), layers.cuda(), num_steps=n, start=start.cuda())
    err = rel_l2(np.asarray(got), want.numpy())
    assert err < 1e-4, (name, opts, err)
    # the device's own stream
    smp.step_noise = None
    a = m.sample(E.cuda(), layers.cuda(), num_steps=n, start=start.cuda())
    b = m.sample(E.cuda(), layers.cuda(), num_steps=n, start=start.cuda())
    a, b = np.asarray(a), np.asarray(b)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    if opts.get("ETA"):
        assert rel_l2(a, b) > 1e-3  # fresh noise per call
    else:
        assert np.array_equal(a, b) and rel_l2(a, want.numpy()) < 1e-4
