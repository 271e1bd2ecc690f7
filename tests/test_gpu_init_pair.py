"""GPU (MI355X): the init conv and the first block's first 3x3x3 conv as one composed launch (kernels_init_pair.hip): a one-channel
5x5x5 conv of c_in x whose weights depend on the output voxel's boundary class (conv1 zero-pads the init conv's OUTPUT in z and r),
plus a table carrying the coordinate channels and both biases.  CD_NO_INIT_PAIR=1 forces the chained sequence, the in-process
reference of the denoise-level tests; the op-level tests compare with torch in float64."""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from helpers import TOL_ORACLE, TOL_REASSOC, seeded_model_cfg
from oracle import torch_oracle as O

pytestmark = pytest.mark.gpu

SWITCH = "CD_NO_INIT_PAIR"
TOL_STATS = 1e-6     # test_chunking_of_the_skip_half_changes_no_output_bit's bound, of the summed terms
_SIGMAS = [0.3, 2.5, 0.05, 11.0, 80.0, 1.0, 0.02, 5.0]

# (grid D x H x W, slabs forced (0: the launcher's own, one plane per workgroup at these batches))
GRIDS = [((2, 3, 2), 0),     # no z- or r-interior
         ((3, 1, 3), 0),     # phi wraps twice under five taps
         ((3, 2, 3), 0),
         ((5, 16, 9), 0),    # Dataset-2's plane: 144 voxels, not a multiple of 32; all nine classes
         ((7, 4, 3), 0),     # seven one-plane slabs
         ((7, 4, 3), 2),     # two slabs of 4 + 3 planes: seams inside a slab and between slabs
         ((3, 50, 18), 0)]   # Dataset-3's plane


def _case(dims, B, seed=7):
    D, H, W = dims
    gen = torch.Generator().manual_seed(seed + 13 * D + 5 * H + W)
    x = torch.randn((B, D, H, W), generator=gen)
    scale = torch.tensor([0.7, 1.3, 0.4][:B])
    w0 = torch.randn((32, 4, 3, 3, 3), generator=gen) * 0.2
    b0 = torch.randn((32,), generator=gen) * 0.1
    w1 = torch.randn((32, 32, 3, 3, 3), generator=gen) * 0.05
    b1 = torch.randn((32,), generator=gen) * 0.1
    r_w, z_d, phi_h = torch.rand((W,), generator=gen), torch.rand((D,), generator=gen), torch.rand((H,), generator=gen)
    return x, scale, w0, b0, w1, b1, r_w, z_d, phi_h


def _stack(x, scale, r_w, z_d, phi_h):
    """cat(c_in x, R, Z, phi) as the denoiser feeds the init conv: (B, 4, D, H, W)."""
    B, D, H, W = x.shape
    return torch.cat([(x * scale.view(B, 1, 1, 1)).unsqueeze(1),
                      r_w.view(1, 1, 1, 1, W).expand(B, 1, D, H, W), z_d.view(1, 1, D, 1, 1).expand(B, 1, D, H, W),
                      phi_h.view(1, 1, 1, H, 1).expand(B, 1, D, H, W)], 1)


def _ref64(x, scale, w0, b0, w1, b1, r_w, z_d, phi_h):
    """conv1(init_conv(cat(c_in x, coords))) in float64 on the CPU with the oracle's cylindrical conv: (B, D, H, W, 32)."""
    d = lambda t: t.double()
    xin = _stack(d(x), d(scale), d(r_w), d(z_d), d(phi_h))
    h = O.cyl_conv3d(xin, d(w0), d(b0), padding=(1, 1, 1))
    return O.cyl_conv3d(h, d(w1), d(b1), padding=(1, 1, 1)).permute(0, 2, 3, 4, 1).contiguous()


_refs = {}


def _shared(dims, B):
    """inputs and the float64 reference of one (grid, batch), computed once and left unchanged"""
    key = (dims, B)
    if key not in _refs:
        c = _case(dims, B)
        _refs[key] = (c, _ref64(*c))
    return _refs[key]


def _composed(ops, c, slabs=0, **kw):
    x, scale, w0, b0, w1, b1, r_w, z_d, phi_h = [t.cuda() for t in c]
    return ops.init_pair_conv(x, w0, b0, w1, b1, profiles=(r_w, z_d, phi_h, 1, 1), scale=scale, slabs=slabs, **kw)


def _launches(fn):
    from calodiffusion_amd import engine
    engine.profile_begin()
    fn()
    return {k: v["launches"] for k, v in engine.profile_end().items()}


def _is_pair(cat):
    return cat.startswith("init_pair_conv")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dims,slabs", GRIDS)
def test_composed_and_chained_against_float64(dims, slabs, B):
    from calodiffusion_amd.engine import Ops
    ops = Ops()
    c, want = _shared(dims, B)
    x, scale, w0, b0, w1, b1, r_w, z_d, phi_h = c
    D = dims[0]
    got = {}
    cats = _launches(lambda: got.__setitem__("y", _composed(ops, c, slabs)))
    y, stats, units = got["y"]
    assert sum(n for k, n in cats.items() if _is_pair(k)) == 1, sorted(cats)  # (every grid of the table is eligible: the composed form ran)
    assert units == (D if slabs == 0 else slabs)
    # the chained device form: the init conv, then the 3x3x3 conv on whichever kernel the ladder gives this grid
    h = ops.init_conv(_stack(x, scale, r_w, z_d, phi_h).cuda(), w0.cuda(), b0.cuda())
    yc = ops.cyl_conv(h, w1.cuda(), b1.cuda())
    e_new, e_old = rel_l2(y.cpu().double().numpy(), want.numpy()), rel_l2(yc.cpu().double().numpy(), want.numpy())
    print(f"{dims} B={B} slabs={units}: composed vs float64 rel L2 {e_new:.3e} | chained vs float64 rel L2 {e_old:.3e}")
    assert torch.isfinite(y).all() and e_new <= TOL_REASSOC
    # channel partials of what was stored: the sum relative to sum |y|, the squares relative to themselves
    ref = y.double().reshape(B, -1, 32)
    scale_s = torch.stack([ref.abs().sum(1), (ref * ref).sum(1)], -1)
    want_s = torch.stack([ref.sum(1), (ref * ref).sum(1)], -1)
    err = float(((stats - want_s).abs() / scale_s).max())
    print(f"{dims} B={B}: channel statistics, max error against fp64 sums {err:.2e} of the summed terms")
    assert err <= TOL_STATS


def test_every_boundary_class_per_voxel():
    """5 x 16 x 9: max |composed - float64| per boundary class (z first / interior / last x r first / interior / last), relative to
    max |float64|.  A wrong weight set is an O(1) error on its class alone."""
    from calodiffusion_amd.engine import Ops
    dims, B = (5, 16, 9), 3
    c, want = _shared(dims, B)
    y, _, _ = _composed(Ops(), c)
    err = (y.cpu().double() - want).abs().amax(dim=(0, 2, 4))  # [D][W]
    top = float(want.abs().max())
    D, _, W = dims
    cls = lambda i, n: 0 if i == 0 else (2 if i == n - 1 else 1)
    worst = {}
    for z in range(D):
        for w in range(W):
            k = (cls(z, D), cls(w, W))
            worst[k] = max(worst.get(k, 0.0), float(err[z, w]) / top)
    for k in sorted(worst):
        print(f"class z={k[0]} r={k[1]}: max |composed - float64| = {worst[k]:.3e} of max |float64|")
    assert len(worst) == 9 and max(worst.values()) <= TOL_REASSOC


def test_guard_bands_around_output_and_partials():
    from calodiffusion_amd.engine import Ops
    dims, B, G, S = (5, 16, 9), 3, 1024, -777.25
    D, H, W = dims
    c, want = _shared(dims, B)
    n_y, n_p = B * D * H * W * 32, B * D * 64
    big_y = torch.full((G + n_y + G,), S, device="cuda")
    big_p = torch.full((G + n_p + G,), S, device="cuda")
    y, stats, units = _composed(Ops(), c, 2, y=big_y[G:G + n_y].view(B, D, H, W, 32), part=big_p[G:G + n_p])
    torch.cuda.synchronize()
    assert units == 2 and rel_l2(y.cpu().double().numpy(), want.numpy()) <= TOL_REASSOC
    for big, n in ((big_y, n_y), (big_p, n_p)):
        assert bool((big[:G] == S).all()) and bool((big[G + n:] == S).all())
    assert bool((big_p[G + B * units * 64:G + n_p] == S).all())  # (packed [B][units][32][2] at the front, nothing beyond)
    assert bool((big_p[G:G + B * units * 64] != S).all())


# ---------------------------------------------------------------------------------------------------- denoise level
BMAX = 66


def _batch(cfg, n, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn([n] + list(cfg["SHAPE_PAD"][1:]), generator=gen)
    E = torch.rand((n, 3 if cfg.get("HGCAL") else 1), generator=gen)
    layers = torch.randn((n, 1 + cfg["SHAPE_FINAL"][2]), generator=gen)
    sigma = torch.tensor([_SIGMAS[i % len(_SIGMAS)] for i in range(n)], dtype=torch.float32)
    return x, E, layers, sigma


def _fixture(name, n):
    """One model, one seeded batch of n samples (smaller batches are prefixes) and the CPU oracle's denoise of the first three."""
    m, cfg = seeded_model_cfg(name)
    x, E, layers, sigma = _batch(cfg, n, 29)
    om = O.OracleModel(cfg, {k: v.detach().cpu() for k, v in m.state_dict().items()})
    with torch.no_grad():
        want3 = om.denoise(x[:3], E[:3], sigma[:3], layers[:3]).numpy()
    return m, cfg, (x.cuda(), E.cuda(), layers.cuda(), sigma.cuda()), want3


@pytest.fixture(scope="module")
def ds2():
    return _fixture("dataset2", BMAX)


@pytest.fixture(scope="module")
def tiny():
    return _fixture("tiny", 3)


def _z_convs(cats, cfg):
    d, h, w = cfg["SHAPE_PAD"][2:]
    return cats.get(f"conv3x3x3_s1 C32->32 @{d}x{h}x{w}", 0)


@pytest.mark.parametrize("name,B", [("tiny", 3), ("dataset2", 1), ("dataset2", 3), ("dataset2", 66)])
def test_denoise_new_sequence_against_chained_and_oracle(request, monkeypatch, name, B):
    m, cfg, (x, E, layers, sigma), want3 = request.getfixturevalue("ds2" if name == "dataset2" else "tiny")
    eng = m.engine()
    monkeypatch.setattr(eng, "safe_denoise", False)
    run = lambda: m.denoise(x[:B], E=E[:B], sigma=sigma[:B], layers=layers[:B])
    new = run()
    cats = _launches(run)
    monkeypatch.setenv(SWITCH, "1")
    old = run()
    cats_old = _launches(run)
    monkeypatch.delenv(SWITCH)
    eng.check_status()
    # one composed launch, one full-resolution 32 -> 32 conv fewer; the chained sequence has none
    assert sum(n for c, n in cats.items() if _is_pair(c)) == 1 and not any(_is_pair(c) for c in cats_old), (sorted(cats), sorted(cats_old))
    assert _z_convs(cats_old, cfg) - _z_convs(cats, cfg) == 1, (cats, cats_old)
    assert sum(cats_old.values()) == sum(cats.values())
    err = float((new - old).norm() / old.norm())
    worst = max(float((new[i] - old[i]).norm() / old[i].norm()) for i in range(B))
    print(f"{name} B={B}: composed vs chained sequence rel L2 {err:.3e} (worst sample {worst:.3e})")
    assert torch.isfinite(new).all() and err < TOL_REASSOC and worst < TOL_REASSOC
    assert torch.equal(run(), new)  # deterministic
    if B <= 3:
        e_o = rel_l2(new.cpu().numpy(), want3[:B])
        print(f"{name} B={B}: composed sequence vs oracle rel L2 {e_o:.3e}")
        assert e_o < TOL_ORACLE


def test_graph_replay_equals_eager_bitwise(ds2):
    from calodiffusion_amd import sample
    m, cfg, (x, E, layers, sigma), _ = ds2
    B = 2
    outs = {}
    for use_graph in (True, False):
        c = dict(cfg)
        c["SAMPLER_OPTIONS"] = dict(cfg.get("SAMPLER_OPTIONS", {}), HIP_GRAPH=use_graph)
        m.sampler_algorithm = sample.DDim(c)
        outs[use_graph] = m.sample(E[:B], layers[:B], num_steps=4, start=x[:B])
    cats = _launches(lambda: m.sample(E[:B], layers[:B], num_steps=4, start=x[:B]))  # (eager: the new sequence is what ran)
    assert sum(n for k, n in cats.items() if _is_pair(k)) == 4, sorted(cats)
    assert np.isfinite(outs[True]).all() and np.array_equal(outs[True], outs[False])


def test_parameter_upload_refreshes_the_composed_data(ds2, monkeypatch):
    """A new conv1 weight of downs[0]'s first block and a new init conv bias reach the composed weights and table with the upload:
    the composed sequence still agrees with the chained one, on the same plan."""
    m, cfg, (x, E, layers, sigma), _ = ds2
    B = 2
    eng = m.engine()
    monkeypatch.setattr(eng, "safe_denoise", False)
    run = lambda: m.denoise(x[:B], E=E[:B], sigma=sigma[:B], layers=layers[:B])
    before = run()
    plan = eng.plan
    w, b = m.model.downs[0][0].block1.proj.conv.weight, m.model.init_conv.conv.bias
    keep_w, keep_b = w.detach().clone(), b.detach().clone()
    gen = torch.Generator().manual_seed(17)
    try:
        with torch.no_grad():
            w.add_((torch.randn(w.shape, generator=gen) * 0.02).to(w.device))
            b.add_((torch.randn(b.shape, generator=gen) * 0.5).to(b.device))
        new = run()
        cats = _launches(run)
        monkeypatch.setenv(SWITCH, "1")
        old = run()
        monkeypatch.delenv(SWITCH)
        assert eng.plan is plan  # (no rebuild)
        assert sum(n for c, n in cats.items() if _is_pair(c)) == 1
        err, moved = float((new - old).norm() / old.norm()), float((new - before).norm() / before.norm())
        print(f"after the upload: composed vs chained rel L2 {err:.3e}; the output moved by {moved:.3e}")
        assert moved > 1e-4 and err < TOL_REASSOC
    finally:
        with torch.no_grad():
            w.copy_(keep_w)
            b.copy_(keep_b)
        run()
        eng.check_status()
