"""CPU: the Dataset-1 geometry converters (calodiffusion_amd/geom1.py) as far as they run on the host -- construction against
the reference's matrices (fixture: tools/gen_golden_ds1_geom.py), the seeded initialisation, state_dict keys, the layout helpers
and the descriptor checks made in Python.  The products are device work: tests/test_gpu_ds1_geom.py."""
import numpy as np
import pytest
import torch

from ds1_geom_cases import TAGS, fixture, geom_converter, nn_converter


@pytest.mark.parametrize("tag", TAGS)
def test_geomconverter_reproduces_the_reference_matrices(tag):
    """weight_mats bit for bit; pinv within 1e-6 of the matrix's largest element (LAPACK's values: a sanity bound, not parity.
    Measured: 0 where the generator ran, 1.5e-7 on a machine with another thread count)."""
    f, gc = fixture(tag), geom_converter(tag)
    assert (gc.dim_r_out, int(gc.alpha_out), gc.num_layers) == (f["R"], f["A"], f["L"])
    assert len(gc.weight_mats) == f["L"] and torch.equal(gc.all_r_areas, gc.all_r_edges[1:] ** 2 - gc.all_r_edges[:-1] ** 2)
    worst = 0.0
    for i, m in enumerate(gc.weight_mats):
        assert np.array_equal(m.numpy(), f[f"weight_mats.{i}"]), i
        ref = f[f"pinv.{i}"]
        gap = float(np.abs(gc.pinv_mats[i].numpy() - ref).max() / np.abs(ref).max())
        worst = max(worst, gap)
        assert gap <= 1e-6, (i, gap)
    print(f"{tag}: pinv worst gap / largest element = {worst:.2e}")


def test_calodiffusion_utils_exports_the_converters():
    from calodiffusion.utils import utils
    from calodiffusion_amd import geom1
    assert utils.GeomConverter is geom1.GeomConverter and utils.NNConverter is geom1.NNConverter


@pytest.mark.parametrize("tag", TAGS)
def test_seeded_initialisation_matches_the_reference(tag):
    """Same values under torch.manual_seed(7): the number and order of RNG draws are the reference's (enc weights bit for bit --
    the same additions on the same draws -- and the dec weights within the pinv bound)."""
    from calodiffusion_amd import geom1
    f, gc = fixture(tag), geom_converter(tag)
    torch.manual_seed(7)
    conv = geom1.NNConverter(geomconverter=gc)
    sd = conv.state_dict()
    assert list(sd) == [f"encs.{i}.weight" for i in range(f["L"])] + [f"decs.{i}.weight" for i in range(f["L"])]
    for k, v in sd.items():
        ref = f["seeded." + k]
        assert v.shape == ref.shape
        if k.startswith("encs"):
            assert np.array_equal(v.numpy(), ref), k
        assert float(np.abs(v.numpy() - ref).max()) <= 1e-6 * float(np.abs(ref).max()), k


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_of_the_reference_loads_strictly(tag):
    f = fixture(tag)
    conv = nn_converter(tag)  # load_state_dict(strict=True) of the fixture's "nn." arrays
    for i in range(f["L"]):
        assert np.array_equal(conv.encs[i].weight.detach().numpy(), f[f"nn.encs.{i}.weight"])
        assert conv.encs[i].bias is None and conv.decs[i].weight.shape == (f["edges"][i].size - 1, f["R"])
    with pytest.raises(RuntimeError):
        conv.load_state_dict({"encs.0.weight": conv.encs[0].weight}, strict=True)


@pytest.mark.parametrize("tag", TAGS)
def test_reshape_and_unreshape_round_trip(tag):
    f, gc = fixture(tag), geom_converter(tag)
    x = torch.rand((4, f["V"]), generator=torch.Generator().manual_seed(3))
    parts = gc.reshape(x)
    assert [tuple(p.shape) for p in parts] == [(4, int(a), e.size - 1) for a, e in zip(f["lay_alphas"], f["edges"])]
    assert torch.equal(gc.unreshape(parts), x)
    # the list form of convert concatenates to exactly what the flat form takes (numpy layers too)
    assert torch.equal(gc.unreshape([p.numpy() for p in parts]), x)
    assert torch.equal(gc.unreshape(gc.reshape(x.numpy())), x)


def _explicit(**over):
    from calodiffusion_amd import geom1
    kw = dict(all_r_edges=torch.tensor([0., 1., 2., 4.]), lay_r_edges=[[0., 2., 4.], [0., 1., 2., 4.]], alpha_out=10,
              lay_alphas=[1, 10], layer_boundaries=[0, 2, 32])
    kw.update(over)
    return geom1.GeomConverter(**kw)


def test_bad_descriptors_raise_naming_the_field():
    assert _explicit().descriptor() == ([0, 2, 32], [1, 10], [2, 3])
    with pytest.raises(ValueError, match=r"lay_alphas\[0\] is 3"):
        _explicit(lay_alphas=[3, 10]).descriptor()
    with pytest.raises(ValueError, match=r"layer_boundaries: layer 1 spans 29"):
        _explicit(layer_boundaries=[0, 2, 31]).descriptor()
    with pytest.raises(ValueError, match=r"layer_boundaries must start at 0 and increase"):
        _explicit(layer_boundaries=[0, 32, 2]).descriptor()
    with pytest.raises(ValueError, match=r"layer_boundaries must hold 3 offsets"):
        _explicit(layer_boundaries=None).descriptor()
    with pytest.raises(ValueError, match=r"lay_r_edges\[1\] has an edge that is not in all_r_edges"):
        _explicit(lay_r_edges=[[0., 2., 4.], [0., 1., 3., 4.]])
    with pytest.raises(ValueError, match="on-chip limits"):
        _explicit(all_r_edges=torch.arange(0., 701.), lay_r_edges=[list(range(701))], lay_alphas=[10], layer_boundaries=[0, 7000]).descriptor()


def test_c_side_refuses_bad_descriptors_without_a_device():
    """cd_radial_create validates before it touches the device: CD_EINVAL and a message, with or without a GPU."""
    import ctypes as C
    from calodiffusion_amd import engine
    lib = engine.load_library()
    i32 = lambda *v: (C.c_int32 * len(v))(*v)  # noqa: E731
    out = C.c_void_p()
    cases = {"strictly increasing": (2, i32(0, 32, 2), i32(1, 10), i32(2, 3), 10, 3),
             "must equal alpha": (2, i32(0, 2, 31), i32(1, 10), i32(2, 3), 10, 3),
             "alpha must be 1 or alpha_out": (2, i32(0, 6, 36), i32(3, 10), i32(2, 3), 10, 3),
             "must be positive": (2, i32(0, 2, 32), i32(1, 10), i32(2, 3), 10, 0),
             "not be null": (2, None, i32(1, 10), i32(2, 3), 10, 3),
             "8192 floats": (1, i32(0, 300), i32(1), i32(300), 1, 30)}
    for needle, (L, bound, alpha, rin, A, R) in cases.items():
        assert lib.cd_radial_create(L, bound, alpha, rin, A, R, C.byref(out), None) == -1, needle
        assert needle in lib.cd_last_error().decode(), (needle, lib.cd_last_error())
        assert not out.value
