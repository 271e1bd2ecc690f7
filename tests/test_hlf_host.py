"""CPU: the host side of the shower observables -- XMLHandler's eta / phi tables, the NumPy restatement the device test leans on
against the reference's own HighLevelFeatures (fixture: tools/gen_golden_hlf.py), the HighLevelFeatures class around a stand-in
for its one device call, and the refusals of cd_hlf_create / cd_hlf_compute, which come before anything touches a device.
(`pytest -s` prints the share of each bound of hlf_cases.assert_within_reference_bounds the restatement uses.)"""
import ctypes as C

import numpy as np
import pytest

import hlf_cases as H
from calodiffusion_amd import engine
from calodiffusion_amd.hlf import HighLevelFeatures
from calodiffusion_amd.xml_handler import XMLHandler


@pytest.mark.parametrize("tag", list(H.TAGS))
def test_xml_handler_eta_phi_equal_the_reference_tables(tag):
    f = H.fixture(tag)
    xml = XMLHandler(H.TAGS[tag][1], filename=H.binning(tag))
    eta, phi = xml.GetEtaPhiAllLayers()
    assert eta is xml.eta_all_layers and phi is xml.phi_all_layers
    assert len(eta) == len(phi) == len(xml.r_bins)
    assert [len(e) for e in eta] == [len(p) for p in phi] == list(np.diff(f["bin_edges"]))
    assert all(e.dtype == np.float64 and p.dtype == np.float64 for e, p in zip(eta, phi))
    assert np.array_equal(np.concatenate(eta), f["eta"]) and np.array_equal(np.concatenate(phi), f["phi"])


def test_index_and_id_quirk_of_the_pion_file():
    """ids 12-14 sit at indices 5-7: index 6 (id 13, ten alpha bins) has no centres, as in the reference."""
    hlf = HighLevelFeatures("pion", filename=H.binning("pion"))
    assert hlf.relevantLayers == [0, 1, 2, 3, 5, 6, 7] and hlf.layersBinnedInAlpha == [1, 2, 3, 13]
    assert hlf.layers_with_centres == [1, 2, 3] == list(H.fixture("pion")["centre_layers"])


@pytest.mark.parametrize("tag", list(H.TAGS))
def test_restatement_agrees_with_the_reference(tag):
    f, geo = H.fixture(tag), H.Geometry.of_fixture(tag)
    rec, hits = H.restate(f["showers"], geo)
    worst = H.assert_within_reference_bounds(rec, H.total_energy(rec), tag)
    print(tag, "worst share of the bound:", {k: round(v, 3) for k, v in worst.items()})
    assert not rec[0].any() and not hits[0].any()  # the empty shower
    one = [geo.relevant.index(l) for l in geo.centres]  # shower 1: one voxel per alpha-binned layer with centres
    assert np.all(hits[1, one] == 1) and np.array_equal(rec[1, one, H.E], rec[1, one, H.MAX])


class _HostHLF(HighLevelFeatures):
    """The class with the restatement in place of its device call."""

    def _records(self, data, N, threshold, chunk):
        geo = H.Geometry(self.bin_edges, np.concatenate(self.eta_all_layers), np.concatenate(self.phi_all_layers),
                         self.relevantLayers, self.layers_with_centres)
        return H.restate(np.asarray(data), geo, threshold)


@pytest.mark.parametrize("tag", list(H.TAGS))
def test_class_attributes_keys_and_dtypes(tag):
    f = H.fixture(tag)
    hlf = _HostHLF(H.TAGS[tag][1], filename=H.binning(tag))
    assert list(hlf.bin_edges) == list(f["bin_edges"]) and hlf.relevantLayers == list(f["relevantLayers"])
    assert hlf.layersBinnedInAlpha == list(f["layersBinnedInAlpha"])
    assert hlf.num_alpha == list(f["num_alpha"]) and hlf.num_voxel == list(f["num_voxel"])
    assert [len(r) for r in hlf.r_edges] == list(f["r_edges_n"]) and np.array_equal(np.concatenate(hlf.r_edges), f["r_edges"])
    assert np.array_equal(np.concatenate(hlf.eta_all_layers), f["eta"]) and np.array_equal(np.concatenate(hlf.phi_all_layers), f["phi"])
    assert hlf.GetEtot() is None and hlf.GetElayers() == {}
    hlf.CalculateFeatures(f["showers"], threshold=1.0)
    assert hlf.GetEtot().dtype == np.float32 and hlf.GetEtot().shape == (8,)
    assert list(hlf.GetElayers()) == list(f["relevantLayers"]) == list(hlf.n_hits) == list(hlf.max_voxel)
    for d in (hlf.GetECEtas(), hlf.GetECPhis(), hlf.GetWidthEtas(), hlf.GetWidthPhis(), hlf.var_etas, hlf.var_phis):
        assert list(d) == list(f["centre_layers"])
        assert all(v.dtype == np.float64 and v.shape == (8,) for v in d.values())
    assert all(v.dtype == np.float32 for v in hlf.E_layers.values()) and all(v.dtype == np.float32 for v in hlf.max_voxel.values())
    assert all(v.dtype == np.int32 for v in hlf.n_hits.values())
    for l in hlf.relevantLayers:
        lo, hi = hlf.bin_edges[l], hlf.bin_edges[l + 1]
        assert np.array_equal(hlf.n_hits[l], (f["showers"][:, lo:hi] > 1.0).sum(-1))
        assert np.array_equal(hlf.max_voxel[l], f["showers"][:, lo:hi].max(-1))
    # E_tot: the layer energies in layer order, in float64, rounded once
    rec, _ = H.restate(f["showers"], H.Geometry.of_fixture(tag))
    assert np.array_equal(hlf.E_tot, H.total_energy(rec).astype(np.float32))
    # a second call replaces every entry
    hlf.CalculateFeatures(f["showers"][:3])
    assert hlf.E_tot.shape == (3,) and all(v.shape == (3,) for v in hlf.EC_etas.values())


@pytest.mark.parametrize("tag", ["small", "pion"])
def test_feature_matrix_columns(tag):
    """FDP.pre_process (train/evaluate.py:26-47) written out over the reference's own values; the pion file is where its loop over
    layersBinnedInAlpha would raise KeyError (id 13)."""
    f = H.fixture(tag)
    hlf = _HostHLF(H.TAGS[tag][1], filename=H.binning(tag))
    with pytest.raises(RuntimeError, match="CalculateFeatures first"):
        hlf.feature_matrix(f["energies"])
    hlf.CalculateFeatures(f["showers"])
    got = hlf.feature_matrix(f["energies"])
    R, K = len(f["relevantLayers"]), len(f["centre_layers"])
    assert got.shape == (8, 1 + R + 4 * K)
    want = np.concatenate([np.log10(f["energies"]), np.log10(f["E_layers"] + 1e-8), f["EC_etas"] / 1e2, f["EC_phis"] / 1e2,
                           f["width_etas"] / 1e2, f["width_phis"] / 1e2], axis=1)
    assert np.array_equal(got[:, 0], want[:, 0])
    # the bounds of hlf_cases carried through the formula, delta at the largest layer.  Layer energies agree to rtol delta and
    # d log10(E) = dE / (E ln 10) < delta; an empty layer is log10(1e-8) in both
    delta = H._delta(int(np.diff(f["bin_edges"]).max()))
    cmax = max(np.abs(f["eta"]).max(), np.abs(f["phi"]).max())
    np.testing.assert_allclose(got[:, 1:1 + R], want[:, 1:1 + R], rtol=0, atol=delta)
    np.testing.assert_allclose(got[:, 1 + R:1 + R + 2 * K], want[:, 1 + R:1 + R + 2 * K], rtol=0, atol=2 * delta * cmax / 1e2)
    # widths: |sqrt a - sqrt b| <= sqrt |a - b| for variances that agree to 4 delta cmax^2
    np.testing.assert_allclose(got[:, 1 + R + 2 * K:], want[:, 1 + R + 2 * K:], rtol=0, atol=np.sqrt(4 * delta) * cmax / 1e2)
    with pytest.raises(ValueError, match="7 energies for 8 showers"):
        hlf.feature_matrix(f["energies"][:7])


def test_wrong_voxel_count_and_plots_are_refused_by_name():
    hlf = HighLevelFeatures("photon", filename=H.binning("photon"))
    called = []
    hlf._records = lambda *a: called.append(a)  # any launch would go through here
    for bad in (np.zeros((4, 367), np.float32), np.zeros((368,), np.float32), np.zeros((2, 1, 368), np.float32)):
        with pytest.raises(ValueError, match=r"expected showers of shape \(N, 368\)"):
            hlf.CalculateFeatures(bad)
    with pytest.raises(ValueError, match="chunk must be positive"):
        hlf.CalculateFeatures(np.zeros((4, 368), np.float32), chunk=0)
    assert not called
    for name in ("DrawAverageShower", "DrawSingleShower", "DrawHistoEtot", "DrawHistoElayers", "DrawHistoECEtas", "DrawHistoECPhis",
                 "DrawHistoWidthEtas", "DrawHistoWidthPhis"):
        with pytest.raises(NotImplementedError, match="plotting is out of scope"):
            getattr(hlf, name)(np.zeros((1, 368), np.float32))


def test_alias_package_exports_the_class():
    from calodiffusion.utils.HighLevelFeatures import HighLevelFeatures as Alias
    assert Alias is HighLevelFeatures


def test_descriptor_matches_the_header_and_the_stub():
    """CdHlfDesc holds pointers, which test_abi's struct parser does not read: compare its three descriptions here."""
    import os
    import re
    from conftest import ROOT
    txt = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "calodiff.h")).read(), flags=re.S)
    body = re.search(r"struct CdHlfDesc \{(.*?)\};", txt, flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls == ["uint32_t struct_size", "int32_t n_layers", "const int32_t* layer_offset", "const double* eta", "const double* phi",
                     "const int32_t* with_centres"]
    want = [("struct_size", C.c_uint32), ("n_layers", C.c_int32), ("layer_offset", C.POINTER(C.c_int32)),
            ("eta", C.POINTER(C.c_double)), ("phi", C.POINTER(C.c_double)), ("with_centres", C.POINTER(C.c_int32))]
    assert list(engine.CdHlfDesc._fields_) == want and C.sizeof(engine.CdHlfDesc) == 40
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("cd_hlf_create", "cd_hlf_destroy", "cd_hlf_compute"):
        assert name in engine._SIGNATURES and re.search(rf"\b{name}\s*\(", txt) and name in md


def test_descriptor_layout_as_the_c_compiler_sees_it(tmp_path):
    """test_abi's _Static_assert for the descriptors it parses, for this one: size and every field offset of the ctypes struct."""
    import os
    import subprocess
    from conftest import ROOT
    lines = ['#include <stddef.h>', '#include "calodiff.h"',
             f'_Static_assert(sizeof(CdHlfDesc) == {C.sizeof(engine.CdHlfDesc)}, "CdHlfDesc");']
    lines += [f'_Static_assert(offsetof(CdHlfDesc, {name}) == {getattr(engine.CdHlfDesc, name).offset}, "{name}");'
              for name, _ in engine.CdHlfDesc._fields_]
    src = tmp_path / "hlf_abi.c"
    src.write_text("\n".join(lines + ["int main(void) { return 0; }", ""]))
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "hlf_abi.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _desc(n_layers, offsets, eta, phi, centres, struct_size=None):
    keep = [(C.c_int32 * len(offsets))(*offsets) if offsets is not None else None,
            (C.c_double * max(len(eta), 1))(*eta) if eta is not None else None,
            (C.c_double * max(len(phi), 1))(*phi) if phi is not None else None,
            (C.c_int32 * len(centres))(*centres) if centres is not None else None]
    d = engine.CdHlfDesc(C.sizeof(engine.CdHlfDesc) if struct_size is None else struct_size, n_layers, *keep)
    return d, keep


@pytest.mark.parametrize("kwargs, message", [
    (dict(offsets=[1, 3, 5]), "layer_offset[0] must be 0"),
    (dict(offsets=[0, 3, 2]), "layer_offset must not decrease (layer 1)"),
    (dict(offsets=[0, 0, 0]), "V == 0"),
    (dict(offsets=None), "layer_offset table is null"),
    (dict(eta=None), "eta table is null"),
    (dict(phi=None), "phi table is null"),
    (dict(centres=None), "with_centres table is null"),
    (dict(struct_size=24), "struct_size is 24"),
    (dict(n_layers=0), "n_layers must be positive"),
])
def test_create_refusals_name_their_cause(kwargs, message):
    lib = engine.load_library()
    args = dict(n_layers=2, offsets=[0, 2, 5], eta=[0.0] * 5, phi=[0.0] * 5, centres=[1, 1])
    args.update(kwargs)
    d, keep = _desc(**args)
    handle = C.c_void_p()
    assert lib.cd_hlf_create(C.byref(d), C.byref(handle), None) == -1
    assert message in lib.cd_last_error().decode() and "cd_hlf_create" in lib.cd_last_error().decode()
    assert not handle.value
    del keep


def test_null_arguments_are_refused():
    lib = engine.load_library()
    assert lib.cd_hlf_compute(None, None, 4, 0.0, None, None, None) == -1
    assert b"cd_hlf_compute: hlf, showers, out and n_hits must not be null" in lib.cd_last_error()
    assert lib.cd_hlf_create(None, None, None) == -1 and b"desc and out must not be null" in lib.cd_last_error()
    assert lib.cd_hlf_destroy(None) == 0
