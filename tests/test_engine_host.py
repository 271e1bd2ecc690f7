"""CPU: the split of the binding into calodiffusion_amd/abi.py (the C ABI), ops.py (the primitive-op wrappers) and engine.py
(the engines) -- ``engine.<name>`` still reaches every name other files use, as the same object as in its new home, and the
modules that only call the library import without the engines -- and the rules of what abi.py shares: WorkspaceCache, which
every owner of library workspaces keeps them in, Handle, which every owner of a library handle is or holds, and the refusals
of _upload.  Needs neither the library nor a GPU."""
import subprocess
import sys
import weakref

import numpy as np
import pytest
import torch

from conftest import ROOT
from calodiffusion_amd import abi, engine, ops
from calodiffusion_amd.abi import WorkspaceCache

# the names other files reach as engine.<name>
SURFACE = """load_library, _check, _stream, _ptr, _dev32, _i32x3, require_gpu, profile_begin, profile_end, set_conv_precision,
get_conv_precision, randn, _SIGNATURES, EXPORTED_SYMBOLS, CD_ABI_VERSION, CD_MAX_SIZES, LIB_PATH, TIME_KINDS, OBJECTIVES,
LOSS_TYPES, SOP_LINCOMB, SOP_DENOISE, SOP_RANDN, SOP_RECORD, SOP_LINDIV, SOP_DENOISE_PS, CdUnetDesc, CdSamplerOp, CdLayerMlpDesc,
CdHlfDesc, CdGeneratorRun, CdClassifierDesc, CdStep, _pack_ops, _check_built_from_these_sources, unet_desc, layer_mlp_desc,
UnetEngine, LayerMlpEngine, Ops""".replace("\n", " ").split(", ")
STAYED = {"_pack_ops", "unet_desc", "layer_mlp_desc", "UnetEngine", "LayerMlpEngine"}


def test_engine_still_reaches_every_name_as_the_same_object():
    assert len(SURFACE) == 40 and STAYED < set(SURFACE)
    for name in SURFACE:
        assert hasattr(engine, name), name
        if name in STAYED:
            assert getattr(engine, name).__module__ == "calodiffusion_amd.engine", name
        else:
            home = ops if name == "Ops" else abi
            assert getattr(engine, name) is getattr(home, name), name
    assert engine.WorkspaceCache is WorkspaceCache


@pytest.mark.parametrize("module", ["abi", "ops", "classifier", "evaluate", "geom1", "hgcal", "hlf", "optim", "postprocess", "preprocess",
                                    "shower_stats", "utils"])
def test_abi_and_ops_import_without_the_engines(module):
    code = (f"import sys, calodiffusion_amd.{module}; "
            "sys.exit(int('calodiffusion_amd.engine' in sys.modules))")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr or f"importing calodiffusion_amd.{module} imported calodiffusion_amd.engine"


class _Destroy:
    """Stands in for a cd_*_destroy: records the handles it is given."""

    def __init__(self, fail=False):
        self.seen, self.fail = [], fail

    def __call__(self, handle):
        self.seen.append(handle.value)
        if self.fail:
            raise RuntimeError("the library is gone")


def test_a_handle_is_destroyed_once_and_never_while_null():
    destroy = _Destroy()
    h = abi.Handle(destroy)
    assert not h.handle  # (null until a create call fills it)
    h.close()
    h.__del__()
    assert destroy.seen == []  # (a failed create frees nothing)
    h.handle.value = 0x1234  # what cd_*_create does through C.byref(h.handle)
    h.close()
    assert destroy.seen == [0x1234] and not h.handle
    h.close()  # (twice is harmless)
    h.__del__()
    assert destroy.seen == [0x1234]


def test_a_handle_going_away_frees_it_and_swallows_a_failing_destroy():
    destroy = _Destroy()
    h = abi.Handle(destroy)
    h.handle.value = 7
    del h
    assert destroy.seen == [7]
    failing = _Destroy(fail=True)
    h = abi.Handle(failing)
    h.handle.value = 9
    h.__del__()  # (interpreter teardown: nothing propagates)
    assert failing.seen == [9]
    with pytest.raises(RuntimeError, match="gone"):
        h.handle.value = 11
        h.close()  # (an explicit close still reports)
    assert not h.handle and failing.seen == [9, 11]


def test_owners_of_a_handle_are_handles():
    from calodiffusion_amd import generator, geom1, hgcal
    for owner in (engine.UnetEngine, generator.Generator, geom1._RadialMap, hgcal._PackedMap):
        assert issubclass(owner, abi.Handle) and "__del__" not in vars(owner), owner


def test_upload_refusals_without_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # (what a machine without a GPU answers)
    with pytest.raises(TypeError, match="shower must be a numeric array"):
        abi._upload(np.array([1.0, None], dtype=object), torch.float32, "shower")
    with pytest.raises(RuntimeError, match=r"convert_flat: calodiffusion_amd computes on the GPU only and torch.cuda.is_available\(\) is False"):
        abi._upload(np.ones((2, 3)), torch.float32, "convert_flat", need_gpu=True)
    with pytest.raises(RuntimeError, match="convert_flat"):  # (before the array is looked at, as geom1 always refused)
        abi._upload(np.array([None], dtype=object), torch.float32, "convert_flat", need_gpu=True)


def _sizer(n, calls):
    def size():
        calls.append(n)
        return n
    return size


def test_a_hit_returns_the_kept_tensor_without_sizing():
    c, calls = WorkspaceCache(), []
    a = c.get("net", (2, None), "cpu", _sizer(64, calls))
    assert a.dtype.is_floating_point is False and a.element_size() == 1 and a.numel() == 64 and a.device.type == "cpu"
    assert c.get("net", (2, None), "cpu", _sizer(999, calls)) is a
    assert c.get("net", [2, None], "cpu", _sizer(999, calls)) is a  # (a key is compared as a tuple)
    assert calls == [64]


def test_a_new_key_evicts_its_own_kind_only():
    c, calls = WorkspaceCache(), []
    net = c.get("net", (2,), "cpu", _sizer(16, calls))
    train = c.get("train", (2,), "cpu", _sizer(32, calls))
    net1 = c.get("net", (1,), "cpu", _sizer(8, calls))
    assert net1 is not net and net1.numel() == 8
    assert c.get("train", (2,), "cpu", _sizer(999, calls)) is train
    assert sorted(c) == [("net", 1), ("train", 2)] and len(c) == 2
    assert c.get("net", (2,), "cpu", _sizer(16, calls)).numel() == 16  # (the evicted key is a miss again)
    assert calls == [16, 32, 8, 16]


def test_the_old_tensor_is_gone_before_the_new_one_is_sized():
    c = WorkspaceCache()
    old = weakref.ref(c.get("train", (2,), "cpu", lambda: 1 << 20))
    other = c.get("vjp", (2, True), "cpu", lambda: 16)
    assert old() is not None
    seen = []

    def size():
        seen.append((old() is None, list(c)))
        return 1 << 10

    new = c.get("train", (1,), "cpu", size)
    assert seen == [(True, [("vjp", 2, True)])], seen
    assert new.numel() == 1 << 10 and c.get("vjp", (2, True), "cpu", lambda: 999) is other
    # the at-least form releases first as well
    old = weakref.ref(c.get("sampler", (2,), "cpu", 64))
    assert c.get("sampler", (2,), "cpu", 128).numel() == 128 and old() is None


def test_at_least_reuses_a_larger_buffer_and_replaces_a_smaller_one():
    c = WorkspaceCache()
    a = c.get(0, (), "cpu", 100)
    assert a.numel() == 100
    assert c.get(0, (), "cpu", 40) is a and c.get(0, (), "cpu", 100) is a
    b = c.get(0, (), "cpu", 101)
    assert b is not a and b.numel() == 101
    assert c.get(0, (), "cpu", 0) is b
    assert c.get(0, (7,), "cpu", 8).numel() == 8  # another key: replaced although the kept one was large enough
    assert c.get(1, (), "cpu", 5).numel() == 5 and sorted(c) == [(0, 7), (1,)]


def test_drop_clear_and_iteration():
    c = WorkspaceCache()
    assert list(c) == [] and len(c) == 0
    for kind, key in (("net", (2, None, "1")), ("train", (2, None, "1")), ("vjp", (2, None, "1", True)), ("bns", (2, None, "1", 3))):
        c.get(kind, key, "cpu", lambda: 4)
    assert list(c) == [("net", 2, None, "1"), ("train", 2, None, "1"), ("vjp", 2, None, "1", True), ("bns", 2, None, "1", 3)]
    assert [k[0] for k in c] == ["net", "train", "vjp", "bns"]
    c.drop("train", "vjp", "sampler")  # (a kind that holds nothing is not an error)
    assert [k[0] for k in c] == ["net", "bns"]
    c.clear()
    assert list(c) == [] and len(c) == 0
