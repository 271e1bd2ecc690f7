"""CPU (hipcc cross-compiles): the headers of csrc/ stand on their own and the include graph keeps its shape -- every header
compiles alone, the units that never walk the network do not reach the plan, nothing in csrc/ is orphaned, and build.SOURCES
lists exactly the .hip files."""
import os
import re
import shutil
import subprocess

import pytest

from calodiffusion_amd.build import CSRC, FLAGS, SOURCES

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".h"))

# units that hold kernels and C-ABI entry points but no launch sequence of the network: they take guarded() and their own
# family's declarations, never the plan
STATELESS = ["kernels_preprocess.hip", "kernels_geom.hip", "kernels_geom_embed.hip", "kernels_radial.hip", "adam.hip", "profiler.hip",
             "layer.hip"]
# unit -> why it may reach CdPlan's definition all the same
PLAN_ALLOWED = {}


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(header):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    flags = [f for f in FLAGS if f != "-fPIC"]
    r = subprocess.run([HIPCC, *flags, "-fsyntax-only", "-x", "hip", os.path.join(CSRC, header)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _quoted_includes(name):
    """(included file relative to csrc/, as written) of every #include "..." in a file of csrc/, preprocessor conditions ignored"""
    text = open(os.path.join(CSRC, name)).read()
    return [(os.path.normpath(os.path.join(os.path.dirname(name), inc)), inc)
            for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', text, re.M)]


def _closure(name):
    seen, todo = set(), [name]
    while todo:
        for path, _ in _quoted_includes(todo.pop()):
            if path not in seen and os.path.exists(os.path.join(CSRC, path)):
                seen.add(path)
                todo.append(path)
    return seen


def test_every_quoted_include_resolves():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h", ".inc")):
            for path, inc in _quoted_includes(name):
                assert os.path.isfile(os.path.join(CSRC, path)), f'{name}: #include "{inc}" does not resolve'


def test_stateless_units_do_not_reach_the_plan():
    defining = [h for h in HEADERS if re.search(r"^struct CdPlan\s*\{", open(os.path.join(CSRC, h)).read(), re.M)]
    assert len(defining) == 1, defining
    for unit in STATELESS:
        assert unit in SOURCES
        if unit not in PLAN_ALLOWED:
            assert defining[0] not in _closure(unit), f"{unit} reaches {defining[0]}"


def test_every_header_is_reached_from_a_source():
    reached = set()
    for src in SOURCES:
        reached |= _closure(src)
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".h", ".inc")):
            assert name in reached, f"{name} is included by no unit of build.SOURCES"


def test_sources_are_the_hip_files():
    assert len(SOURCES) == len(set(SOURCES))
    assert sorted(SOURCES) == sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
