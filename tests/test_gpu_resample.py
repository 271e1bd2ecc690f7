"""GPU (MI355X): the strided (3,4,4) down-sampling conv and the phi-periodic transposed conv at tile seams, flat-range unit
boundaries, 96 and 128 channels and in every arithmetic, forward and backward, against the fp64 oracle on the CPU.

The shapes are those of resample_cases.py; test_resample_host.py asserts, from the launchers' arithmetic, that each one has the
seam, the kernel or the rung it is here for.  Every sample is compared on its own (relative L2 per sample), forward results
against TOL_OP, gradients against the TOL of test_gpu_backward.py; a failure names the case, the sample and the (z, phi, r, channel)
of the largest error.  The test cannot see which kernel or tile ran: with the timer on (the default) all candidates are launched
and the fastest one's output is compared, CD_NO_AUTOTUNE takes the first-ranked one, CD_FLAT_TILE forces a flat tiling."""
import json
import os
import subprocess
import sys

import pytest

import resample_cases as R
from helpers import ops  # noqa: F401  (a fixture)
from resample_runs import run_conv_backward, run_convt_backward, run_convt_forward, run_flat_forced, run_strided_forward

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PREC = os.environ.get("CD_CONV_PRECISION", "f16x2")
PREC = PREC if PREC in R.PRECISIONS else "f16x2"


def _assert(res, arithmetic=PREC):
    for label, (err, where, tol) in res.items():
        kind = "rel L2" if label.endswith((".dw", ".db")) else "worst per-sample rel L2"
        print("%s [%s]: %s %.3e (tolerance %.0e)" % (label, arithmetic, kind, err, tol))
    for label, (err, where, tol) in res.items():
        assert err < tol, "%s [%s]: %.3e >= %.0e; %s" % (label, arithmetic, err, tol, where)


# ---- forward -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in R.CONVT_CASES])
def test_transposed_conv_forward_at_tile_seams(ops, name):
    """No (TZ, TH) tile holds the grid (a tile may still span one axis, except in the two cases where none that fits does): z halos,
    phi wraps at a seam, ragged last tiles, all stride-parity classes with output padding in phi and r, CT = 1..4; and a batch of
    40 with more workgroups than CUs, each sample compared."""
    _assert(run_convt_forward(ops, name))


@pytest.mark.parametrize("autotune", [True, False], ids=["timer", "first_ranked"])
@pytest.mark.parametrize("name", [c.name for c in R.TILED_CASES])
def test_strided_conv_forward_on_the_halo_tiled_kernels(ops, name, autotune, monkeypatch):
    """Grids the flat kernel declines and no halo tile covers (5 x 22 x 18; 7 x 50 x 18, Dataset-3's level-0 width, where every tile
    wraps phi at a seam), 32..128 channels in and out.  The timed run and the first-ranked run use different batches: the tuner's
    cache, keyed by batch, cannot answer for the run without the timer."""
    c = R.by_name(R.TILED_CASES, name)
    if not autotune:
        monkeypatch.setenv("CD_NO_AUTOTUNE", "1")
    _assert(run_strided_forward(ops, name, nsamples=c.batch if autotune else c.batch + 1))


def _flat_params():
    out = [(c.name, None) for c in R.FLAT_CASES]
    for c in R.FLAT_CASES:
        out += [(c.name, t) for t in c.tilings.get(PREC, ())]
    return out


@pytest.mark.parametrize("name,tiling", _flat_params(), ids=["%s-%s" % (n, "unforced" if t is None else "%dx%d" % t) for n, t in _flat_params()])
def test_strided_conv_forward_on_the_flat_kernels(ops, name, tiling):
    """Flat-range units from one row tile to the whole sample, forced by CD_FLAT_TILE, and the launcher's own choice."""
    _assert(run_strided_forward(ops, name) if tiling is None else run_flat_forced(ops, name, *tiling))


# ---- backward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in R.CONV_BWD_CASES])
def test_strided_conv_backward_at_seams_and_on_every_weight_gradient_rung(ops, name):
    """dx on the transposed kernel with dy rescaled by a power of two from its maximum (|dy| ~ 1, 3e-7 and 2e4 at one seam shape), both z
    strides; dw on the strided fp16 kernel's rungs of 4, 2 and 1 coarse planes, and on the generic kernel where it declines."""
    _assert(run_conv_backward(ops, name))


@pytest.mark.parametrize("name", [c.name for c in R.CONVT_BWD_CASES])
def test_transposed_conv_backward_at_seams(ops, name):
    """dx: the strided conv of dy on the halo-tiled kernels (kz = 3 with every output padding -- an odd phi extent is folded first --
    and kz = 4) and on the flat kernels (geometries 2 and 3); dw: the strided weight gradient with the roles swapped, kd = 4 included."""
    _assert(run_convt_backward(ops, name))


# ---- every arithmetic ----------------------------------------------------------------------------------------------------
def child_labels(mode):
    labels = list(R.CHILD_FWD_T)
    for name in R.CHILD_FWD_S:
        labels.append(name)
        if name in [c.name for c in R.FLAT_CASES]:
            labels += ["%s@%d,%d" % ((name,) + t) for t in R.by_name(R.FLAT_CASES, name).tilings.get(mode, ())]
    for name in R.CHILD_BWD + R.CHILD_BWD_T:
        labels += [name + ".dx", name + ".dw", name + ".db"]
    return labels


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
def test_resampling_convs_in_the_other_arithmetics(mode):
    """CD_CONV_PRECISION is latched per process: one child interpreter per arithmetic runs the seam cases.  bf16x3: the transposed
    conv's full-range kernel (conv_transpose_kernel, taken whenever the arithmetic is not f16x2), the three-term flat and halo-tiled
    kernels; f32: the f32 halo-tiled kernel for every strided conv."""
    env = dict(os.environ, CD_CONV_PRECISION=mode)
    env.pop("CD_FLAT_TILE", None)
    env.pop("CD_NO_AUTOTUNE", None)
    code = ("import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r);"
            "from resample_runs import child_errors; print(json.dumps(child_errors(%r)))" % (os.path.dirname(HERE), HERE, mode))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert sorted(res) == sorted(child_labels(mode))
    _assert({k: tuple(v) for k, v in res.items()}, mode)
