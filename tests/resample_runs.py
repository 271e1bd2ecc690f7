"""The device runs of the resampling-conv cases (resample_cases.py), shared by tests/test_gpu_resample.py and the child
interpreters it starts, one per latched CD_CONV_PRECISION.  Each run returns {label: (error, where, tolerance)}."""
import os

import numpy as np

import resample_cases as R
from conftest import rel_l2
from helpers import TOL_BWD, TOL_OP, back


def cl(ops, a):
    return ops.to_channels_last(a.detach().contiguous().cuda())


def _whole(got, want):
    """(relative L2, where) of a tensor that is a sum over the batch (dw, db)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want)
    d = np.where(np.isfinite(got - want), np.abs(got - want), np.inf)
    idx = tuple(int(i) for i in np.unravel_index(int(np.argmax(d)), d.shape))
    err = rel_l2(got, want)
    return (err if np.isfinite(err) else float("inf")), "largest error at index %r: got %r, want %r" % (idx, float(got[idx]), float(want[idx]))


def run_convt_forward(ops, name):
    c = R.by_name(R.CONVT_CASES, name)
    x, w, b, want = R.convt_forward(name)
    y = back(ops, ops.cyl_conv_transpose(cl(ops, x), w.cuda(), b.cuda(), c.kz, c.sz, c.out_pad))
    return {name: R.worst_sample(y, want) + (TOL_OP,)}


def run_strided_forward(ops, name, nsamples=None, label=None):
    c = R.by_name(R.TILED_CASES + R.FLAT_CASES, name)
    x, w, b, want = R.strided_forward(name)
    n = nsamples or c.batch
    y = back(ops, ops.cyl_conv(cl(ops, x[:n]), w.cuda(), b.cuda(), stride=c.stride))
    return {label or name: R.worst_sample(y, want[:n]) + (TOL_OP,)}


def run_flat_forced(ops, name, nt, vt):
    """one forward under CD_FLAT_TILE=nt,vt (read by the launcher on every call); the variable is restored"""
    old = os.environ.get("CD_FLAT_TILE")
    os.environ["CD_FLAT_TILE"] = "%d,%d" % (nt, vt)
    try:
        return run_strided_forward(ops, name, label="%s@%d,%d" % (name, nt, vt))
    finally:
        if old is None:
            del os.environ["CD_FLAT_TILE"]
        else:
            os.environ["CD_FLAT_TILE"] = old


def run_conv_backward(ops, name):
    c = R.by_name(R.CONV_BWD_CASES, name)
    x, w, dy, dx_w, dw_w, db_w = R.conv_backward(name)
    dx, dw, db = ops.conv_backward(cl(ops, x), w.cuda(), cl(ops, dy), stride=c.stride)
    return {name + ".dx": R.worst_sample(back(ops, dx), dx_w) + (TOL_BWD,),
            name + ".dw": _whole(dw.cpu().numpy(), dw_w) + (TOL_BWD,), name + ".db": _whole(db.cpu().numpy(), db_w) + (TOL_BWD,)}


def run_convt_backward(ops, name):
    c = R.by_name(R.CONVT_BWD_CASES, name)
    x, w, dy, dx_w, dw_w, db_w = R.convt_backward(name)
    dx, dw, db = ops.conv_transpose_backward(cl(ops, x), w.cuda(), cl(ops, dy), c.kz, c.sz, c.out_pad)
    return {name + ".dx": R.worst_sample(back(ops, dx), dx_w) + (TOL_BWD,),
            name + ".dw": _whole(dw.cpu().numpy(), dw_w) + (TOL_BWD,), name + ".db": _whole(db.cpu().numpy(), db_w) + (TOL_BWD,)}


def child_errors(mode):
    """(child process of the test below) the seam cases of CHILD_*, forward and backward, in the process's arithmetic"""
    from calodiffusion_amd.engine import Ops
    ops = Ops()
    res = {}
    for name in R.CHILD_FWD_T:
        res.update(run_convt_forward(ops, name))
    for name in R.CHILD_FWD_S:
        res.update(run_strided_forward(ops, name))
        if name in [c.name for c in R.FLAT_CASES]:
            for nt, vt in R.by_name(R.FLAT_CASES, name).tilings.get(mode, ()):
                res.update(run_flat_forced(ops, name, nt, vt))
    for name in R.CHILD_BWD:
        res.update(run_conv_backward(ops, name))
    for name in R.CHILD_BWD_T:
        res.update(run_convt_backward(ops, name))
    return {k: [v[0] if np.isfinite(v[0]) else 1e300, v[1], v[2]] for k, v in res.items()}
