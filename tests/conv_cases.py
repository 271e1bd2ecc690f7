"""Convolution cases shared by the conv parity tests and the child interpreters they start (one per latched CD_CONV_PRECISION):
a random 3x3x3 conv, optionally over a concatenated input, against the CPU oracle, as one relative-L2 figure."""
import torch

from conftest import gold, rel_l2
from helpers import back, cl, t


def conv_case(ops, gen, B, c0, c1, cout, shape, nb=3):
    from oracle import torch_oracle as O
    cin = c0 + c1
    x = torch.randn((B, cin) + shape, generator=gen)
    w, bias = torch.randn((cout, cin, 3, 3, 3), generator=gen) * 0.05, torch.randn(cout, generator=gen)
    nb = B if nb is None else min(B, nb)
    want = O.cyl_conv3d(x[:nb], w, bias, padding=(1, 1, 1)).numpy()
    if c1:
        y = ops.cyl_conv(cl(ops, x[:, :c0].contiguous().numpy()), w.cuda(), bias.cuda(), x1_cl=cl(ops, x[:, c0:].contiguous().numpy()))
    else:
        y = ops.cyl_conv(cl(ops, x.numpy()), w.cuda(), bias.cuda())
    return rel_l2(back(ops, y)[:nb], want)


def halo_tiled_errors():
    """(child process of test_halo_tiled_kernels_in_every_precision) 3x3x3 convs, one of them over a concatenated input, and a
    golden down-sampling conv."""
    from calodiffusion_amd.engine import Ops
    ops = Ops()
    gen = torch.Generator().manual_seed(17)
    errs = {"c32": conv_case(ops, gen, 2, 32, 0, 32, (9, 16, 9)), "c32+32": conv_case(ops, gen, 2, 32, 32, 64, (6, 4, 2))}
    g = gold("primitives_conv")
    y = back(ops, ops.cyl_conv(cl(ops, g["down_d2.x"]), t(g["down_d2.w"]).cuda(), t(g["down_d2.b"]).cuda(),
                               stride=(2 if int(g["down_d2.cz"]) else 1, 2, 2)))
    errs["down_d2"] = rel_l2(y, g["down_d2.y"])
    return errs
