"""What the host and GPU tests of the resampling convs share: the case tables, Python mirrors of the launchers' eligibility and
candidate arithmetic (each names its source), the fp64 references and the per-sample comparison.

The strided (3,4,4) down-sampling conv and the phi-periodic transposed conv pick their kernel and its tile from LDS byte counts.
A test shape checks a tile seam, a flat-range unit boundary or a weight-gradient rung only while that arithmetic puts it there:
test_resample_host.py asserts, on the mirrors below, the property every case exists for, test_gpu_resample.py runs the cases.

Grids are (z, phi, r); phi is periodic.  The arithmetics are CD_CONV_PRECISION's f16x2 (default), bf16x3 and f32."""
import functools
from collections import namedtuple

import numpy as np
import torch

KIB = 1024
PRECISIONS = ("f16x2", "bf16x3", "f32")
# bytes per staged voxel and 16-channel sub-chunk of the flat-range kernels (kernels_conv_flat.hip:548; f32 has no strided flat kernel)
FLAT_VOX_BYTES = {"f16x2": 80, "bf16x3": 96}
# ... and per voxel and 32-channel chunk of the halo-tiled kernels (kernels_conv.hip:257)
TILED_VOX_BYTES = {"f16x2": 80, "bf16x3": 96, "f32": 144}


# ------------------------------------------------------------------------------------------------------------
# grids
# ------------------------------------------------------------------------------------------------------------
def conv_out(din, k, stride):
    """output grid of the strided conv, padding 1 everywhere, circular in phi (ops.hip:84)"""
    return tuple((d + 2 - kk) // s + 1 for d, kk, s in zip(din, k, stride))


def convt_out(din, kz, sz, out_pad):
    """output grid of the transposed conv (ops.hip:126)"""
    return ((din[0] - 1) * sz - 2 + kz, 2 * din[1] + out_pad[1], 2 * din[2] + out_pad[2])


# ------------------------------------------------------------------------------------------------------------
# transposed conv: launch_conv_transpose_mfma (kernels_conv_transpose.hip:356-375)
# ------------------------------------------------------------------------------------------------------------
CONVT_LDS_LIMIT = 140 * KIB
CONVT_VOX_PAD = 4   # LDS_VOX_PAD: floats of padding per staged voxel


def convt_class_extents(dout, sz):
    """(Az, Bh): the output grid in parity-class index space, oz = sz a + pz, ophi = 2 b + pphi"""
    return (dout[0] + sz - 1) // sz, (dout[1] + 1) // 2


def convt_tile_lds(tz, th, win, cin):
    return ((tz + 2) * (th + 2) * win + 1) * (cin + CONVT_VOX_PAD) * 4


def convt_all_tiles(cin, din, dout, sz, batch=1):
    """every (TZ, TH, score) the enumeration keeps, in its order: tiles of at most 140 KiB, without those a larger TH (TZ) covers
    in the same number of tiles"""
    az, bh = convt_class_extents(dout, sz)
    out = []
    for tz in range(1, az + 1):
        for th in range(1, bh + 1):
            if convt_tile_lds(tz, th, din[2], cin) > CONVT_LDS_LIMIT:
                break
            if th != bh and (bh + th - 1) // th == (bh + th) // (th + 1):
                continue
            if tz != az and (az + tz - 1) // tz == (az + tz) // (tz + 1):
                continue
            nblocks = batch * ((az + tz - 1) // tz) * ((bh + th - 1) // th)
            ratio = tz * th / ((tz + 2) * (th + 2))
            fill = 1.0 if nblocks >= 512 else nblocks / 512.0
            out.append((tz, th, ratio * fill))
    return out


def convt_candidates(cin, din, dout, sz, batch):
    """the tiles that are timed (the first is the one taken without timing): the eight best by score and a spread of the rest"""
    ranked = sorted(convt_all_tiles(cin, din, dout, sz, batch), key=lambda t: -t[2])  # (sorted() is stable, like std::stable_sort)
    cand = ranked[:8]
    if len(ranked) > 8:
        cand += ranked[8::(len(ranked) - 8) // 6 + 1][:6]
    return [(tz, th) for tz, th, _ in cand]


def convt_has_whole_tile(cin, din, dout, sz):
    az, bh = convt_class_extents(dout, sz)
    return any((tz, th) == (az, bh) for tz, th, _ in convt_all_tiles(cin, din, dout, sz))


def convt_ct(cout):
    """output-channel tiles of 32 per workgroup: the CT template instance (kernels_conv_transpose.hip:391-396)"""
    return cout // 32


ConvT = namedtuple("ConvT", "name c din kz sz out_pad batch")
CONVT_CASES = (
    ConvT("t32_10x8x9", 32, (10, 8, 9), 3, 2, (0, 0, 0), 2),
    ConvT("t32_6x12x9_ds3l1", 32, (6, 12, 9), 3, 2, (0, 1, 1), 2),    # output 11 x 25 x 19: a slice of Dataset-3's level-1 up conv
    ConvT("t64_7x12x4", 64, (7, 12, 4), 3, 2, (0, 1, 1), 2),
    ConvT("t96_5x7x6_nocz", 96, (5, 7, 6), 3, 1, (0, 0, 0), 2),       # COMPRESS_Z off, CT = 3
    ConvT("t128_9x9x9_k4", 128, (9, 9, 9), 4, 2, (0, 0, 1), 2),       # every candidate seamed in z and phi, CT = 4
    ConvT("t32_4x8x5_b40", 32, (4, 8, 5), 3, 2, (0, 0, 1), 40),       # more workgroups than CUs
    ConvT("t128_6x6x5", 128, (6, 6, 5), 3, 2, (0, 1, 0), 2),
    ConvT("t64_8x8x18", 64, (8, 8, 18), 3, 2, (0, 0, 0), 2),          # wide in r: every candidate seamed in z and phi at 64 channels
)
CONVT_NO_WHOLE_TILE = ("t32_10x8x9", "t32_6x12x9_ds3l1", "t64_7x12x4", "t96_5x7x6_nocz", "t128_9x9x9_k4", "t128_6x6x5", "t64_8x8x18")
# no tile that fits spans z, none spans phi: whichever the timer picks has both seams (elsewhere a tile may span one axis)
CONVT_SEAMED_BOTH = ("t128_9x9x9_k4", "t64_8x8x18")
CONVT_CT = {"t96_5x7x6_nocz": 3, "t128_9x9x9_k4": 4, "t128_6x6x5": 4}


# ------------------------------------------------------------------------------------------------------------
# strided conv, flat-range kernels: try_launch_conv3_flat (kernels_conv_flat.hip:534-651)
# ------------------------------------------------------------------------------------------------------------
K344 = (3, 4, 4)
FLAT_CAND = ((8, 2), (4, 1), (8, 1), (12, 3), (16, 2), (16, 4), (4, 2), (6, 2), (6, 3), (2, 1), (3, 1), (1, 1), (2, 2), (12, 2), (8, 4),
             (6, 1), (3, 3))   # kCand, :612
FLAT_WS = ((8, 4), (8, 2), (4, 2), (4, 4), (8, 3), (6, 2), (2, 2), (3, 1), (1, 1), (2, 1))  # kWs (bf16x3 only), :635
FLAT_INSTANCES = {(v, c) for v in (1, 2, 3, 4) for c in (1, 2)} | {(1, 3), (2, 3)}  # launch_conv_flat_split16, kernels_conv_flat16.hip:356


def flat_geo(k, stride):
    """the kernel geometry number (:539-541); None: not a flat-range geometry"""
    if tuple(k) == (3, 3, 3) and tuple(stride) == (1, 1, 1):
        return 0
    if tuple(k) == K344 and tuple(stride[1:]) == (2, 2) and stride[0] in (1, 2):
        return 1 if stride[0] == 2 else 2
    if tuple(k) == (4, 4, 4) and tuple(stride) == (2, 2, 2):
        return 3
    return None


def flat_ct_max(cout):
    """output-channel tiles per workgroup (:545, the same split as launch_conv_mfma's, kernels_conv.hip:234)"""
    ct = cout // 32
    return ct if ct <= 3 else 2


def flat_planes(nt, din, k, stride):
    """planes(NT): plane capacity of the LDS image of a unit of 32 NT output voxels (:549)"""
    dout = conv_out(din, k, stride)
    return ((32 * nt - 1) // (dout[1] * dout[2]) + 1) * stride[0] + k[0]


def flat_lds(nt, din, k, stride, vox_bytes):
    return (flat_planes(nt, din, k, stride) * din[1] * din[2] + 1) * vox_bytes


def flat_candidates(din, k, stride, cout, batch, prec):
    """the (NT, VT, CT) tilings the launcher times for arithmetic `prec`, warp-specialised ones as (NMW, -NLW, CT); [] = declined"""
    if prec not in FLAT_VOX_BYTES or flat_geo(k, stride) is None:
        return []
    vb = FLAT_VOX_BYTES[prec]
    ovox = int(np.prod(conv_out(din, k, stride)))
    ctmax = flat_ct_max(cout)
    if (cout // 32) % ctmax:
        return []
    cand = []
    small = ovox * batch <= 64 * 1024
    for pas in range(2 if small and ctmax > 1 else 1):
        ct = ctmax if pas == 0 else 1
        for nt, vt in FLAT_CAND:
            if vt * ct > 8 or (ct == 3 and vt > 2):
                continue
            if prec == "f16x2" and vt * ct > 4:
                continue
            extra_ok = ovox <= 128 and vt == 1 and nt <= 8
            if 32 * (nt - 1) >= ovox and not extra_ok:
                continue
            if flat_lds(nt, din, k, stride, vb) > 150 * KIB:
                continue
            if pas == 1 and nt > 4:
                continue
            cand.append((nt, vt, ct))
    if prec == "bf16x3":
        for nmw, nlw in FLAT_WS:
            if 32 * (nmw - 1) >= ovox:
                continue
            if 2 * flat_lds(nmw, din, k, stride, 96) + nmw * ctmax * 64 * 4 > 160 * KIB - 256:
                continue
            cand.append((nmw, -nlw, ctmax))
    return cand


def flat_accepts(din, k, stride, cout, batch, prec):
    """whether a conv of process arithmetic `prec` runs on a flat-range kernel: the ladder (kernels_conv.hip:290-293) tries the f16x2
    image, then the bf16x3 image; the f32 image has a flat kernel for geometry 0 only"""
    if prec == "f32":
        return False
    if prec == "f16x2" and flat_candidates(din, k, stride, cout, batch, "f16x2"):
        return True
    return bool(flat_candidates(din, k, stride, cout, batch, "bf16x3"))


def flat_override_valid(nt, vt, din, k, stride, cout, prec):
    """CD_FLAT_TILE=nt,vt is taken (:607-608) and the tiling has a kernel instance (launch_conv_flat_split16): otherwise the launcher
    falls through to its candidates, or to the next rung, without a word"""
    if prec not in FLAT_VOX_BYTES or vt <= 0:
        return False
    ctmax = flat_ct_max(cout)
    ok = nt % vt == 0 and nt // vt <= 8 and vt * ctmax <= 8 and flat_lds(nt, din, k, stride, FLAT_VOX_BYTES[prec]) <= 160 * KIB
    ok = ok and (prec != "f16x2" or vt * ctmax <= 4)
    return ok and (vt, ctmax) in FLAT_INSTANCES


def flat_units(nt, din, k, stride):
    """workgroups per sample: flat ranges of 32 NT output voxels (:596)"""
    ovox = int(np.prod(conv_out(din, k, stride)))
    return (ovox + 32 * nt - 1) // (32 * nt)


# ------------------------------------------------------------------------------------------------------------
# strided conv, halo-tiled kernels: conv_tile_candidates (kernels_conv.hip:173-210)
# ------------------------------------------------------------------------------------------------------------
def tiled_lds(tz, th, din, k, stride, vox_bytes):
    iz, ih = (tz - 1) * stride[0] + k[0], (th - 1) * stride[1] + k[1]
    return (iz * ih * din[2] + 1) * vox_bytes


def tiled_tiles(din, k, stride, vox_bytes):
    """every (TZ, TH) output tile of at most 150 KiB the enumeration visits"""
    dout = conv_out(din, k, stride)
    out = []
    for tz in range(1, min(dout[0], 12) + 1):
        for nth in range(1, dout[1] + 1):
            th = (dout[1] + nth - 1) // nth
            if nth > 1 and (dout[1] + nth - 2) // (nth - 1) == th:
                continue
            if tiled_lds(tz, th, din, k, stride, vox_bytes) <= 150 * KIB:
                out.append((tz, th))
    return out


def tiled_whole_grid_lds(din, k, stride, vox_bytes):
    dout = conv_out(din, k, stride)
    return tiled_lds(dout[0], dout[1], din, k, stride, vox_bytes)


Strided = namedtuple("Strided", "name cin cout din stride batch")
CHANNEL_PAIRS = ((32, 32), (32, 64), (64, 96), (128, 128))
# batch: the autotuned run takes the first `batch` samples, the CD_NO_AUTOTUNE run all batch + 1 (the tuner's cache is keyed by batch)
TILED_CASES = tuple(Strided("s%d_%d_%s" % (ci, co, "x".join(map(str, din))), ci, co, din, (2, 2, 2), 2)
                    for din in ((5, 22, 18), (7, 50, 18)) for ci, co in CHANNEL_PAIRS) + (
    Strided("s32_32_7x50x18_nocz", 32, 32, (7, 50, 18), (1, 2, 2), 2),)   # (at z stride 1 the flat kernel takes 5 x 22 x 18)

# tilings: the CD_FLAT_TILE=nt,vt values forced in each arithmetic.  The override's LDS bound (160 KiB of 80 / 96-byte records) caps
# nt, so the fewest units per sample differ: test_resample_host.py asserts each list reaches the fewest its arithmetic allows.
Flat = namedtuple("Flat", "name cin cout din stride batch tilings")
FLAT_CASES = (
    Flat("f64_96_9x16x9", 64, 96, (9, 16, 9), (2, 2, 2), 3,                              # Dataset-2 level-0 slice, CT = 3
         {"f16x2": ((1, 1), (2, 1), (3, 1), (5, 1)), "bf16x3": ((1, 1), (2, 1), (2, 2), (3, 1), (4, 2))}),
    Flat("f32_64_9x25x9", 32, 64, (9, 25, 9), (2, 2, 2), 2,                              # odd phi, CT = 2
         {"f16x2": ((1, 1), (2, 1), (2, 2), (3, 1), (4, 2)), "bf16x3": ((1, 1), (2, 1), (2, 2), (3, 1), (3, 3))}),
    Flat("f32_32_6x25x9_nocz", 32, 32, (6, 25, 9), (1, 2, 2), 2,                         # z stride 1
         {"f16x2": ((1, 1), (2, 2), (3, 1), (4, 4), (9, 3)), "bf16x3": ((1, 1), (2, 2), (3, 1), (4, 4), (6, 2))}),
)


# ------------------------------------------------------------------------------------------------------------
# strided weight gradient: try_launch_wgrad_strided_f16x2 (kernels_wgrad16.hip:973-1018)
# ------------------------------------------------------------------------------------------------------------
WG_VB = 144   # bytes per fp16 record (kernels_wgrad16.hip:55)


def wgrad_strided_lds(nz, fine, kd, sz):
    """lds_for(nz): nz coarse planes of gradient rows + the fine planes under them (:983-986)"""
    coarse = conv_out(fine, (kd, 4, 4), (sz, 2, 2))
    rp = (nz * coarse[1] * coarse[2] + 15) & ~15
    prow = (fine[1] + 3) * (fine[2] + 2)
    return (rp + 1) * WG_VB + ((nz - 1) * sz + kd) * prow * WG_VB


def wgrad_strided_nz(fine, kd, sz):
    """the rung: coarse planes per unit, 0 = declined (:987-990)"""
    coarse = conv_out(fine, (kd, 4, 4), (sz, 2, 2))
    for nz in (4, 2, 1):
        if nz <= coarse[0] and wgrad_strided_lds(nz, fine, kd, sz) <= 160 * KIB:
            return nz
    return 0


# ------------------------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------------------------
# conv_backward (conv_backward.hip:22-95): an even phi ring sends dx to the transposed kernel with dy as its input (cin = the conv's
# cout, grid = the conv's output), rescaled by a power of two from max |dy|; an odd ring to the naive kernel.  dw: the strided fp16
# kernel on the rung its LDS formula picks, or, declined (the seam grids are too wide for it), the generic 48-tap kernel.
ConvBwd = namedtuple("ConvBwd", "name cin cout din stride batch dy_scale")
CONV_BWD_CASES = (
    ConvBwd("b32_64_5x22x18", 32, 64, (5, 22, 18), (2, 2, 2), 2, 1.0),
    ConvBwd("b32_64_5x22x18_tiny_dy", 32, 64, (5, 22, 18), (2, 2, 2), 2, 3e-7),
    ConvBwd("b32_64_5x22x18_huge_dy", 32, 64, (5, 22, 18), (2, 2, 2), 2, 2e4),
    ConvBwd("b32_32_7x50x18", 32, 32, (7, 50, 18), (2, 2, 2), 2, 1.0),
    ConvBwd("b64_96_5x22x18_nocz", 64, 96, (5, 22, 18), (1, 2, 2), 2, 1.0),
    # the three rungs of the weight gradient (the last on an odd ring: dx from the naive kernel)
    ConvBwd("b32_32_9x8x5_nz4", 32, 32, (9, 8, 5), (2, 2, 2), 2, 1.0),
    ConvBwd("b32_64_9x16x9_nz2", 32, 64, (9, 16, 9), (2, 2, 2), 3, 1.0),
    ConvBwd("b32_32_5x25x9_nz1", 32, 32, (5, 25, 9), (2, 2, 2), 2, 1.0),
)
CONV_BWD_SEAMED = ("b32_64_5x22x18", "b32_64_5x22x18_tiny_dy", "b32_64_5x22x18_huge_dy", "b32_32_7x50x18", "b64_96_5x22x18_nocz")
CONV_BWD_NZ = {"b32_32_9x8x5_nz4": 4, "b32_64_9x16x9_nz2": 2, "b32_32_5x25x9_nz1": 1}

# conv_transpose_backward (conv_backward.hip:98-147): an odd output phi extent is folded onto the even ring first; dx is the strided
# conv of dy (geometry 1 / 2 for kz = 3, 3 for kz = 4) on the flat or the halo-tiled kernels; dw the strided rung with the roles swapped.
ConvTBwd = namedtuple("ConvTBwd", "name c din kz sz out_pad batch")
CONVT_BWD_CASES = tuple(ConvTBwd("u32_6x12x9_op%d%d" % op[1:], 32, (6, 12, 9), 3, 2, op, 2)
                        for op in ((0, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1))) + (
    ConvTBwd("u32_5x12x9_k4", 32, (5, 12, 9), 4, 2, (0, 1, 0), 2),      # dx: geometry 3 has no flat tile -> halo-tiled, 64 taps
    ConvTBwd("u64_5x8x4_k4_flat", 64, (5, 8, 4), 4, 2, (0, 0, 1), 2),   # dx: geometry 3 on the flat kernel, several units
    ConvTBwd("u32_5x8x5_nocz_flat", 32, (5, 8, 5), 3, 1, (0, 0, 0), 3),  # dx: geometry 2 on the flat kernel
)
CONVT_BWD_TILED = tuple(c.name for c in CONVT_BWD_CASES[:5])
CONVT_BWD_FLAT = ("u64_5x8x4_k4_flat", "u32_5x8x5_nocz_flat")
CONVT_BWD_WGRAD_KD4 = "u64_5x8x4_k4_flat"   # dw on the strided fp16 kernel with kd = 4 (the wide grids above decline it)


def convt_bwd_dx_geom(case):
    """(din, k, stride) of the strided conv that computes dx: over the folded output grid"""
    dout = convt_out(case.din, case.kz, case.sz, case.out_pad)
    return (dout[0], dout[1] & ~1, dout[2]), (case.kz, 4, 4), (case.sz, 2, 2)


# what a child interpreter of another arithmetic runs
CHILD_FWD_T = ("t32_6x12x9_ds3l1", "t96_5x7x6_nocz", "t128_9x9x9_k4", "t64_8x8x18")
CHILD_FWD_S = ("s32_32_5x22x18", "s64_96_7x50x18", "s128_128_5x22x18", "f32_64_9x25x9")
CHILD_BWD = ("b32_64_5x22x18", "b32_64_5x22x18_tiny_dy", "b32_32_5x25x9_nz1")
CHILD_BWD_T = ("u32_6x12x9_op11", "u32_5x12x9_k4", "u64_5x8x4_k4_flat")


def by_name(table, name):
    return next(c for c in table if c.name == name)


# ------------------------------------------------------------------------------------------------------------
# references (fp64, CPU) and comparison
# ------------------------------------------------------------------------------------------------------------
def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 31 - 1)


@functools.lru_cache(maxsize=None)
def strided_forward(name):
    """(x, w, b, fp64 y) of a TILED_CASES / FLAT_CASES row, batch + 1 samples"""
    from oracle import torch_oracle as O
    c = by_name(TILED_CASES + FLAT_CASES, name)
    gen = torch.Generator().manual_seed(_seed(name))
    x = torch.randn((c.batch + 1, c.cin) + c.din, generator=gen)
    w, b = torch.randn((c.cout, c.cin) + K344, generator=gen) * 0.05, torch.randn(c.cout, generator=gen)
    with torch.no_grad():
        y = O.cyl_conv3d(x.double(), w.double(), b.double(), stride=c.stride, padding=(1, 1, 1))
    return x, w, b, y.numpy()


@functools.lru_cache(maxsize=None)
def convt_forward(name):
    from oracle import torch_oracle as O
    c = by_name(CONVT_CASES, name)
    gen = torch.Generator().manual_seed(_seed(name))
    x = torch.randn((c.batch, c.c) + c.din, generator=gen)
    w, b = torch.randn((c.c, c.c, c.kz, 4, 4), generator=gen) * 0.05, torch.randn(c.c, generator=gen)
    with torch.no_grad():
        y = O.cyl_conv_transpose3d(x.double(), w.double(), b.double(), (c.sz, 2, 2), c.out_pad)
    return x, w, b, y.numpy()


@functools.lru_cache(maxsize=None)
def conv_backward(name):
    """(x, w, dy, fp64 dx, dw, db) of a CONV_BWD_CASES row"""
    from oracle import torch_oracle as O
    c = by_name(CONV_BWD_CASES, name)
    gen = torch.Generator().manual_seed(_seed(name))
    x = torch.randn((c.batch, c.cin) + c.din, generator=gen)
    w, b = torch.randn((c.cout, c.cin) + K344, generator=gen) * 0.1, torch.randn(c.cout, generator=gen)
    xd, wd, bd = (v.double().requires_grad_() for v in (x, w, b))
    y = O.cyl_conv3d(xd, wd, bd, stride=c.stride, padding=(1, 1, 1))
    dy = torch.randn(y.shape, generator=gen) * c.dy_scale
    y.backward(dy.double())
    return x, w, dy, xd.grad.numpy(), wd.grad.numpy(), bd.grad.numpy()


@functools.lru_cache(maxsize=None)
def convt_backward(name):
    from oracle import torch_oracle as O
    c = by_name(CONVT_BWD_CASES, name)
    gen = torch.Generator().manual_seed(_seed(name))
    x = torch.randn((c.batch, c.c) + c.din, generator=gen)
    w, b = torch.randn((c.c, c.c, c.kz, 4, 4), generator=gen) * 0.1, torch.randn(c.c, generator=gen)
    xd, wd, bd = (v.double().requires_grad_() for v in (x, w, b))
    y = O.cyl_conv_transpose3d(xd, wd, bd, (c.sz, 2, 2), c.out_pad)
    dy = torch.randn(y.shape, generator=gen)
    y.backward(dy.double())
    return x, w, dy, xd.grad.numpy(), wd.grad.numpy(), bd.grad.numpy()


def per_sample_rel_l2(got, want):
    """relative L2 of every sample of (B, C, z, phi, r) arrays, in fp64"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    flat = (got - want).reshape(len(want), -1)
    return np.linalg.norm(flat, axis=1) / np.maximum(np.linalg.norm(want.reshape(len(want), -1), axis=1), 1e-300)


def worst_sample(got, want):
    """(largest per-sample relative L2, a description of where: the sample and the (z, phi, r, channel) of its largest error)"""
    errs = per_sample_rel_l2(got, want)
    errs = np.where(np.isfinite(errs), errs, np.inf)
    i = int(np.argmax(errs))
    d = np.abs(np.asarray(got[i], dtype=np.float64) - want[i])
    d = np.where(np.isfinite(d), d, np.inf)
    ch, z, phi, r = np.unravel_index(int(np.argmax(d)), d.shape)
    return float(errs[i]), "sample %d of %d, largest error at (z, phi, r, channel) = (%d, %d, %d, %d): got %r, want %r" % (
        i, len(errs), z, phi, r, ch, float(got[i][ch, z, phi, r]), float(want[i][ch, z, phi, r]))
