// The deepest U-Net level with company: ONE launch whose first `batch` workgroups run the level (deep_body.inc, one workgroup per
// sample, as kernels_deep.hip launches it alone) and whose remaining workgroups run a K-block of a full-resolution z-slide
// convolution (conv_zs_body.inc) that needs nothing from the level.
//
// Why: the level gives one workgroup to each sample -- at the headline batch of 64 it holds 64 of the chip's 256 CUs for ~0.2 ms
// and cannot be spread further.  The first conv of level 0's first up-block reads cat(x, skip0): its skip half
// depends only on skips[0], which is final before the level-0 -> 1 strided conv runs, so that K-block (half the conv's arithmetic)
// can run on the CUs the level leaves idle instead of after it.  It runs FIRST of the conv's two K-blocks here and therefore carries
// the bias; the x half follows the transposed conv as a continuation launch (ConvFusion::add_src) and carries the statistics.
//
// Form: the level's workgroups have the lowest indices, so they are dispatched first -- they are the critical path.  The two roles
// never wait for each other (no flags, no atomics between them): the only consumer of the side job's output is the later x-half
// launch on the same stream.  Both roles need a whole CU (256 threads at 512 registers, > 80 KB of LDS), so the launch has the
// resources of the larger of the two and loses no occupancy.
#include "kernels_deep.h"
#include "kernels_conv.h"
#include "split16.h"
#include "gn_defer.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace cd {

#include "deep_body.inc"
#include "conv_zs_body.inc"

namespace {

static_assert(DC_THREADS == 256, "both roles are programs of four waves");

struct DeepSideArgs {
  DeepArgs deep;
  ConvZsArgs side;  // whole planes, unnormalised input, one output-channel tile: z3_wave<.., false, 0>
  int ndeep;        // workgroups [0, ndeep) run the level for sample blockIdx.x; workgroup ndeep + b * nchunk + c chunk c of sample b
};

template <int NT>
__global__ void __launch_bounds__(256, 1) deep_level_side_kernel(DeepSideArgs a) {
  extern __shared__ __attribute__((aligned(16))) char ds_lds[];
  const int bx = blockIdx.x;
  if (bx < a.ndeep) {
    deep_level_body<NT>(a.deep, ds_lds, bx);
    return;
  }
  const int j = bx - a.ndeep;
  ZsBlk kb;
  kb.y = j / a.side.nchunk;
  kb.x = j - kb.y * a.side.nchunk;
  kb.z = 0;
  kb.nx = a.side.nchunk;
  switch (threadIdx.x >> 6) {
    case 0: z3_wave<0, false, 0, 0, ZS_NSL>(a.side, ds_lds, kb); break;
    case 1: z3_wave<1, false, 0, 0, ZS_NSL>(a.side, ds_lds, kb); break;
    case 2: z3_wave<2, false, 0, 0, ZS_NSL>(a.side, ds_lds, kb); break;
    default: z3_wave<3, false, 0, 0, ZS_NSL>(a.side, ds_lds, kb); break;
  }
}

template <int NT>
void launch_deep_side_inst(const DeepSideArgs& a, unsigned grid, size_t lds, hipStream_t s) {
  static bool attr_set = false;
  if (!attr_set) {
    CD_HIP(hipFuncSetAttribute((const void*)deep_level_side_kernel<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_set = true;
  }
  hipLaunchKernelGGL(deep_level_side_kernel<NT>, dim3(grid), dim3(256), lds, s, a);
  CD_HIP(hipGetLastError());
}

// LDS of the side role: whole planes of up to ZS_NSL * 32 voxels in the one-wave-per-SIMD form (try_launch_conv_zslide's lds_for)
int side_ring(const Dims3& d) { return d.h * d.w >= 2 * ZS_STEP ? 4 : 5; }
size_t side_lds(const Dims3& d) {
  const size_t plane = ((size_t)d.h * d.w * ZS_VB + 255) & ~(size_t)255;
  return (size_t)ZS_ZERO + Z3_COEF + (size_t)side_ring(d) * plane + 2 * Z3_XCH;
}

}  // namespace

int deep_side_conv_chunks(int batch, int cin_side, int cout, Dims3 dims) {
  // (read per call, like CD_NO_DEEP_LEVEL: the tests switch sequences inside one process; a captured graph replays what was decided
  // at capture time)
  if (getenv("CD_NO_DEEP_SIDE_CONV")) return 0;
  // the z-slide launcher's own A/B switches (read once, as it does) keep their meaning: with any of them set the conv runs as before
  static const bool zs_switched = getenv("CD_NO_ZSLIDE") || getenv("CD_ZS_V1") || getenv("CD_ZS_STRIP") || getenv("CD_ZS_DBG") ||
                                  getenv("CD_ZS_NSL5") || getenv("CD_ZS_NSL");
  if (zs_switched) return 0;
  if (Z3_PAD || cin_side != 32 || cout != 32 || batch < 1) return 0;
  const int PV = dims.h * dims.w;
  if (PV < ZS_STEP || PV > ZS_NSL * 32 || side_lds(dims) > 160 * 1024) return 0;  // whole planes only
  const int64_t svox = (int64_t)dims.d * PV;
  // Chunks per sample: the count that brings the grid of batch * (1 + n) workgroups closest to a whole number of rounds of the
  // 256 CUs from below (64 samples: 3), the smaller count on a tie.  At most 8: a chunk restages ~2.5 planes of halo and prologue,
  // and the job only has to end before the level does.
  int best = 0;
  int64_t best_gap = 0;
  for (int n = 1; n <= 8 && svox >= (int64_t)2 * ZS_STEP * n; ++n) {
    const int64_t cv = ((svox + n - 1) / n + ZS_STEP - 1) / ZS_STEP * ZS_STEP;
    if ((svox + cv - 1) / cv != n) continue;  // (rounding the chunk to whole steps left fewer chunks)
    const int64_t total = (int64_t)batch * (1 + n);
    const int64_t gap = (total + 255) / 256 * 256 - total;
    if (!best || gap < best_gap) { best = n; best_gap = gap; }
  }
  return best;
}

void launch_deep_level_side(const DeepLevelDesc& d, const float* x_in, float* x_out, int batch, int* status, const DeepSideConv& sc,
                            hipStream_t s) {
  DeepSideArgs a;
  double flops = 0.0;
  const size_t lds_deep = deep_fill_args(d, x_in, x_out, status, &a.deep, &flops);
  const int nchunk = deep_side_conv_chunks(batch, sc.cin, sc.cout, sc.dims);
  CD_REQUIRE(nchunk > 0 && sc.in && sc.wpk && sc.out, "internal: deep level launched with an ineligible side conv");
  const int PV = sc.dims.h * sc.dims.w;
  const int64_t svox = (int64_t)sc.dims.d * PV;
  ConvZsArgs& z = a.side;
  z = ConvZsArgs{};
  z.in = sc.in; z.ldc = sc.ldc; z.coef = nullptr; z.coef_c = sc.cin; z.act = 0;
  z.wpk = (const u32x4*)sc.wpk; z.CTtot = sc.cout / 32;
  z.bias = sc.bias; z.acc_delta = 0; z.out = sc.out; z.cout = sc.cout; z.ch_part = nullptr;
  z.D = sc.dims.d; z.H = sc.dims.h; z.W = sc.dims.w; z.NR = side_ring(sc.dims); z.HS = sc.dims.h;
  z.nchunk = nchunk;
  z.CV = (int)(((svox + nchunk - 1) / nchunk + ZS_STEP - 1) / ZS_STEP * ZS_STEP);
  z.status = status; z.defer = GnDefer(); z.choff = 0; z.in_absmax = nullptr; z.dbg = 0;
  a.ndeep = batch;
  const size_t lds_side = side_lds(sc.dims);
  const size_t lds = lds_deep > lds_side ? lds_deep : lds_side;
  const int64_t grid = (int64_t)batch * (1 + nchunk);
  CD_REQUIRE(lds <= 160 * 1024 && grid < (1ll << 31), "deep level + side conv: launch geometry out of range");
  const double vox = (double)d.dims.vox();
  char cat[128];
  std::snprintf(cat, sizeof cat, "deep_level C%d/%d @%dx%dx%d + conv3x3x3 K-block C%d->%d @%dx%dx%d", d.Ca, d.Cb, d.dims.d, d.dims.h,
                d.dims.w, sc.cin, sc.cout, sc.dims.d, sc.dims.h, sc.dims.w);
  prof::Scope scope(cat, s, flops * batch + 2.0 * 27 * sc.cin * sc.cout * (double)svox * batch,
                    8.0 * batch * vox * d.Ca + 4.0 * batch * (double)svox * (sc.cin + sc.cout));
  const int NT = (int)((d.dims.vox() + 31) / 32);
  switch (NT) {
    case 1: launch_deep_side_inst<1>(a, (unsigned)grid, lds, s); break;
    case 2: launch_deep_side_inst<2>(a, (unsigned)grid, lds, s); break;
    case 3: launch_deep_side_inst<3>(a, (unsigned)grid, lds, s); break;
    default: launch_deep_side_inst<4>(a, (unsigned)grid, lds, s); break;
  }
}

}  // namespace cd
