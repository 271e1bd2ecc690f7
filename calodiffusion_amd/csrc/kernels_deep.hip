// The deepest U-Net level as ONE launch: everything CondUnet.forward (calodiffusion/models/models.py:713-743) does on the
// coarsest grid -- downs[-1] (ResnetBlock, ResnetBlock, Residual(PreNorm(LinearAttention))), mid_block1, mid_attn, mid_block2,
// ups[0] (ResnetBlock on cat(x, skip), ResnetBlock, attention) -- for grids where a whole sample is at most 128 voxels
// (Dataset-2: 12 x 4 x 2 = 96 voxels, 32 / 64 channels).
//
// As separate launches that level was 13 kernels per denoise step, 0.33 of the 2.0 ms, for ~1.5 % of the arithmetic: every
// launch paid a launch gap, a GroupNorm fold from global partials, an L2 round trip of its input and output and its own
// prologue / epilogue around 1-4 us of MFMA work.  Here ONE workgroup (4 waves, one per SIMD, 512 registers each: the
// accumulators of all row tiles, a deep weight-fragment ring and the block's shortcut tile live in registers together) owns one
// sample from the strided conv's output to the transposed conv's input and the activations never leave the CU:
//
//  * state in LDS as fp32 rows [voxel][channel]: X (the running tensor, also every block's shortcut), SKIP (the level's skip
//    connection), H1 (a block's first conv output).  GroupNorm statistics are workgroup-local sums.
//  * a 3x3x3 conv = conv_small's scheme (kernels_conv_small.hip) on those rows: the input -- normalised on the fly where it is
//    a block's second conv -- is split to f16x2 (split16.h) into a zero / phi-halo padded record image, every tap is
//    "record + constant"; the (tap, k-step) pairs are dealt round-robin over the waves of an output-channel tile (K split:
//    each weight fragment is fetched from L2 once per workgroup and applied to all row tiles), the K slices are summed through
//    LDS (the exchange re-uses the image), slice s of a channel tile ends up owning row tiles s, s + KS, ... in registers: bias,
//    statistics, GroupNorm + SiLU (+ embedding) and the shortcut are applied there.
//  * the 1x1 shortcut conv of a block that changes width runs on the block's own conv1 image (centre tap), each owner wave
//    computing its own tile (K = cin is small: no K split, no exchange).
//  * linear attention = the arithmetic of kernels_attn.hip's single-launch form with x read from / written to LDS.
//
// The reference ops: ResnetBlock models.py:172-200, Block :147-169, LinearAttention / PreNorm / Residual :281-329, 111-117.
#include "kernels_deep.h"
#include "kernels_conv.h"
#include "split16.h"

#include <cstdio>
#include <cstdlib>

namespace cd {

#include "deep_body.inc"

namespace {

template <int NT>
__global__ void __launch_bounds__(DC_THREADS) deep_level_kernel(DeepArgs a) {
  extern __shared__ __attribute__((aligned(16))) char dc_lds[];
  deep_level_body<NT>(a, dc_lds, blockIdx.x);
}

template <int NT>
void launch_deep_inst(const DeepArgs& a, int batch, size_t lds, hipStream_t s) {
  static bool attr_set = false;
  if (!attr_set) {
    CD_HIP(hipFuncSetAttribute((const void*)deep_level_kernel<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_set = true;
  }
  hipLaunchKernelGGL(deep_level_kernel<NT>, dim3((unsigned)batch), dim3(DC_THREADS), lds, s, a);
  CD_HIP(hipGetLastError());
}

}  // namespace

bool deep_level_eligible(const DeepLevelDesc& d) {
  // (read on every call, once per forward: the parity tests switch between this launch and the per-op kernels in one process;
  // a captured step graph replays whatever was decided at capture time)
  if (getenv("CD_NO_DEEP_LEVEL")) return false;
  for (int i = 0; i < 6; ++i)
    if (!d.res[i].w1 || !d.res[i].w2) return false;
  return deep_level_layout(d, nullptr) != 0;
}

void launch_deep_level(const DeepLevelDesc& d, const float* x_in, float* x_out, int batch, int* status, hipStream_t s) {
  DeepArgs a{};
  double flops = 0.0;
  const size_t lds = deep_fill_args(d, x_in, x_out, status, &a, &flops);
  const double vox = (double)d.dims.vox();
  char cat[96];
  std::snprintf(cat, sizeof cat, "deep_level C%d/%d @%dx%dx%d", d.Ca, d.Cb, d.dims.d, d.dims.h, d.dims.w);
  prof::Scope scope(cat, s, flops * batch, 8.0 * batch * vox * d.Ca);
  const int NT = (int)((d.dims.vox() + 31) / 32);
#ifdef CD_DEEP_STAMPS
  a.dbg = getenv("CD_DEEP_ABL") ? atoi(getenv("CD_DEEP_ABL")) : 0;
  static const bool dbg = getenv("CD_DEEP_DBG") != nullptr;
  unsigned long long zero[16] = {0};
  if (dbg) CD_HIP(hipMemcpyToSymbol(HIP_SYMBOL(dc_stamp_buf), zero, sizeof zero));
#endif
  switch (NT) {
    case 1: launch_deep_inst<1>(a, batch, lds, s); break;
    case 2: launch_deep_inst<2>(a, batch, lds, s); break;
    case 3: launch_deep_inst<3>(a, batch, lds, s); break;
    default: launch_deep_inst<4>(a, batch, lds, s); break;
  }
#ifdef CD_DEEP_STAMPS
  if (dbg) {
    unsigned long long st[16];
    CD_HIP(hipStreamSynchronize(s));
    CD_HIP(hipMemcpyFromSymbol(st, HIP_SYMBOL(dc_stamp_buf), sizeof st));
    unsigned long long tot = 0;
    for (int i = 0; i < 8; ++i) tot += st[i];
    std::fprintf(stderr, "[deep stamps] stage: top barrier %llu prefetch+zero %llu rows %llu barrier %llu\n", st[8], st[9], st[10], st[0]);
    st[0] += st[8] + st[9] + st[10];
    std::fprintf(stderr, "[deep stamps] stage %llu shortcut %llu mfma %llu exchange %llu gn %llu close %llu attn %llu io %llu  total %llu (s_memtime ticks)\n",
                 st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7], tot);
  }
#endif
}

}  // namespace cd
