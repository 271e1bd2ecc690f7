// "z-slide" 3x3x3 stride-1 phi-periodic convolution for the full-resolution level of the U-Net (CylindricalConv,
// calodiffusion/models/models.py:65-96 as used by Block.proj :153) -- the kernel that dominates a denoise step.
//
// Arithmetic ("f16x2"): gfx950's f32-input MFMA runs at 1/16 of the 16-bit rate.  Every fp32 operand is split into two
// fp16 terms, x = x1 + 2^-11 x2' with x1 = f16(x), x2' = f16((x - x1) * 2^11) (22 significant bits; the 2^11 keeps the
// second term out of the fp16 subnormals), and the product is formed from three MFMAs into two fp32 accumulators,
//     A += x1*w1          B += x1*w2' + x2'*w1          result = A + 2^-11 B           (dropped: x2*w2 <= 2^-22 relative)
// fp16 x fp16 products are exact in fp32 and v_mfma_f32_32x32x16_f16 accumulates in fp32: the result carries fp32
// rounding-level error (measured 3.7e-7 relative on K = 864 against 3.7e-7 for an fp32 dot product) at 3/16 of the
// matrix-pipe time of the f32 MFMA.  Values beyond the fp16 range (|x| > 65504) turn into inf/NaN in the output and raise
// the plan's range flag; the bf16x3 / f32 kernels (CD_CONV_PRECISION) have the full fp32 range.
//
// Structure (one workgroup = 4 waves = one CU, one contiguous chunk of one sample's flattened (z, phi, r) voxels):
//  * the 27 taps x 2 sixteen-channel k-steps are SPLIT OVER THE 4 WAVES and each wave keeps its 13-14 (tap, k-step)
//    weight fragments in registers for the whole chunk (112 VGPRs): no weight traffic at all inside the loop;
//  * input planes live in a 5-slot LDS ring (144 B per voxel: 2 k-steps x 2 terms x 16 fp16 + 16 B pad => conflict-free
//    ds_read_b128 A-fragments); every input plane is fetched, normalised (fused GroupNorm + SiLU + embedding), split and
//    written ONCE per chunk, one plane per step, its global loads issued before the step's MFMAs and converted after;
//  * a step = 128 output voxels = 4 row tiles; every wave runs its K-slice over all 4 tiles, the partial 32x32 tiles
//    are exchanged through LDS (48 KiB) and wave t sums, adds bias, stores and accumulates the channel statistics of
//    tile t.  Fixed summation order => deterministic.
#include "kernels_conv.h"
#include "split16.h"
#include "gn_defer.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace cd {

// packed f16x2 weights: [k-step = ci/16][tap][ct = co/32][term][lane = h*32+j][8 fp16] = W_term[co = ct*32+j][ci = ks*16+8h+0..7]
__device__ __forceinline__ void pack_weights_f16x2_elem(size_t idx, const float* __restrict__ w, u32x4* __restrict__ wpk, int cout,
                                                        int cin, int taps, int transposed, int flip) {
  const int lane = idx & 63;
  size_t rest = idx >> 6;
  const int CT = (cout + 31) / 32;
  const int ct = rest % CT;
  rest /= CT;
  const int tap = rest % taps;
  const int ks = rest / taps;
  const int h = lane >> 5, j = lane & 31;
  const int co = ct * 32 + j;
  f32x4 v[2];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int ci = ks * 16 + h * 8 + e;
    const int st = flip ? taps - 1 - tap : tap;
    const size_t src = transposed ? ((size_t)ci * cout + co) * taps + st : ((size_t)co * cin + ci) * taps + st;
    v[e >> 2][e & 3] = (co < cout && ci < cin) ? w[src] : 0.f;
  }
  u32x2 a1, a2, b1, b2;
  split2(v[0], a1, a2);
  split2(v[1], b1, b2);
  u32x4* dst = wpk + (((size_t)(ks * taps + tap) * CT + ct) * 2) * 64 + lane;
  dst[0] = u32x4{a1[0], a1[1], b1[0], b1[1]};
  dst[64] = u32x4{a2[0], a2[1], b2[0], b2[1]};
}
__global__ void pack_weights_f16x2_kernel(const float* __restrict__ w, u32x4* __restrict__ wpk, int cout, int cin, int taps,
                                          size_t total, int transposed, int flip) {
  const size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x;  // one thread per (ks, tap, ct, lane)
  if (idx >= total) return;
  pack_weights_f16x2_elem(idx, w, wpk, cout, cin, taps, transposed, flip);
}
// the f16x2 images of every tensor of a plan in one launch (PackJob, kernels_conv.h): blockIdx.y = job
__global__ void __launch_bounds__(256) pack_jobs_f16x2_kernel(const PackJob* __restrict__ jobs) {
  const PackJob j = jobs[blockIdx.y];
  if (!j.f16) return;
  const size_t t0 = blockIdx.x * (size_t)256 + threadIdx.x, stride = gridDim.x * (size_t)256;
  for (size_t i = t0; i < j.n_f16; i += stride)
    pack_weights_f16x2_elem(i, j.src, (u32x4*)j.f16, j.cout, j.cin, j.taps, j.kind == 2 || j.tr, j.flip);
}
void launch_pack_jobs_f16x2(const PackJob* d_jobs, int njobs, hipStream_t s) {
  if (njobs <= 0) return;
  hipLaunchKernelGGL(pack_jobs_f16x2_kernel, dim3(48, (unsigned)njobs), dim3(256), 0, s, d_jobs);
  CD_HIP(hipGetLastError());
}

void launch_pack_weights_f16x2(const float* w_torch, void* wpk, int cout, int cin, int taps, hipStream_t s, bool transposed,
                               bool flip) {
  CD_REQUIRE(cin % 16 == 0, "f16x2 convolution needs input channels in multiples of 16");
  const size_t total = (size_t)(cin / 16) * taps * ((cout + 31) / 32) * 64;
  hipLaunchKernelGGL(pack_weights_f16x2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, w_torch, (u32x4*)wpk, cout,
                     cin, taps, total, transposed ? 1 : 0, flip ? 1 : 0);
  CD_HIP(hipGetLastError());
}

#include "conv_zs_body.inc"

namespace {

// NSL: staging pieces per thread and plane = plane images of up to 32 NSL voxels (5: 160 -- Dataset-2's whole planes; 7: 224 --
// Dataset-3's strips of 10 phi rows + 2 halo rows of 18 voxels instead of 5 + 2, HGCal's of 6 + 2 rows of 21 instead of 4 + 2:
// less halo restaged per output row; 8: 256 -- Dataset-3's level-1 planes of 25 x 9 voxels whole)
template <bool ACC, int MODE, int DBG = 0, int NSL = ZS_NSL>
__global__ void __launch_bounds__(256, 1) conv_zslide_sw_f16x2_kernel(ConvZsArgs a) {
  extern __shared__ __attribute__((aligned(16))) char zs_lds[];
  const ZsBlk kb = zs_blk_of_grid();
  switch (threadIdx.x >> 6) {
    case 0: z3_wave<0, ACC, MODE, DBG, NSL>(a, zs_lds, kb); break;
    case 1: z3_wave<1, ACC, MODE, DBG, NSL>(a, zs_lds, kb); break;
    case 2: z3_wave<2, ACC, MODE, DBG, NSL>(a, zs_lds, kb); break;
    default: z3_wave<3, ACC, MODE, DBG, NSL>(a, zs_lds, kb); break;
  }
}

// launch of one K-block: the specialisation for (continuation, normed input, strips, rescaled input)
void z3_launch(const ConvZsArgs& a, bool acc, dim3 grid, size_t lds, hipStream_t s) {
  const int mode = ((a.coef || a.defer.part) ? 1 : 0) | (a.HS < a.H ? 2 : 0) | (a.in_absmax ? 4 : 0);
  const int staged = (a.HS + (a.HS < a.H ? 2 : 0)) * a.W;  // voxels of a plane image
  const int nsl = staged > 7 * 32 ? 8 : (staged > ZS_NSL * 32 ? 7 : ZS_NSL);
#define Z3_CASE(ACCV, M, N)                                                                                                           \
  if (acc == ACCV && mode == M && nsl == N) {                                                                                         \
    static bool attr = false;                                                                                                         \
    if (!attr) {                                                                                                                      \
      CD_HIP(hipFuncSetAttribute((const void*)conv_zslide_sw_f16x2_kernel<ACCV, M, 0, N>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                 160 * 1024));                                                                                        \
      attr = true;                                                                                                                    \
    }                                                                                                                                 \
    hipLaunchKernelGGL((conv_zslide_sw_f16x2_kernel<ACCV, M, 0, N>), grid, dim3(256), lds, s, a);                                      \
    return;                                                                                                                           \
  }
  Z3_CASE(false, 0, 5) Z3_CASE(false, 1, 5) Z3_CASE(false, 2, 5) Z3_CASE(false, 3, 5) Z3_CASE(false, 4, 5) Z3_CASE(false, 6, 5)
  Z3_CASE(true, 0, 5) Z3_CASE(true, 2, 5) Z3_CASE(true, 4, 5) Z3_CASE(true, 6, 5)
  Z3_CASE(false, 0, 7) Z3_CASE(false, 1, 7) Z3_CASE(false, 2, 7) Z3_CASE(false, 3, 7) Z3_CASE(false, 4, 7) Z3_CASE(false, 6, 7)
  Z3_CASE(true, 0, 7) Z3_CASE(true, 2, 7) Z3_CASE(true, 4, 7) Z3_CASE(true, 6, 7)
  Z3_CASE(false, 0, 8) Z3_CASE(false, 1, 8) Z3_CASE(false, 2, 8) Z3_CASE(false, 3, 8) Z3_CASE(false, 4, 8) Z3_CASE(false, 6, 8)
  Z3_CASE(true, 0, 8) Z3_CASE(true, 2, 8) Z3_CASE(true, 4, 8) Z3_CASE(true, 6, 8)
#undef Z3_CASE
  CD_REQUIRE(false, "z-slide conv: no kernel instance for this combination of continuation / normalised / strip / rescaled input");
}

}  // namespace

// Eligible: 3x3x3 stride 1 on grids whose planes -- or phi strips of them (HS rows, HS | H, with one halo row either side) --
// hold 64..160 voxels and fit the LDS ring: Dataset-2's 16x9 planes whole, Dataset-3's 50x18 in 10 strips of 5 rows, HGCal's
// 12x21 in 3 strips of 4.  Returns false otherwise.
bool try_launch_conv_zslide(const float* in0, int c0, const float* in1, int c1, const void* wpk_f16x2, const float* bias, float* out,
                            int batch, int cout, const ConvGeom& g, hipStream_t s, const ConvFusion& fu) {
  // (environment switches of this launcher are read once: it sits on the eager hot path, one call per K-block)
  static const bool no_zslide = getenv("CD_NO_ZSLIDE") != nullptr;
  static const int strip_env = getenv("CD_ZS_STRIP") ? atoi(getenv("CD_ZS_STRIP")) : 0;  // testing: force a strip height
  static const int dbg_env = getenv("CD_ZS_DBG") ? atoi(getenv("CD_ZS_DBG")) : 0;
  if (no_zslide) return false;
  if (!(g.kd == 3 && g.kh == 3 && g.kw == 3 && g.sz == 1 && g.sh == 1 && g.sw == 1)) return false;
  if (cout % 32 || c0 % 32 || c1 % 32) return false;
  const int H = g.in.h, W = g.in.w;
  auto ring_for = [&](int hs) { return hs * W >= 2 * ZS_STEP ? 4 : 5; };
  // the one-wave-per-SIMD form is specialised at compile time; anything outside its instances (a normalised input without the
  // activation, a normalised AND rescaled input) takes the matrix-wave / helper-wave form, as does CD_ZS_V1=1 (A/B)
  static const bool v1_env = getenv("CD_ZS_V1") != nullptr;
  const bool normed_in = fu.coef || fu.defer.part;
  const bool v1 = v1_env || (normed_in && !fu.act) || (normed_in && fu.in_absmax) || (normed_in && (c0 + c1) > 32);
  auto lds_for = [&](int hs) {
    const int rows = hs + (hs < H ? 2 : 0);
    const size_t ring = (size_t)ring_for(hs) * (((size_t)rows * W * ZS_VB + 255) & ~(size_t)255);
    const size_t ring3 = Z3_PAD ? (size_t)ring_for(hs) * ((((size_t)rows * (W + 1) + 1) * ZS_VB + 255) & ~(size_t)255) : ring;
    return v1 ? (size_t)ZS_ZERO + ring + ZS_PART : (size_t)ZS_ZERO + Z3_COEF + ring3 + 2 * Z3_XCH;
  };
  // voxels of a plane image the staging threads cover: 5 pieces of 32; the one-wave-per-SIMD form also has a 7-piece instance for
  // strips (CD_ZS_NSL5=1: without it, A/B)
  static const bool nsl5_env = getenv("CD_ZS_NSL5") != nullptr;
  static const int nsl_env = getenv("CD_ZS_NSL") ? atoi(getenv("CD_ZS_NSL")) : 8;  // (A/B: cap the pieces at 5, 7 or 8)
  const int max_staged = (v1 || nsl5_env) ? ZS_NSL * 32 : std::min(8, std::max(5, nsl_env)) * 32;
  int HS = 0;
  for (int hs = H; hs >= 1; --hs) {  // the largest strip that fits: least halo restaging
    if (H % hs) continue;
    const int rows = hs + (hs < H ? 2 : 0);
    if (hs * W < ZS_STEP || rows * W > max_staged || lds_for(hs) > 160 * 1024) continue;
    HS = hs;
    break;
  }
  if (!HS) return false;
  if (strip_env) {
    const int hs = strip_env;
    const int rows = hs + (hs < H ? 2 : 0);
    if (hs >= 1 && H % hs == 0 && hs * W >= ZS_STEP && rows * W <= max_staged && lds_for(hs) <= 160 * 1024) HS = hs;
  }
  const int nstrip = H / HS;
  const int SPV = HS * W;
  const int64_t svox = (int64_t)g.in.d * SPV;  // voxels per strip
  if (svox < 2 * ZS_STEP) return false;
  const size_t lds = lds_for(HS);
  // what the kernels assume about this launch, checked where it is cheap: the GroupNorm fold of the prologue builds its table of
  // all defer.C channels plus its scratch (gn_defer_scratch_bytes) inside the exchange region, before the first exchange
  if (fu.defer.part) {
    CD_REQUIRE(fu.defer.C >= c0 + c1 && fu.defer.C % 4 == 0, "z-slide conv: the deferred GroupNorm must cover the input channels");
    CD_REQUIRE((size_t)fu.defer.C * 16 + (size_t)gn_defer_scratch_bytes(fu.defer.C) <= (size_t)(v1 ? ZS_PART : 2 * Z3_XCH),
               "z-slide conv: the GroupNorm fold's scratch does not fit the exchange region");
  }
  CD_REQUIRE(lds <= 160 * 1024 && (int64_t)batch * (H / HS) <= 65535 * 64, "z-slide conv: launch geometry out of range");
  const int CTtot = cout / 32;
  // chunks per strip: fill the 256 CUs (one workgroup each) with as few rounds and as little halo restaging as possible
  int best = 1;
  double best_eff = 0.0;
  const int max_chunks = (int)(svox / (2 * ZS_STEP));
  for (int n = 1; n <= max_chunks && n <= 64; ++n) {
    const int64_t cv = ((svox + n - 1) / n + ZS_STEP - 1) / ZS_STEP * ZS_STEP;
    const int nc = (int)((svox + cv - 1) / cv);
    if (nc != n) continue;
    const int64_t total = (int64_t)batch * nstrip * nc * CTtot;
    const int64_t rounds = (total + 255) / 256;
    const double planes = (double)cv / SPV;
    const double eff = (double)total / (rounds * 256.0) * planes / (planes + 2.5);  // halo planes + prologue
    if (eff > best_eff * 1.0001) { best_eff = eff; best = n; }
  }
  int nchunk = best;
  if (fu.zs_chunks > 0) {
    const int64_t cv = ((svox + fu.zs_chunks - 1) / fu.zs_chunks + ZS_STEP - 1) / ZS_STEP * ZS_STEP;
    CD_REQUIRE(fu.zs_chunks <= max_chunks && (svox + cv - 1) / cv == fu.zs_chunks, "z-slide conv: the requested chunk count does not divide this grid");
    nchunk = fu.zs_chunks;
  }
#ifdef CD_ZS_EXPERIMENTS
  if (getenv("CD_ZS_NCHUNK")) nchunk = atoi(getenv("CD_ZS_NCHUNK"));  // (tools/zs_power.sh: the same workgroup program on fewer CUs)
#endif
  const int CV = (int)(((svox + nchunk - 1) / nchunk + ZS_STEP - 1) / ZS_STEP * ZS_STEP);
  static bool attr_set = false;
  if (!attr_set) {
    CD_HIP(hipFuncSetAttribute((const void*)conv_zslide_f16x2_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    CD_HIP(hipFuncSetAttribute((const void*)conv_zslide_f16x2_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_set = true;
  }
  const int nblk = (c0 + c1) / 32;
  for (int kb = 0; kb < nblk; ++kb) {
    ConvZsArgs a;
    const int ch = kb * 32;
    if (ch < c0) { a.in = in0 + ch; a.ldc = c0; }
    else { a.in = in1 + (ch - c0); a.ldc = c1; }
    a.coef = fu.coef ? fu.coef + (size_t)ch * 4 : nullptr;
    a.coef_c = c0 + c1;
    a.defer = fu.defer;
    a.choff = ch;
    a.in_absmax = fu.in_absmax;
    a.act = fu.act;
    a.wpk = (const u32x4*)wpk_f16x2 + (size_t)(kb * 2) * 27 * CTtot * 128;
    a.CTtot = CTtot;
    a.bias = kb == 0 ? bias : nullptr;
    const bool add0 = kb == 0 && fu.add_src && !bias;  // out = conv + add_src: the first K-block runs as a continuation of add_src
    a.acc_delta = add0 ? (long long)((const char*)fu.add_src - (const char*)out) : 0;
    a.out = out;
    a.cout = cout;
    a.ch_part = kb == nblk - 1 ? fu.ch_part : nullptr;
    a.D = g.in.d; a.H = g.in.h; a.W = g.in.w; a.HS = HS; a.NR = ring_for(HS);
    a.nchunk = nchunk; a.CV = CV;
    a.status = fu.status;
    a.dbg = dbg_env;
    const dim3 grid((unsigned)(nstrip * nchunk), (unsigned)batch, (unsigned)CTtot);
#ifdef CD_ZS_EXPERIMENTS
    if (kb == 0 && a.dbg == 2048 && !v1) {  // stamps: print the per-wave cycle sums of one launch
      const bool normed = a.coef || a.defer.part;
      CD_REQUIRE(!a.in_absmax && a.HS == a.H, "CD_ZS_DBG=2048: whole planes, unscaled input");
      if (normed) {
        CD_HIP(hipFuncSetAttribute((const void*)conv_zslide_sw_f16x2_kernel<false, 1, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        hipLaunchKernelGGL((conv_zslide_sw_f16x2_kernel<false, 1, 1>), grid, dim3(256), lds, s, a);
      } else {
        CD_HIP(hipFuncSetAttribute((const void*)conv_zslide_sw_f16x2_kernel<false, 0, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        hipLaunchKernelGGL((conv_zslide_sw_f16x2_kernel<false, 0, 1>), grid, dim3(256), lds, s, a);
      }
      CD_HIP(hipGetLastError());
      static int nlaunch = 0;
      if (++nlaunch == 10) {
        CD_HIP(hipDeviceSynchronize());
        static unsigned long long h[256 * 4 * 12];
        CD_HIP(hipMemcpyFromSymbol(h, HIP_SYMBOL(z3_stamp_buf), sizeof h));
        for (int wg : {0, 100, 255})
          for (int w = 0; w < 4; ++w) {
            const unsigned long long* d = h + ((size_t)wg * 4 + w) * 12;
            const double n = (double)d[7], nc = d[6] ? (double)d[6] : 1.;
            std::fprintf(stderr, "[z3 stamps] wg %3d wave %d: per step: load wait %5.0f (per convert %5.0f)  convert %5.0f (per convert %5.0f)  issue+reduce %5.0f  prepare %5.0f  matrix %5.0f  barrier %5.0f   (%llu converts in %llu steps)  prologue %llu  kernel %llu cycles\n",
                         wg, w, d[0] / n, d[0] / nc, d[1] / n, d[1] / nc, d[2] / n, d[3] / n, d[4] / n, d[5] / n, d[6], d[7], d[8], d[9]);
          }
      }
      continue;
    }
#define ZS_DBG_CASE(D)                                                                                                     \
  case D:                                                                                                                  \
    CD_HIP(hipFuncSetAttribute((const void*)conv_zslide_f16x2_kernel<false, D>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                               160 * 1024));                                                                               \
    hipLaunchKernelGGL((conv_zslide_f16x2_kernel<false, D>), grid, dim3(512), lds, s, a);                                   \
    break;
    if (kb == 0 && a.dbg && v1) {
      switch (a.dbg) {
        ZS_DBG_CASE(2) ZS_DBG_CASE(4) ZS_DBG_CASE(6) ZS_DBG_CASE(22) ZS_DBG_CASE(38) ZS_DBG_CASE(70)
        default: CD_REQUIRE(false, "CD_ZS_DBG: not an instantiated experiment");
      }
      CD_HIP(hipGetLastError());
      continue;
    }
#endif
    if (v1) {
      if (kb == 0 && !add0) hipLaunchKernelGGL(conv_zslide_f16x2_kernel<false>, grid, dim3(512), lds, s, a);
      else hipLaunchKernelGGL(conv_zslide_f16x2_kernel<true>, grid, dim3(512), lds, s, a);
    } else {
      z3_launch(a, kb != 0 || add0, grid, lds, s);
    }
    CD_HIP(hipGetLastError());
  }
  if (fu.add_src && !bias && fu.add_done) *fu.add_done = 1;
  if (fu.units) *fu.units = nstrip * nchunk * 4;
  return true;
}

}  // namespace cd
