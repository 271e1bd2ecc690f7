// What the convolution translation units share (internal): the MFMA shorthands and bf16 split, the argument blocks the
// dispatcher (kernels_conv.hip) fills, the per-family launch functions it calls, and the on-device tiling selection.
//   kernels_conv.hip            precision state, weight packing, tiling candidates, launch_conv_mfma (the ladder)
//   kernels_conv_tiled.hip      halo-tiled kernels: conv_mfma_kernel (f32), conv_tiled_bf16x3_kernel (bf16x3 / f16x2)
//   kernels_conv_flat.hip       flat-range kernels: f32 and warp-specialised bf16x3; try_launch_conv3_flat (their tiling ladder)
//   kernels_conv_flat16.hip     flat-range kernel on the 16-bit pipes: conv3_flat_bf16x3_kernel (bf16x3 / f16x2)
//   kernels_conv_transpose.hip  transposed conv;  kernels_pointwise.hip  1x1x1 conv;  kernels_init_conv.hip  init conv
#pragma once
#include "kernels_conv.h"
#include "split16.h"
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>

namespace cd {

#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)
#define MFMA_BF16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, (a)), __builtin_bit_cast(bf16x8, (b)), (c), 0, 0, 0)

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
  const bf16x2 v = {(__bf16)lo, (__bf16)hi};  // v_cvt_pk_bf16_f32, round to nearest even
  return __builtin_bit_cast(unsigned, v);
}
// exact three-way split of 4 floats -> three 8-byte groups of 4 bf16
__device__ __forceinline__ void split3(const f32x4 x, u32x2& t1, u32x2& t2, u32x2& t3) {
  f32x4 r = x;
  t1 = u32x2{pack_bf16(r[0], r[1]), pack_bf16(r[2], r[3])};
  r[0] -= __uint_as_float(t1[0] << 16); r[1] -= __uint_as_float(t1[0] & 0xffff0000u);
  r[2] -= __uint_as_float(t1[1] << 16); r[3] -= __uint_as_float(t1[1] & 0xffff0000u);
  t2 = u32x2{pack_bf16(r[0], r[1]), pack_bf16(r[2], r[3])};
  r[0] -= __uint_as_float(t2[0] << 16); r[1] -= __uint_as_float(t2[0] & 0xffff0000u);
  r[2] -= __uint_as_float(t2[1] << 16); r[3] -= __uint_as_float(t2[1] & 0xffff0000u);
  t3 = u32x2{pack_bf16(r[0], r[1]), pack_bf16(r[2], r[3])};
}

// ---- halo-tiled kernels (kernels_conv_tiled.hip): forward conv, 3x3x3 stride 1 and the strided (3,4,4) down-sampling conv ----
struct ConvKArgs {
  const float* in0;
  const float* in1;
  int c0, c1;
  const float* wpk;
  const float* bias;
  float* out;
  int Din, Hin, Win, Do, Ho, Wo;
  int KD, KH, KW, SZ, SH, SW;
  int TZ, TH, nTZ, nTH;  // output tile (z, phi) extents and tile counts; tiles span the full r extent
  int IZ, IH;            // staged input tile extents (with halo)
  int cout, CTtot;
  const float* coef;     // fused GroupNorm(+SiLU) of the input, see ConvFlatArgs
  int act;
};
struct ConvTiled3Args {
  ConvKArgs k;       // geometry / tiling / pointers (wpk = packed bf16x3 weights)
  float* ch_part;    // optional channel statistics of the output: [B][nTZ*nTH][cout][2]
  int* status;       // f16x2: bit 0 <- a staged value exceeded the fp16 range
};
// the kernel instance for VT row tiles per wave and CT output-channel tiles per workgroup (NTERM = 3: bf16x3, 2: f16x2)
void launch_conv_tiled_f32(int VT, int CT, const ConvKArgs& a, dim3 grid, int threads, size_t lds, hipStream_t s);
void launch_conv_tiled_split16(int VT, int CT, int NTERM, const ConvTiled3Args& a, dim3 grid, int threads, size_t lds, hipStream_t s);

// ---- flat-range kernels (kernels_conv_flat.hip; the 16-bit split kernel: kernels_conv_flat16.hip) ----
struct ConvFlatArgs {
  const float* in0;
  const float* in1;
  int c0, c1;
  const float* wpk;
  const float* bias;
  float* out;
  int D, H, W;     // input extents
  int Do, Ho, Wo;  // output extents (== input for stride 1)
  int R;       // output voxels per workgroup (multiple of 32)
  int P;       // plane capacity of the LDS tile
  int cout, CTtot;
  int dbg;     // timing experiments only (CD_FLAT_DBG): 1 = skip staging, 2 = skip the MFMA taps
  // fused GroupNorm: `coef` = per-(sample, input channel) {scale, shift, add, -} applied (with SiLU if `act`) while the
  // input is staged; `ch_part` = per-(sample, workgroup, output channel) {sum, sum of squares} of this conv's output.
  const float* coef;
  int act;
  float* ch_part;
  int* status = nullptr;  // f16x2 only: bit 0 <- a staged value exceeded the fp16 range
  GnDefer defer;          // split-16 kernels: fold the input normalisation in the prologue (table at lds + coef_lds_off)
  int coef_lds_off = 0;
  const unsigned* in_absmax = nullptr;  // f16x2: power-of-two input rescaling (ConvFusion::in_absmax)
  const float* add_src = nullptr;       // split-16 kernels: out = conv + add_src (ConvFusion::add_src)
};
// returns false when the whole-plane LDS tile does not fit (wide grids such as Dataset-3's 50x18 planes).
// prec = 3 / 2 runs the split-bf16 / split-fp16 kernel on `wpk` = that packed image; 0 the f32 MFMA kernel (stride-1 3x3x3 only).
bool try_launch_conv3_flat(const float* in0, int c0, const float* in1, int c1, const void* wpk, const float* bias, float* out,
                           int batch, int cout, const ConvGeom& g, hipStream_t s, const ConvFusion& fu,
                           int prec /* 0 = f32 MFMA, 3 = bf16x3, 2 = f16x2 */);
// the split-16 instance for VT row tiles per wave, CT channel tiles per workgroup and geometry `geo`; false = there is none
// (f16x2 holds two accumulators per tile: VT * CT <= 4)
bool launch_conv_flat_split16(int VT, int CT, int NTERM, int geo, const ConvFlatArgs& a, dim3 grid, int threads, size_t lds, hipStream_t s);

// ---- one-time on-device selection among candidate tilings of one conv geometry (all candidates give bit-identical
// results: the per-output summation order does not depend on the tiling).  Never runs during stream capture. ----
std::map<std::string, int>& tune_cache();  // kernels_conv.hip
template <typename F>
int autotune(const std::string& key, int ncand, F&& run, hipStream_t s) {
  auto it = tune_cache().find(key);
  if (it != tune_cache().end()) return it->second;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (getenv("CD_NO_AUTOTUNE") || hipStreamIsCapturing(s, &st) != hipSuccess || st != hipStreamCaptureStatusNone || prof::enabled())
    return -1;  // caller falls back to its heuristic (not cached)
  hipEvent_t e0, e1;
  CD_HIP(hipEventCreate(&e0));
  CD_HIP(hipEventCreate(&e1));
  int best = 0;
  float best_ms = 1e30f;
  for (int i = 0; i < ncand; ++i) {
    run(i);  // warm-up (also sets function attributes)
    CD_HIP(hipEventRecord(e0, s));
    run(i);
    run(i);
    CD_HIP(hipEventRecord(e1, s));
    CD_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    CD_HIP(hipEventElapsedTime(&ms, e0, e1));
    if (getenv("CD_TUNE_VERBOSE") && atoi(getenv("CD_TUNE_VERBOSE")) > 1) std::fprintf(stderr, "[calodiff autotune]   %s cand %d: %.1f us\n", key.c_str(), i, ms * 500.f);
    if (ms < best_ms) { best_ms = ms; best = i; }
  }
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  tune_cache()[key] = best;
  if (getenv("CD_TUNE_VERBOSE")) std::fprintf(stderr, "[calodiff autotune] %s -> candidate %d (%.1f us)\n", key.c_str(), best, best_ms * 500.f);
  return best;
}

}  // namespace cd
