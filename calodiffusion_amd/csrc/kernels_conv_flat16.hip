// Flat-range convolution on the 16-bit matrix pipes for gfx950: conv3_flat_bf16x3_kernel, bf16x3 and f16x2 arms (tiling and
// host side: kernels_conv_flat.hip).
#include "conv_internal.h"
#include "gn_defer.h"

namespace cd {

// ------------------------------------------------------------------------------------------------------------
// 3x3x3 stride-1 conv on the bf16 matrix pipe with fp32-grade accuracy ("bf16x3").
//
// gfx950's f32-input MFMA runs at 1/16 of the bf16 rate.  Every fp32 operand is therefore split exactly into three bf16
// terms, x = x1 + x2 + x3 (x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2): 24 significant bits), and the
// product is formed from the six term pairs whose magnitude is >= 2^-16 of the leading one:
//     x*w ~= x1*w1 + (x1*w2 + x2*w1) + (x1*w3 + x2*w2 + x3*w1)          (dropped terms <= 2^-24 relative)
// Each bf16 x bf16 product is exact in fp32 and accumulation is fp32 inside v_mfma_f32_32x32x16_bf16, so the result has
// fp32 rounding-level error (measured: ~2x the error of an fp32 FMA chain, 1e-6 relative on K = 864), at 6/16 of the
// matrix-pipe time of the f32 MFMA.  Weights are split once at pack time; activations are split while they are staged
// into LDS (after the optional fused GroupNorm+SiLU), 96 B per voxel per 16-channel sub-chunk.
// Same flat-range tiling, LDS plane image, software pipeline, and fused statistics epilogue as conv3_flat_kernel.
// ------------------------------------------------------------------------------------------------------------
// Geometry is a template parameter: (KD,KH,KW) taps, z stride SZ, phi/r stride SXY; padding is always (1, circular 1, 1).
// Instantiated for the 3x3x3 stride-1 conv and the (3,4,4) down-sampling conv with z stride 2 or 1.
// NTERM = 3: bf16x3 (96 B per voxel per sub-chunk); NTERM = 2: f16x2 (split16.h; 64 B + 16 B pad = 80 B, an odd number of
// 16-B slots => conflict-free ds_read_b128), two accumulators per tile folded after the K loop.
template <int VT, int CT, int KD, int KH, int KW, int SZ, int SXY, int NTERM>
__global__ void __launch_bounds__(512, (VT * CT * (NTERM == 2 ? 2 : 1) <= 2 ? 3 : 2)) conv3_flat_bf16x3_kernel(ConvFlatArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  char* ldsb = (char*)lds;
  constexpr int T = KD * KH * KW;
  constexpr int VB = NTERM == 3 ? 96 : 80;   // bytes per staged voxel
  constexpr int WS = 64 * NTERM;             // u32x4 per (tap, ct) in the packed weights
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x;
  const int b = blockIdx.y;
  const int ct0 = blockIdx.z * CT;
  const int HW = a.H * a.W;          // input plane
  const int vox = a.D * HW;          // input voxels per sample
  const int HWo = a.Ho * a.Wo;
  const int voxo = a.Do * HWo;       // output voxels per sample
  const int v0 = blockIdx.x * a.R;
  const int vend = min(v0 + a.R, voxo);
  // (index arithmetic by reciprocal -- (v + 0.5) / d is never within float error of an integer for v < 2^20: a run-time integer
  // division is ~40 vector instructions, and this prologue had four to ten of them in workgroups that live ~15 us)
  const float inv_hwo = 1.f / (float)HWo, inv_wo = 1.f / (float)a.Wo;
  auto fdiv = [](int x, float inv) { return (int)(((float)x + 0.5f) * inv); };
  const int zA = fdiv(v0, inv_hwo) * SZ - 1;                   // first staged input plane (may be -1: zero plane)
  const int zB = fdiv(vend - 1, inv_hwo) * SZ + KD - 2;        // last staged input plane
  const int nstage = (zB - zA + 1) * HW;
  const int NZ = a.P * HW;  // all-zero voxel
  const int half = lane >> 5, col = lane & 31;
  if (a.defer.part) gn_defer_to_lds(a.defer, b, (float*)(ldsb + a.coef_lds_off), ldsb + a.coef_lds_off + a.defer.C * 16);
  const bool normed = a.coef || a.defer.part;
  if (tid < VB / 4) ((float*)(ldsb + (size_t)NZ * VB))[tid] = 0.f;

  // per-lane geometry of its output voxel in each of the wave's VT row tiles: LDS index of the (kz=0, kh=1, kw=1) tap,
  // phi-row offsets with wrap-around for each kh, r-validity bit for each kw
  int nb[VT], rowoff[VT][KH], ooff[VT];
  unsigned wmask[VT];
  bool any_valid = false;
#pragma unroll
  for (int vt = 0; vt < VT; ++vt) {
    const int v = v0 + (wave * VT + vt) * 32 + col;
    const bool valid = v < vend;
    const int vv = valid ? v : v0;
    const int oz = fdiv(vv, inv_hwo);
    const int r = vv - oz * HWo;
    const int oh = fdiv(r, inv_wo), ow = r - oh * a.Wo;
    const int ih0 = oh * SXY, iw0 = ow * SXY;
    nb[vt] = (oz * SZ - 1 - zA) * HW + ih0 * a.W + iw0;
    unsigned m = 0;
#pragma unroll
    for (int kh = 0; kh < KH; ++kh) {
      int ih = ih0 + kh - 1;
      ih = ih < 0 ? ih + a.H : (ih >= a.H ? ih - a.H : ih);
      ih = ih >= a.H ? ih - a.H : ih;  // H == 2 with a 4-wide kernel wraps twice
      rowoff[vt][kh] = (ih - ih0) * a.W;
    }
#pragma unroll
    for (int kw = 0; kw < KW; ++kw) {
      const int iw = iw0 + kw - 1;
      if (valid && iw >= 0 && iw < a.W) m |= 1u << kw;
    }
    wmask[vt] = m;
    ooff[vt] = valid ? v * a.cout : -1;
    any_valid |= valid;
  }
  const bool wave_active = __any(any_valid);

  f32x16 acc[VT][CT], accB[NTERM == 2 ? VT : 1][NTERM == 2 ? CT : 1];
#pragma unroll
  for (int vt = 0; vt < VT; ++vt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        acc[vt][ct][r] = 0.f;
        if (NTERM == 2) accB[vt][ct][r] = 0.f;
      }

  float amax = 0.f;
  float gscale = 1.f, ginv = 1.f;
  if (NTERM == 2 && a.in_absmax) pow2_scale_for(*a.in_absmax, &gscale, &ginv);
  const int nsub = (a.c0 + a.c1) >> 4;
  const int gbase = zA * HW;
  const int nslots = nstage * 4;  // one slot = 4 channels of one voxel

  auto tap_voxel = [&](int vt, int tap) -> int {
#ifdef CD_FLAT_ABL_TAPS  // ablation (experiment builds only): what the per-tap address arithmetic costs -- WRONG results
    return nb[vt] + tap;
#endif
    const int kz = tap / (KH * KW), kh = (tap / KW) % KH, kw = tap % KW;
    const int n = nb[vt] + kz * HW + rowoff[vt][kh] + kw - 1;
    return ((wmask[vt] >> kw) & 1u) ? n : NZ;
  };

  for (int sc = 0; sc < nsub; ++sc) {
    const float* src;
    int ldc, coff;
    if (sc * 16 < a.c0) {
      src = a.in0; ldc = a.c0; coff = sc * 16;
    } else {
      src = a.in1; ldc = a.c1; coff = sc * 16 - a.c0;
    }
    const int pq = tid & 3;  // this thread always stages channel quad pq of a voxel
    src += (size_t)b * vox * ldc + coff + pq * 4;
    f32x4 cf[4];
    if (a.defer.part) {
#pragma unroll
      for (int e = 0; e < 4; ++e) cf[e] = *(const f32x4*)(ldsb + a.coef_lds_off + (sc * 16 + pq * 4 + e) * 16);
    } else if (a.coef) {
#pragma unroll
      for (int e = 0; e < 4; ++e) cf[e] = *(const f32x4*)(a.coef + ((size_t)b * (a.c0 + a.c1) + sc * 16 + pq * 4 + e) * 4);
    }
    __syncthreads();
    for (int s0 = tid; s0 < ((a.dbg & 1) ? 0 : nslots); s0 += 4 * nthreads) {
      f32x4 val[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int sidx = s0 + k * nthreads;
        const int g = gbase + (sidx >> 2);
        val[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (sidx < nslots && g >= 0 && g < vox) {
          val[k] = *(const f32x4*)(src + (size_t)g * ldc);
          if (normed) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              float t = cf[e][0] * val[k][e] + cf[e][1];
              if (a.act) t = cd_fast_silu(t);
              val[k][e] = t + cf[e][2];
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int sidx = s0 + k * nthreads;
        if (sidx < nslots) {
          char* d = ldsb + (size_t)(sidx >> 2) * VB + pq * 8;
          if (NTERM == 3) {
            u32x2 t1, t2, t3;
            split3(val[k], t1, t2, t3);
            *(u32x2*)d = t1;
            *(u32x2*)(d + 32) = t2;
            *(u32x2*)(d + 64) = t3;
          } else {
            const f32x4 vs = val[k] * gscale;
            amax = fmaxf(amax, fmaxf(fmaxf(fabsf(vs[0]), fabsf(vs[1])), fmaxf(fabsf(vs[2]), fabsf(vs[3]))));
            u32x2 t1, t2;
            split2(vs, t1, t2);
            *(u32x2*)d = t1;
            *(u32x2*)(d + 32) = t2;
          }
        }
      }
    }
    __syncthreads();
    if (!wave_active || (a.dbg & 2)) continue;

#pragma unroll
    for (int vt = 0; vt < VT; ++vt) asm volatile("" : "+v"(nb[vt]));

    const u32x4* wq = (const u32x4*)a.wpk + ((size_t)sc * T * a.CTtot + ct0) * WS + lane;
    // Register rings: weight fragments (L1/L2) are requested WD taps ahead, LDS fragments AD taps ahead.
#ifndef CD_FLAT_WD
#define CD_FLAT_WD 3
#endif
#ifndef CD_FLAT_AD
#define CD_FLAT_AD 2
#endif
    // Measured again in round 3 (same box, alternating runs): WD 1 / AD 1 -> 3 / 2 takes the strided 32->32 conv from 48.8 to 41.8 us
    // and the 128->32 conv at 23x8x4 from 46.9 to 41.3 us (one tap of cover = 3 VT CT MFMAs is less than an L2 round trip for the
    // narrow tilings), -2 % on the Dataset-2 step, -4 % on HGCal; 4 / 2 the same, 5 / 3 slower (registers).
    // (the f16x2 arm only: the three-term bf16 arm spills hundreds of registers with the deeper rings and keeps one tap of cover;
    // restricting them to the narrow f16x2 tilings as well was measured 0.8 % slower on the Dataset-2 step)
    constexpr bool DEEP = NTERM == 2;
    constexpr int WD = DEEP ? CD_FLAT_WD : 1, AD = DEEP ? CD_FLAT_AD : 1;
    u32x4 bw[WD + 1][CT][NTERM], av[AD + 1][VT][NTERM];
    auto load_w = [&](int tap) {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int t = 0; t < NTERM; ++t) bw[tap % (WD + 1)][ct][t] = wq[((size_t)tap * a.CTtot + ct) * WS + t * 64];
    };
    auto load_a = [&](int tap) {
#pragma unroll
      for (int vt = 0; vt < VT; ++vt) {
        const char* p = ldsb + (size_t)tap_voxel(vt, tap) * VB + half * 16;
#pragma unroll
        for (int t = 0; t < NTERM; ++t) av[tap % (AD + 1)][vt][t] = *(const u32x4*)(p + t * 32);
      }
    };
#pragma unroll
    for (int t0 = 0; t0 < WD; ++t0) load_w(t0);
#pragma unroll
    for (int t0 = 0; t0 < AD; ++t0) load_a(t0);
#pragma unroll
    for (int tap = 0; tap < T; ++tap) {
      if (tap + WD < T) load_w(tap + WD);
      if (tap + AD < T) load_a(tap + AD);
      __builtin_amdgcn_sched_barrier(0);
      const int wc = tap % (WD + 1), ac = tap % (AD + 1);
#pragma unroll
      for (int vt = 0; vt < VT; ++vt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          if (NTERM == 3) {
            f32x16 c = acc[vt][ct];
            c = MFMA_BF16(av[ac][vt][NTERM - 1], bw[wc][ct][0], c);  // x3*w1
            c = MFMA_BF16(av[ac][vt][1], bw[wc][ct][1], c);          // x2*w2
            c = MFMA_BF16(av[ac][vt][0], bw[wc][ct][NTERM - 1], c);  // x1*w3
            c = MFMA_BF16(av[ac][vt][1], bw[wc][ct][0], c);          // x2*w1
            c = MFMA_BF16(av[ac][vt][0], bw[wc][ct][1], c);          // x1*w2
            c = MFMA_BF16(av[ac][vt][0], bw[wc][ct][0], c);          // x1*w1
            acc[vt][ct] = c;
          } else {
            acc[vt][ct] = MFMA_F16(av[ac][vt][0], bw[wc][ct][0], acc[vt][ct]);    // x1*w1
            accB[vt][ct] = MFMA_F16(av[ac][vt][0], bw[wc][ct][1], accB[vt][ct]);  // x1*w2'
            accB[vt][ct] = MFMA_F16(av[ac][vt][1], bw[wc][ct][0], accB[vt][ct]);  // x2'*w1
          }
        }
    }
  }

  if (NTERM == 2) {
#pragma unroll
    for (int vt = 0; vt < VT; ++vt)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[vt][ct][r] = (acc[vt][ct][r] + accB[vt][ct][r] * (1.f / 2048.f)) * ginv;
  }
  if (NTERM == 2 && a.status && amax > 65504.f) atomicOr(a.status, 1);
  float* outb = a.out + (size_t)b * voxo * a.cout;
  float bv[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) bv[ct] = a.bias ? a.bias[(ct0 + ct) * 32 + col] : 0.f;
  if (a.add_src) {  // (the loads of all rows first: one round trip, not one per row)
    const float* addb = a.add_src + (size_t)b * voxo * a.cout;
#pragma unroll
    for (int vt = 0; vt < VT; ++vt) {
      float ad[16][CT];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int off = __shfl(ooff[vt], (r & 3) + 8 * (r >> 2) + 4 * half, 64);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) ad[r][ct] = off >= 0 ? addb[off + (ct0 + ct) * 32 + col] : 0.f;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[vt][ct][r] += ad[r][ct];
    }
  }
#pragma unroll
  for (int vt = 0; vt < VT; ++vt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
      const int off = __shfl(ooff[vt], row, 64);
      if (off >= 0) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) outb[off + (ct0 + ct) * 32 + col] = acc[vt][ct][r] + bv[ct];
      }
    }
  }
  if (a.ch_part) {
    float s1[CT], s2[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) s1[ct] = s2[ct] = 0.f;
#pragma unroll
    for (int vt = 0; vt < VT; ++vt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
        const bool ok = __shfl(ooff[vt], row, 64) >= 0;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const float v = ok ? acc[vt][ct][r] + bv[ct] : 0.f;
          s1[ct] += v;
          s2[ct] += v * v;
        }
      }
    __syncthreads();
    const int nw = nthreads >> 6;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const float t1 = s1[ct] + __shfl_xor(s1[ct], 32, 64), t2 = s2[ct] + __shfl_xor(s2[ct], 32, 64);
      if (half == 0) {
        lds[((wave * CT + ct) * 32 + col) * 2] = t1;
        lds[((wave * CT + ct) * 32 + col) * 2 + 1] = t2;
      }
    }
    __syncthreads();
    for (int i = tid; i < CT * 32; i += nthreads) {
      float t1 = 0.f, t2 = 0.f;
      for (int w = 0; w < nw; ++w) {
        t1 += lds[((w * CT * 32) + i) * 2];
        t2 += lds[((w * CT * 32) + i) * 2 + 1];
      }
      float* dst = a.ch_part + (((size_t)b * gridDim.x + blockIdx.x) * a.cout + ct0 * 32 + i) * 2;
      dst[0] = t1;
      dst[1] = t2;
    }
  }
}

namespace {
template <int VT, int CT, int KD, int KH, int KW, int SZ, int SXY, int NTERM>
void launch_flat3_geo(const ConvFlatArgs& a, dim3 grid, int threads, size_t lds, hipStream_t s) {
  static bool attr_set = false;
  if (!attr_set) {
    CD_HIP(hipFuncSetAttribute((const void*)conv3_flat_bf16x3_kernel<VT, CT, KD, KH, KW, SZ, SXY, NTERM>,
                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_set = true;
  }
  hipLaunchKernelGGL((conv3_flat_bf16x3_kernel<VT, CT, KD, KH, KW, SZ, SXY, NTERM>), grid, dim3(threads), lds, s, a);
  CD_HIP(hipGetLastError());
}
// geo: 0 = 3x3x3 stride 1, 1 = (3,4,4) stride (2,2,2), 2 = (3,4,4) stride (1,2,2), 3 = (4,4,4) stride (2,2,2)
template <int VT, int CT, int NTERM>
void launch_flat3_inst(const ConvFlatArgs& a, dim3 grid, int threads, size_t lds, hipStream_t s, int geo = 0) {
  if (geo == 0) launch_flat3_geo<VT, CT, 3, 3, 3, 1, 1, NTERM>(a, grid, threads, lds, s);
  else if (geo == 1) launch_flat3_geo<VT, CT, 3, 4, 4, 2, 2, NTERM>(a, grid, threads, lds, s);
  else if (geo == 2) launch_flat3_geo<VT, CT, 3, 4, 4, 1, 2, NTERM>(a, grid, threads, lds, s);
  else launch_flat3_geo<VT, CT, 4, 4, 4, 2, 2, NTERM>(a, grid, threads, lds, s);
}
}  // namespace

bool launch_conv_flat_split16(int VT, int CT, int NTERM, int geo, const ConvFlatArgs& a, dim3 grid, int threads, size_t lds, hipStream_t s) {
#define CD_FLAT_CASE(V, C)                                                                 \
  if (VT == V && CT == C) {                                                                \
    if (NTERM == 3) launch_flat3_inst<V, C, 3>(a, grid, threads, lds, s, geo);             \
    else if constexpr (V * C <= 4) launch_flat3_inst<V, C, 2>(a, grid, threads, lds, s, geo); \
    else return false;                                                                     \
    return true;                                                                           \
  }
  CD_FLAT_CASE(1, 1) CD_FLAT_CASE(2, 1) CD_FLAT_CASE(3, 1) CD_FLAT_CASE(4, 1)
  CD_FLAT_CASE(1, 2) CD_FLAT_CASE(2, 2) CD_FLAT_CASE(3, 2) CD_FLAT_CASE(4, 2)
  CD_FLAT_CASE(1, 3) CD_FLAT_CASE(2, 3)
#undef CD_FLAT_CASE
  return false;
}

}  // namespace cd
