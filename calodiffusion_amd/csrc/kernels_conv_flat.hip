// Flat-range 3x3x3 / strided convolution kernels for gfx950 (f32 MFMA, warp-specialised persistent bf16x3; the plain split-16
// kernel is in kernels_conv_flat16.hip) and the host code that picks a tiling among them; operand layout as in kernels_conv.hip.
#include "conv_internal.h"
#include "gn_defer.h"
#include <vector>

namespace cd {

// ------------------------------------------------------------------------------------------------------------
// 3x3x3 stride-1 conv, "flat range" variant (the hot kernel: 92 % of the model's FLOPs).
//
// A workgroup owns R = 32*NT consecutive voxels of ONE sample in flattened (z, phi, r) order, so every MFMA row tile is
// full whatever the grid extents are (45x16x9 has 144-voxel planes = 4.5 tiles).  It stages the z-planes that range
// touches (+1 halo plane each side, zero-filled outside the tensor) as WHOLE planes: phi wraps by index arithmetic,
// r edges are predicated to a zero slot, so no halo rows/columns are stored.  Input channels stream through LDS in
// 16-channel sub-chunks (64 B per voxel, XOR-swizzled 16-B slots => conflict-free ds_read_b128 without padding):
// ~46 KiB for R = 256 on Dataset-2, i.e. three workgroups per CU whose staging and MFMA phases overlap.
// The 27 taps are fully unrolled: weight fragments (1-KiB wave loads, L1/L2 resident) and LDS fragments of tap t+1
// are in flight while the 8*VT*CT MFMAs of tap t issue.
// Sub-chunk k' of a 32-channel chunk = channels [8k', 8k'+8) (lane half 0) and [16+8k', 16+8k'+8) (lane half 1), so the
// packed weight layout of kernels_conv.h is used unchanged (fragments q = 2k', 2k'+1).
// ------------------------------------------------------------------------------------------------------------
template <int VT, int CT>
__global__ void __launch_bounds__(512, (VT * CT <= 2 ? 3 : 2)) conv3_flat_kernel(ConvFlatArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x;
  const int b = blockIdx.y;
  const int ct0 = blockIdx.z * CT;
  const int HW = a.H * a.W;
  const int vox = a.D * HW;
  const int v0 = blockIdx.x * a.R;
  const int vend = min(v0 + a.R, vox);
  const int zA = v0 / HW - 1;
  const int zB = (vend - 1) / HW + 1;
  const int nstage = (zB - zA + 1) * HW;   // voxels staged per sub-chunk
  const int NZ = a.P * HW;                 // index of the all-zero voxel
  const int half = lane >> 5, col = lane & 31;
  if (tid < 16) lds[NZ * 16 + tid] = 0.f;

  // per-lane geometry of its voxel in each of the wave's VT row tiles
  int nb[VT], rowm[VT], rowp[VT], ooff[VT];
  unsigned wmask[VT];
  bool any_valid = false;
#pragma unroll
  for (int vt = 0; vt < VT; ++vt) {
    const int v = v0 + (wave * VT + vt) * 32 + col;
    const bool valid = v < vend;
    const int vv = valid ? v : v0;
    const int r = vv % HW;
    const int h = r / a.W, w = r - h * a.W;
    nb[vt] = vv - zA * HW;
    rowm[vt] = (h == 0 ? a.H - 1 : -1) * a.W;
    rowp[vt] = (h == a.H - 1 ? -(a.H - 1) : 1) * a.W;
    unsigned m = 0;
    if (valid) m = (w > 0 ? 1u : 0u) | 2u | (w + 1 < a.W ? 4u : 0u);
    wmask[vt] = m;
    ooff[vt] = valid ? v * a.cout : -1;
    any_valid |= valid;
  }
  const bool wave_active = __any(any_valid);

  f32x16 acc[VT][CT];
#pragma unroll
  for (int vt = 0; vt < VT; ++vt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[vt][ct][r] = 0.f;

  const int nsub = (a.c0 + a.c1) >> 4;
  const int gbase = zA * HW;  // global voxel index of LDS voxel 0
  const int nslots = nstage * 4;

  // LDS image: voxel n = 64 B = two 32-B pairs; pair (lane half) hp sits at ((hp ^ (n>>2)) & 1): 2-way conflicts at most
  // on the ds_read_b128 fragment reads, no padding.  A lane's two fragments are adjacent (immediate offset +16 B).
  auto frag_addr = [&](int n) -> const float* { return lds + n * 16 + ((half ^ (n >> 2)) & 1) * 8; };
  auto tap_voxel = [&](int vt, int tap) -> int {
    const int dz = tap / 9 - 1, dh = (tap / 3) % 3 - 1, dw = tap % 3 - 1;
    const int n = nb[vt] + dz * HW + (dh < 0 ? rowm[vt] : (dh > 0 ? rowp[vt] : 0)) + dw;
    return ((wmask[vt] >> (dw + 1)) & 1u) ? n : NZ;
  };

  for (int sc = 0; sc < nsub; ++sc) {
    const int chunk = sc >> 1, kq = sc & 1;
    const float* src;
    int ldc, coff;
    if (chunk * 32 < a.c0) {
      src = a.in0; ldc = a.c0; coff = chunk * 32;
    } else {
      src = a.in1; ldc = a.c1; coff = chunk * 32 - a.c0;
    }
    src += (size_t)b * vox * ldc + coff + kq * 8;
    // this thread always stages the same 4 channels of a sub-chunk (slot index mod 4 is tid mod 4)
    f32x4 cf[4];
    if (a.coef) {
      const int c = chunk * 32 + kq * 8 + ((tid & 3) >> 1) * 16 + (tid & 1) * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) cf[e] = *(const f32x4*)(a.coef + ((size_t)b * (a.c0 + a.c1) + c + e) * 4);
    }
    __syncthreads();
    // stage: 4 independent 16-B loads in flight per thread before the first LDS write
    for (int s0 = tid; s0 < ((a.dbg & 1) ? 0 : nslots); s0 += 4 * nthreads) {
      f32x4 val[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int sidx = s0 + k * nthreads;
        const int n = sidx >> 2, p = sidx & 3;
        const int g = gbase + n;
        val[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (sidx < nslots && g >= 0 && g < vox) {
          val[k] = *(const f32x4*)(src + (size_t)g * ldc + (p >> 1) * 16 + (p & 1) * 4);
          if (a.coef) {  // zero padding applies to the NORMALISED activation, so only in-range voxels are transformed
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
        const int n = sidx >> 2, p = sidx & 3;
        if (sidx < nslots) *(f32x4*)(lds + n * 16 + ((((p >> 1) ^ (n >> 2)) & 1) * 2 + (p & 1)) * 4) = val[k];
      }
    }
    __syncthreads();
    if (!wave_active || (a.dbg & 2)) continue;

    // keep the per-tap address arithmetic inside this loop (hoisting 27*VT addresses costs ~100 VGPRs)
#pragma unroll
    for (int vt = 0; vt < VT; ++vt) asm volatile("" : "+v"(nb[vt]));

    const f32x4* wq = (const f32x4*)a.wpk + ((size_t)chunk * 27 * a.CTtot + ct0) * 256 + kq * 128 + lane;
    // software pipeline over the 27 taps: fragments of tap t+1 are requested before the MFMAs of tap t issue
    f32x4 bw[2][CT][2], av[2][VT][2];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      bw[0][ct][0] = wq[(size_t)ct * 256];
      bw[0][ct][1] = wq[(size_t)ct * 256 + 64];
    }
#pragma unroll
    for (int vt = 0; vt < VT; ++vt) {
      const float* p = frag_addr(tap_voxel(vt, 0));
      av[0][vt][0] = *(const f32x4*)p;
      av[0][vt][1] = *(const f32x4*)(p + 4);
    }
#pragma unroll
    for (int tap = 0; tap < 27; ++tap) {
      const int cur = tap & 1, nxt = cur ^ 1;
      if (tap + 1 < 27) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          bw[nxt][ct][0] = wq[((size_t)(tap + 1) * a.CTtot + ct) * 256];
          bw[nxt][ct][1] = wq[((size_t)(tap + 1) * a.CTtot + ct) * 256 + 64];
        }
#pragma unroll
        for (int vt = 0; vt < VT; ++vt) {
          const float* p = frag_addr(tap_voxel(vt, tap + 1));
          av[nxt][vt][0] = *(const f32x4*)p;
          av[nxt][vt][1] = *(const f32x4*)(p + 4);
        }
      }
      __builtin_amdgcn_sched_barrier(0);  // keep the requests ahead of this tap's MFMAs (hipcc otherwise sinks them)
#pragma unroll
      for (int vt = 0; vt < VT; ++vt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[vt][ct] = MFMA32(av[cur][vt][0][e], bw[cur][ct][0][e], acc[vt][ct]);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[vt][ct] = MFMA32(av[cur][vt][1][e], bw[cur][ct][1][e], acc[vt][ct]);
        }
    }
  }

  float* outb = a.out + (size_t)b * vox * a.cout;
  float bv[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) bv[ct] = a.bias ? a.bias[(ct0 + ct) * 32 + col] : 0.f;
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
    // per-channel {sum, sum of squares} of this workgroup's outputs, reduced in a fixed order (deterministic)
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
    __syncthreads();  // every wave is done with the LDS tile
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

// ------------------------------------------------------------------------------------------------------------
// Warp-specialised, persistent variant of the bf16x3 flat conv.
//
// One workgroup per CU loops over its share of (sample, voxel-range) units.  NLW loader waves stage the NEXT
// 16-channel sub-chunk (global -> fused GroupNorm/SiLU -> exact bf16 split -> LDS buffer B) on the vector ALU while NMW
// matrix waves run the taps of the CURRENT sub-chunk out of LDS buffer A on the matrix pipe; one barrier per phase swaps
// the buffers.  Staging (VALU / LDS-write bound) and MFMAs (matrix-pipe bound) therefore overlap inside a CU instead of
// alternating, and the pipeline runs seamlessly across units (the first sub-chunk of unit u+1 is staged during the last
// phase of unit u).  Each matrix wave owns one 32-voxel row tile of the unit (R = 32*NMW voxels); the per-unit channel
// statistics are handed to the loader waves through a small LDS scratch and written by them one phase later.
// ------------------------------------------------------------------------------------------------------------
template <int CT, int KD, int KH, int KW, int SZ, int SXY>
__global__ void __launch_bounds__(768) conv_flat_ws_kernel(ConvFlatArgs a, int nlw, int units_per_sample, int total_units) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int T = KD * KH * KW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nmw = (blockDim.x >> 6) - nlw;
  const bool loader = wave < nlw;
  const int ct0 = blockIdx.z * CT;
  const int HW = a.H * a.W, vox = a.D * HW;
  const int HWo = a.Ho * a.Wo, voxo = a.Do * HWo;
  const int NZ = a.P * HW;
  const size_t buf_bytes = ((size_t)NZ + 1) * 96;
  char* bufp[2] = {(char*)lds, (char*)lds + buf_bytes};
  float* scratch = (float*)((char*)lds + 2 * buf_bytes);  // [nmw][CT*32][2]
  const int half = lane >> 5, col = lane & 31;
  const int nsub = (a.c0 + a.c1) >> 4;
  if (tid < 48) ((float*)(bufp[tid / 24] + (size_t)NZ * 96))[tid % 24] = 0.f;

  // units of this workgroup: u = blockIdx.x + k*gridDim.x
  const int my_units = (total_units - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
  const int nph = my_units * nsub;

  // ---- loader side ------------------------------------------------------------------------------------------
  auto stage = [&](int ph, char* dst) {
    const int u = blockIdx.x + (ph / nsub) * gridDim.x, sc = ph % nsub;
    const int b = u / units_per_sample, ux = u - b * units_per_sample;
    const int v0 = ux * a.R, vend = min(v0 + a.R, voxo);
    const int zA = (v0 / HWo) * SZ - 1, zB = ((vend - 1) / HWo) * SZ + KD - 2;
    const int nslots = (zB - zA + 1) * HW * 4, gbase = zA * HW;
    const float* src;
    int ldc, coff;
    if (sc * 16 < a.c0) {
      src = a.in0; ldc = a.c0; coff = sc * 16;
    } else {
      src = a.in1; ldc = a.c1; coff = sc * 16 - a.c0;
    }
    const int pq = tid & 3, nth = nlw * 64;
    src += (size_t)b * vox * ldc + coff + pq * 4;
    f32x4 cf[4];
    if (a.coef) {
#pragma unroll
      for (int e = 0; e < 4; ++e) cf[e] = *(const f32x4*)(a.coef + ((size_t)b * (a.c0 + a.c1) + sc * 16 + pq * 4 + e) * 4);
    }
    // all loads of a batch are issued before the first conversion: with only nlw waves loading, memory-level
    // parallelism (bytes in flight per CU), not issue rate, sets the staging time
    constexpr int LB = 12;
    for (int s0 = tid; s0 < nslots; s0 += LB * nth) {
      f32x4 val[LB];
#pragma unroll
      for (int k = 0; k < LB; ++k) {
        const int sidx = s0 + k * nth;
        const int g = gbase + (sidx >> 2);
        val[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (sidx < nslots && g >= 0 && g < vox) {
          val[k] = *(const f32x4*)(src + (size_t)g * ldc);
          if (a.coef) {
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
      for (int k = 0; k < LB; ++k) {
        const int sidx = s0 + k * nth;
        if (sidx < nslots) {
          u32x2 t1, t2, t3;
          split3(val[k], t1, t2, t3);
          char* d = dst + (size_t)(sidx >> 2) * 96 + pq * 8;
          *(u32x2*)d = t1;
          *(u32x2*)(d + 32) = t2;
          *(u32x2*)(d + 64) = t3;
        }
      }
    }
  };

  if (loader) stage(0, bufp[0]);
  __syncthreads();

  // ---- matrix-wave state --------------------------------------------------------------------------------------
  f32x16 acc[CT];
  int nb = 0, ooff = -1, rowoff[KH];
  unsigned wmask = 0;
  int cur_b = 0;

  for (int ph = 0; ph < nph; ++ph) {
    const int cur = ph & 1;
    const int sc = ph % nsub;
    if (loader) {
      if (ph + 1 < nph) stage(ph + 1, bufp[cur ^ 1]);
      // statistics of the unit that finished in the previous phase
      if (a.ch_part && sc == 0 && ph > 0) {
        const int u = blockIdx.x + (ph / nsub - 1) * gridDim.x;
        for (int i = tid; i < CT * 32; i += nlw * 64) {
          float t1 = 0.f, t2 = 0.f;
          for (int w = 0; w < nmw; ++w) {
            t1 += scratch[((w * CT * 32) + i) * 2];
            t2 += scratch[((w * CT * 32) + i) * 2 + 1];
          }
          float* dst = a.ch_part + ((size_t)u * a.cout + ct0 * 32 + i) * 2;  // u = b*units_per_sample + ux
          dst[0] = t1;
          dst[1] = t2;
        }
      }
    } else {
      const int mw = wave - nlw;
      if (sc == 0) {
        const int u = blockIdx.x + (ph / nsub) * gridDim.x;
        cur_b = u / units_per_sample;
        const int ux = u - cur_b * units_per_sample;
        const int v0 = ux * a.R, vend = min(v0 + a.R, voxo);
        const int zA = (v0 / HWo) * SZ - 1;
        const int v = v0 + mw * 32 + col;
        const bool valid = v < vend;
        const int vv = valid ? v : v0;
        const int oz = vv / HWo;
        const int r = vv - oz * HWo;
        const int oh = r / a.Wo, ow = r - oh * a.Wo;
        const int ih0 = oh * SXY, iw0 = ow * SXY;
        nb = (oz * SZ - 1 - zA) * HW + ih0 * a.W + iw0;
        unsigned m = 0;
#pragma unroll
        for (int kh = 0; kh < KH; ++kh) {
          int ih = ih0 + kh - 1;
          ih = ih < 0 ? ih + a.H : (ih >= a.H ? ih - a.H : ih);
          ih = ih >= a.H ? ih - a.H : ih;
          rowoff[kh] = (ih - ih0) * a.W;
        }
#pragma unroll
        for (int kw = 0; kw < KW; ++kw) {
          const int iw = iw0 + kw - 1;
          if (valid && iw >= 0 && iw < a.W) m |= 1u << kw;
        }
        wmask = m;
        ooff = valid ? v * a.cout : -1;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int r2 = 0; r2 < 16; ++r2) acc[ct][r2] = 0.f;
      }
      if (__any(ooff >= 0)) {
        const char* ldsb = bufp[cur];
        auto tap_ptr = [&](int tap) -> const char* {
          const int kz = tap / (KH * KW), kh = (tap / KW) % KH, kw = tap % KW;
          const int n = nb + kz * HW + rowoff[kh] + kw - 1;
          return ldsb + (size_t)(((wmask >> kw) & 1u) ? n : NZ) * 96 + half * 16;
        };
        asm volatile("" : "+v"(nb));
        const u32x4* wq = (const u32x4*)a.wpk + ((size_t)sc * T * a.CTtot + ct0) * 192 + lane;
        u32x4 bw[2][CT][3], av[2][3];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int t = 0; t < 3; ++t) bw[0][ct][t] = wq[(size_t)ct * 192 + t * 64];
        {
          const char* p = tap_ptr(0);
#pragma unroll
          for (int t = 0; t < 3; ++t) av[0][t] = *(const u32x4*)(p + t * 32);
        }
#pragma unroll
        for (int tap = 0; tap < T; ++tap) {
          const int c = tap & 1, nx = c ^ 1;
          if (tap + 1 < T) {
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
              for (int t = 0; t < 3; ++t) bw[nx][ct][t] = wq[((size_t)(tap + 1) * a.CTtot + ct) * 192 + t * 64];
            const char* p = tap_ptr(tap + 1);
#pragma unroll
            for (int t = 0; t < 3; ++t) av[nx][t] = *(const u32x4*)(p + t * 32);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            f32x16 cc = acc[ct];
            cc = MFMA_BF16(av[c][2], bw[c][ct][0], cc);
            cc = MFMA_BF16(av[c][1], bw[c][ct][1], cc);
            cc = MFMA_BF16(av[c][0], bw[c][ct][2], cc);
            cc = MFMA_BF16(av[c][1], bw[c][ct][0], cc);
            cc = MFMA_BF16(av[c][0], bw[c][ct][1], cc);
            cc = MFMA_BF16(av[c][0], bw[c][ct][0], cc);
            acc[ct] = cc;
          }
        }
      }
      if (sc == nsub - 1) {
        float* outb = a.out + (size_t)cur_b * voxo * a.cout;
        float bv[CT], s1[CT], s2[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          bv[ct] = a.bias ? a.bias[(ct0 + ct) * 32 + col] : 0.f;
          s1[ct] = s2[ct] = 0.f;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
          const int off = __shfl(ooff, row, 64);
          if (off >= 0) {
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
              const float v = acc[ct][r] + bv[ct];
              outb[off + (ct0 + ct) * 32 + col] = v;
              s1[ct] += v;
              s2[ct] += v * v;
            }
          }
        }
        if (a.ch_part) {
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            const float t1 = s1[ct] + __shfl_xor(s1[ct], 32, 64), t2 = s2[ct] + __shfl_xor(s2[ct], 32, 64);
            if (half == 0) {
              scratch[((mw * CT + ct) * 32 + col) * 2] = t1;
              scratch[((mw * CT + ct) * 32 + col) * 2 + 1] = t2;
            }
          }
        }
      }
    }
    __syncthreads();
  }
  // statistics of the last unit
  if (loader && a.ch_part && nph > 0) {
    const int u = blockIdx.x + (my_units - 1) * gridDim.x;
    for (int i = tid; i < CT * 32; i += nlw * 64) {
      float t1 = 0.f, t2 = 0.f;
      for (int w = 0; w < nmw; ++w) {
        t1 += scratch[((w * CT * 32) + i) * 2];
        t2 += scratch[((w * CT * 32) + i) * 2 + 1];
      }
      float* dst = a.ch_part + ((size_t)u * a.cout + ct0 * 32 + i) * 2;
      dst[0] = t1;
      dst[1] = t2;
    }
  }
}

namespace {
template <int CT, int KD, int KH, int KW, int SZ, int SXY>
void launch_ws_geo(const ConvFlatArgs& a, dim3 grid, int threads, size_t lds, int nlw, int ups, int total, hipStream_t s) {
  static bool attr_set = false;
  if (!attr_set) {
    CD_HIP(hipFuncSetAttribute((const void*)conv_flat_ws_kernel<CT, KD, KH, KW, SZ, SXY>,
                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_set = true;
  }
  hipLaunchKernelGGL((conv_flat_ws_kernel<CT, KD, KH, KW, SZ, SXY>), grid, dim3(threads), lds, s, a, nlw, ups, total);
  CD_HIP(hipGetLastError());
}
template <int CT>
void launch_ws_inst(const ConvFlatArgs& a, dim3 grid, int threads, size_t lds, int nlw, int ups, int total, hipStream_t s, int geo) {
  if (geo == 0) launch_ws_geo<CT, 3, 3, 3, 1, 1>(a, grid, threads, lds, nlw, ups, total, s);
  else if (geo == 1) launch_ws_geo<CT, 3, 4, 4, 2, 2>(a, grid, threads, lds, nlw, ups, total, s);
  else if (geo == 2) launch_ws_geo<CT, 3, 4, 4, 1, 2>(a, grid, threads, lds, nlw, ups, total, s);
  else launch_ws_geo<CT, 4, 4, 4, 2, 2>(a, grid, threads, lds, nlw, ups, total, s);
}

template <int VT, int CT>
void launch_flat_inst(const ConvFlatArgs& a, dim3 grid, int threads, size_t lds, hipStream_t s) {
  static bool attr_set = false;
  if (!attr_set) {
    CD_HIP(hipFuncSetAttribute((const void*)conv3_flat_kernel<VT, CT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_set = true;
  }
  hipLaunchKernelGGL((conv3_flat_kernel<VT, CT>), grid, dim3(threads), lds, s, a);
  CD_HIP(hipGetLastError());
}

bool launch_conv_flat_f32(int VT, int CT, const ConvFlatArgs& a, dim3 grid, int threads, size_t lds, hipStream_t s) {
#define CD_FLAT_CASE(V, C)                                   \
  if (VT == V && CT == C) {                                  \
    launch_flat_inst<V, C>(a, grid, threads, lds, s);        \
    return true;                                             \
  }
  CD_FLAT_CASE(1, 1) CD_FLAT_CASE(2, 1) CD_FLAT_CASE(3, 1) CD_FLAT_CASE(4, 1)
  CD_FLAT_CASE(1, 2) CD_FLAT_CASE(2, 2) CD_FLAT_CASE(3, 2) CD_FLAT_CASE(4, 2)
  CD_FLAT_CASE(1, 3) CD_FLAT_CASE(2, 3)
#undef CD_FLAT_CASE
  return false;
}
}  // namespace

bool try_launch_conv3_flat(const float* in0, int c0, const float* in1, int c1, const void* wpk, const float* bias, float* out,
                           int batch, int cout, const ConvGeom& g, hipStream_t s, const ConvFusion& fu, int prec) {
  const bool bf16x3 = prec != 0;  // any 16-bit split kernel
  if (getenv("CD_NO_FLAT")) return false;
  int geo = -1;
  if (g.kd == 3 && g.kh == 3 && g.kw == 3 && g.sz == 1 && g.sh == 1 && g.sw == 1) geo = 0;
  else if (g.kd == 3 && g.kh == 4 && g.kw == 4 && g.sh == 2 && g.sw == 2 && (g.sz == 1 || g.sz == 2)) geo = g.sz == 2 ? 1 : 2;
  else if (g.kd == 4 && g.kh == 4 && g.kw == 4 && g.sh == 2 && g.sw == 2 && g.sz == 2) geo = 3;  // input gradient of an up conv
  if (geo < 0 || (geo != 0 && !bf16x3)) return false;
  const Dims3 d = g.in;
  const int CTtot = cout / 32;
  const int CTmax = CTtot <= 3 ? CTtot : 2;
  if (CTtot % CTmax) return false;
  const int HW = d.h * d.w, HWo = g.out.h * g.out.w;
  const size_t vox_bytes = prec == 3 ? 96 : (prec == 2 ? 80 : 64);
  auto planes = [&](int NT) { return ((32 * NT - 1) / HWo + 1) * g.sz + g.kd; };
  // what every flat-range launch is told: sources, geometry, the NT-tile range of a workgroup, the fused input coefficients and
  // output statistics.  status, in_absmax, add_src and defer keep their defaults (off); dbg is the caller's to set
  auto args_for = [&](int NT) {
    ConvFlatArgs a;
    a.in0 = in0; a.in1 = in1; a.c0 = c0; a.c1 = c1; a.wpk = (const float*)wpk; a.bias = bias; a.out = out;
    a.D = d.d; a.H = d.h; a.W = d.w; a.Do = g.out.d; a.Ho = g.out.h; a.Wo = g.out.w;
    a.R = 32 * NT; a.P = planes(NT); a.cout = cout; a.CTtot = CTtot;
    a.coef = fu.coef; a.act = fu.act; a.ch_part = fu.ch_part;
    return a;
  };
  // CT = output-channel tiles per workgroup: CTmax shares one staged input tile between them; 1 spreads them over
  // gridDim.z (shorter MFMA chains: wins on the deep, latency-bound levels)
  auto launch = [&](int NT, int VT, int CT) -> bool {
    if (VT < 0) {  // warp-specialised persistent kernel
      const int NLW = -VT;
      ConvFlatArgs a = args_for(NT);
      a.dbg = 0;
      const size_t lds = 2 * ((size_t)a.P * HW + 1) * 96 + (size_t)NT * CT * 64 * 4;
      const int ups = (int)((g.out.vox() + a.R - 1) / a.R);
      const int total = ups * batch;
      const int nblk = total < 256 ? total : 256;
      dim3 grid((unsigned)nblk, 1, (unsigned)(CTtot / CT));
      if (fu.units) *fu.units = ups;
      const int threads = (NT + NLW) * 64;
      switch (CT) {
        case 1: launch_ws_inst<1>(a, grid, threads, lds, NLW, ups, total, s, geo); break;
        case 2: launch_ws_inst<2>(a, grid, threads, lds, NLW, ups, total, s, geo); break;
        case 3: launch_ws_inst<3>(a, grid, threads, lds, NLW, ups, total, s, geo); break;
        default: return false;
      }
      return true;
    }
    ConvFlatArgs a = args_for(NT);
    a.dbg = getenv("CD_FLAT_DBG") ? atoi(getenv("CD_FLAT_DBG")) : 0;
    a.status = fu.status; a.in_absmax = fu.in_absmax;
    a.add_src = prec >= 2 && !bias ? fu.add_src : nullptr;  // (the split-16 kernels only: the caller adds the tensor itself otherwise)
    size_t lds = ((size_t)a.P * HW + 1) * vox_bytes;
    const size_t red = (size_t)(NT / VT) * CT * 32 * 2 * 4;  // cross-wave reduction scratch of the stats epilogue
    if (lds < red) lds = red;
    if (fu.defer.part) {  // (only reached with prec != 0: launch_conv_mfma materialises the table for the f32 kernels)
      lds = (lds + 15) & ~(size_t)15;
      a.defer = fu.defer;
      a.coef_lds_off = (int)lds;
      lds += (size_t)fu.defer.C * 16 + gn_defer_scratch_bytes(fu.defer.C);
      if (lds > 160 * 1024) return false;
    }
    dim3 grid((unsigned)((g.out.vox() + a.R - 1) / a.R), (unsigned)batch, (unsigned)(CTtot / CT));
    if (fu.units) *fu.units = (int)grid.x;
    const int threads = (NT / VT) * 64;
    const bool launched = prec != 0 ? launch_conv_flat_split16(VT, CT, prec, geo, a, grid, threads, lds, s)
                                    : launch_conv_flat_f32(VT, CT, a, grid, threads, lds, s);
    if (!launched) return false;  // no kernel instance for that tiling
    if (a.add_src && fu.add_done) *fu.add_done = 1;
    return true;
  };
  if (const char* ov = getenv("CD_FLAT_TILE")) {
    int nt, vt;
    if (sscanf(ov, "%d,%d", &nt, &vt) == 2 && nt % vt == 0 && nt / vt <= 8 && vt * CTmax <= 8 &&
        ((size_t)planes(nt) * HW + 1) * vox_bytes <= 160 * 1024 && (prec != 2 || vt * CTmax <= 4))
      return launch(nt, vt, CTmax);
  }
  // candidate tilings: (tiles per workgroup, tiles per wave)
  static const int kCand[][2] = {{8, 2}, {4, 1}, {8, 1}, {12, 3}, {16, 2}, {16, 4}, {4, 2}, {6, 2}, {6, 3}, {2, 1},
                                 {3, 1}, {1, 1}, {2, 2}, {12, 2}, {8, 4}, {6, 1}, {3, 3}};
  struct Cand { int nt, vt, ct; };
  std::vector<Cand> cand;
  const bool small = g.out.vox() * batch <= 64 * 1024;  // deep levels: also try one output tile per workgroup
  for (int pass = 0; pass < (small && CTmax > 1 ? 2 : 1); ++pass) {
    const int CT = pass == 0 ? CTmax : 1;
    for (auto& c : kCand) {
      const int NT = c[0], VT = c[1];
      if (VT * CT > 8 || (CT == 3 && VT > 2)) continue;
      if (prec == 2 && VT * CT > 4) continue;
      // (more row tiles than the sample has: skipped -- except one tile per wave on grids of <= 128 output voxels, where the
      // surplus waves have no rows but share the staging, whose few threads are the latency of such launches)
      static const bool no_extra_waves = getenv("CD_FLAT_NO_EXTRA_WAVES") != nullptr;
      const bool extra_ok = !no_extra_waves && g.out.vox() <= 128 && VT == 1 && NT <= 8;
      if ((int64_t)32 * (NT - 1) >= g.out.vox() && !extra_ok) continue;
      if (((size_t)planes(NT) * HW + 1) * vox_bytes > 150 * 1024) continue;
      if (pass == 1 && NT > 4) continue;
      cand.push_back({NT, VT, CT});
    }
  }
  if (prec == 3 && !getenv("CD_NO_WS")) {
    // warp-specialised persistent variants: (matrix waves, -loader waves); two LDS buffers + statistics scratch
    static const int kWs[][2] = {{8, 4}, {8, 2}, {4, 2}, {4, 4}, {8, 3}, {6, 2}, {2, 2}, {3, 1}, {1, 1}, {2, 1}};
    for (auto& c : kWs) {
      const int NMW = c[0], NLW = c[1];
      if ((int64_t)32 * (NMW - 1) >= g.out.vox()) continue;
      const size_t lds = 2 * ((size_t)planes(NMW) * HW + 1) * 96 + (size_t)NMW * CTmax * 64 * 4;
      if (lds > 160 * 1024 - 256) continue;
      cand.push_back({NMW, -NLW, CTmax});
    }
  }
  if (cand.empty()) return false;
  char key[192];
  std::snprintf(key, sizeof key, "flat%s g%d %dx%dx%d c%d+%d->%d b%d", prec == 3 ? "_bf16x3" : (prec == 2 ? "_f16x2" : "_f32"), geo,
                d.d, d.h, d.w, c0, c1, cout, batch);
  const int pick = autotune(key, (int)cand.size(), [&](int i) { launch(cand[i].nt, cand[i].vt, cand[i].ct); }, s);
  const Cand& c = cand[pick < 0 ? 0 : pick];
  return launch(c.nt, c.vt, c.ct);
}

}  // namespace cd
