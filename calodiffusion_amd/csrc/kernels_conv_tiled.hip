// Halo-tiled convolution kernels for gfx950: a workgroup owns an output tile (TZ, TH, full r) and stages its input tile with the
// phi halo rows (wrapped) and z halo planes (zero-filled).  The f32 MFMA form (see kernels_conv.hip for the operand layout) and the
// 16-bit split forms; launch_conv_mfma falls back to them where the flat-range kernels do not fit.
#include "conv_internal.h"

namespace cd {

template <int VT, int CT>
__global__ void __launch_bounds__(512) conv_mfma_kernel(ConvKArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x;
  int bid = blockIdx.x;
  const int thi = bid % a.nTH;
  bid /= a.nTH;
  const int tzi = bid % a.nTZ;
  const int b = bid / a.nTZ;
  const int ct0 = blockIdx.y * CT;
  const int oz0 = tzi * a.TZ, oh0 = thi * a.TH;
  const int tileVox = a.IZ * a.IH * a.Win;
  const int ZERO = tileVox * 36;
  const int half = lane >> 5, col = lane & 31;
  if (tid < 36) lds[ZERO + tid] = 0.f;

  int abase[VT], ooff[VT];
  unsigned wmask[VT];
  bool any_valid = false;
#pragma unroll
  for (int vt = 0; vt < VT; ++vt) {
    const int v = (wave * VT + vt) * 32 + col;
    const int ow = v % a.Wo;
    const int t = v / a.Wo;
    const int oh = t % a.TH, oz = t / a.TH;
    const bool valid = (oz < a.TZ) && (oz0 + oz < a.Do) && (oh0 + oh < a.Ho);
    abase[vt] = ((oz * a.SZ * a.IH + oh * a.SH) * a.Win + ow * a.SW - 1) * 36 + half * 16;
    unsigned m = 0;
    for (int kw = 0; kw < a.KW; ++kw) {
      const int iw = ow * a.SW + kw - 1;
      if (valid && iw >= 0 && iw < a.Win) m |= 1u << kw;
    }
    wmask[vt] = m;
    ooff[vt] = valid ? (((oz0 + oz) * a.Ho + oh0 + oh) * a.Wo + ow) * a.cout : -1;
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

  const int nchunk = (a.c0 + a.c1) >> 5;
  const int T = a.KD * a.KH * a.KW;
  const int gz0 = oz0 * a.SZ - 1, gh0 = oh0 * a.SH - 1;
  const int items = tileVox * 8;
  const size_t in_vox = (size_t)a.Din * a.Hin * a.Win;

  for (int chunk = 0; chunk < nchunk; ++chunk) {
    const float* src;
    int ldc, coff;
    if (chunk * 32 < a.c0) {
      src = a.in0; ldc = a.c0; coff = chunk * 32;
    } else {
      src = a.in1; ldc = a.c1; coff = chunk * 32 - a.c0;
    }
    src += (size_t)b * in_vox * ldc + coff;
    __syncthreads();  // all reads of the previous chunk's tile are done
    for (int idx = tid; idx < items; idx += nthreads) {
      const int q = idx & 7, vox = idx >> 3;
      const int iw = vox % a.Win;
      const int r = vox / a.Win;
      const int ih = r % a.IH, iz = r / a.IH;
      const int gz = gz0 + iz;
      int gh = (gh0 + ih) % a.Hin;
      if (gh < 0) gh += a.Hin;
      f32x4 val = {0.f, 0.f, 0.f, 0.f};
      if (gz >= 0 && gz < a.Din) {
        val = *(const f32x4*)(src + ((size_t)(gz * a.Hin + gh) * a.Win + iw) * ldc + q * 4);
        if (a.coef) {
          const float* cfp = a.coef + ((size_t)b * (a.c0 + a.c1) + chunk * 32 + q * 4) * 4;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const f32x4 cf = *(const f32x4*)(cfp + e * 4);
            float t = cf[0] * val[e] + cf[1];
            if (a.act) t = cd_fast_silu(t);
            val[e] = t + cf[2];
          }
        }
      }
      *(f32x4*)(lds + vox * 36 + q * 4) = val;
    }
    __syncthreads();
    if (!wave_active) continue;

    const f32x4* wq = (const f32x4*)a.wpk + (size_t)chunk * T * a.CTtot * 256 + lane;
    for (int kd = 0; kd < a.KD; ++kd) {
      for (int kh = 0; kh < a.KH; ++kh) {
        const int rowoff = (kd * a.IH + kh) * a.Win * 36;
        for (int kw = 0; kw < a.KW; ++kw) {
          const int tap = (kd * a.KH + kh) * a.KW + kw;
          f32x4 bw[CT][4];
#pragma unroll
          for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int q = 0; q < 4; ++q) bw[ct][q] = wq[((size_t)tap * a.CTtot + ct0 + ct) * 256 + q * 64];
#pragma unroll
          for (int vt = 0; vt < VT; ++vt) {
            const int off = ((wmask[vt] >> kw) & 1u) ? abase[vt] + rowoff + kw * 36 : ZERO + half * 16;
            f32x4 av[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) av[q] = *(const f32x4*)(lds + off + q * 4);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
              for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[vt][ct] = MFMA32(av[q][e], bw[ct][q][e], acc[vt][ct]);
          }
        }
      }
    }
  }

  // epilogue: C/D layout of the 32x32 tile: column (output channel) = lane&31, row (voxel) = (r&3) + 8*(r>>2) + 4*(lane>>5)
  float* outb = a.out + (size_t)b * a.Do * a.Ho * a.Wo * a.cout;
#pragma unroll
  for (int vt = 0; vt < VT; ++vt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
      const int off = __shfl(ooff[vt], row, 64);
      if (off >= 0) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const int co = (ct0 + ct) * 32 + col;
          const float bv = a.bias ? a.bias[co] : 0.f;
          outb[off + co] = acc[vt][ct][r] + bv;
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------
// (TZ, TH) halo-tiled bf16x3 conv: same split-bf16 arithmetic as conv3_flat_bf16x3_kernel for grids whose z-planes are
// too wide for the whole-plane LDS image (Dataset-3 level 0: 50x18 = 900-voxel planes).  Tile geometry as in
// conv_mfma_kernel: output tile (TZ, TH, full r), staged input tile with phi halo rows (wrapped) and z halo planes
// (zero-filled); 96 B per voxel per 16-channel sub-chunk; runtime tap loop.
// ------------------------------------------------------------------------------------------------------------
// NTERM = 3: bf16x3; NTERM = 2: f16x2 (split16.h: 64 B + 16 B pad per voxel and sub-chunk, two accumulators per tile folded after
// the K loop, fp16 range flag) -- the arithmetic of the other f16x2 kernels for the convs only this tiling fits (Dataset-3's
// down-sampling conv out of 50x18 planes: 370 us per launch as bf16x3).
template <int VT, int CT, int NTERM>
__global__ void __launch_bounds__(512, (VT * CT * (NTERM == 2 ? 2 : 1) <= 2 ? 3 : 2)) conv_tiled_bf16x3_kernel(ConvTiled3Args args) {
  constexpr int VB = NTERM == 3 ? 96 : 80;  // bytes per staged voxel
  constexpr int WS = 64 * NTERM;            // u32x4 per (tap, ct) in the packed weights
  extern __shared__ __attribute__((aligned(16))) float lds[];
  char* ldsb = (char*)lds;
  const ConvKArgs& a = args.k;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x;
  int bid = blockIdx.x;
  const int thi = bid % a.nTH;
  bid /= a.nTH;
  const int tzi = bid % a.nTZ;
  const int b = bid / a.nTZ;
  const int ct0 = blockIdx.y * CT;
  const int oz0 = tzi * a.TZ, oh0 = thi * a.TH;
  const int tileVox = a.IZ * a.IH * a.Win;
  const int ZERO = tileVox * VB;  // byte offset of the all-zero voxel
  const int half = lane >> 5, col = lane & 31;
  if (tid < 24) ((float*)(ldsb + ZERO))[tid] = 0.f;

  int abase[VT], ooff[VT];
  unsigned wmask[VT];
  bool any_valid = false;
#pragma unroll
  for (int vt = 0; vt < VT; ++vt) {
    const int v = (wave * VT + vt) * 32 + col;
    const int ow = v % a.Wo;
    const int t = v / a.Wo;
    const int oh = t % a.TH, oz = t / a.TH;
    const bool valid = (oz < a.TZ) && (oz0 + oz < a.Do) && (oh0 + oh < a.Ho);
    abase[vt] = ((oz * a.SZ * a.IH + oh * a.SH) * a.Win + ow * a.SW - 1) * VB + half * 16;
    unsigned m = 0;
    for (int kw = 0; kw < a.KW; ++kw) {
      const int iw = ow * a.SW + kw - 1;
      if (valid && iw >= 0 && iw < a.Win) m |= 1u << kw;
    }
    wmask[vt] = m;
    ooff[vt] = valid ? (((oz0 + oz) * a.Ho + oh0 + oh) * a.Wo + ow) * a.cout : -1;
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

  const int nsub = (a.c0 + a.c1) >> 4;
  const int T = a.KD * a.KH * a.KW;
  const int gz0 = oz0 * a.SZ - 1, gh0 = oh0 * a.SH - 1;
  const int items = tileVox * 4;
  const size_t in_vox = (size_t)a.Din * a.Hin * a.Win;

  for (int sc = 0; sc < nsub; ++sc) {
    const float* src;
    int ldc, coff;
    if (sc * 16 < a.c0) {
      src = a.in0; ldc = a.c0; coff = sc * 16;
    } else {
      src = a.in1; ldc = a.c1; coff = sc * 16 - a.c0;
    }
    const int pq = tid & 3;
    src += (size_t)b * in_vox * ldc + coff + pq * 4;
    f32x4 cf[4];
    if (a.coef) {
#pragma unroll
      for (int e = 0; e < 4; ++e) cf[e] = *(const f32x4*)(a.coef + ((size_t)b * (a.c0 + a.c1) + sc * 16 + pq * 4 + e) * 4);
    }
    __syncthreads();
    // a thread keeps its channel quad (pq) and walks the tile's voxels in steps of nthreads / 4, four voxels per trip with their loads
    // in flight together; each voxel's (iw, ih, iz) advances by one trip's stride with carries -- five integer divisions by
    // run-time values per item (~40 instructions each) were most of this loop
    {
      const int vq = nthreads >> 2;          // voxels between a thread's slots
      int viw[4], vih[4], viz[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int vox = (tid >> 2) + k * vq;
        viw[k] = vox % a.Win;
        const int r = vox / a.Win;
        vih[k] = r % a.IH;
        viz[k] = r / a.IH;
      }
      const int DW = nthreads % a.Win, dr = nthreads / a.Win, DH = dr % a.IH, DZ = dr / a.IH;  // one trip = nthreads voxels on
      for (int i0 = tid; i0 < items; i0 += 4 * nthreads) {
        f32x4 val[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int idx = i0 + k * nthreads;
          val[k] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (idx < items) {
            const int gz = gz0 + viz[k];
            int gh = gh0 + vih[k];  // (circular in phi: gh0 >= -1, the tile's rows reach at most Hin - 1 + its halo)
            gh = gh < 0 ? gh + a.Hin : gh;
            gh = gh >= a.Hin ? gh - a.Hin : gh;
            gh = gh >= a.Hin ? gh - a.Hin : gh;
            if (gz >= 0 && gz < a.Din) {
              val[k] = *(const f32x4*)(src + ((size_t)(gz * a.Hin + gh) * a.Win + viw[k]) * ldc);
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
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int idx = i0 + k * nthreads;
          if (idx < items) {
            char* d = ldsb + (size_t)(idx >> 2) * VB + pq * 8;
            if (NTERM == 3) {
              u32x2 t1, t2, t3;
              split3(val[k], t1, t2, t3);
              *(u32x2*)d = t1;
              *(u32x2*)(d + 32) = t2;
              *(u32x2*)(d + 64) = t3;
            } else {
              amax = fmaxf(amax, fmaxf(fmaxf(fabsf(val[k][0]), fabsf(val[k][1])), fmaxf(fabsf(val[k][2]), fabsf(val[k][3]))));
              u32x2 t1, t2;
              split2(val[k], t1, t2);
              *(u32x2*)d = t1;
              *(u32x2*)(d + 32) = t2;
            }
          }
          viw[k] += DW; vih[k] += DH; viz[k] += DZ;
          if (viw[k] >= a.Win) { viw[k] -= a.Win; vih[k] += 1; }
          if (vih[k] >= a.IH) { vih[k] -= a.IH; viz[k] += 1; }
        }
      }
    }
    __syncthreads();
    if (!wave_active) continue;

    const u32x4* wq = (const u32x4*)a.wpk + ((size_t)sc * T * a.CTtot + ct0) * WS + lane;
    // The taps as one flat sequence, software-pipelined over a ring of three weight sets: the (L2) weight loads of tap t + 2 are
    // requested before the MFMAs of tap t.  (Loaded inside the tap they were an L2 round trip per VT x CT MFMA blocks.)  Requests
    // past the end repeat the last tap instead of being conditional.
    u32x4 bw0[CT][NTERM], bw1[CT][NTERM], bw2[CT][NTERM];
    auto loadw = [&](u32x4 (&bw)[CT][NTERM], int tap) {
      const int tc = min(tap, T - 1);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int t = 0; t < NTERM; ++t) bw[ct][t] = wq[((size_t)tc * a.CTtot + ct) * WS + t * 64];
    };
    int kd = 0, kh = 0, kw = 0;  // of the tap whose MFMAs run next
    auto run_tap = [&](const u32x4 (&bw)[CT][NTERM]) {
      const int rowoff = (kd * a.IH + kh) * a.Win * VB;
#pragma unroll
      for (int vt = 0; vt < VT; ++vt) {
        const int off = ((wmask[vt] >> kw) & 1u) ? abase[vt] + rowoff + kw * VB : ZERO + half * 16;
        u32x4 av[NTERM];
#pragma unroll
        for (int t = 0; t < NTERM; ++t) av[t] = *(const u32x4*)(ldsb + off + t * 32);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          if (NTERM == 3) {
            f32x16 c = acc[vt][ct];
            c = MFMA_BF16(av[2], bw[ct][0], c);
            c = MFMA_BF16(av[NTERM - 2], bw[ct][NTERM - 2], c);
            c = MFMA_BF16(av[0], bw[ct][NTERM - 1], c);
            c = MFMA_BF16(av[NTERM - 2], bw[ct][0], c);
            c = MFMA_BF16(av[0], bw[ct][NTERM - 2], c);
            c = MFMA_BF16(av[0], bw[ct][0], c);
            acc[vt][ct] = c;
          } else {
            acc[vt][ct] = MFMA_F16(av[0], bw[ct][0], acc[vt][ct]);
            accB[vt][ct] = MFMA_F16(av[0], bw[ct][NTERM - 1], accB[vt][ct]);
            accB[vt][ct] = MFMA_F16(av[NTERM - 1], bw[ct][0], accB[vt][ct]);
          }
        }
      }
      if (++kw == a.KW) { kw = 0; if (++kh == a.KH) { kh = 0; ++kd; } }
    };
    loadw(bw0, 0);
    loadw(bw1, 1);
    for (int tap = 0; tap < T; tap += 3) {
      loadw(bw2, tap + 2);
      __builtin_amdgcn_sched_barrier(0);
      run_tap(bw0);
      __builtin_amdgcn_sched_barrier(0);
      loadw(bw0, tap + 3);
      __builtin_amdgcn_sched_barrier(0);
      if (tap + 1 < T) run_tap(bw1);
      __builtin_amdgcn_sched_barrier(0);
      loadw(bw1, tap + 4);
      __builtin_amdgcn_sched_barrier(0);
      if (tap + 2 < T) run_tap(bw2);
    }
  }

  if (NTERM == 2) {
#pragma unroll
    for (int vt = 0; vt < VT; ++vt)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[vt][ct][r] += accB[vt][ct][r] * (1.f / 2048.f);
    if (args.status && amax > 65504.f) atomicOr(args.status, 1);
  }
  float* outb = a.out + (size_t)b * a.Do * a.Ho * a.Wo * a.cout;
  float bv[CT], s1[CT], s2[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    bv[ct] = a.bias ? a.bias[(ct0 + ct) * 32 + col] : 0.f;
    s1[ct] = s2[ct] = 0.f;
  }
#pragma unroll
  for (int vt = 0; vt < VT; ++vt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
      const int off = __shfl(ooff[vt], row, 64);
      if (off >= 0) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const float v = acc[vt][ct][r] + bv[ct];
          outb[off + (ct0 + ct) * 32 + col] = v;
          s1[ct] += v;
          s2[ct] += v * v;
        }
      }
    }
  }
  if (args.ch_part) {
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
    const int unit = tzi * a.nTH + thi, units = a.nTZ * a.nTH;
    for (int i = tid; i < CT * 32; i += nthreads) {
      float t1 = 0.f, t2 = 0.f;
      for (int w = 0; w < nw; ++w) {
        t1 += lds[((w * CT * 32) + i) * 2];
        t2 += lds[((w * CT * 32) + i) * 2 + 1];
      }
      float* dst = args.ch_part + (((size_t)b * units + unit) * a.cout + ct0 * 32 + i) * 2;
      dst[0] = t1;
      dst[1] = t2;
    }
  }
}

namespace {
template <int VT, int CT>
void launch_conv_inst(const ConvKArgs& a, dim3 grid, int threads, size_t lds, hipStream_t s) {
  static bool attr_set = false;
  if (!attr_set) {
    CD_HIP(hipFuncSetAttribute((const void*)conv_mfma_kernel<VT, CT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_set = true;
  }
  hipLaunchKernelGGL((conv_mfma_kernel<VT, CT>), grid, dim3(threads), lds, s, a);
  CD_HIP(hipGetLastError());
}

template <int VT, int CT, int NTERM = 3>
void launch_tiled3_inst(const ConvTiled3Args& a, dim3 grid, int threads, size_t lds, hipStream_t s) {
  static bool attr_set = false;
  if (!attr_set) {
    CD_HIP(hipFuncSetAttribute((const void*)conv_tiled_bf16x3_kernel<VT, CT, NTERM>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_set = true;
  }
  hipLaunchKernelGGL((conv_tiled_bf16x3_kernel<VT, CT, NTERM>), grid, dim3(threads), lds, s, a);
  CD_HIP(hipGetLastError());
}
}  // namespace

void launch_conv_tiled_f32(int VT, int CT, const ConvKArgs& a, dim3 grid, int threads, size_t lds, hipStream_t s) {
#define CD_CONV_CASE(V, C)                                        \
  if (VT == V && CT == C) {                                       \
    launch_conv_inst<V, C>(a, grid, threads, lds, s);             \
    return;                                                       \
  }
  CD_CONV_CASE(1, 1) CD_CONV_CASE(2, 1) CD_CONV_CASE(3, 1) CD_CONV_CASE(4, 1)
  CD_CONV_CASE(5, 1) CD_CONV_CASE(6, 1) CD_CONV_CASE(7, 1) CD_CONV_CASE(8, 1)
  CD_CONV_CASE(1, 2) CD_CONV_CASE(2, 2) CD_CONV_CASE(3, 2) CD_CONV_CASE(4, 2)
  CD_CONV_CASE(1, 3) CD_CONV_CASE(2, 3)
#undef CD_CONV_CASE
  CD_REQUIRE(false, "conv: no kernel instance for the chosen tiling");
}

void launch_conv_tiled_split16(int VT, int CT, int NTERM, const ConvTiled3Args& a, dim3 grid, int threads, size_t lds, hipStream_t s) {
  if (NTERM == 2) {  // two accumulators per tile: at most two tiles per wave
    if (VT == 1 && CT == 1) { launch_tiled3_inst<1, 1, 2>(a, grid, threads, lds, s); return; }
    if (VT == 2 && CT == 1) { launch_tiled3_inst<2, 1, 2>(a, grid, threads, lds, s); return; }
    if (VT == 1 && CT == 2) { launch_tiled3_inst<1, 2, 2>(a, grid, threads, lds, s); return; }
    CD_REQUIRE(false, "conv: no f16x2 tiled kernel instance for the chosen tiling");
  }
#define CD_T3_CASE(V, C)                                              \
  if (VT == V && CT == C) {                                           \
    launch_tiled3_inst<V, C>(a, grid, threads, lds, s);               \
    return;                                                           \
  }
  CD_T3_CASE(1, 1) CD_T3_CASE(2, 1) CD_T3_CASE(3, 1) CD_T3_CASE(4, 1)
  CD_T3_CASE(1, 2) CD_T3_CASE(2, 2) CD_T3_CASE(3, 2) CD_T3_CASE(4, 2)
  CD_T3_CASE(1, 3) CD_T3_CASE(2, 3)
#undef CD_T3_CASE
  CD_REQUIRE(false, "conv: no bf16x3 tiled kernel instance for the chosen tiling");
}

}  // namespace cd
