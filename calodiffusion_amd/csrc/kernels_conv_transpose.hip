// Transposed convolution (Upsample) for gfx950, f32 MFMA and f16x2 forms; operand layout as in kernels_conv.hip.
#include "conv_internal.h"
#include <algorithm>
#include <vector>

namespace cd {

static constexpr int LDS_VOX_PAD = 4;  // floats of padding per LDS voxel: stride 36/68/100 words => conflict-free ds_read_b128

// ------------------------------------------------------------------------------------------------------------
// transposed conv (Upsample): gather form, output voxels grouped by stride-parity class so that all 32 voxels of an
// MFMA tile share one set of valid taps.
//   out[o] = sum_k in[(o + pad - k)/s] * w[ci][co][k]   over k with (o + pad - k) % s == 0
//   pad = (1, kH-1 after a circular halo of 1, 1)  (models.py:45,59-61)
// ------------------------------------------------------------------------------------------------------------
struct ConvTArgs {
  const float* in;
  int cin;
  const float* wpk;
  const float* bias;
  float* out;
  int Din, Hin, Win, Do, Ho, Wo;
  int KZ, SZ;
  int cout, CTtot;
  int TZ, TH, nTZ, nTH;  // tile extents in class-index space: oz = SZ*a + pz, oh = 2*b + ph
  int Cw;                // ceil(Wo/2)
  int CS;                // LDS voxel stride in floats
  const u32x4* wpk16;    // f16x2 image [k-step][tap][ct][term][lane] (conv_transpose_f16x2_kernel)
  int* status;           // bit 0: a staged value exceeded the fp16 range
  const unsigned* in_absmax;  // power-of-two input rescaling (gradients: ConvFusion::in_absmax) or null
  int tr_off = 0;             // (f16x2 kernel) float offset of the per-wave output transpose tiles behind the input tile
};

template <int CT>
__global__ void __launch_bounds__(256) conv_transpose_kernel(ConvTArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  int bid = blockIdx.x;
  const int thi = bid % a.nTH;
  bid /= a.nTH;
  const int tzi = bid % a.nTZ;
  const int b = bid / a.nTZ;
  const int a0 = tzi * a.TZ, b0 = thi * a.TH;
  const int PZ = a.TZ + 2, PH = a.TH + 2;
  const int tileVox = PZ * PH * a.Win;
  const int ZERO = tileVox * a.CS;
  const int half = lane >> 5, col = lane & 31;
  for (int i = tid; i < a.CS; i += blockDim.x) lds[ZERO + i] = 0.f;

  // stage all input channels of the haloed tile
  {
    const int c4 = a.cin >> 2;
    const int items = tileVox * c4;
    const float* src = a.in + (size_t)b * a.Din * a.Hin * a.Win * a.cin;
    for (int idx = tid; idx < items; idx += blockDim.x) {
      const int q = idx % c4, vox = idx / c4;
      const int iw = vox % a.Win;
      const int r = vox / a.Win;
      const int lh = r % PH, lz = r / PH;
      const int gz = a0 - 1 + lz;
      int gh = (b0 - 1 + lh) % a.Hin;
      if (gh < 0) gh += a.Hin;
      f32x4 val = {0.f, 0.f, 0.f, 0.f};
      if (gz >= 0 && gz < a.Din) val = *(const f32x4*)(src + ((size_t)(gz * a.Hin + gh) * a.Win + iw) * a.cin + q * 4);
      *(f32x4*)(lds + vox * a.CS + q * 4) = val;
    }
  }
  __syncthreads();

  const int ncls = a.SZ * 4;
  const int njt = (a.TZ * a.TH * a.Cw + 31) / 32;
  const int nchunk = a.cin >> 5;
  const int T = a.KZ * 16;
  float* outb = a.out + (size_t)b * a.Do * a.Ho * a.Wo * a.cout;

  for (int job = wave; job < ncls * njt; job += nw) {
    const int cls = job / njt, jt = job % njt;
    const int pz = cls >> 2, ph = (cls >> 1) & 1, pw = cls & 1;
    const int v = jt * 32 + col;
    const int c = v % a.Cw;
    const int t = v / a.Cw;
    const int bb = t % a.TH, aa = t / a.TH;
    const int oz = a.SZ * (a0 + aa) + pz, oh = 2 * (b0 + bb) + ph, ow = 2 * c + pw;
    const bool valid = (aa < a.TZ) && (oz < a.Do) && (oh < a.Ho) && (ow < a.Wo);
    if (!__any(valid)) continue;
    const int ooff = valid ? ((oz * a.Ho + oh) * a.Wo + ow) * a.cout : -1;

    f32x16 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;

    for (int kz = (pz + 1) % a.SZ; kz < a.KZ; kz += a.SZ) {
      const int lz = aa + (pz + 1 - kz) / a.SZ + 1;
      for (int kh = (ph + 3) & 1; kh < 4; kh += 2) {
        const int lh = bb + (ph + 3 - kh) / 2;  // (.. )/2 - 1 (circular halo) + 1 (tile halo)
        for (int kw = (pw + 1) & 1; kw < 4; kw += 2) {
          const int iw = c + (pw + 1 - kw) / 2;
          const bool ok = valid && iw >= 0 && iw < a.Win;
          const int off = ok ? ((lz * PH + lh) * a.Win + iw) * a.CS + half * 16 : ZERO + half * 16;
          const int tap = (kz * 4 + kh) * 4 + kw;
          for (int chunk = 0; chunk < nchunk; ++chunk) {
            f32x4 av[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) av[q] = *(const f32x4*)(lds + off + chunk * 32 + q * 4);
            const f32x4* wq = (const f32x4*)a.wpk + ((size_t)(chunk * T + tap) * a.CTtot) * 256 + lane;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
              f32x4 bw[4];
#pragma unroll
              for (int q = 0; q < 4; ++q) bw[q] = wq[ct * 256 + q * 64];
#pragma unroll
              for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[ct] = MFMA32(av[q][e], bw[q][e], acc[ct]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
      const int off = __shfl(ooff, row, 64);
      if (off >= 0) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const int co = ct * 32 + col;
          outb[off + co] = acc[ct][r] + (a.bias ? a.bias[co] : 0.f);
        }
      }
    }
  }
}

// The same gather on the fp16 matrix pipe (f16x2, see kernels_conv_zs.hip): the haloed input tile is split into two fp16
// terms while it is staged (record = [k-step][term][16 fp16] + 16 B pad, the byte size of the fp32 record), every valid
// (tap, 16-channel k-step) costs two ds_read_b128 and three MFMAs per 32 output channels instead of eight f32 MFMAs of twice
// the duration.
template <int CT>
__global__ void __launch_bounds__(256) conv_transpose_f16x2_kernel(ConvTArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  int bid = blockIdx.x;
  const int thi = bid % a.nTH;
  bid /= a.nTH;
  const int tzi = bid % a.nTZ;
  const int b = bid / a.nTZ;
  const int a0 = tzi * a.TZ, b0 = thi * a.TH;
  const int PZ = a.TZ + 2, PH = a.TH + 2;
  const int tileVox = PZ * PH * a.Win;
  const int ZERO = tileVox * a.CS;
  const int half = lane >> 5, col = lane & 31;
  for (int i = tid; i < a.CS; i += blockDim.x) lds[ZERO + i] = 0.f;

  float gscale = 1.f, ginv = 1.f;
  if (a.in_absmax) pow2_scale_for(*a.in_absmax, &gscale, &ginv);
  {  // stage + split all input channels of the haloed tile
    const int c4 = a.cin >> 2;
    const float* src = a.in + (size_t)b * a.Din * a.Hin * a.Win * a.cin;
    float amax = 0.f;
    auto stage = [&](int vox, int q, int iw, int lh, int lz) {
      const int gz = a0 - 1 + lz;
      int gh = b0 - 1 + lh;  // (circular halo: -1 .. b0 + TH < 2 Hin)
      gh = gh < 0 ? gh + a.Hin : gh;
      gh = gh >= a.Hin ? gh - a.Hin : gh;
      gh = gh >= a.Hin ? gh - a.Hin : gh;  // (a tile of a ring shorter than its halo: TH + 2 <= 3 Hin always)
      f32x4 val = {0.f, 0.f, 0.f, 0.f};
      if (gz >= 0 && gz < a.Din) val = *(const f32x4*)(src + ((size_t)(gz * a.Hin + gh) * a.Win + iw) * a.cin + q * 4);
      val *= gscale;
      amax = fmaxf(amax, fmaxf(fmaxf(fabsf(val[0]), fabsf(val[1])), fmaxf(fabsf(val[2]), fabsf(val[3]))));
      u32x2 t1, t2;
      split2(val, t1, t2);
      char* dst = (char*)(lds + vox * a.CS) + (q >> 2) * 64 + (q & 3) * 8;
      *(u32x2*)dst = t1;
      *(u32x2*)(dst + 32) = t2;
    };
    const int nthr = blockDim.x;
    if (nthr % c4 == 0) {
      // a thread keeps its channel quad and walks the tile's voxels in steps of nthr / c4, its (iw, lh, lz) advanced with carries:
      // six integer divisions by run-time values per item (~40 instructions each) were most of this loop
      const int q = tid % c4, vstep = nthr / c4;
      int vox = tid / c4;
      int iw = vox % a.Win, r = vox / a.Win;
      int lh = r % PH, lz = r / PH;
      const int dw = vstep % a.Win, dr = vstep / a.Win, dh = dr % PH, dz = dr / PH;
      for (; vox < tileVox; vox += vstep) {
        stage(vox, q, iw, lh, lz);
        iw += dw; lh += dh; lz += dz;
        if (iw >= a.Win) { iw -= a.Win; lh += 1; }
        if (lh >= PH) { lh -= PH; lz += 1; }
      }
    } else {
      const int items = tileVox * c4;
      for (int idx = tid; idx < items; idx += nthr) {
        const int q = idx % c4, vox = idx / c4;
        const int iw = vox % a.Win;
        const int r = vox / a.Win;
        stage(vox, q, iw, r % PH, r / PH);
      }
    }
    if (a.status && amax > 65504.f) atomicOr(a.status, 1);
  }
  __syncthreads();

  // (the z stride is 1 or 2 -- the launcher checks it: shifts and masks below where run-time integer divisions by a.SZ cost ~30 vector
  // instructions each, per tap and parity class, in a kernel that PMC shows bound by vector issue: 21 VALU instructions per MFMA)
  const int szs = a.SZ - 1;  // log2(SZ)
  const int ncls = a.SZ * 4;
  const int njt = (a.TZ * a.TH * a.Cw + 31) / 32;
  const int nks = a.cin >> 4;
  const int T = a.KZ * 16;
  float* outb = a.out + (size_t)b * a.Do * a.Ho * a.Wo * a.cout;

  // Work = (row tile jt, parity class cls).  With at least one tile per wave a wave takes tiles jt = wave, wave + nw, .. and runs all
  // SZ x 4 classes on each: the tile's 32 class-space positions are decomposed once (four integer divisions by run-time values per
  // lane) instead of once per class.  Tiles of fewer row tiles than waves (the deepest levels) spread (class, tile) pairs over the
  // waves instead.
  const bool tile_major = njt >= nw;
  for (int item = wave; item < (tile_major ? njt : ncls * njt); item += nw) {
    const int jt = tile_major ? item : item % njt;
    const int v = jt * 32 + col;
    const int c = v % a.Cw;
    const int t = v / a.Cw;
    const int bb = t % a.TH, aa = t / a.TH;
  for (int ci = 0; ci < (tile_major ? ncls : 1); ++ci) {
    const int cls = tile_major ? ci : item / njt;
    const int pz = cls >> 2, ph = (cls >> 1) & 1, pw = cls & 1;
    const int oz = ((a0 + aa) << szs) + pz, oh = 2 * (b0 + bb) + ph, ow = 2 * c + pw;
    const bool valid = (aa < a.TZ) && (oz < a.Do) && (oh < a.Ho) && (ow < a.Wo);
    if (!__any(valid)) continue;
    const int ooff = valid ? ((oz * a.Ho + oh) * a.Wo + ow) * a.cout : -1;

    f32x16 accA[CT], accB[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) { accA[ct][r] = 0.f; accB[ct][r] = 0.f; }

    // The class's taps -- kz in {kz0, kz0 + SZ, ..}, two kh, two kw -- times the k-steps as ONE flat sequence of stages, software-
    // pipelined over a ring of four: the fragment (LDS) and weight (L2) loads of stage j + 3 are requested before the MFMAs of
    // stage j -- three stages = 9 MFMAs = ~300 cycles of cover for an L2 round trip.  (As nested loops every k-step waited for its
    // own weight loads: a round trip per 3 MFMAs.)  Requests past the end repeat the last stage instead of being conditional: a
    // conditional load in a pipelined loop costs a full vmcnt(0) per trip.
    const int kz0 = (pz + 1) & szs, kh0 = (ph + 3) & 1, kw0 = (pw + 1) & 1;
    const int nkz = (a.KZ - kz0 + a.SZ - 1) >> szs;
    const int nstage = nkz * 4 * nks;
    struct Stage {
      u32x4 x1, x2, w[CT][2];
    };
    int ti_n = 0, ks_n = 0, tap_n = 0;  // the next stage to request: tap number (kz-major), k-step; its weight tap index
    const char* rec_n = nullptr;        // ... and this lane's record of that tap
    auto setup = [&](int ti) {
      const int kz = kz0 + ((ti >> 2) << szs), kh = kh0 + ((ti >> 1) & 1) * 2, kw = kw0 + (ti & 1) * 2;
      const int lz = aa + ((pz + 1 - kz) >> szs) + 1;  // (pz + 1 - kz is a multiple of SZ, possibly negative: the arithmetic shift is exact)
      const int lh = bb + ((ph + 3 - kh) >> 1);  // (.. )/2 - 1 (circular halo) + 1 (tile halo); even by the choice of kh0
      const int iw = c + ((pw + 1 - kw) >> 1);   // even by the choice of kw0
      const bool ok = valid && iw >= 0 && iw < a.Win;
      rec_n = (const char*)(lds + (ok ? ((lz * PH + lh) * a.Win + iw) * a.CS : ZERO)) + half * 16;
      tap_n = (kz * 4 + kh) * 4 + kw;
    };
    setup(0);
    auto fetch = [&](Stage& st) {
      st.x1 = *(const u32x4*)(rec_n + ks_n * 64);
      st.x2 = *(const u32x4*)(rec_n + ks_n * 64 + 32);
      const u32x4* wq = a.wpk16 + ((size_t)(ks_n * T + tap_n) * a.CTtot) * 128 + lane;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        st.w[ct][0] = wq[ct * 128];
        st.w[ct][1] = wq[ct * 128 + 64];
      }
      if (ks_n + 1 < nks) ++ks_n;
      else if (ti_n + 1 < nkz * 4) { ks_n = 0; setup(++ti_n); }
    };
    auto mfmas = [&](const Stage& st) {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        accA[ct] = MFMA_F16(st.x1, st.w[ct][0], accA[ct]);
        accB[ct] = MFMA_F16(st.x1, st.w[ct][1], accB[ct]);
        accB[ct] = MFMA_F16(st.x2, st.w[ct][0], accB[ct]);
      }
    };
    Stage s0, s1, s2, s3;
    fetch(s0);
    fetch(s1);
    fetch(s2);
    for (int j = 0; j < nstage; j += 4) {
      fetch(s3);
      __builtin_amdgcn_sched_barrier(0);
      mfmas(s0);
      __builtin_amdgcn_sched_barrier(0);
      fetch(s0);
      __builtin_amdgcn_sched_barrier(0);
      if (j + 1 < nstage) mfmas(s1);
      __builtin_amdgcn_sched_barrier(0);
      fetch(s1);
      __builtin_amdgcn_sched_barrier(0);
      if (j + 2 < nstage) mfmas(s2);
      __builtin_amdgcn_sched_barrier(0);
      fetch(s2);
      __builtin_amdgcn_sched_barrier(0);
      if (j + 3 < nstage) mfmas(s3);
    }
    // the tile's rows (output voxels of one parity class: 128 contiguous bytes each per channel tile) leave as 16-byte quads after
    // a transpose through the wave's LDS tile (behind the input tile): row 8 k + (lane >> 3), channels 4 (lane & 7) .. + 3
    float* tr = lds + a.tr_off + wave * (32 * 36);
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const float bv = a.bias ? a.bias[ct * 32 + col] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r)
        tr[((r & 3) + 8 * (r >> 2) + 4 * half) * 36 + col] = (accA[ct][r] + accB[ct][r] * (1.f / 2048.f)) * ginv + bv;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (one wave: its own LDS writes are visible to its reads in order)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int row = 8 * k + (lane >> 3);
        const int off = __shfl(ooff, row, 64);
        const f32x4 q = *(const f32x4*)(tr + row * 36 + (lane & 7) * 4);
        if (off >= 0) *(f32x4*)(outb + off + ct * 32 + (lane & 7) * 4) = q;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the tile buffer is reused)
    }
  }
  }
}

template <int CT>
static void launch_convT_inst(const ConvTArgs& a, dim3 grid, size_t lds, hipStream_t s) {
  static bool attr_set = false;
  if (!attr_set) {
    CD_HIP(hipFuncSetAttribute((const void*)conv_transpose_kernel<CT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    CD_HIP(hipFuncSetAttribute((const void*)conv_transpose_f16x2_kernel<CT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_set = true;
  }
  if (a.wpk16) hipLaunchKernelGGL((conv_transpose_f16x2_kernel<CT>), grid, dim3(256), lds, s, a);
  else hipLaunchKernelGGL((conv_transpose_kernel<CT>), grid, dim3(256), lds, s, a);
  CD_HIP(hipGetLastError());
}

void launch_conv_transpose_mfma(const float* in, int cin, const float* wpk, const float* bias, float* out, int batch,
                                int cout, Dims3 din, Dims3 dout, int kz, int sz, hipStream_t s, const void* wpk_f16x2,
                                int* status, const unsigned* in_absmax) {
  CD_REQUIRE(cin % 32 == 0 && cout % 32 == 0, "conv_transpose: channels must be multiples of 32");
  CD_REQUIRE(sz == 1 || sz == 2, "conv_transpose: z stride must be 1 or 2");
  const bool full_range = conv_precision() != PREC_F16X2;
  ConvTArgs a;
  a.wpk16 = full_range ? nullptr : (const u32x4*)wpk_f16x2;
  a.status = status;
  a.in_absmax = in_absmax;
  a.in = in; a.cin = cin; a.wpk = wpk; a.bias = bias; a.out = out;
  a.Din = din.d; a.Hin = din.h; a.Win = din.w; a.Do = dout.d; a.Ho = dout.h; a.Wo = dout.w;
  a.KZ = kz; a.SZ = sz; a.cout = cout; a.CTtot = cout / 32;
  a.Cw = (dout.w + 1) / 2;
  a.CS = cin + LDS_VOX_PAD;
  const int Az = (dout.d + sz - 1) / sz, Bh = (dout.h + 1) / 2;
  // candidate (TZ, TH) tiles in class-index space; ranked by useful/haloed volume, a spread of them is timed once
  struct TT { int tz, th; double score; };
  std::vector<TT> all;
  for (int TZ = 1; TZ <= Az; ++TZ)
    for (int TH = 1; TH <= Bh; ++TH) {
      const size_t lds = ((size_t)(TZ + 2) * (TH + 2) * din.w + 1) * a.CS * 4;
      if (lds > 140 * 1024) break;  // (+ 18 KB of output transpose tiles in the f16x2 kernel)
      if (TH != Bh && (Bh + TH - 1) / TH == (Bh + TH) / (TH + 1)) continue;  // a larger TH gives the same tile count
      if (TZ != Az && (Az + TZ - 1) / TZ == (Az + TZ) / (TZ + 1)) continue;
      const long nblocks = (long)batch * ((Az + TZ - 1) / TZ) * ((Bh + TH - 1) / TH);
      const double ratio = (double)TZ * TH / ((double)(TZ + 2) * (TH + 2));
      const double fill = nblocks >= 512 ? 1.0 : (double)nblocks / 512.0;
      all.push_back({TZ, TH, ratio * fill});
    }
  CD_REQUIRE(!all.empty(), "conv_transpose: no tile fits in LDS");
  std::stable_sort(all.begin(), all.end(), [](const TT& x, const TT& y) { return x.score > y.score; });
  std::vector<TT> cand;
  for (size_t i = 0; i < all.size() && cand.size() < 8; ++i) cand.push_back(all[i]);
  for (size_t i = 8; i < all.size() && cand.size() < 14; i += (all.size() - 8) / 6 + 1) cand.push_back(all[i]);
  char cat[128];
  std::snprintf(cat, sizeof cat, "convT%dx4x4 C%d->%d @%dx%dx%d", kz, cin, cout, din.d, din.h, din.w);
  prof::Scope scope(cat, s, 2.0 * kz * 16 * cin * cout * (double)din.vox() * batch,
                    4.0 * batch * ((double)din.vox() * cin + (double)dout.vox() * cout));
  auto launch = [&](const TT& t) {
    ConvTArgs b = a;
    b.TZ = t.tz; b.TH = t.th;
    b.nTZ = (Az + b.TZ - 1) / b.TZ; b.nTH = (Bh + b.TH - 1) / b.TH;
    size_t lds = ((size_t)(b.TZ + 2) * (b.TH + 2) * din.w + 1) * b.CS * 4;
    if (b.wpk16) {  // four per-wave 32 x 36 float tiles behind the input tile (16-byte aligned)
      lds = (lds + 15) & ~(size_t)15;
      b.tr_off = (int)(lds / 4);
      lds += 4 * 32 * 36 * 4;
    }
    dim3 grid((unsigned)(batch * b.nTZ * b.nTH));
    switch (b.CTtot) {
      case 1: launch_convT_inst<1>(b, grid, lds, s); break;
      case 2: launch_convT_inst<2>(b, grid, lds, s); break;
      case 3: launch_convT_inst<3>(b, grid, lds, s); break;
      case 4: launch_convT_inst<4>(b, grid, lds, s); break;
      default: CD_REQUIRE(false, "conv_transpose: more than 128 output channels unsupported");
    }
  };
  char key[192];
  std::snprintf(key, sizeof key, "%s k%d s%d b%d%s", cat, kz, sz, batch, a.wpk16 ? " f16x2" : "");
  const int pick = autotune(key, (int)cand.size(), [&](int i) { launch(cand[i]); }, s);
  launch(cand[pick < 0 ? 0 : pick]);
}

}  // namespace cd
