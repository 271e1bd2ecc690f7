// Weight gradients of the convolutions (training step and cd_denoise_vjp; the reference relies on torch autograd through
// Conv3d / ConvTranspose3d, models.py:25-96):
//     dW[a][b][tap] = sum over samples and voxels of g[o][a] * x[in(o, tap)][b]
// a contraction over VOXELS on the channels-last tensors of the forward path, generic in taps / stride so that it serves 3x3x3,
// 1x1x1, the strided down conv and -- with the roles of the two tensors swapped -- the transposed up conv.
//   wgrad_kernel          any taps / stride: one workgroup per (32x32 tile, voxel chunk), operands from global memory
//   wgrad1x1_kernel       1x1x1: a streaming pass over both tensors, rows staged in LDS
//   wgrad_flat_kernel     stride-1 3x3x3 in fp32: persistent, LDS-staged flat voxel ranges
//   (kernels_wgrad16.hip  stride-1 3x3x3 and the strided (KD,4,4) conv on the fp16 matrix pipe)
// Every kernel leaves 32x32 partial tiles per slot (chunk or workgroup); the slot reductions below sum them in a fixed order
// (deterministic, no float atomics) and write the torch layout.  launch_wgrad, at the bottom, is the ladder that picks the
// kernel and its reduction (wgrad_internal.h: the rungs).
#include "conv_internal.h"
#include "wgrad_internal.h"
#include <cstdio>
#include <cstdlib>

namespace cd {

// ------------------------------------------------------------------------------------------------------------
// Weight gradient.
//   g : (B, Og, A)  channels-last "output side" tensor (A = rows of dW), voxel grid (Dg, Hg, Wg)
//   x : (B, Ox, Bc) channels-last "input side" tensor (Bc = columns of dW), voxel grid (Dx, Hx, Wx)
//   dW[a][b][tap] = sum_{n, o} g[n][o][a] * x[n][in(o, tap)][b],  in(o,tap) = (oz*SZ + kz - 1, (oh*S + kh - 1) mod Hx, ow*S + kw - 1)
//   (zero outside z / r).  For a transposed conv the caller passes g = layer input, x = output gradient: same geometry.
// One workgroup = one 32x32 (a, b) tile x one voxel chunk; its 4 waves split the taps; every lane half takes one voxel of
// a pair (K = 2 per MFMA).  Partials [chunk][tap][32][32] are reduced in a fixed order by wgrad_reduce_kernel
// (deterministic, no float atomics), which also writes the torch layout.
// ------------------------------------------------------------------------------------------------------------
struct WgradArgs {
  const float* g;
  const float* x;
  int A, Bc;              // channel counts (ld of g / x)
  int xld, xoff;          // x may be a channel slice of a wider tensor (skip concat): row stride and offset
  int Dg, Hg, Wg, Dx, Hx, Wx;
  int KD, KH, KW, SZ, S;
  int batch;
  int per_sample;         // 1: no reduction over the batch (attention context gradient); partial index includes n
  int chunk_vox;          // output voxels per chunk (even)
  int nchunks;            // chunks per sample
  float* partial;         // [(n if per_sample)][chunk (x batch if !per_sample)][tileA][tileB][tap][32][32]
};

template <int TPW>  // taps per wave (upper bound); blockDim = 64 * ceil(T / TPW)
__global__ void __launch_bounds__(1024) wgrad_kernel(WgradArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, col = lane & 31;
  const int T = a.KD * a.KH * a.KW;
  const int tilesB = a.Bc / 32;
  const int ta = blockIdx.y / tilesB, tb = blockIdx.y % tilesB;
  const int chunk = blockIdx.x % a.nchunks;
  const int n = blockIdx.x / a.nchunks;
  const int Og = a.Dg * a.Hg * a.Wg, Ox = a.Dx * a.Hx * a.Wx;
  const int tap0 = wave * TPW;
  const int ntap = min(TPW, T - tap0);

  f32x16 acc[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  const float* gb = a.g + (size_t)n * Og * a.A + ta * 32 + col;
  const float* xb = a.x + (size_t)n * Ox * a.xld + a.xoff + tb * 32 + col;
  const int o0 = chunk * a.chunk_vox;
  const int o1 = min(o0 + a.chunk_vox, Og);
  if (T == 1 && a.S == 1 && a.SZ == 1 && TPW == 1) {
    // pointwise conv: in(o) = o.  Eight voxel pairs per trip: 16 loads in flight, no index arithmetic (the general loop below
    // spent ~100 VALU instructions of div/mod per 64-cycle MFMA and one memory round trip per voxel pair)
    constexpr int U = 8;
    int ob = o0;  // wave-uniform pair base: both lane halves run the same MFMAs (EXEC does not mask an MFMA)
    for (; ob + 2 * U <= o1; ob += 2 * U) {
      const int o = ob + half;
      float gv[U], xv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        gv[u] = gb[(size_t)(o + 2 * u) * a.A];
        xv[u] = xb[(size_t)(o + 2 * u) * a.xld];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) acc[0] = MFMA32(gv[u], xv[u], acc[0]);
    }
    for (; ob < o0 + a.chunk_vox; ob += 2) {
      const int o = ob + half;
      const bool ov = o < o1;
      const float gv = ov ? gb[(size_t)o * a.A] : 0.f;
      const float xv = ov ? xb[(size_t)o * a.xld] : 0.f;
      acc[0] = MFMA32(gv, xv, acc[0]);
    }
  } else if (ntap > 0) {
    // tap geometry of this wave, hoisted out of the voxel loop (div / mod by run-time kernel extents)
    int dz[TPW], dh[TPW], dw[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int tap = min(tap0 + t, T - 1);
      const int kw = tap % a.KW, kh = (tap / a.KW) % a.KH, kz = tap / (a.KW * a.KH);
      dz[t] = kz - (a.KD == 1 ? 0 : 1);
      dh[t] = kh - (a.KH == 1 ? 0 : 1);
      dw[t] = kw - (a.KW == 1 ? 0 : 1);
    }
    // U voxel pairs per trip: their U * (1 + TPW) loads are all in flight before the first MFMA
    constexpr int U = TPW >= 3 ? 3 : 4;
    for (int ob = o0; ob < o0 + a.chunk_vox; ob += 2 * U) {
      float gv[U], xv[U][TPW];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int o = ob + 2 * u + half;
        const bool ov = o < o1;
        const int oo = ov ? o : o0;
        const float g0 = gb[(size_t)oo * a.A];
        gv[u] = ov ? g0 : 0.f;
        const int ow = oo % a.Wg;
        const int t2 = oo / a.Wg;
        const int oh = t2 % a.Hg, oz = t2 / a.Hg;
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
          const int iz = oz * a.SZ + dz[t], iw = ow * a.S + dw[t];
          int ih = oh * a.S + dh[t];
          ih = ih < 0 ? ih + a.Hx : (ih >= a.Hx ? ih - a.Hx : ih);
          ih = ih >= a.Hx ? ih - a.Hx : ih;
          const bool ok = ov && iz >= 0 && iz < a.Dx && iw >= 0 && iw < a.Wx;
          const float v = xb[ok ? ((size_t)(iz * a.Hx + ih) * a.Wx + iw) * a.xld : 0];
          xv[u][t] = ok ? v : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int t = 0; t < TPW; ++t)
          if (t < ntap) acc[t] = MFMA32(gv[u], xv[u][t], acc[t]);
    }
  }
  // C layout: col = lane&31 (b), row = (r&3) + 8*(r>>2) + 4*half (a)
  const size_t slot = a.per_sample ? ((size_t)n * a.nchunks + chunk) : ((size_t)chunk * a.batch + n);
  float* pbase = a.partial + ((slot * (a.A / 32) + ta) * tilesB + tb) * (size_t)T * 1024;
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    if (t < ntap) {
      float* p = pbase + (size_t)(tap0 + t) * 1024;
#pragma unroll
      for (int r = 0; r < 16; ++r) p[((r & 3) + 8 * (r >> 2) + 4 * half) * 32 + col] = acc[t][r];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------
// Weight gradient of a 1x1x1 conv (ResnetBlock shortcuts, the attention's to_qkv / to_out and -- per sample -- its context
// gradient): dW[a][b] = sum over rows of g[row][a] x[row][b], a tiny output over a very long K, i.e. a streaming pass over the two
// tensors.  Round 4: wgrad_kernel<1> ran it as ~12 k single-wave workgroups of dword loads, a pre-reduction of their 4096 partials
// and the final reduction -- three launches and ~60 us for the 107 MB of the level-0 to_qkv gradient, 27 times per training step.
// Here a workgroup of four waves loops over units of R rows: both tensors' rows are staged in LDS with 16-byte loads (fp32, row
// pitch = 32 mod 64 floats so that the two half-waves of an operand read hit disjoint banks), wave w runs rows 32 w .. 32 w + 31
// of the unit as 16 K-steps of v_mfma_f32_32x32x2_f32 for each of the workgroup's (a, b) tiles (lanes are channels, the lane
// half is the row of the pair: exact fp32, nothing to rescale), accumulators live across all units, and the four waves' sums are
// added in a fixed order through LDS into ONE partial per workgroup.  Segments: the whole batch (rows contiguous across samples)
// or, per_sample, one sample each.
// ------------------------------------------------------------------------------------------------------------
struct Wgrad1Args {
  const float* g;   // (rows, A)
  const float* x;   // (rows, xld) read at channel offset xoff, Bc channels
  int A, Bc, xld, xoff;
  int ldA, ldB;     // LDS row pitches (floats)
  int R;            // rows per unit (multiple of 128)
  long long rows_per_seg;
  int units_per_seg, wgs_per_seg;
  int tilesB, ntiles;
  float* partial;   // [gridDim.x][tilesA][tilesB][32][32]
  int dbg;          // ablation (CD_W1_DBG): 1 = no MFMAs, 2 = no global loads
};

// NQ: 16-byte quads of a unit per thread = ceil(R (A + Bc) / 4 / 256); W1_NT: (a, b) tiles per workgroup (blockIdx.y takes the next
// W1_NT; the launcher picks a divisor of the tile count, so every tile index below is valid)
template <int NQ, int W1_NT>
__global__ void __launch_bounds__(256) wgrad1x1_kernel(Wgrad1Args a) {
  extern __shared__ __attribute__((aligned(16))) float w1[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, col = lane & 31;
  const int seg = blockIdx.x / a.wgs_per_seg, wq = blockIdx.x % a.wgs_per_seg;
  const int tile0 = blockIdx.y * W1_NT;
  float* const sG = w1;
  float* const sX = w1 + (size_t)a.R * a.ldA;
  int ga[W1_NT], xb[W1_NT];  // channel offsets of this lane's operand element per tile
#pragma unroll
  for (int t = 0; t < W1_NT; ++t) {
    const int tile = tile0 + t;
    ga[t] = (tile / a.tilesB) * 32 + col;
    xb[t] = (tile % a.tilesB) * 32 + col;
  }
  f32x16 acc[W1_NT];
#pragma unroll
  for (int t = 0; t < W1_NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  const float* gseg = a.g + (size_t)seg * a.rows_per_seg * a.A;
  const float* xseg = a.x + (size_t)seg * a.rows_per_seg * a.xld + a.xoff;
  const int qa = a.A >> 2, qb = a.Bc >> 2, qrow = qa + qb;  // 16-byte quads per row: g's, then x's
  const int nq = a.R * qrow;
  // exact small-integer division by reciprocal: (i + 0.5) / qrow is never within float error of an integer for i < 2^20
  const float inv_qrow = 1.f / (float)qrow;
  auto row_of = [&](int i) { return (int)(((float)i + 0.5f) * inv_qrow); };
  // a unit's rows travel global -> registers -> LDS; the loads of unit u + 1 are issued before the MFMAs of unit u and land under
  // them (one memory round trip per unit was most of a workgroup's time: the first version took 45 us for the 107 MB of the level-0
  // to_qkv gradient)
  f32x4 v[NQ];
  auto issue = [&](int u) {
    const long long r0 = (long long)u * a.R;
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
      const int i = tid + k * 256;
      const int row = row_of(i), q = i - row * qrow;
      v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (i < nq && r0 + row < a.rows_per_seg && !(a.dbg & 2))
        v[k] = q < qa ? *(const f32x4*)(gseg + (size_t)(r0 + row) * a.A + q * 4)
                      : *(const f32x4*)(xseg + (size_t)(r0 + row) * a.xld + (q - qa) * 4);
    }
  };
  int u = wq;
  if (u < a.units_per_seg) issue(u);
  for (; u < a.units_per_seg; u += a.wgs_per_seg) {
    __syncthreads();  // the previous unit has been consumed
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
      const int i = tid + k * 256;
      if (i < nq) {
        const int row = row_of(i), q = i - row * qrow;
        if (q < qa) *(f32x4*)(sG + (size_t)row * a.ldA + q * 4) = v[k];
        else *(f32x4*)(sX + (size_t)row * a.ldB + (q - qa) * 4) = v[k];
      }
    }
    __syncthreads();
    if (u + a.wgs_per_seg < a.units_per_seg) issue(u + a.wgs_per_seg);
    for (int rb = wave * 32; rb < ((a.dbg & 1) ? 0 : a.R); rb += 128) {
      // eight K-steps' operands are requested before their MFMAs (as a plain loop every MFMA waited for its own LDS round trip
      // behind a branch: 400 cycles per 64-cycle instruction)
#pragma unroll
      for (int s0 = 0; s0 < 16; s0 += 8) {
        float gv[8][W1_NT], xv[8][W1_NT];
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2) {
          const int row = rb + 2 * (s0 + s2) + half;
#pragma unroll
          for (int t = 0; t < W1_NT; ++t) {
            gv[s2][t] = sG[row * a.ldA + ga[t]];
            xv[s2][t] = sX[row * a.ldB + xb[t]];
          }
        }
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2)
#pragma unroll
          for (int t = 0; t < W1_NT; ++t) acc[t] = MFMA32(gv[s2][t], xv[s2][t], acc[t]);
      }
    }
  }
  // the four waves' sums, wave 0 first, through LDS: one partial per workgroup
  __syncthreads();
#pragma unroll
  for (int t = 0; t < W1_NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) w1[((wave * W1_NT + t) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * 32 + col] = acc[t][r];
  __syncthreads();
  const int tilesA = a.A / 32;
  for (int i = tid; i < W1_NT * 1024; i += 256) {
    const int t = i >> 10, e = i & 1023;
    const float v = ((w1[(0 * W1_NT + t) * 1024 + e] + w1[(1 * W1_NT + t) * 1024 + e]) + w1[(2 * W1_NT + t) * 1024 + e]) +
                    w1[(3 * W1_NT + t) * 1024 + e];
    const int tile = tile0 + t;
    a.partial[(((size_t)blockIdx.x * tilesA + tile / a.tilesB) * a.tilesB + tile % a.tilesB) * 1024 + e] = v;
  }
}

// returns false when the shape does not fit (the caller runs wgrad_kernel<1>)
bool try_launch_wgrad1x1(const WgradOp& op, int* nslots_out, hipStream_t s) {
  static const bool off = getenv("CD_NO_WGRAD1X1") != nullptr;
  const int A = op.A, Bc = op.Bc;
  const int64_t vox = op.geom.out.vox();
  if (off || A % 32 || Bc % 32 || op.xld % 4 || op.xoff % 4) return false;
  const size_t partial_slots = (size_t)wgrad_chunks(vox, op.batch, op.per_sample, A, Bc, 1) * op.batch;  // what the caller's buffer holds
  Wgrad1Args a;
  a.g = op.g; a.x = op.x; a.A = A; a.Bc = Bc; a.xld = op.xld; a.xoff = op.xoff;
  a.ldA = A + (A % 64 == 32 ? 0 : 32);
  a.ldB = Bc + (Bc % 64 == 32 ? 0 : 32);
  a.tilesB = Bc / 32;
  a.ntiles = (A / 32) * (Bc / 32);
  a.R = 128;
  const int NT = a.ntiles % 4 == 0 ? 4 : (a.ntiles % 3 == 0 ? 3 : (a.ntiles % 2 == 0 ? 2 : (a.ntiles == 1 ? 1 : 0)));
  if (!NT) return false;
  const size_t stage = (size_t)a.R * (a.ldA + a.ldB) * 4, red = (size_t)4 * NT * 4096;
  const size_t lds = stage > red ? stage : red;
  if (lds > 160 * 1024) return false;
  a.rows_per_seg = op.per_sample ? vox : (int64_t)op.batch * vox;
  const int64_t units = (a.rows_per_seg + a.R - 1) / a.R;
  CD_REQUIRE(units < (1ll << 30), "wgrad 1x1: too many rows");
  a.units_per_seg = (int)units;
  const int groups = a.ntiles / NT;
  // workgroups: two per CU where the staging fits twice (one streams while the other multiplies), at least 2 units each
  const int nseg = op.per_sample ? op.batch : 1;
  int64_t want = (lds <= 80 * 1024 ? 512 : 256) / groups / nseg;
  if (want < 1) want = 1;
  if (want > units) want = units;
  if ((size_t)want * nseg > partial_slots) want = (int64_t)(partial_slots / nseg);
  if (want < 1) return false;
  a.wgs_per_seg = (int)want;
  a.partial = op.partial;
  static const int dbg = getenv("CD_W1_DBG") ? atoi(getenv("CD_W1_DBG")) : 0;
  a.dbg = dbg;
  const int nqt = (a.R * ((A + Bc) / 4) + 255) / 256;
  const dim3 grid((unsigned)(a.wgs_per_seg * nseg), (unsigned)groups);
#define W1_CASE(N, T)                                                                                                           \
  if (nqt <= N && NT == T) {                                                                                                    \
    static bool attr = false;                                                                                                   \
    if (!attr) {                                                                                                                \
      CD_HIP(hipFuncSetAttribute((const void*)wgrad1x1_kernel<N, T>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));   \
      attr = true;                                                                                                              \
    }                                                                                                                           \
    hipLaunchKernelGGL((wgrad1x1_kernel<N, T>), grid, dim3(256), lds, s, a);                                                    \
    CD_HIP(hipGetLastError());                                                                                                  \
    *nslots_out = a.wgs_per_seg;                                                                                                \
    return true;                                                                                                                \
  }
#define W1_CASES(N) W1_CASE(N, 1) W1_CASE(N, 2) W1_CASE(N, 3) W1_CASE(N, 4)
  W1_CASES(8) W1_CASES(16) W1_CASES(24) W1_CASES(32)
#undef W1_CASES
#undef W1_CASE
  return false;  // (wider than 128 + 128 channels: the general kernel)
}

// ------------------------------------------------------------------------------------------------------------
// Weight gradient of the stride-1 3x3x3 conv, LDS-staged and persistent (the hot backward kernel).
// A workgroup loops over (sample, 256-voxel flat range) units; per unit it stages the output-gradient rows [R][32] and
// the input z-planes the range touches (+1 halo plane each side, zero outside) as [voxel][32] fp32, plus a per-voxel
// record (LDS index, phi/r edge flags).  Its waves split the 27 taps; a wave keeps one 32x32 accumulator per tap in
// registers across ALL its units and writes ONE partial per workgroup (grid = CU count => 256 partial slots instead of one
// per voxel chunk).  K = 2 voxels per v_mfma_f32_32x32x2_f32: lane half h takes voxel 2p+h, lanes are channels, so both
// LDS operand reads are conflict-free 128-B rows.
// ------------------------------------------------------------------------------------------------------------
struct WgradFlatArgs {
  const float* g;   // (B, vox, A)
  const float* x;   // (B, vox, xld) read at channel offset xoff
  int A, xld, xoff;
  int D, H, W;
  int R, P;         // voxels per unit, plane capacity
  int units_per_sample, total_units;
  float* partial;   // [gridDim.x][tilesA][tilesB][27][32][32]
  int tilesB;
};

template <int TPW>
__global__ void __launch_bounds__(64 * ((27 + TPW - 1) / TPW)) wgrad_flat_kernel(WgradFlatArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int NW = (27 + TPW - 1) / TPW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, col = lane & 31;
  const int ta = blockIdx.y / a.tilesB, tb = blockIdx.y % a.tilesB;
  const int HW = a.H * a.W, vox = a.D * HW;
  float* gL = lds;                                   // [R][32]
  float* xL = lds + a.R * 32;                        // [P*HW][32]
  int* tbl = (int*)(xL + (size_t)a.P * HW * 32);     // [R]

  // this wave's taps
  int toff[TPW], tdh[TPW], tdw[TPW];
  int ntap = 0;
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int tap = wave + t * NW;
    const int dz = tap / 9 - 1, dh = (tap / 3) % 3 - 1, dw = tap % 3 - 1;
    toff[t] = dz * HW + dh * a.W + dw;
    tdh[t] = dh;
    tdw[t] = dw;
    if (tap < 27) ntap = t + 1;
  }
  f32x16 acc[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  for (int u = blockIdx.x; u < a.total_units; u += gridDim.x) {
    const int n = u / a.units_per_sample, ux = u - n * a.units_per_sample;
    const int v0 = ux * a.R, vend = min(v0 + a.R, vox);
    const int zA = v0 / HW - 1, zB = (vend - 1) / HW + 1;
    const int nstage = (zB - zA + 1) * HW, gbase = zA * HW;
    __syncthreads();  // previous unit fully consumed
    {
      const float* gs = a.g + ((size_t)n * vox + v0) * a.A + ta * 32;
      for (int i0 = tid; i0 < a.R * 8; i0 += 4 * blockDim.x) {
        f32x4 val[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int i = i0 + k * blockDim.x;
          val[k] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (i < a.R * 8 && v0 + (i >> 3) < vend) val[k] = *(const f32x4*)(gs + (size_t)(i >> 3) * a.A + (i & 7) * 4);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int i = i0 + k * blockDim.x;
          if (i < a.R * 8) *(f32x4*)(gL + (i >> 3) * 32 + (i & 7) * 4) = val[k];
        }
      }
      const float* xs = a.x + (size_t)n * vox * a.xld + a.xoff + tb * 32;
      for (int i0 = tid; i0 < nstage * 8; i0 += 4 * blockDim.x) {
        f32x4 val[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int i = i0 + k * blockDim.x;
          const int gv = gbase + (i >> 3);
          val[k] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (i < nstage * 8 && gv >= 0 && gv < vox) val[k] = *(const f32x4*)(xs + (size_t)gv * a.xld + (i & 7) * 4);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int i = i0 + k * blockDim.x;
          if (i < nstage * 8) *(f32x4*)(xL + (i >> 3) * 32 + (i & 7) * 4) = val[k];
        }
      }
      for (int v = tid; v < a.R; v += blockDim.x) {
        const int gv = v0 + v;
        int rec = -1;
        if (gv < vend) {
          const int r = gv % HW;
          const int h = r / a.W, w = r - h * a.W;
          rec = (gv - gbase) | (w == 0 ? 1 << 20 : 0) | (w == a.W - 1 ? 1 << 21 : 0) | (h == 0 ? 1 << 22 : 0) |
                (h == a.H - 1 ? 1 << 23 : 0);
        }
        tbl[v] = rec;
      }
    }
    __syncthreads();
    // 4 voxel pairs per trip: all their LDS operands are requested before the first MFMA of the group issues
    constexpr int UP = 4;
    for (int p0 = 0; p0 < a.R; p0 += 2 * UP) {
      float gv[UP], xv[UP][TPW];
#pragma unroll
      for (int k = 0; k < UP; ++k) {
        const int p = p0 + 2 * k;
        const int rec = p < a.R ? tbl[p + half] : -1;
        gv[k] = p < a.R ? gL[(p + half) * 32 + col] : 0.f;
        const int nb = rec & 0xfffff;
        const bool vvalid = rec >= 0;
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
          int nidx = nb + toff[t];
          if (tdh[t] < 0 && (rec & (1 << 22))) nidx += HW;        // wrap phi: row -1 -> H-1
          if (tdh[t] > 0 && (rec & (1 << 23))) nidx -= HW;        // row H -> 0
          const bool ok = vvalid && t < ntap && !(tdw[t] < 0 && (rec & (1 << 20))) && !(tdw[t] > 0 && (rec & (1 << 21)));
          xv[k][t] = ok ? xL[nidx * 32 + col] : 0.f;
        }
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int k = 0; k < UP; ++k)
#pragma unroll
        for (int t = 0; t < TPW; ++t)
          if (t < ntap) acc[t] = MFMA32(gv[k], xv[k][t], acc[t]);
    }
  }
  float* pbase = a.partial + (((size_t)blockIdx.x * (a.A / 32) + ta) * a.tilesB + tb) * (size_t)27 * 1024;
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int tap = wave + t * NW;
    if (tap < 27) {
      float* pp = pbase + (size_t)tap * 1024;
#pragma unroll
      for (int r = 0; r < 16; ++r) pp[((r & 3) + 8 * (r >> 2) + 4 * half) * 32 + col] = acc[t][r];
    }
  }
}

// returns false when not even a 32-voxel unit's planes fit in LDS (the caller runs wgrad_kernel<3>)
bool try_launch_wgrad_flat(const WgradOp& op, int* nslots, hipStream_t s) {
  if (getenv("CD_NO_WGRAD_FLAT")) return false;
  const Dims3 d = op.geom.out;
  const int A = op.A, Bc = op.Bc;
  const int HW = d.h * d.w;
  int R = 256;
  while (R > 32 && (int64_t)(R / 2) >= d.vox()) R /= 2;
  int P = (R - 1) / HW + 4;
  size_t lds = ((size_t)R * 32 + (size_t)P * HW * 32 + R) * 4;
  while (lds > 150 * 1024 && R > 32) {
    R /= 2;
    P = (R - 1) / HW + 4;
    lds = ((size_t)R * 32 + (size_t)P * HW * 32 + R) * 4;
  }
  if (lds > 150 * 1024) return false;
  WgradFlatArgs f;
  f.g = op.g; f.x = op.x; f.A = A; f.xld = op.xld; f.xoff = op.xoff; f.D = d.d; f.H = d.h; f.W = d.w; f.R = R; f.P = P;
  f.units_per_sample = (int)((d.vox() + R - 1) / R);
  f.total_units = f.units_per_sample * op.batch;
  f.partial = op.partial; f.tilesB = Bc / 32;
  const int tiles = (A / 32) * (Bc / 32);
  int nblk = 256 / tiles;  // partial slots: one per workgroup
  if (nblk < 32) nblk = 32;
  if (nblk > f.total_units) nblk = f.total_units;
  static bool attr_set = false;
  if (!attr_set) {
    CD_HIP(hipFuncSetAttribute((const void*)wgrad_flat_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_set = true;
  }
  hipLaunchKernelGGL(wgrad_flat_kernel<4>, dim3(nblk, tiles), dim3(64 * 7), lds, s, f);
  CD_HIP(hipGetLastError());
  *nslots = nblk;
  return true;
}

// ------------------------------------------------------------------------------------------------------------
// Slot reductions: dW (torch layout: dW[a][b][tap], a = the Conv3d weight's out channel) = sum over slots of the partial tiles.
// b_total / b_off: the b columns are a slice of a wider weight (second source of a channel concat).  blockIdx.y = sample of a
// per-sample gradient.
// ------------------------------------------------------------------------------------------------------------
__global__ void wgrad_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dw, int A, int Bc, int T, int nslots,
                                    size_t sample_stride_partial, size_t sample_stride_out, int b_total, int b_off, int slot_step = 1) {
  const size_t total = (size_t)A * Bc * T;
  const size_t sstride = total * (size_t)slot_step;  // the slots left by wgrad_prereduce_kernel are slot_step apart
  const size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int n = blockIdx.y;
  // idx enumerates the partial-tile order: [ta][tb][tap][row a][col b]
  const int cb = idx & 31, ra = (idx >> 5) & 31;
  size_t rest = idx >> 10;
  const int tap = rest % T;
  rest /= T;
  const int tilesB = Bc / 32;
  const int tb = rest % tilesB, ta = rest / tilesB;
  const float* p = partial + (size_t)n * sample_stride_partial + idx;
  // 16 independent loads in flight per thread (the slot loop is latency-bound otherwise); fixed summation order
  float acc8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int k = 0;
  for (; k + 16 <= nslots; k += 16) {
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = p[(size_t)(k + j) * sstride];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc8[j & 7] += v[j];
  }
  for (; k < nslots; ++k) acc8[k & 7] += p[(size_t)k * sstride];
  const float s = ((acc8[0] + acc8[1]) + (acc8[2] + acc8[3])) + ((acc8[4] + acc8[5]) + (acc8[6] + acc8[7]));
  const int ga = ta * 32 + ra, gb2 = tb * 32 + cb;
  dw[(size_t)n * sample_stride_out + ((size_t)ga * b_total + b_off + gb2) * T + tap] = s;
}

// The same reduction with hundreds of slots (one per workgroup of the persistent weight-gradient kernels), two levels in one
// launch: a block of 256 threads = 64 consecutive outputs x 4 slot lanes (one wave each: a wave's load is 256 contiguous bytes of
// one slot); wave w sums slots w, w + 4, ... with 16 loads in flight, the four waves are combined in a fixed order through LDS.
// Deterministic; 4 rounds of loads for 256 slots where the single-level loop needs 16.  `block`: which 64 outputs of this gradient.
__device__ __forceinline__ void wgrad_reduce1_block(const float* __restrict__ partial, float* __restrict__ dw, int A, int Bc, int T,
                                                    int nslots, int b_total, int b_off, size_t block) {
  const size_t total = (size_t)A * Bc * T;
  const int oi = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const size_t idx = block * 64 + oi;
  float acc = 0.f;
  if (idx < total) {
    const float* p = partial + idx;
    float a8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int k = sl;
    for (; k + 4 * 15 < nslots; k += 4 * 16) {
      float v[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = p[(size_t)(k + 4 * j) * total];
#pragma unroll
      for (int j = 0; j < 16; ++j) a8[j & 7] += v[j];
    }
    for (int j = 0; k < nslots; k += 4, ++j) a8[j & 7] += p[(size_t)k * total];
    acc = ((a8[0] + a8[1]) + (a8[2] + a8[3])) + ((a8[4] + a8[5]) + (a8[6] + a8[7]));
  }
  __shared__ float sR[4][64];
  sR[sl][oi] = acc;
  __syncthreads();
  if (threadIdx.x < 64 && idx < total) {
    const float sum = (sR[0][oi] + sR[1][oi]) + (sR[2][oi] + sR[3][oi]);
    const int cb = idx & 31, ra = (idx >> 5) & 31;
    size_t rest = idx >> 10;
    const int tap = rest % T;
    rest /= T;
    const int tilesB = Bc / 32;
    const int tb = rest % tilesB, ta = rest / tilesB;
    const int ga = ta * 32 + ra, gb2 = tb * 32 + cb;
    dw[((size_t)ga * b_total + b_off + gb2) * T + tap] = sum;
  }
}
__global__ void __launch_bounds__(256) wgrad_reduce1_kernel(const float* __restrict__ partial, float* __restrict__ dw, int A, int Bc,
                                                            int T, int nslots, size_t sample_stride_partial, size_t sample_stride_out,
                                                            int b_total, int b_off) {
  const int n = blockIdx.y;
  wgrad_reduce1_block(partial + (size_t)n * sample_stride_partial, dw + (size_t)n * sample_stride_out, A, Bc, T, nslots, b_total, b_off,
                      blockIdx.x);
}
// All queued slot reductions of a training step in one launch (WgradReduceQueue, kernels_wgrad.h): a block finds its job by binary
// search over the jobs' first blocks.
struct WgradReduceJobs {
  WgradReduceJob job[WgradReduceQueue::kMax];
  int n;
};
__global__ void __launch_bounds__(256) wgrad_reduce_jobs_kernel(WgradReduceJobs J) {
  int lo = 0, hi = J.n - 1;
  while (lo < hi) {  // last job whose first_block <= blockIdx.x
    const int mid = (lo + hi + 1) >> 1;
    if (J.job[mid].first_block <= blockIdx.x) lo = mid;
    else hi = mid - 1;
  }
  const WgradReduceJob& j = J.job[lo];
  wgrad_reduce1_block(j.partial, j.dw, j.A, j.Bc, j.T, j.nslots, j.b_total, j.b_off, blockIdx.x - j.first_block);
}
void wgrad_queue_flush(WgradReduceQueue* q, hipStream_t s) {
  if (!q || q->n <= 0) return;
  WgradReduceJobs J;
  for (int i = 0; i < q->n; ++i) J.job[i] = q->job[i];
  J.n = q->n;
  hipLaunchKernelGGL(wgrad_reduce_jobs_kernel, dim3(q->blocks), dim3(256), 0, s, J);
  CD_HIP(hipGetLastError());
  q->n = 0;
  q->blocks = 0;
}
// the reduction of `partial` as a job of q; false (no queue) if it has to be launched here
static bool wgrad_queue_push(WgradReduceQueue* q, const float* partial, float* dw, int A, int Bc, int T, int nslots, int b_total,
                             int b_off, hipStream_t s) {
  if (!q) return false;
  if (q->n == WgradReduceQueue::kMax) wgrad_queue_flush(q, s);  // (deeper networks than the shipped ones: flush and go on)
  WgradReduceJob& j = q->job[q->n++];
  j.partial = partial; j.dw = dw; j.A = A; j.Bc = Bc; j.T = T; j.nslots = nslots;
  j.b_total = b_total; j.b_off = b_off; j.first_block = q->blocks;
  q->blocks += (unsigned)(((size_t)A * Bc * T + 63) / 64);
  return true;
}

// First level of the slot reduction when there are many slots (the 1x1 convs write 4096 four-KiB partials: a single-level
// reduce is 1024 threads x 4096 serial loads = 75 us of a 100 us weight gradient).  Group g sums its `per` consecutive slots
// in a fixed order into the group's first slot, in place; wgrad_reduce_kernel then sums the group heads (slot_step = per).
__global__ void wgrad_prereduce_kernel(float* __restrict__ partial, size_t total, int nslots, int per) {
  const size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int k0 = blockIdx.y * per, k1 = min(k0 + per, nslots);
  float* p = partial + idx;
  float acc8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int k = k0;
  for (; k + 16 <= k1; k += 16) {
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = p[(size_t)(k + j) * total];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc8[j & 7] += v[j];
  }
  for (; k < k1; ++k) acc8[(k - k0) & 7] += p[(size_t)k * total];
  p[(size_t)k0 * total] = ((acc8[0] + acc8[1]) + (acc8[2] + acc8[3])) + ((acc8[4] + acc8[5]) + (acc8[6] + acc8[7]));
}
// returns the slot step for wgrad_reduce_kernel and updates *nslots to the number of group heads
static int wgrad_prereduce(float* partial, size_t total, int* nslots, hipStream_t s) {
  if (*nslots < 256) return 1;
  const int per = 64, groups = (*nslots + per - 1) / per;
  hipLaunchKernelGGL(wgrad_prereduce_kernel, dim3((unsigned)((total + 255) / 256), (unsigned)groups), dim3(256), 0, s, partial, total,
                     *nslots, per);
  CD_HIP(hipGetLastError());
  *nslots = groups;
  return per;
}

// What a rung left in op.partial, and with it the slot reduction of one launch_wgrad (`nslots` slots of T taps, per sample if
// op.per_sample):
enum WgradSlots {
  SLOTS_CHUNKS,      // wgrad_kernel, a slot per voxel chunk (thousands): launched here; a pre-reduction in groups of 64 from 256 slots
                     // on (not per sample), then the single-level kernel
  SLOTS_WORKGROUPS,  // a slot per workgroup of a persistent 27- or 48-tap kernel (up to 256): a job of the caller's queue if there
                     // is one, else the two-level kernel from 64 slots on and the single-level kernel below
  SLOTS_ROWS_1X1     // wgrad1x1_kernel's workgroups: queued likewise, else always the two-level kernel
};
static void launch_wgrad_reduce(const WgradOp& op, int T, int nslots, WgradSlots kind, hipStream_t s) {
  const int A = op.A, Bc = op.Bc, b_total = op.b_total > 0 ? op.b_total : Bc;
  const size_t total = (size_t)A * Bc * T, sample_stride = (size_t)nslots * total;
  const unsigned samples = op.per_sample ? op.batch : 1;
  if (kind != SLOTS_CHUNKS && wgrad_queue_push(op.aux.queue, op.partial, op.dw, A, Bc, T, nslots, b_total, op.b_off, s)) return;
  static const bool one_level = getenv("CD_WGRAD_REDUCE_1LEVEL") != nullptr;
  if (kind == SLOTS_ROWS_1X1 || (kind == SLOTS_WORKGROUPS && nslots >= 64 && !one_level)) {
    hipLaunchKernelGGL(wgrad_reduce1_kernel, dim3((unsigned)((total + 63) / 64), samples), dim3(256), 0, s, op.partial, op.dw, A, Bc, T,
                       nslots, sample_stride, total, b_total, op.b_off);
  } else {
    const int step = kind == SLOTS_CHUNKS && !op.per_sample ? wgrad_prereduce(op.partial, total, &nslots, s) : 1;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256), samples), dim3(256), 0, s, op.partial, op.dw, A, Bc, T,
                       nslots, sample_stride, total, b_total, op.b_off, step);
  }
  CD_HIP(hipGetLastError());
}

// chunks per sample: enough workgroups to fill the chip, chunks of >= 128 voxels, partial volume <= 32 MiB
int wgrad_chunks(int64_t out_vox, int batch, bool per_sample, int A, int Bc, int T) {
  int64_t want = per_sample ? 8 : (512 + batch - 1) / batch;
  if (T == 1) want = per_sample ? 32 : (4096 + batch - 1) / batch;  // single-wave workgroups, 4 KiB partials: use many
  const int64_t cap = (out_vox + (T == 1 ? 63 : 127)) / (T == 1 ? 64 : 128);
  if (want > cap) want = cap;
  const int64_t per_slot = (int64_t)A * Bc * T * 4;
  int64_t mem = (32ll << 20) / (per_slot * (per_sample ? 1 : batch));
  if (mem < 1) mem = 1;
  if (want > mem) want = mem;
  return (int)(want < 1 ? 1 : want);
}
size_t wgrad_partial_floats(int64_t out_vox, int batch, bool per_sample, int A, int Bc, int T) {
  size_t slots = (size_t)wgrad_chunks(out_vox, batch, per_sample, A, Bc, T) * batch;
  if (T == 27 && slots < 256) slots = 256;  // the persistent stride-1 kernel writes one partial per workgroup
  return slots * A * Bc * T;
}

// the generic kernel: any taps and strides, a slot per voxel chunk (and sample, unless per_sample)
static void launch_wgrad_chunked(const WgradOp& op, int* nslots, hipStream_t s) {
  const ConvGeom& k = op.geom;
  const int A = op.A, Bc = op.Bc, T = k.kd * k.kh * k.kw;
  WgradArgs a;
  a.g = op.g; a.x = op.x; a.A = A; a.Bc = Bc; a.xld = op.xld; a.xoff = op.xoff;
  a.Dg = k.out.d; a.Hg = k.out.h; a.Wg = k.out.w; a.Dx = k.in.d; a.Hx = k.in.h; a.Wx = k.in.w;
  a.KD = k.kd; a.KH = k.kh; a.KW = k.kw; a.SZ = k.sz; a.S = k.sh; a.batch = op.batch; a.per_sample = op.per_sample ? 1 : 0;
  a.nchunks = wgrad_chunks(k.out.vox(), op.batch, op.per_sample, A, Bc, T);
  int cv = (int)((k.out.vox() + a.nchunks - 1) / a.nchunks);
  a.chunk_vox = (cv + 1) & ~1;
  a.partial = op.partial;
  dim3 grid((unsigned)(a.nchunks * op.batch), (unsigned)((A / 32) * (Bc / 32)));
  // few taps per wave => small accumulator footprint => many resident waves to hide the operand-load latency
  if (T == 1) hipLaunchKernelGGL(wgrad_kernel<1>, grid, dim3(64), 0, s, a);  // one wave per workgroup (nothing to split)
  else if (T <= 4) hipLaunchKernelGGL(wgrad_kernel<1>, grid, dim3(64 * T), 0, s, a);
  else if (T <= 27) hipLaunchKernelGGL(wgrad_kernel<3>, grid, dim3(64 * ((T + 2) / 3)), 0, s, a);
  else hipLaunchKernelGGL(wgrad_kernel<4>, grid, dim3(64 * ((T + 3) / 4)), 0, s, a);
  CD_HIP(hipGetLastError());
  *nslots = op.per_sample ? a.nchunks : a.nchunks * op.batch;
}

bool wgrad_x_norm_supported(const ConvGeom& g) {
  return g.kd * g.kh * g.kw == 27 && g.sz == 1 && g.sh == 1 && g.out.vox() == g.in.vox() && wgrad_f16x2_eligible(g.out);
}

// The ladder: the first rung that takes the shape runs, then the slot reduction that goes with it.
void launch_wgrad(const WgradOp& op, hipStream_t s) {
  const ConvGeom& k = op.geom;
  const int A = op.A, Bc = op.Bc, T = k.kd * k.kh * k.kw;
  CD_REQUIRE(A % 32 == 0 && Bc % 32 == 0, "wgrad: channel counts must be multiples of 32");
  CD_REQUIRE(!op.xcoef || (!op.per_sample && wgrad_x_norm_supported(k)),
             "wgrad: a normalised x operand is only read by the fp16-pipe 3x3x3 kernel");
  CD_REQUIRE(!op.per_sample || !op.aux.queue, "wgrad: per-sample reductions are not queued");
  const bool same_grid = k.sz == 1 && k.sh == 1 && k.out.vox() == k.in.vox();
  const bool conv333 = T == 27 && same_grid && !op.per_sample;  // 27 taps, stride 1, same grid, summed over the batch
  char cat[96];
  std::snprintf(cat, sizeof cat, "wgrad T%d C%dx%d n%ld", T, A, Bc, (long)k.out.vox());
  prof::Scope scope(cat, s, 2.0 * T * A * Bc * (double)k.out.vox() * op.batch,
                    4.0 * op.batch * ((double)k.out.vox() * A + (double)k.in.vox() * Bc));
  int nslots = 0;
  WgradSlots kind = SLOTS_WORKGROUPS;
  if (conv333 && wgrad_f16x2_eligible(k.out)) {  // 1. stride-1 3x3x3 on the fp16 pipe
    CD_REQUIRE(try_launch_wgrad_f16x2(op, &nslots, s), "internal: wgrad f16x2");
  } else if (conv333 && try_launch_wgrad_flat(op, &nslots, s)) {  // 2. stride-1 3x3x3 in fp32: LDS-staged, persistent
  } else if (k.kh == 4 && k.kw == 4 && k.sh == 2 && !op.per_sample &&
             try_launch_wgrad_strided_f16x2(op, &nslots, s)) {  // 3. the strided (KD,4,4) convs on the fp16 pipe
  } else if (T == 1 && same_grid && try_launch_wgrad1x1(op, &nslots, s)) {  // 4. 1x1x1 streaming
    kind = SLOTS_ROWS_1X1;
  } else {  // 5. any taps and strides
    launch_wgrad_chunked(op, &nslots, s);
    kind = SLOTS_CHUNKS;
  }
  launch_wgrad_reduce(op, T, nslots, kind, s);
}

}  // namespace cd
