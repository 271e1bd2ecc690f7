// Kernels of the classifier two-sample test (include/calodiff.h, "classifier two-sample test"): the reference's DNN
// (calodiffusion/tests/hgcal_metrics.py:185-209: Linear -> LeakyReLU -> Dropout, num_layer + 1 times, then Linear -> 1) trained with
// BCEWithLogitsLoss (:68-84) on batches of at most CD_CLS_MAX_BATCH rows, and its evaluation pass (:105-123).
//
// cls_gemm_kernel.  One kernel serves the three matrix products of a layer,
//   forward  y  (rows, n_out) = x . w^T       A = x (k contiguous),  B = w   (k contiguous)
//   dgrad    dx (rows, n_in)  = g . w         A = g (k contiguous),  B = w^T (k strided)
//   wgrad    dw (n_out, n_in) = g^T . x       A = g^T (k strided),   B = x^T (k strided), k = the batch: no split-K, no atomics
// as C (M, N) = A (M, K) . B (N, K)^T with both operands addressed by (row stride, k stride).  Every product is the exact
// three-term bf16 split of split16.h (bf16x3: x = x1 + x2 + x3, 24 bits, fp32 range) on v_mfma_f32_32x32x16_bf16 with fp32
// accumulation: the six partial products down to 2^-16 of the largest, smallest first.  A workgroup of WM x 2 waves owns a
// (32 WM) x 64 tile of C, a wave one 32 x 32 MFMA tile.  K runs in chunks of 64: the staging threads load fp32 (the next chunk's
// loads are in flight under this chunk's MFMAs), split each group of four k once and write the three bf16 images to LDS, 144 bytes
// a row (128 + 16 of padding: the 16 rows of a ds_read_b128 lane group land on 64 different banks), so an operand fragment is one
// 16-byte read per term.  Rows and k beyond the matrix are staged as zeros: nothing is read or written outside the caller's
// tensors, and padded columns cannot leak (a zero operand row gives an exactly zero product).  A C element is the sum of four
// accumulators, (p0 + p1) + (p2 + p3), accumulator (16-step mod 4) taking its 16-steps of k in ascending order (a quarter of
// the sequential fp32 roundings each), whatever the tile shape or grid: results are bitwise reproducible.
// Epilogue (forward): + bias[n], LeakyReLU, dropout.  The dropout decision of (row-in-batch r, column c) of layer l at step s is
// word r & 3 of Philox4x32-10 (philox.h) at counter {c, r >> 2, l, lo32(s)} under key {lo32(seed), hi32(seed) ^ hi32(s)}: kept
// where the word is >= floor(p 2^32), scaled by 1 / (1 - p).  The four rows r & ~3 ... of a column share one Philox call, and
// an accumulator register quad (reg & 3) of the 32x32 C/D map is exactly such a row group.  cls_gate_kernel (backward) and
// cls_mask_kernel (the bytes a test reads) call the same device function; nothing is stored between forward and backward.
//
// cls_gate_kernel.  g = dy * mask * scale * act'(y) and its column sums db.  act' is read off the layer's OUTPUT y: a kept
// element is scale * leaky(z), which has the sign of z for slope >= 0, so act' = (y > 0 ? 1 : slope) -- z == 0 takes the slope
// as torch's leaky_relu_backward does.  A workgroup takes 64 columns, its four waves interleaved groups of four rows; the four
// partial column sums are added in wave order.  For the layer before the output layer dy is the outer product dz[r] w_out[c]
// (never materialised) and the same pass leaves dw_out[c] = sum_r dz[r] y[r][c].
#include "kernels_classifier.h"
#include "conv_internal.h"
#include "philox.h"

#include <cmath>

namespace cd {
namespace {

constexpr int kClsChunk = 64;  // k per LDS image
constexpr int kClsRowB = 144;  // bytes of an image row: 64 bf16 + 16 bytes of padding

__device__ __forceinline__ void cls_dropout_words(const ClsDropout& d, int rowgroup, int col, uint32_t w[4]) {
  w[0] = (uint32_t)col; w[1] = (uint32_t)rowgroup; w[2] = (uint32_t)d.layer; w[3] = (uint32_t)d.step;
  philox4x32_10(w, (uint32_t)d.seed, (uint32_t)(d.seed >> 32) ^ (uint32_t)(d.step >> 32));
}

struct ClsGemmArgs {
  const float* A;
  int64_t sam, sak;  // A(m, k) = A[m * sam + k * sak]
  const float* B;
  int64_t sbn, sbk;  // B(n, k) = B[n * sbn + k * sbk]
  float* C;
  int64_t ldc;
  int M, N, K;
  const float* bias;  // [N] or null
  int act;
  float slope;
  ClsDropout drop;
};

// the staging of a ROWS x 64 operand chunk by T threads: groups of four consecutive k
template <int ROWS, int T, bool KCONTIG>
struct ClsStage {
  static constexpr int G = ROWS * 16 / T;
  static_assert(G * T == ROWS * 16, "whole groups per thread");
  f32x4 v[G];
  // KCONTIG: sixteen threads walk a row's 64 k (256 consecutive bytes); else consecutive threads take consecutive rows of one k
  static __device__ __forceinline__ void where(int gi, int& row, int& q) {
    if (KCONTIG) { row = gi >> 4; q = gi & 15; } else { row = gi % ROWS; q = gi / ROWS; }
  }
  __device__ __forceinline__ void fetch(const float* __restrict__ P, int64_t sr, int64_t sk, int r0, int R, int k0, int K, int t) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      int row, q;
      where(t + g * T, row, q);
      const int rg = r0 + row;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = k0 + 4 * q + j;
        v[g][j] = (rg < R && k < K) ? P[(int64_t)rg * sr + (int64_t)k * sk] : 0.f;  // the address is formed for elements of the matrix only
      }
    }
  }
  __device__ __forceinline__ void store(char* img, int t) const {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      int row, q;
      where(t + g * T, row, q);
      u32x2 t1, t2, t3;
      split3(v[g], t1, t2, t3);
      char* at = img + row * kClsRowB + q * 8;
      *(u32x2*)(at) = t1;
      *(u32x2*)(at + ROWS * kClsRowB) = t2;
      *(u32x2*)(at + 2 * ROWS * kClsRowB) = t3;
    }
  }
};

template <int WM, bool AK, bool BK>
__global__ void __launch_bounds__(128 * WM) cls_gemm_kernel(ClsGemmArgs a) {
  constexpr int BM = 32 * WM, BN = 64, T = 128 * WM;
  __shared__ __attribute__((aligned(16))) char img_a[3 * BM * kClsRowB];
  __shared__ __attribute__((aligned(16))) char img_b[3 * BN * kClsRowB];
  const int t = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  ClsStage<BM, T, AK> sa;
  ClsStage<BN, T, BK> sb;
  f32x16 part[4];  // four accumulators, one per 16-step of a chunk: a quarter of the sequential roundings each
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) part[j][i] = 0.f;
  sa.fetch(a.A, a.sam, a.sak, m0, a.M, 0, a.K, t);
  sb.fetch(a.B, a.sbn, a.sbk, n0, a.N, 0, a.K, t);
  const char* fa = img_a + (32 * wm + r) * kClsRowB + h * 16;
  const char* fb = img_b + (32 * wn + r) * kClsRowB + h * 16;
  auto mfma6 = [&](f32x16 acc, int s) {
    u32x4 av[3], bv[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      av[e] = *(const u32x4*)(fa + e * BM * kClsRowB + s * 32);
      bv[e] = *(const u32x4*)(fb + e * BN * kClsRowB + s * 32);
    }
    acc = MFMA_BF16(av[2], bv[0], acc);
    acc = MFMA_BF16(av[1], bv[1], acc);
    acc = MFMA_BF16(av[0], bv[2], acc);
    acc = MFMA_BF16(av[1], bv[0], acc);
    acc = MFMA_BF16(av[0], bv[1], acc);
    return MFMA_BF16(av[0], bv[0], acc);
  };
  for (int k0 = 0; k0 < a.K; k0 += kClsChunk) {
    sa.store(img_a, t);
    sb.store(img_b, t);
    __syncthreads();
    if (k0 + kClsChunk < a.K) {
      sa.fetch(a.A, a.sam, a.sak, m0, a.M, k0 + kClsChunk, a.K, t);
      sb.fetch(a.B, a.sbn, a.sbk, n0, a.N, k0 + kClsChunk, a.K, t);
    }
    const int left = a.K - k0;  // a chunk runs the 16-steps it has
    part[0] = mfma6(part[0], 0);
    if (left > 16) part[1] = mfma6(part[1], 1);
    if (left > 32) part[2] = mfma6(part[2], 2);
    if (left > 48) part[3] = mfma6(part[3], 3);
    __syncthreads();
  }

  // C/D map of the 32x32 tile: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const int n = n0 + 32 * wn + r;
  if (n >= a.N) return;
  const float bias = a.bias ? a.bias[n] : 0.f;
  const f32x16 acc = (part[0] + part[1]) + (part[2] + part[3]);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int mq = m0 + 32 * wm + 8 * q + 4 * h;  // a multiple of four: one dropout row group
    if (mq >= a.M) continue;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (a.drop.threshold) cls_dropout_words(a.drop, mq >> 2, n, w);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v = acc[4 * q + i] + bias;
      if (a.act) v = v > 0.f ? v : v * a.slope;
      if (a.drop.threshold) v = w[i] >= a.drop.threshold ? v * a.drop.scale : 0.f;
      if (mq + i < a.M) a.C[(int64_t)(mq + i) * a.ldc + n] = v;
    }
  }
}

template <bool AK, bool BK>
void launch_cls_gemm(const ClsGemmArgs& a, hipStream_t s) {
  // 64 x 64 tiles where they fill the chip, else 32 x 64 (the forward pass of a 256-row batch: 128 -> 256 workgroups)
  const int64_t big = (int64_t)((a.M + 63) / 64) * ((a.N + 63) / 64);
  if (big >= 256) {
    hipLaunchKernelGGL((cls_gemm_kernel<2, AK, BK>), dim3((unsigned)((a.N + 63) / 64), (unsigned)((a.M + 63) / 64)), dim3(256), 0, s, a);
  } else {
    hipLaunchKernelGGL((cls_gemm_kernel<1, AK, BK>), dim3((unsigned)((a.N + 63) / 64), (unsigned)((a.M + 31) / 32)), dim3(128), 0, s, a);
  }
  CD_HIP(hipGetLastError());
}

struct ClsGateArgs {
  const float* dy;      // (rows, n) or null
  const float* dz;      // [rows], with w_next where dy is null
  const float* w_next;  // [n]
  float* dw_next;       // [n] or null
  const float* y;       // (rows, n): the layer's output
  const uint8_t* mask;  // (rows, n) or null
  int act;
  float slope;
  ClsDropout drop;
  float* g;   // (rows, n)
  float* db;  // [n]
  int rows, n;
};

__global__ void __launch_bounds__(256) cls_gate_kernel(ClsGateArgs a) {
  __shared__ float red[2][4][64];
  const int t = threadIdx.x, cl = t & 63, rl = t >> 6, c = blockIdx.x * 64 + cl, N = a.n;
  float sdb = 0.f, sdw = 0.f;
  if (c < N) {
    const float wn = a.dy ? 0.f : a.w_next[c];
    const int groups = (a.rows + 3) >> 2;
    for (int rg = rl; rg < groups; rg += 4) {
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      if (!a.mask && a.drop.threshold) cls_dropout_words(a.drop, rg, c, w);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 4 * rg + i;
        if (r < a.rows) {
          const int64_t at = (int64_t)r * N + c;
          const float yv = a.y[at];
          const float dyv = a.dy ? a.dy[at] : a.dz[r] * wn;
          const bool keep = a.mask ? a.mask[at] != 0 : w[i] >= a.drop.threshold;
          float g = 0.f;
          if (keep) {
            g = dyv * a.drop.scale;
            if (a.act) g = yv > 0.f ? g : g * a.slope;
          }
          a.g[at] = g;
          sdb += g;
          if (a.dw_next) sdw += a.dz[r] * yv;
        }
      }
    }
  }
  red[0][rl][cl] = sdb;
  red[1][rl][cl] = sdw;
  __syncthreads();
  if (rl == 0 && c < N) {
    a.db[c] = ((red[0][0][cl] + red[0][1][cl]) + red[0][2][cl]) + red[0][3][cl];
    if (a.dw_next) a.dw_next[c] = ((red[1][0][cl] + red[1][1][cl]) + red[1][2][cl]) + red[1][3][cl];
  }
}

// a wave per row: lane j adds columns j, j + 64, ... in ascending order, the lanes combine by a fixed butterfly
__global__ void __launch_bounds__(256) cls_rowdot_kernel(const float* __restrict__ hmat, const float* __restrict__ w, const float* __restrict__ b,
                                                        float* __restrict__ z, int rows, int n) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* hr = hmat + (int64_t)row * n;
  double s = 0.0;  // fp32 products are exact in fp64: the logit, a sum with cancellation, is rounded once
  for (int c = lane; c < n; c += 64) s += (double)hr[c] * (double)w[c];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) z[row] = (float)(s + (double)b[0]);
}

__global__ void __launch_bounds__(256) cls_gather_kernel(const float* __restrict__ x, const float* __restrict__ labels, int64_t rows_total,
                                                        const int32_t* __restrict__ idx, int d, float* __restrict__ xb, float* __restrict__ yb) {
  const int r = blockIdx.x;
  const int64_t ix = idx[r];
  const bool ok = ix >= 0 && ix < rows_total;  // checked before the row's address is formed
  const float nan = __uint_as_float(0x7fc00000u);
  for (int c = threadIdx.x; c < d; c += 256) xb[(int64_t)r * d + c] = ok ? x[ix * d + c] : nan;
  if (yb && threadIdx.x == 0) yb[r] = ok && labels ? labels[ix] : (labels ? nan : 0.f);
}

// one workgroup, rows <= 256: max(z, 0) - z y + log1p(exp(-|z|)) in fp64, summed by a fixed tree
__global__ void __launch_bounds__(256) cls_loss_kernel(const float* __restrict__ z, const float* __restrict__ y, int rows, double* __restrict__ loss,
                                                      float* __restrict__ dz, float* __restrict__ db_out) {
  __shared__ double ls[256];
  __shared__ float ds[256];
  const int t = threadIdx.x;
  double l = 0.0;
  float d = 0.f;
  if (t < rows) {
    const double zd = (double)z[t], yd = (double)y[t];
    l = fmax(zd, 0.0) - zd * yd + log1p(exp(-fabs(zd)));
    d = (float)((1.0 / (1.0 + exp(-zd)) - yd) / (double)rows);
    dz[t] = d;
  }
  ls[t] = l;
  ds[t] = d;
  __syncthreads();
  for (int half = 128; half >= 1; half >>= 1) {
    if (t < half) {
      ls[t] += ls[t + half];
      ds[t] += ds[t + half];
    }
    __syncthreads();
  }
  if (t == 0) {
    *loss = ls[0] / (double)rows;
    if (db_out) *db_out = ds[0];
  }
}

__global__ void __launch_bounds__(256) cls_mask_kernel(ClsDropout drop, int rows, int n, uint8_t* __restrict__ mask) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int groups = (rows + 3) >> 2;
  if (i >= (int64_t)groups * n) return;
  const int rg = (int)(i / n), c = (int)(i - (int64_t)rg * n);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  if (drop.threshold) cls_dropout_words(drop, rg, c, w);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (4 * rg + k < rows) mask[(int64_t)(4 * rg + k) * n + c] = w[k] >= drop.threshold ? 1 : 0;
}

}  // namespace

ClsDropout cls_dropout(float p, uint64_t seed, uint64_t step, int layer) {
  ClsDropout d;
  d.seed = seed; d.step = step; d.layer = layer;
  if (p > 0.f) {
    const double thr = std::floor((double)p * 4294967296.0);
    d.threshold = thr >= 4294967295.0 ? 4294967295u : (uint32_t)thr;
    d.scale = (float)(1.0 / (1.0 - (double)p));
  }
  return d;
}

void launch_cls_linear(const float* x, const float* w, const float* bias, float* y, int rows, int n_in, int n_out, int act, float slope,
                       const ClsDropout& drop, hipStream_t s) {
  ClsGemmArgs a{};
  a.A = x; a.sam = n_in; a.sak = 1;
  a.B = w; a.sbn = n_in; a.sbk = 1;
  a.C = y; a.ldc = n_out;
  a.M = rows; a.N = n_out; a.K = n_in;
  a.bias = bias; a.act = act; a.slope = slope; a.drop = drop;
  launch_cls_gemm<true, true>(a, s);
}

void launch_cls_dgrad(const float* g, const float* w, float* dx, int rows, int n_in, int n_out, hipStream_t s) {
  ClsGemmArgs a{};
  a.A = g; a.sam = n_out; a.sak = 1;
  a.B = w; a.sbn = 1; a.sbk = n_in;
  a.C = dx; a.ldc = n_in;
  a.M = rows; a.N = n_in; a.K = n_out;
  launch_cls_gemm<true, false>(a, s);
}

void launch_cls_wgrad(const float* g, const float* x, float* dw, int rows, int n_in, int n_out, hipStream_t s) {
  ClsGemmArgs a{};
  a.A = g; a.sam = 1; a.sak = n_out;
  a.B = x; a.sbn = 1; a.sbk = n_in;
  a.C = dw; a.ldc = n_in;
  a.M = n_out; a.N = n_in; a.K = rows;
  launch_cls_gemm<false, false>(a, s);
}

void launch_cls_gate(const float* dy, const float* dz, const float* w_next, float* dw_next, const float* y, const uint8_t* mask, int act,
                     float slope, const ClsDropout& drop, float* g, float* db, int rows, int n_out, hipStream_t s) {
  ClsGateArgs a{};
  a.dy = dy; a.dz = dz; a.w_next = w_next; a.dw_next = dw_next; a.y = y; a.mask = mask; a.act = act; a.slope = slope; a.drop = drop;
  a.g = g; a.db = db; a.rows = rows; a.n = n_out;
  hipLaunchKernelGGL(cls_gate_kernel, dim3((unsigned)((n_out + 63) / 64)), dim3(256), 0, s, a);
  CD_HIP(hipGetLastError());
}

void launch_cls_rowdot(const float* h, const float* w, const float* b, float* z, int rows, int n, hipStream_t s) {
  hipLaunchKernelGGL(cls_rowdot_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, h, w, b, z, rows, n);
  CD_HIP(hipGetLastError());
}

void launch_cls_gather(const float* x, const float* labels, int64_t rows_total, const int32_t* idx, int count, int d, float* xb, float* yb,
                       hipStream_t s) {
  hipLaunchKernelGGL(cls_gather_kernel, dim3((unsigned)count), dim3(256), 0, s, x, labels, rows_total, idx, d, xb, yb);
  CD_HIP(hipGetLastError());
}

void launch_cls_loss(const float* z, const float* y, int rows, double* loss, float* dz, float* db_out, hipStream_t s) {
  hipLaunchKernelGGL(cls_loss_kernel, dim3(1), dim3(256), 0, s, z, y, rows, loss, dz, db_out);
  CD_HIP(hipGetLastError());
}

void launch_cls_mask(const ClsDropout& drop, int rows, int n, uint8_t* mask, hipStream_t s) {
  const int64_t cells = (int64_t)((rows + 3) / 4) * n;
  hipLaunchKernelGGL(cls_mask_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, drop, rows, n, mask);
  CD_HIP(hipGetLastError());
}

}  // namespace cd
