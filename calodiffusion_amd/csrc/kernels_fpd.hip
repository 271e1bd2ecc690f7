// Bootstrap moments for the Frechet physics distance (include/calodiff.h, "Frechet physics distance"): the mean and covariance of
// rows of a float64 feature matrix gathered through index lists, what jetnet.evaluation.fpd computes per batch with np.mean and
// np.cov for the reference's FDP (calodiffusion/train/evaluate.py:66-79).
//
// With y_k = x[idx_k] - centre the work is the Gram matrix G = Y^T Y of an (n, d) matrix, n up to 50 000 and d = 226 for
// Datasets 2 and 3: it runs on v_mfma_f64_16x16x4_f64.  Y gets one more column, the constant 1 at index d, so that G[i][d] is
// the column sum S_i from the same products; the d + 1 columns are padded with zeros to T tiles of 16.  The A and the B operand
// of that instruction have the same lane map (lane l: row l >> 4 of the four, column l & 15 of the tile), so one image of four
// rows serves both sides of every tile pair.  Only tile pairs ti <= tj are computed.
//
// gram kernel: a workgroup of eight waves owns one slice of CD_FPD_SLICE_ROWS consecutive list positions of one set and all of
// its T (T + 1) / 2 tile pairs, pair p on wave p % 8 in accumulator p / 8 (at most 20 accumulators of 8 registers a wave, two
// waves a SIMD).  The rows come through LDS 16 at a time: 32 lanes read 256 consecutive bytes of a gathered row, subtract the
// centre and store; the next 16 rows are on their way in registers, and the list entries of the 16 after them, while the MFMAs
// of these run.  An index is compared with [0, rows) before the row's address is formed; a bad one loads nothing, raises the
// slice's flag and reports its position.
// Each wave stores its accumulators as they lie in registers (value r of lane l at r * 64 + l).
// moments kernel: one workgroup per tile pair sums the slices' partial tiles in ascending slice order -- the split depends on n
// alone and nothing is accumulated with atomics, so a set has the same bits in any call -- and forms mean and cov.  The C/D map
// of the f64 instruction is col = l & 15, row = (l >> 4) + 4 r (NOT the f32 one).  Elements i <= j are stored to [i][j] and
// [j][i] from the same register.
#include "guarded.h"

namespace cd {
namespace {

constexpr int kFpdWaves = 8, kFpdThreads = 64 * kFpdWaves;
constexpr int kFpdChunk = 16;                                      // rows in LDS at a time: thread t stages row t >> 5
constexpr int kFpdMaxTiles = (CD_FPD_MAX_D + 1 + 15) / 16;         // 17
constexpr int kFpdAcc = (kFpdMaxTiles * (kFpdMaxTiles + 1) / 2 + kFpdWaves - 1) / kFpdWaves;  // 20 tile pairs a wave
constexpr int kFpdCols = (kFpdMaxTiles * 16 + 31) / 32;            // 9 columns a staging thread
constexpr int kFpdStride = (kFpdMaxTiles | 1) * 16;                // doubles between LDS rows (largest)
constexpr int kFpdGroup = 64;                                      // sets a launch takes its counts for, as kernel arguments
static_assert(kFpdThreads == 32 * kFpdChunk, "a staging thread per 32 columns of a row");

struct FpdCounts {
  int n[kFpdGroup];
};

typedef double fpd_acc __attribute__((ext_vector_type(4)));

// tile pair p of the T (T + 1) / 2 pairs ti <= tj, row-major
__device__ __host__ __forceinline__ void fpd_pair(int p, int T, int& ti, int& tj) {
  int a = 0;
  while (p >= T - a) {
    p -= T - a;
    ++a;
  }
  ti = a;
  tj = a + p;
}
__device__ __forceinline__ int fpd_pair_index(int ti, int tj, int T) { return ti * T - ti * (ti - 1) / 2 + (tj - ti); }

struct FpdArgs {
  const double* x;
  int64_t rows;
  int d, T;
  const double* centre;
  const int32_t* idx;
  int64_t idx_stride;
  int set0, slices;  // first set of this launch; slices of workspace per set
  double* part;      // [set][slice][pair][256]
  int32_t* flags;    // [set][slice]
  int32_t* status;
};

// Q: accumulators a wave holds, 8 Q >= pairs.  A wave's slot beyond the last pair works on tile pair (0, 0) and stores nothing, which
// keeps the MFMA loop free of branches.
template <int Q>
__global__ __launch_bounds__(kFpdThreads) void fpd_gram_kernel(FpdArgs a, FpdCounts counts) {
  __shared__ double image[kFpdChunk * kFpdStride];
  const int set = a.set0 + blockIdx.y, slice = blockIdx.x;
  const int n = counts.n[blockIdx.y];
  const int k_lo = slice * CD_FPD_SLICE_ROWS;
  if (k_lo >= n) return;
  const int k_hi = n < k_lo + CD_FPD_SLICE_ROWS ? n : k_lo + CD_FPD_SLICE_ROWS;
  const int T = a.T, W = T * 16, stride = (T | 1) * 16, pairs = T * (T + 1) / 2, d = a.d;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;

  unsigned at[Q];  // first column in the image of the pair's two tiles: ti * 16 | tj * 16 << 16 (wave-uniform)
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int p = wave + kFpdWaves * q;
    int ti = 0, tj = 0;
    if (p < pairs) fpd_pair(p, T, ti, tj);
    at[q] = (unsigned)(ti * 16) | (unsigned)(tj * 16) << 16;
  }
  fpd_acc acc[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) acc[q] = fpd_acc{0.0, 0.0, 0.0, 0.0};

  // staging: row r of the 16, columns c0, c0 + 32, ...
  const int r = threadIdx.x >> 5, c0 = threadIdx.x & 31;
  const int32_t* list = a.idx + (int64_t)set * a.idx_stride;
  int bad = 0;
  double cen[kFpdCols], v[kFpdCols];
#pragma unroll
  for (int m = 0; m < kFpdCols; ++m) cen[m] = c0 + 32 * m < d ? a.centre[c0 + 32 * m] : 0.0;
  // Three stages in flight: the index of chunk c + 2 is loaded while the row of chunk c + 1 is on its way (raw values, in v) and
  // chunk c is in LDS under the MFMAs, so neither the index nor the row latency is waited for with the matrix pipe idle.
  int ix_ahead = 0;                       // list entry of the chunk after the one in v (0 where there is none)
  bool listed = false, ok = false;        // of the chunk in v: has a list entry; the entry is a row of x
  auto fetch_index = [&](int k0) {        // entries beyond the set's count are never read
    ix_ahead = k0 + r < k_hi ? list[k0 + r] : 0;
  };
  auto fetch_row = [&](int k0) {          // the row of list position k0 + r, whose entry is in ix_ahead
    const int k = k0 + r;
    const int64_t ix = ix_ahead;
    listed = k < k_hi;
    ok = listed && ix >= 0 && ix < a.rows;
    if (listed && !ok) {
      bad = 1;
      if (c0 == 0) atomicMax(a.status, (int32_t)(1 + (int64_t)set * a.idx_stride + k));
    }
    const double* row = a.x + (ok ? ix : 0) * d;  // formed from a checked index only; read only under `ok`
#pragma unroll
    for (int m = 0; m < kFpdCols; ++m) {
      const int col = c0 + 32 * m;
      v[m] = 0.0;
      if (ok && col < d) v[m] = row[col];
    }
  };
  const int lg = lane >> 4, lc = lane & 15;
  fetch_index(k_lo);
  fetch_row(k_lo);
  fetch_index(k_lo + kFpdChunk);
  for (int k0 = k_lo; k0 < k_hi; k0 += kFpdChunk) {
#pragma unroll
    for (int m = 0; m < kFpdCols; ++m) {
      const int col = c0 + 32 * m;
      const double y = ok && col < d ? v[m] - cen[m] : (col == d && listed ? 1.0 : 0.0);
      if (col < W) image[r * stride + col] = y;
    }
    __syncthreads();
    if (k0 + kFpdChunk < k_hi) {
      fetch_row(k0 + kFpdChunk);
      fetch_index(k0 + 2 * kFpdChunk);
    }
#pragma unroll 1
    for (int ks = 0; ks < kFpdChunk / 4; ++ks) {  // the operands of pair q + 1 are read before the MFMA of pair q is issued
      const double* four = image + (ks * 4 + lg) * stride + lc;
      double fa = four[at[0] & 0xffffu], fb = four[at[0] >> 16];
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        double na = 0.0, nb = 0.0;
        if (q + 1 < Q) {
          na = four[at[q + 1] & 0xffffu];
          nb = four[at[q + 1] >> 16];
        }
        acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa, fb, acc[q], 0, 0, 0);
        fa = na;
        fb = nb;
      }
    }
    __syncthreads();
  }
  double* out = a.part + ((int64_t)set * a.slices + slice) * pairs * 256;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    if (wave + kFpdWaves * q < pairs) {
      double* o = out + (int64_t)(wave + kFpdWaves * q) * 256 + lane;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[64 * e] = acc[q][e];
    }
  }
  const int any = __syncthreads_or(bad);
  if (threadIdx.x == 0) a.flags[(int64_t)set * a.slices + slice] = any;
}

// grid (pairs, sets of the launch), 256 threads: thread t owns value t >> 6 of lane t & 63 of the pair's tile
__global__ __launch_bounds__(256) void fpd_moments_kernel(FpdArgs a, FpdCounts counts, double* __restrict__ mean, double* __restrict__ cov) {
  __shared__ double S[32];
  __shared__ int bad_set;
  const int set = a.set0 + blockIdx.y, n = counts.n[blockIdx.y], d = a.d, T = a.T, pairs = T * (T + 1) / 2;
  const int ns = (n + CD_FPD_SLICE_ROWS - 1) / CD_FPD_SLICE_ROWS;
  const int t = threadIdx.x;
  int ti, tj;
  fpd_pair((int)blockIdx.x, T, ti, tj);
  const double* part = a.part + (int64_t)set * a.slices * pairs * 256;
  const int64_t slice_step = (int64_t)pairs * 256;
  if (t < 32) {  // S_i = G[i][d] for the 16 rows and the 16 columns of this pair: tile pair (i / 16, T - 1), row i % 16, column d % 16
    const int i = (t < 16 ? ti : tj) * 16 + (t & 15), row = i & 15;
    const double* src = part + (int64_t)fpd_pair_index(i >> 4, T - 1, T) * 256 + (row >> 2) * 64 + (row & 3) * 16 + (d & 15);
    double s = 0.0;
    for (int sl = 0; sl < ns; ++sl) s += src[sl * slice_step];
    S[t] = s;
  }
  if (t == 32) {
    int any = 0;
    for (int sl = 0; sl < ns; ++sl) any |= a.flags[(int64_t)set * a.slices + sl];
    bad_set = any;
  }
  __syncthreads();
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const int rg = t >> 6, l = t & 63;
  const int ii = (l >> 4) + 4 * rg, jj = l & 15;  // the f64 C/D map
  const int i = ti * 16 + ii, j = tj * 16 + jj;
  const double* src = part + (int64_t)blockIdx.x * 256 + t;
  double g = 0.0;
  for (int sl = 0; sl < ns; ++sl) g += src[sl * slice_step];
  if (i <= j && j < d) {
    const double c = bad_set ? nan : (g - S[ii] * S[16 + jj] / (double)n) / (double)(n - 1);
    cov[((int64_t)set * d + i) * d + j] = c;
    cov[((int64_t)set * d + j) * d + i] = c;
  }
  if (ti == tj && t < 16) {  // the diagonal pairs write the mean of their 16 columns
    const int c = ti * 16 + t;
    if (c < d) mean[(int64_t)set * d + c] = bad_set ? nan : a.centre[c] + S[t] / (double)n;
  }
}

int fpd_tiles(int d) { return (d + 1 + 15) / 16; }

// accumulators a wave: the instantiation for 1, up to 6, 9, 12, 15 and 17 tiles (8 Q >= T (T + 1) / 2)
int fpd_class(int T) { return T <= 1 ? 1 : T <= 6 ? 3 : T <= 9 ? 6 : T <= 12 ? 10 : T <= 15 ? 15 : kFpdAcc; }

size_t fpd_bytes(int d, int sets, int max_count) {
  const size_t T = (size_t)fpd_tiles(d), slices = ((size_t)max_count + CD_FPD_SLICE_ROWS - 1) / CD_FPD_SLICE_ROWS;
  return (size_t)sets * slices * (T * (T + 1) / 2 * 2048 + 256);
}

}  // namespace
}  // namespace cd

extern "C" {

size_t cd_fpd_workspace_bytes(int d, int sets, int max_count) {
  if (d < 1 || d > CD_FPD_MAX_D || sets < 1 || max_count < 2) {
    set_error("cd_fpd_workspace_bytes: needs 1 <= d <= " + std::to_string(CD_FPD_MAX_D) + ", sets >= 1 and max_count >= 2, got d = " +
              std::to_string(d) + ", sets = " + std::to_string(sets) + ", max_count = " + std::to_string(max_count));
    return 0;
  }
  return fpd_bytes(d, sets, max_count);
}

int cd_fpd_moments(const double* x, int64_t rows, int d, const double* centre, const int32_t* idx, int64_t idx_stride,
                   const int32_t* counts, int sets, double* mean, double* cov, int32_t* status, void* workspace, size_t workspace_bytes,
                   void* stream) {
  return guarded([&] {
    CD_REQUIRE(x && centre && idx && counts && mean && cov && status && workspace,
               "cd_fpd_moments: x, centre, idx, counts, mean, cov, status and workspace must not be null");
    CD_REQUIRE(d >= 1 && d <= CD_FPD_MAX_D, "cd_fpd_moments: d must be in [1, " + std::to_string(CD_FPD_MAX_D) + "], got " + std::to_string(d));
    CD_REQUIRE(rows > 0, "cd_fpd_moments: rows must be positive, got " + std::to_string(rows));
    CD_REQUIRE(sets >= 1, "cd_fpd_moments: sets must be at least 1, got " + std::to_string(sets));
    int max_count = 0;
    for (int s = 0; s < sets; ++s) {
      CD_REQUIRE(counts[s] >= 2, "cd_fpd_moments: counts[" + std::to_string(s) + "] = " + std::to_string(counts[s]) +
                                     ", a covariance needs at least 2 rows");
      if (counts[s] > max_count) max_count = counts[s];
    }
    CD_REQUIRE(idx_stride >= max_count, "cd_fpd_moments: idx_stride " + std::to_string(idx_stride) + " is less than the largest count " +
                                            std::to_string(max_count));
    CD_REQUIRE((int64_t)sets * idx_stride < INT32_MAX, "cd_fpd_moments: sets * idx_stride must be below 2^31 - 1 (the status word is int32)");
    CD_REQUIRE(((uintptr_t)workspace & 7) == 0, "cd_fpd_moments: workspace must be 8-byte aligned");
    const size_t need = fpd_bytes(d, sets, max_count);
    CD_REQUIRE(workspace_bytes >= need, "cd_fpd_moments: workspace of " + std::to_string(workspace_bytes) + " bytes, needs " +
                                            std::to_string(need) + " (cd_fpd_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    FpdArgs a;
    a.x = x; a.rows = rows; a.d = d; a.T = fpd_tiles(d); a.centre = centre; a.idx = idx; a.idx_stride = idx_stride;
    a.slices = (max_count + CD_FPD_SLICE_ROWS - 1) / CD_FPD_SLICE_ROWS;
    const int pairs = a.T * (a.T + 1) / 2;
    a.part = static_cast<double*>(workspace);
    a.flags = reinterpret_cast<int32_t*>(a.part + (size_t)sets * a.slices * pairs * 256);
    a.status = status;
    CD_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    for (int set0 = 0; set0 < sets; set0 += kFpdGroup) {  // the counts travel as kernel arguments, kFpdGroup sets a launch
      const int ns = sets - set0 < kFpdGroup ? sets - set0 : kFpdGroup;
      FpdCounts c{};
      int most = 0;
      for (int k = 0; k < ns; ++k) {
        c.n[k] = counts[set0 + k];
        if (c.n[k] > most) most = c.n[k];
      }
      a.set0 = set0;
      const int slices = (most + CD_FPD_SLICE_ROWS - 1) / CD_FPD_SLICE_ROWS;
      const dim3 grid((unsigned)slices, (unsigned)ns), block(kFpdThreads);
      switch (fpd_class(a.T)) {
        case 1: hipLaunchKernelGGL(fpd_gram_kernel<1>, grid, block, 0, s, a, c); break;
        case 3: hipLaunchKernelGGL(fpd_gram_kernel<3>, grid, block, 0, s, a, c); break;
        case 6: hipLaunchKernelGGL(fpd_gram_kernel<6>, grid, block, 0, s, a, c); break;
        case 10: hipLaunchKernelGGL(fpd_gram_kernel<10>, grid, block, 0, s, a, c); break;
        case 15: hipLaunchKernelGGL(fpd_gram_kernel<15>, grid, block, 0, s, a, c); break;
        default: hipLaunchKernelGGL(fpd_gram_kernel<kFpdAcc>, grid, block, 0, s, a, c); break;
      }
      CD_HIP(hipGetLastError());
      hipLaunchKernelGGL(fpd_moments_kernel, dim3((unsigned)pairs, (unsigned)ns), dim3(256), 0, s, a, c, mean, cov);
      CD_HIP(hipGetLastError());
    }
  });
}

}  // extern "C"
