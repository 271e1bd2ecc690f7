// Kernel physics distance and separation powers (include/calodiff.h, "Kernel physics distance and separation powers"): what the
// reference's metrics program computes beside the Frechet distance over the same feature matrix (calodiffusion/tests/hgcal_metrics.py:
// 401-432) -- jetnet.evaluation.kpd and a histogram per feature column for utils._separation_power (utils/utils.py:167-175).
//
// cd_kpd_sums.  A batch of the distance is an MMD estimate with the kernel k(a, b) = (gamma a.b + 1)^degree over m real and n
// generated rows drawn with replacement: the sums of three m x m, n x n and m x n kernel matrices.  The matrices are never formed.
// With W = [X; Y] the N = m + n gathered rows of the batch, all three are regions of the symmetric Gram matrix W W^T:
//
// gram kernel: a workgroup of four waves owns one block of CD_KPD_BLOCK = 64 x 64 list POSITIONS (bi, bj), bi <= bj, of one batch.
// The 64 + 64 rows come through LDS 32 feature columns at a time (32 lanes read 256 consecutive bytes of a gathered row; the next
// 32 columns are on their way in registers while the MFMAs of these run; d is padded with zeros to a multiple of 4 and the last
// chunk runs only the steps it has).  Wave w owns rows 16 w ... 16 w + 15 of the block and all four 16-column tiles: per four
// columns one A operand and four B operands, five 8-byte LDS reads for four v_mfma_f64_16x16x4_f64.  The A and the B operand of
// that instruction have the same lane map here (lane l: row l & 15 of the tile, column l >> 4 of the four), and the LDS row
// stride of 34 doubles puts the 32 lanes of one read cycle on 32 different bank pairs.  The C/D map is col = l & 15,
// row = (l >> 4) + 4 r (NOT the f32 one).
// An index is compared with [0, rows) before the row's address is formed; a bad one loads nothing, raises the block's flag and
// reports its position.  Entries beyond a list's count are never read.
// Epilogue: v = (gamma g + 1)^degree by repeated multiplication, weighed by the region of its two POSITIONS p <= q:
//   an off-diagonal block (bi < bj) holds each unordered pair once: XX and YY elements count twice (both orders), XY once;
//   a diagonal block holds both orders: p == q is dropped (equal positions, whatever rows they drew), XX and YY count once,
//   XY once where p < m <= q, and its mirror q < m <= p not at all.
// Each lane adds its 16 elements in a fixed order, the lanes combine by a fixed butterfly, the waves in ascending order: one
// partial {XX, YY, XY, flag} per workgroup.
// sums kernel: one workgroup per batch; thread t adds the partials t, t + 256, ... in ascending block order and the 256 threads
// combine by a fixed tree.  The split depends on (m, n) alone and nothing is accumulated with atomics, so a batch has the same
// bits wherever it sits in a call.  (One thread adding 12 403 partials in turn would spend the launch waiting on its own loads.)
//
// cd_column_histograms.  One pass over a row range of the matrix: a workgroup takes CD_HIST_CHUNK_ROWS rows of 64 columns, whose
// edges it keeps in LDS; wave w takes rows w, w + 4, ... and lane j column j, each thread counting into a table row of its own
// (no atomics: nobody else writes there; 16-bit counts, a thread sees 64 values).  The bin of a value is found arithmetically
// and corrected against the edges it was given, so the counts are those of np.histogram's searchsorted whatever rounding
// np.linspace put into the edges.  The four waves' tables are added on the way out, and a second launch adds the workgroups'
// tables in ascending order.
#include "guarded.h"

namespace cd {
namespace {

constexpr int kKpdThreads = 256, kKpdWaves = 4;
constexpr int kKpdChunk = 32;                 // feature columns in LDS at a time
constexpr int kKpdStride = kKpdChunk + 2;     // doubles between LDS rows: lane (i, g) of a read at bank pair (2 i + g) mod 32
constexpr int kKpdRows = 2 * CD_KPD_BLOCK;    // the block's rows, then its columns
constexpr int kKpdPerThread = kKpdRows * kKpdChunk / kKpdThreads;  // 16 staged values a thread and chunk
constexpr int kKpdGroup = 32;                 // batches a launch takes its counts for, as kernel arguments
static_assert(CD_KPD_BLOCK == 16 * kKpdWaves, "a 16-row tile per wave");
static_assert(kKpdThreads == 8 * kKpdChunk, "a staging thread per column of 8 rows");

struct KpdCounts {
  int m[kKpdGroup], n[kKpdGroup];
};

struct KpdArgs {
  const double* x;
  int64_t rows;
  int d;
  const int32_t* idx;
  int64_t idx_stride;
  int pair0;           // first batch of this launch
  int64_t blocks;      // partials of workspace per batch
  double gamma;
  int degree;
  double* part;        // [batch][block][4] = {XX, YY, XY, flag}
  int32_t* status;
};

typedef double kpd_acc __attribute__((ext_vector_type(4)));

__host__ __device__ __forceinline__ int64_t kpd_blocks(int64_t rows) {
  const int64_t nb = (rows + CD_KPD_BLOCK - 1) / CD_KPD_BLOCK;
  return nb * (nb + 1) / 2;
}

// first block of block row bi among the nb (nb + 1) / 2 blocks bi <= bj, row-major
__device__ __forceinline__ int64_t kpd_row_start(int64_t bi, int64_t nb) { return bi * nb - bi * (bi - 1) / 2; }

__global__ __launch_bounds__(kKpdThreads) void kpd_gram_kernel(KpdArgs a, KpdCounts counts) {
  __shared__ double image[kKpdRows * kKpdStride];
  __shared__ int64_t row_at[kKpdRows];  // first element of the row in x; -1: no row (beyond the lists, or a bad index)
  __shared__ double red[kKpdWaves][3];
  const int m = counts.m[blockIdx.y], n = counts.n[blockIdx.y], N = m + n, d = a.d;
  const int64_t nb = (N + CD_KPD_BLOCK - 1) / CD_KPD_BLOCK;
  const int64_t p = blockIdx.x;
  if (p >= nb * (nb + 1) / 2) return;
  const int pair = a.pair0 + blockIdx.y;
  // block p -> (bi, bj): the root of bi (2 nb + 1 - bi) / 2 = p, then set right by whole steps
  int64_t bi = (int64_t)(((double)(2 * nb + 1) - sqrt((double)(2 * nb + 1) * (double)(2 * nb + 1) - 8.0 * (double)p)) * 0.5);
  bi = bi < 0 ? 0 : bi > nb - 1 ? nb - 1 : bi;
  while (bi > 0 && kpd_row_start(bi, nb) > p) --bi;
  while (bi + 1 < nb && kpd_row_start(bi + 1, nb) <= p) ++bi;
  const int64_t bj = bi + (p - kpd_row_start(bi, nb));
  const int t = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;

  int bad = 0;
  if (t < kKpdRows) {
    const int64_t pos = (t < CD_KPD_BLOCK ? bi : bj) * CD_KPD_BLOCK + (t & (CD_KPD_BLOCK - 1));
    int64_t at = -1;
    if (pos < N) {  // entries beyond a list's count are never read
      const int64_t set = 2 * (int64_t)pair + (pos >= m), k = pos < m ? pos : pos - m;
      const int64_t ix = a.idx[set * a.idx_stride + k];
      if (ix >= 0 && ix < a.rows) {
        at = ix * d;  // formed from a checked index only
      } else {
        bad = 1;
        atomicMax(a.status, (int32_t)(1 + set * a.idx_stride + k));
      }
    }
    row_at[t] = at;
  }
  __syncthreads();

  // staging: column c of the chunk, rows r0, r0 + 8, ...
  const int c = t & (kKpdChunk - 1), r0 = t >> 5;
  const int dpad = (d + 3) & ~3;
  double v[kKpdPerThread];
  auto fetch = [&](int c0) {
    const int col = c0 + c;
#pragma unroll
    for (int j = 0; j < kKpdPerThread; ++j) {
      const int64_t at = row_at[r0 + 8 * j];
      v[j] = 0.0;
      if (at >= 0 && col < d) v[j] = a.x[at + col];
    }
  };
  kpd_acc acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = kpd_acc{0.0, 0.0, 0.0, 0.0};
  const int li = lane & 15, lg = lane >> 4;
  fetch(0);
  for (int c0 = 0; c0 < dpad; c0 += kKpdChunk) {
#pragma unroll
    for (int j = 0; j < kKpdPerThread; ++j) image[(r0 + 8 * j) * kKpdStride + c] = v[j];
    __syncthreads();
    if (c0 + kKpdChunk < dpad) fetch(c0 + kKpdChunk);
    const int steps = dpad - c0 < kKpdChunk ? (dpad - c0) >> 2 : kKpdChunk >> 2;
    for (int ks = 0; ks < steps; ++ks) {
      const double* four = image + ks * 4 + lg;
      const double fa = four[(wave * 16 + li) * kKpdStride];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double fb = four[(CD_KPD_BLOCK + q * 16 + li) * kKpdStride];
        acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa, fb, acc[q], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  const bool diagonal = bi == bj;
  double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t pi = bi * CD_KPD_BLOCK + wave * 16 + lg + 4 * r, pj = bj * CD_KPD_BLOCK + q * 16 + li;  // the f64 C/D map
      if (pi < N && pj < N) {
        const double base = fma(acc[q][r], a.gamma, 1.0);
        double k = base;
        for (int e = 1; e < a.degree; ++e) k *= base;
        const bool ix = pi < m, jx = pj < m;
        const double same = diagonal ? (pi != pj ? k : 0.0) : 2.0 * k;  // what the element adds to XX or YY, were it one of theirs
        s[0] += ix && jx ? same : 0.0;
        s[1] += !ix && !jx ? same : 0.0;
        s[2] += ix && !jx ? k : 0.0;  // !ix && jx: in a diagonal block the mirror of a counted element; elsewhere pi < pj rules it out
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s[e] += __shfl_xor(s[e], off, 64);
    if (lane == 0) red[wave][e] = s[e];
  }
  const int any = __syncthreads_or(bad);
  if (t < 4) {
    double o = any ? 1.0 : 0.0;
    if (t < 3) o = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    a.part[((int64_t)pair * a.blocks + p) * 4 + t] = o;
  }
}

// grid (batches of the launch), 256 threads
__global__ __launch_bounds__(256) void kpd_sums_kernel(KpdArgs a, KpdCounts counts, double* __restrict__ sums) {
  __shared__ double tree[4][256];
  const int pair = a.pair0 + blockIdx.x, t = threadIdx.x;
  const int64_t blocks = kpd_blocks((int64_t)counts.m[blockIdx.x] + counts.n[blockIdx.x]);
  const double* part = a.part + (int64_t)pair * a.blocks * 4;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t b = t; b < blocks; b += 256) {
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] += part[b * 4 + e];
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) tree[e][t] = s[e];
  __syncthreads();
  for (int half = 128; half >= 1; half >>= 1) {
    if (t < half) {
#pragma unroll
      for (int e = 0; e < 4; ++e) tree[e][t] += tree[e][t + half];
    }
    __syncthreads();
  }
  if (t < 3) sums[(int64_t)pair * 3 + t] = tree[3][0] != 0.0 ? __longlong_as_double(0x7ff8000000000000LL) : tree[t][0];
}

size_t kpd_bytes(int sets, int max_count) { return (size_t)(sets / 2) * (size_t)kpd_blocks(2 * (int64_t)max_count) * 4 * sizeof(double); }

// ---- column histograms ------------------------------------------------------------------------------------------------------

constexpr int kHistThreads = 256, kHistCols = 64, kHistLanes = kHistThreads / kHistCols;  // 64 columns a workgroup, a row lane per wave
constexpr int kHistAhead = 16;                                                               // values of a column in flight per thread
constexpr int kHistRowsPerLane = CD_HIST_CHUNK_ROWS / kHistLanes;
static_assert(kHistRowsPerLane % kHistAhead == 0 && kHistRowsPerLane < 65536, "whole groups of loads; a count fits 16 bits");

__host__ __device__ __forceinline__ int hist_edge_stride(int nedges) { return nedges | 1; }  // doubles between two columns' edges in LDS
// the columns' edges, then a count table [lane][column][bin] of 16-bit counts (a thread counts at most kHistRowsPerLane values)
size_t hist_lds_bytes(int nedges) {
  return (size_t)kHistCols * ((size_t)hist_edge_stride(nedges) * sizeof(double) + (size_t)kHistLanes * (nedges - 1) * sizeof(uint16_t));
}

// grid (row chunks, groups of 64 columns)
__global__ __launch_bounds__(kHistThreads) void hist_count_kernel(const double* __restrict__ x, int64_t row_begin, int64_t row_count, int d,
                                                                  const double* __restrict__ edges, int nedges, uint32_t* __restrict__ part) {
  extern __shared__ double hist_lds[];
  const int nb = nedges - 1, se = hist_edge_stride(nedges), t = threadIdx.x, lane = t & (kHistCols - 1), w = t >> 6;
  double* es = hist_lds;                                                   // [64][se]
  uint16_t* table = reinterpret_cast<uint16_t*>(hist_lds + kHistCols * se);  // [4][64][nb]
  const int c0 = blockIdx.y * kHistCols, j = c0 + lane;
  for (int i = t; i < kHistCols * nedges; i += kHistThreads) {
    const int cl = i / nedges, k = i - cl * nedges;
    es[cl * se + k] = c0 + cl < d ? edges[(int64_t)(c0 + cl) * nedges + k] : 0.0;
  }
  for (int i = t; i < kHistLanes * kHistCols * nb; i += kHistThreads) table[i] = 0;
  __syncthreads();
  if (j < d) {
    const double* e = es + lane * se;
    const double lo = e[0], hi = e[nb];
    const double scale = hi > lo ? (double)nb / (hi - lo) : 0.0;
    uint16_t* mine = table + (w * kHistCols + lane) * nb;  // this thread's alone: no atomics
    const int64_t r_lo = (int64_t)blockIdx.x * CD_HIST_CHUNK_ROWS + w;  // rows r_lo, r_lo + 4, ...: a wave reads 512 consecutive bytes of a row
    const double* col = x + row_begin * d + j;
    for (int i0 = 0; i0 < kHistRowsPerLane; i0 += kHistAhead) {
      double v[kHistAhead];
#pragma unroll
      for (int u = 0; u < kHistAhead; ++u) {
        const int64_t r = r_lo + (int64_t)kHistLanes * (i0 + u);
        v[u] = r < row_count ? col[r * d] : __longlong_as_double(0x7ff8000000000000LL);
      }
#pragma unroll
      for (int u = 0; u < kHistAhead; ++u) {
        if (v[u] >= lo && v[u] <= hi) {  // NaN fails both
          int k = (int)((v[u] - lo) * scale);
          k = k < 0 ? 0 : k > nb - 1 ? nb - 1 : k;
          while (k > 0 && v[u] < e[k]) --k;               // bin k is [e[k], e[k + 1]), the last one closed on the right
          while (k < nb - 1 && v[u] >= e[k + 1]) ++k;
          mine[k] = (uint16_t)(mine[k] + 1);
        }
      }
    }
  }
  __syncthreads();
  uint32_t* out = part + (int64_t)blockIdx.x * d * nb;
  for (int i = t; i < kHistCols * nb; i += kHistThreads) {
    const int cl = i / nb, k = i - cl * nb;
    if (c0 + cl < d) {
      uint32_t s = 0u;
#pragma unroll
      for (int l = 0; l < kHistLanes; ++l) s += table[(l * kHistCols + cl) * nb + k];
      out[(c0 + cl) * nb + k] = s;
    }
  }
}

__global__ __launch_bounds__(256) void hist_sum_kernel(const uint32_t* __restrict__ part, int64_t groups, int cells, uint32_t* __restrict__ counts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cells) return;
  uint32_t s = 0u;
#pragma unroll 8
  for (int64_t g = 0; g < groups; ++g) s += part[g * cells + i];
  counts[i] = s;
}

int64_t hist_groups(int64_t row_count) { return (row_count + CD_HIST_CHUNK_ROWS - 1) / CD_HIST_CHUNK_ROWS; }

std::string hist_limits(const char* who) {
  return std::string(who) + ": needs 1 <= d <= " + std::to_string(CD_FPD_MAX_D) + ", 2 <= nedges <= " + std::to_string(CD_HIST_MAX_EDGES) +
         " (edges and count tables of 64 columns in LDS) and 1 <= row_count < 2^32";
}

bool hist_ok(int64_t row_count, int d, int nedges) {
  return d >= 1 && d <= CD_FPD_MAX_D && nedges >= 2 && nedges <= CD_HIST_MAX_EDGES && row_count >= 1 && row_count < ((int64_t)1 << 32);
}

}  // namespace
}  // namespace cd

extern "C" {

size_t cd_kpd_workspace_bytes(int sets, int max_count) {
  if (sets < 2 || sets % 2 != 0 || max_count < 2 || max_count > CD_KPD_MAX_COUNT) {
    set_error("cd_kpd_workspace_bytes: needs an even sets >= 2 and 2 <= max_count <= " + std::to_string(CD_KPD_MAX_COUNT) + ", got sets = " +
              std::to_string(sets) + ", max_count = " + std::to_string(max_count));
    return 0;
  }
  return kpd_bytes(sets, max_count);
}

int cd_kpd_sums(const double* x, int64_t rows, int d, const int32_t* idx, int64_t idx_stride, const int32_t* counts, int sets, double gamma,
                int degree, double* sums, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  return guarded([&] {
    CD_REQUIRE(x && idx && counts && sums && status && workspace, "cd_kpd_sums: x, idx, counts, sums, status and workspace must not be null");
    CD_REQUIRE(d >= 1 && d <= CD_FPD_MAX_D, "cd_kpd_sums: d must be in [1, " + std::to_string(CD_FPD_MAX_D) + "], got " + std::to_string(d));
    CD_REQUIRE(rows > 0 && rows <= INT64_MAX / CD_FPD_MAX_D, "cd_kpd_sums: rows must be positive, got " + std::to_string(rows));
    CD_REQUIRE(sets >= 2 && sets % 2 == 0, "cd_kpd_sums: sets must be even and at least 2 (real and generated lists in turn), got " +
                                               std::to_string(sets));
    CD_REQUIRE(degree >= 1 && degree <= 8, "cd_kpd_sums: degree must be in [1, 8], got " + std::to_string(degree));
    int max_count = 0;
    for (int s = 0; s < sets; ++s) {
      CD_REQUIRE(counts[s] >= 2 && counts[s] <= CD_KPD_MAX_COUNT, "cd_kpd_sums: counts[" + std::to_string(s) + "] = " + std::to_string(counts[s]) +
                                                                      ", a list holds 2 to " + std::to_string(CD_KPD_MAX_COUNT) + " rows");
      if (counts[s] > max_count) max_count = counts[s];
    }
    CD_REQUIRE(idx_stride >= max_count, "cd_kpd_sums: idx_stride " + std::to_string(idx_stride) + " is less than the largest count " +
                                            std::to_string(max_count));
    CD_REQUIRE((int64_t)sets * idx_stride < INT32_MAX, "cd_kpd_sums: sets * idx_stride must be below 2^31 - 1 (the status word is int32)");
    CD_REQUIRE(((uintptr_t)workspace & 7) == 0, "cd_kpd_sums: workspace must be 8-byte aligned");
    const size_t need = kpd_bytes(sets, max_count);
    CD_REQUIRE(workspace_bytes >= need, "cd_kpd_sums: workspace of " + std::to_string(workspace_bytes) + " bytes, needs " + std::to_string(need) +
                                            " (cd_kpd_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    KpdArgs a;
    a.x = x; a.rows = rows; a.d = d; a.idx = idx; a.idx_stride = idx_stride; a.gamma = gamma; a.degree = degree;
    a.blocks = kpd_blocks(2 * (int64_t)max_count);
    a.part = static_cast<double*>(workspace);
    a.status = status;
    CD_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    const int pairs = sets / 2;
    for (int pair0 = 0; pair0 < pairs; pair0 += kKpdGroup) {  // the counts travel as kernel arguments, kKpdGroup batches a launch
      const int np = pairs - pair0 < kKpdGroup ? pairs - pair0 : kKpdGroup;
      KpdCounts c{};
      int64_t most = 0;
      for (int k = 0; k < np; ++k) {
        c.m[k] = counts[2 * (pair0 + k)];
        c.n[k] = counts[2 * (pair0 + k) + 1];
        const int64_t b = kpd_blocks((int64_t)c.m[k] + c.n[k]);
        if (b > most) most = b;
      }
      a.pair0 = pair0;
      hipLaunchKernelGGL(kpd_gram_kernel, dim3((unsigned)most, (unsigned)np), dim3(kKpdThreads), 0, s, a, c);
      CD_HIP(hipGetLastError());
      hipLaunchKernelGGL(kpd_sums_kernel, dim3((unsigned)np), dim3(256), 0, s, a, c, sums);
      CD_HIP(hipGetLastError());
    }
  });
}

size_t cd_column_histograms_workspace_bytes(int64_t row_count, int d, int nedges) {
  if (!hist_ok(row_count, d, nedges)) {
    set_error(hist_limits("cd_column_histograms_workspace_bytes") + ", got row_count = " + std::to_string(row_count) + ", d = " + std::to_string(d) +
              ", nedges = " + std::to_string(nedges));
    return 0;
  }
  return (size_t)hist_groups(row_count) * (size_t)d * (size_t)(nedges - 1) * sizeof(uint32_t);
}

int cd_column_histograms(const double* x, int64_t row_begin, int64_t row_count, int d, const double* edges, int nedges, uint32_t* counts,
                         void* workspace, size_t workspace_bytes, void* stream) {
  return guarded([&] {
    CD_REQUIRE(x && edges && counts && workspace, "cd_column_histograms: x, edges, counts and workspace must not be null");
    CD_REQUIRE(row_begin >= 0, "cd_column_histograms: row_begin must not be negative, got " + std::to_string(row_begin));
    CD_REQUIRE(hist_ok(row_count, d, nedges), hist_limits("cd_column_histograms") + ", got row_count = " + std::to_string(row_count) + ", d = " +
                                                  std::to_string(d) + ", nedges = " + std::to_string(nedges));
    CD_REQUIRE(((uintptr_t)workspace & 3) == 0, "cd_column_histograms: workspace must be 4-byte aligned");
    const int64_t groups = hist_groups(row_count);
    const int cells = d * (nedges - 1);
    const size_t need = (size_t)groups * (size_t)cells * sizeof(uint32_t);
    CD_REQUIRE(workspace_bytes >= need, "cd_column_histograms: workspace of " + std::to_string(workspace_bytes) + " bytes, needs " +
                                            std::to_string(need) + " (cd_column_histograms_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    uint32_t* part = static_cast<uint32_t*>(workspace);
    hipLaunchKernelGGL(hist_count_kernel, dim3((unsigned)groups, (unsigned)((d + kHistCols - 1) / kHistCols)), dim3(kHistThreads),
                       hist_lds_bytes(nedges), s, x, row_begin, row_count, d, edges, nedges, part);
    CD_HIP(hipGetLastError());
    hipLaunchKernelGGL(hist_sum_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, part, groups, cells, counts);
    CD_HIP(hipGetLastError());
  });
}

}  // extern "C"
