// Shower statistics (include/calodiff.h, "shower statistics"): the sums behind the reference's plot classes
// (calodiffusion/utils/plots.py) in one pass over the showers, and the energy-conserving cell threshold
// (utils.apply_mask_conserveE, utils/utils.py:1021-1032).
//
// cd_shower_stats_compute.  A shower is (L, n): L layers of n cells.  A wave owns U showers (U = 4, 2 or 1, the most whose
// staging fits kStatsLdsBudget) and walks their layers in order; a workgroup is four such waves and takes the next 4 U showers
// of the batch per trip.  Per layer:
//   1. lane j loads the cells j, j + 64, ... of each of its U showers (coalesced dwords: a layer starts at any element), stores
//      them to the wave's LDS rows and adds them to the layer's moment sums beside the r / cos / sin tables, which are read once
//      for the U showers (24 bytes a cell against the showers' 4: from cache, and the reason U is not 1 where LDS allows more);
//   2. a fixed tree combines the 64 lanes: the two quad steps hand each lane one of the U showers (as kernels_hlf.hip), two row
//      rotations finish the 16-lane rows with full-rate DPP moves and two cross-row exchanges finish the wave, so a sum moves
//      through the LDS crossbar twice and not six times; lanes 0 .. U - 1 store the records;
//   3. the lane that owns a bin (radial bins first, then angular: one list) walks the bin's cells of this layer -- a CSR list
//      built at create time, ascending, whose part for this layer the workgroup has copied to LDS beside the cells -- and adds
//      them from LDS to the bin's running sum, which lives in LDS between layers and is touched by its owner alone.
// Every sum is fp64 and its order is a function of the geometry alone: no atomics, no workspace, the same bits for a shower
// wherever it stands.  A shower beyond the batch reads the last one's rows and stores nothing, so the barriers of a trip are
// uniform.
//
// cd_threshold_conserve.  A row is short (9 or 18 cells on the grids, the cells of a layer for HGCal): 16 lanes (a DPP row) take
// a row, lane j the cells j, j + 16, ..., sum the clamped row and its kept cells in fp64, combine by the row tree, and write the
// row back scaled on a second walk (the row is in cache).
#include "guarded.h"

#include <cmath>
#include <vector>

// One geometry on the device (cd_shower_stats_create)
struct CdShowerStats {
  int L = 0, n = 0, n_r = 0, n_a = 0;
  double* r = nullptr;         // L n
  double* cs = nullptr;        // L n cosines
  double* sn = nullptr;        // L n sines
  int32_t* start = nullptr;    // L (n_r + n_a) + 1 offsets into cells: the cells of (layer, bin), bins = radial then angular
  uint16_t* cells = nullptr;   // cell index inside the layer, ascending inside a list
  ~CdShowerStats() {
    if (r) (void)hipFree(r);
    if (cs) (void)hipFree(cs);
    if (sn) (void)hipFree(sn);
    if (start) (void)hipFree(start);
    if (cells) (void)hipFree(cells);
  }
};

namespace cd {
namespace {

constexpr int kStatsWaves = 4, kStatsThreads = 64 * kStatsWaves;
constexpr int kStatsMaxBlocks = 2048;          // eight workgroups on each of 256 CUs
constexpr size_t kStatsLdsBudget = 40 * 1024;  // per workgroup, where more than one shower a wave is a choice
constexpr int kStatsMaxCells = 4096, kStatsMaxLayers = 512, kStatsMaxBins = 256;

// LDS of a workgroup with U showers a wave: the bins' running sums (fp64) and the staged layer (fp32) of its 4 U showers, then
// the layer's part of the CSR list, shared by the waves: bins + 1 offsets and at most 2 n cell indices (a cell is in at most one
// radial and one angular bin)
inline size_t stats_lds_bytes(int U, int n, int bins) {
  return (size_t)kStatsWaves * U * ((size_t)bins * 8 + (size_t)n * 4) + ((size_t)bins + 1) * 4 + (size_t)n * 4;
}

template <int CTRL>
struct Dpp {
  __device__ __forceinline__ int operator()(int x) const { return __builtin_amdgcn_update_dpp(x, x, CTRL, 0xF, 0xF, true); }
};
using QuadXor1 = Dpp<0xB1>;  // quad_perm [1, 0, 3, 2]
using QuadXor2 = Dpp<0x4E>;  // quad_perm [2, 3, 0, 1]
using RowRor4 = Dpp<0x124>;
using RowRor8 = Dpp<0x128>;
template <int MASK>
struct LaneXor {  // across the 16-lane rows: through the LDS crossbar
  __device__ __forceinline__ int operator()(int x) const { return __shfl_xor(x, MASK, 64); }
};

template <typename P>
__device__ __forceinline__ double moved(double x, P p) {
  const long long b = __double_as_longlong(x);
  const unsigned lo = (unsigned)p((int)(unsigned)b), hi = (unsigned)p((int)(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

struct StatsAcc {
  double e = 0.0, er = 0.0, err = 0.0, ec = 0.0, es = 0.0;
  float mx = -INFINITY;
  int hits = 0, occ = 0;
};

// a += the partner's s
template <typename P>
__device__ __forceinline__ void take(StatsAcc& a, const StatsAcc& s, P p) {
  a.e += moved(s.e, p);
  a.er += moved(s.er, p);
  a.err += moved(s.err, p);
  a.ec += moved(s.ec, p);
  a.es += moved(s.es, p);
  a.mx = fmaxf(a.mx, __int_as_float(p(__float_as_int(s.mx))));
  a.hits += p(s.hits);
  a.occ += p(s.occ);
}

__device__ __forceinline__ StatsAcc pick(bool first, const StatsAcc& x, const StatsAcc& y) {
  StatsAcc r;
  r.e = first ? x.e : y.e;
  r.er = first ? x.er : y.er;
  r.err = first ? x.err : y.err;
  r.ec = first ? x.ec : y.ec;
  r.es = first ? x.es : y.es;
  r.mx = first ? x.mx : y.mx;
  r.hits = first ? x.hits : y.hits;
  r.occ = first ? x.occ : y.occ;
  return r;
}

// a lane keeps x or y (sel: y) and adds the partner's copy of the one it keeps
template <typename P>
__device__ __forceinline__ StatsAcc fold(const StatsAcc& x, const StatsAcc& y, bool sel, P p) {
  StatsAcc keep = pick(sel, y, x);
  take(keep, pick(sel, x, y), p);
  return keep;
}

// The tree over the wave's 64 lanes for the U showers each lane holds sums of.  Returns the sums of shower `mine` (set here:
// lane 0 .. U - 1 hold the showers of the wave between them), over all lanes.
template <int U>
__device__ __forceinline__ StatsAcc stats_tree(const StatsAcc (&a)[U], int lane, int& mine) {
  const bool odd = lane & 1, upper = lane & 2;
  StatsAcc t;
  if constexpr (U == 4) {
    const StatsAcc k0 = fold(a[0], a[2], odd, QuadXor1{}), k1 = fold(a[1], a[3], odd, QuadXor1{});
    t = fold(k0, k1, upper, QuadXor2{});
    mine = (odd ? 2 : 0) + (upper ? 1 : 0);
  } else if constexpr (U == 2) {
    t = fold(a[0], a[1], odd, QuadXor1{});
    take(t, t, QuadXor2{});
    mine = odd ? 1 : 0;
  } else {
    t = a[0];
    take(t, t, QuadXor1{});
    take(t, t, QuadXor2{});
    mine = 0;
  }
  take(t, t, RowRor4{});
  take(t, t, RowRor8{});
  take(t, t, LaneXor<16>{});
  take(t, t, LaneXor<32>{});
  return t;
}

template <int U>
__global__ __launch_bounds__(kStatsThreads) void shower_stats_kernel(
    const double* __restrict__ tab_r, const double* __restrict__ tab_c, const double* __restrict__ tab_s,
    const int32_t* __restrict__ start, const uint16_t* __restrict__ cells, const float* __restrict__ showers, int L, int n, int n_r,
    int n_a, int batch, float hit_thr, float occ_thr, double* __restrict__ records, int32_t* __restrict__ counts,
    double* __restrict__ r_profile, double* __restrict__ a_profile) {
  extern __shared__ double stats_lds[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int bins = n_r + n_a;
  const bool profiles = r_profile || a_profile;
  // the wave's part of the workgroup's LDS: U x bins running sums, then (after every wave's sums) U x n staged cells
  double* prof = stats_lds + (size_t)wave * U * bins;
  float* stage0 = reinterpret_cast<float*>(stats_lds + (size_t)kStatsWaves * U * bins);
  float* stage = stage0 + (size_t)wave * U * n;
  int32_t* lstart = reinterpret_cast<int32_t*>(stage0 + (size_t)kStatsWaves * U * n);  // bins + 1, relative to the layer's first entry
  uint16_t* lcells = reinterpret_cast<uint16_t*>(lstart + bins + 1);
  const int64_t V = (int64_t)L * n;
  constexpr int kTrip = kStatsWaves * U;
  for (int64_t b0 = (int64_t)blockIdx.x * kTrip; b0 < batch; b0 += (int64_t)gridDim.x * kTrip) {
    const int64_t first = b0 + wave * U;
    const float* row[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {  // a shower beyond the batch reads the last one's rows and stores nothing
      const int64_t b = first + u < batch ? first + u : batch - 1;
      row[u] = showers + b * V;
    }
    if (profiles)
      for (int k = lane; k < U * bins; k += 64) prof[k] = 0.0;
    for (int l = 0; l < L; ++l) {
      const int64_t at = (int64_t)l * n;
      StatsAcc a[U];
#pragma unroll 2
      for (int i = lane; i < n; i += 64) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = row[u][at + i];
        const double r = tab_r[at + i], c = tab_c[at + i], s = tab_s[at + i];
        const double r2 = r * r;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          stage[u * n + i] = v[u];
          const double e = (double)v[u];
          a[u].e += e;
          a[u].er = fma(r, e, a[u].er);
          a[u].err = fma(r2, e, a[u].err);
          a[u].ec = fma(c, e, a[u].ec);
          a[u].es = fma(s, e, a[u].es);
          a[u].mx = fmaxf(a[u].mx, v[u]);
          a[u].hits += v[u] > hit_thr ? 1 : 0;
          a[u].occ += v[u] > occ_thr ? 1 : 0;
        }
      }
      int mine;
      const StatsAcc t = stats_tree<U>(a, lane, mine);
      if (lane < U && first + mine < batch) {
        const int64_t it = (first + mine) * L + l;
        double* o = records + it * 6;
        o[0] = t.e; o[1] = (double)t.mx; o[2] = t.er; o[3] = t.err; o[4] = t.ec; o[5] = t.es;
        counts[it * 2] = t.hits;
        counts[it * 2 + 1] = t.occ;
      }
      if (profiles) {
        // the layer's lists beside its cells: an index fetched from memory inside the walk would put a trip to the cache into
        // every step of a bin's chain of additions
        const int32_t* st = start + (int64_t)l * bins;
        const int32_t base = st[0], len = st[bins] - base;
        for (int k = threadIdx.x; k <= bins; k += kStatsThreads) lstart[k] = st[k] - base;
        for (int k = threadIdx.x; k < len; k += kStatsThreads) lcells[k] = cells[base + k];
        __syncthreads();  // the layer is staged
        for (int b = lane; b < bins; b += 64) {
          if (b < n_r ? !r_profile : !a_profile) continue;
          const int lo = lstart[b], hi = lstart[b + 1];
          if (lo == hi) continue;
          double s[U];
#pragma unroll
          for (int u = 0; u < U; ++u) s[u] = prof[u * bins + b];
          int k = lo;
          for (; k + 4 <= hi; k += 4) {  // four indices, then their cells, then the additions in the list's order
            int c[4];
            float v[4][U];
#pragma unroll
            for (int q = 0; q < 4; ++q) c[q] = lcells[k + q];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
              for (int u = 0; u < U; ++u) v[q][u] = stage[u * n + c[q]];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
              for (int u = 0; u < U; ++u) s[u] += (double)v[q][u];
          }
          for (; k < hi; ++k) {
            const int c = lcells[k];
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] += (double)stage[u * n + c];
          }
#pragma unroll
          for (int u = 0; u < U; ++u) prof[u * bins + b] = s[u];
        }
        __syncthreads();  // before the next layer overwrites the stage
      }
    }
    if (profiles) {
      for (int k = lane; k < U * bins; k += 64) {
        const int u = k / bins, b = k - u * bins;
        if (first + u >= batch) continue;
        if (b < n_r) {
          if (r_profile) r_profile[(first + u) * n_r + b] = prof[k];
        } else if (a_profile) {
          a_profile[(first + u) * n_a + (b - n_r)] = prof[k];
        }
      }
    }
  }
}

constexpr int kCutGroup = 16, kCutRowsPerBlock = kStatsThreads / kCutGroup;
constexpr int kCutMaxBlocks = 16384;

// the row tree: every lane of the 16 ends with the sum
__device__ __forceinline__ double row_sum(double x) {
  x += moved(x, QuadXor1{});
  x += moved(x, QuadXor2{});
  x += moved(x, RowRor4{});
  x += moved(x, RowRor8{});
  return x;
}

__global__ __launch_bounds__(kStatsThreads) void threshold_conserve_kernel(float* __restrict__ x, const uint8_t* __restrict__ mask,
                                                                           int64_t rows, int row_len, float emin) {
  const int j = threadIdx.x % kCutGroup, g = threadIdx.x / kCutGroup;
  // every group of a wave walks the same number of rows (the tree needs all 64 lanes); a row beyond the end is not touched
  for (int64_t r0 = (int64_t)blockIdx.x * kCutRowsPerBlock; r0 < rows; r0 += (int64_t)gridDim.x * kCutRowsPerBlock) {
    const int64_t r = r0 + g;
    const bool live = r < rows;
    float* xr = x + (live ? r : 0) * row_len;
    const uint8_t* mr = mask ? mask + (live ? r : 0) * row_len : nullptr;
    double T = 0.0, K = 0.0;
    for (int i = j; live && i < row_len; i += kCutGroup) {
      const float v = xr[i];
      const bool drop = mr ? mr[i] != 0 : v < emin;
      const double c = v < 0.0f ? 0.0 : (double)v;
      T += c;
      K += drop ? 0.0 : c;
    }
    T = row_sum(T);
    K = row_sum(K);
    const float scale = (float)((T + 1e-10) / (K + 1e-10));
    if (!live) continue;
    for (int i = j; i < row_len; i += kCutGroup) {
      const float v = xr[i];
      const bool drop = mr ? mr[i] != 0 : v < emin;
      xr[i] = drop ? 0.0f : (v < 0.0f ? 0.0f : v) * scale;
    }
  }
}

}  // namespace
}  // namespace cd

extern "C" {

int cd_shower_stats_create(const CdShowerStatsDesc* desc, CdShowerStats** out, void* stream) {
  return guarded([&] {
    const std::string who = "cd_shower_stats_create: ";
    CD_REQUIRE(desc && out, who + "desc and out must not be null");
    CD_REQUIRE(desc->struct_size == sizeof(CdShowerStatsDesc), who + "CdShowerStatsDesc.struct_size is " + std::to_string(desc->struct_size) +
                                                                   ", this library expects " + std::to_string(sizeof(CdShowerStatsDesc)));
    const int L = desc->n_layers, n = desc->n_cells, n_r = desc->n_rbins, n_a = desc->n_abins;
    CD_REQUIRE(L >= 1 && L <= kStatsMaxLayers, who + "n_layers must be in [1, " + std::to_string(kStatsMaxLayers) + "], got " + std::to_string(L));
    CD_REQUIRE(n >= 1 && n <= kStatsMaxCells, who + "n_cells must be in [1, " + std::to_string(kStatsMaxCells) + "], got " + std::to_string(n));
    CD_REQUIRE(n_r >= 1 && n_r <= kStatsMaxBins, who + "n_rbins must be in [1, " + std::to_string(kStatsMaxBins) + "], got " + std::to_string(n_r));
    CD_REQUIRE(n_a >= 0 && n_a <= kStatsMaxBins, who + "n_abins must be in [0, " + std::to_string(kStatsMaxBins) + "], got " + std::to_string(n_a));
    CD_REQUIRE(desc->r_bin, who + "the r_bin table is null");
    CD_REQUIRE(desc->r_coord, who + "the r_coord table is null");
    CD_REQUIRE(desc->angle, who + "the angle table is null");
    CD_REQUIRE((desc->a_bin != nullptr) == (n_a > 0), who + "an a_bin table goes with n_abins > 0 and a null one with n_abins == 0");
    const size_t V = (size_t)L * n;
    const int bins = n_r + n_a;
    std::vector<double> cs(V), sn(V);
    for (size_t i = 0; i < V; ++i) {
      CD_REQUIRE(desc->r_bin[i] >= -1 && desc->r_bin[i] < n_r, who + "r_bin[" + std::to_string(i) + "] = " + std::to_string(desc->r_bin[i]) +
                                                                    " is outside [-1, " + std::to_string(n_r) + ")");
      if (n_a)
        CD_REQUIRE(desc->a_bin[i] >= -1 && desc->a_bin[i] < n_a, who + "a_bin[" + std::to_string(i) + "] = " + std::to_string(desc->a_bin[i]) +
                                                                      " is outside [-1, " + std::to_string(n_a) + ")");
      CD_REQUIRE(std::isfinite(desc->r_coord[i]), who + "r_coord[" + std::to_string(i) + "] is not finite");
      CD_REQUIRE(std::isfinite(desc->angle[i]), who + "angle[" + std::to_string(i) + "] is not finite");
      cs[i] = std::cos(desc->angle[i]);
      sn[i] = std::sin(desc->angle[i]);
    }
    // the cells of every (layer, bin) in ascending cell order: count, prefix, fill
    std::vector<int32_t> start((size_t)L * bins + 1, 0);
    for (int l = 0; l < L; ++l)
      for (int i = 0; i < n; ++i) {
        const size_t at = (size_t)l * n + i;
        if (desc->r_bin[at] >= 0) ++start[(size_t)l * bins + desc->r_bin[at] + 1];
        if (n_a && desc->a_bin[at] >= 0) ++start[(size_t)l * bins + n_r + desc->a_bin[at] + 1];
      }
    for (size_t k = 1; k < start.size(); ++k) start[k] += start[k - 1];
    std::vector<uint16_t> cells((size_t)start.back() + 1);  // (+ 1: never an empty allocation)
    std::vector<int32_t> fill(start.begin(), start.end() - 1);
    for (int l = 0; l < L; ++l)
      for (int i = 0; i < n; ++i) {
        const size_t at = (size_t)l * n + i;
        if (desc->r_bin[at] >= 0) cells[fill[(size_t)l * bins + desc->r_bin[at]]++] = (uint16_t)i;
        if (n_a && desc->a_bin[at] >= 0) cells[fill[(size_t)l * bins + n_r + desc->a_bin[at]]++] = (uint16_t)i;
      }
    hipStream_t s = (hipStream_t)stream;
    struct Owner {
      CdShowerStats* m;
      ~Owner() { delete m; }
    } own{new CdShowerStats};
    CdShowerStats* m = own.m;
    m->L = L; m->n = n; m->n_r = n_r; m->n_a = n_a;
    CD_HIP(hipMalloc(&m->r, sizeof(double) * V));
    CD_HIP(hipMalloc(&m->cs, sizeof(double) * V));
    CD_HIP(hipMalloc(&m->sn, sizeof(double) * V));
    CD_HIP(hipMalloc(&m->start, sizeof(int32_t) * start.size()));
    CD_HIP(hipMalloc(&m->cells, sizeof(uint16_t) * cells.size()));
    CD_HIP(hipMemcpyAsync(m->r, desc->r_coord, sizeof(double) * V, hipMemcpyHostToDevice, s));
    CD_HIP(hipMemcpyAsync(m->cs, cs.data(), sizeof(double) * V, hipMemcpyHostToDevice, s));
    CD_HIP(hipMemcpyAsync(m->sn, sn.data(), sizeof(double) * V, hipMemcpyHostToDevice, s));
    CD_HIP(hipMemcpyAsync(m->start, start.data(), sizeof(int32_t) * start.size(), hipMemcpyHostToDevice, s));
    CD_HIP(hipMemcpyAsync(m->cells, cells.data(), sizeof(uint16_t) * cells.size(), hipMemcpyHostToDevice, s));
    CD_HIP(hipStreamSynchronize(s));  // the host arrays may go away after the call
    *out = m;
    own.m = nullptr;
  });
}

int cd_shower_stats_destroy(CdShowerStats* stats) {
  return guarded([&] { delete stats; });
}

int cd_shower_stats_compute(const CdShowerStats* stats, const float* showers, int batch, float hit_threshold, float sparsity_eps,
                            double* records, int32_t* counts, double* r_profile, double* a_profile, void* stream) {
  return guarded([&] {
    CD_REQUIRE(stats && showers && records && counts, "cd_shower_stats_compute: stats, showers, records and counts must not be null");
    CD_REQUIRE(batch > 0, "cd_shower_stats_compute: batch must be positive");
    CD_REQUIRE(!a_profile || stats->n_a > 0, "cd_shower_stats_compute: a_profile for a geometry without a_bin");
    const int bins = stats->n_r + stats->n_a;
    const int U = stats_lds_bytes(4, stats->n, bins) <= kStatsLdsBudget ? 4 : stats_lds_bytes(2, stats->n, bins) <= kStatsLdsBudget ? 2 : 1;
    const size_t lds = stats_lds_bytes(U, stats->n, bins);
    int64_t blocks = ((int64_t)batch + kStatsWaves * U - 1) / (kStatsWaves * U);
    if (blocks > kStatsMaxBlocks) blocks = kStatsMaxBlocks;
    auto launch = [&](auto kernel) {
      if (lds > 64 * 1024) CD_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kStatsThreads), lds, (hipStream_t)stream, stats->r, stats->cs, stats->sn,
                         stats->start, stats->cells, showers, stats->L, stats->n, stats->n_r, stats->n_a, batch, hit_threshold, sparsity_eps,
                         records, counts, r_profile, a_profile);
    };
    if (U == 4) launch(shower_stats_kernel<4>);
    else if (U == 2) launch(shower_stats_kernel<2>);
    else launch(shower_stats_kernel<1>);
    CD_HIP(hipGetLastError());
  });
}

int cd_threshold_conserve(float* x, const uint8_t* mask, int64_t rows, int row_len, float emin, void* stream) {
  return guarded([&] {
    CD_REQUIRE(x, "cd_threshold_conserve: x must not be null");
    CD_REQUIRE(rows >= 0, "cd_threshold_conserve: rows must not be negative");
    CD_REQUIRE(row_len >= 1 && row_len <= kStatsMaxCells, "cd_threshold_conserve: row_len must be in [1, " + std::to_string(kStatsMaxCells) +
                                                              "], got " + std::to_string(row_len));
    if (rows == 0) return;
    int64_t blocks = (rows + kCutRowsPerBlock - 1) / kCutRowsPerBlock;
    if (blocks > kCutMaxBlocks) blocks = kCutMaxBlocks;
    hipLaunchKernelGGL(threshold_conserve_kernel, dim3((unsigned)blocks), dim3(kStatsThreads), 0, (hipStream_t)stream, x, mask, rows,
                       row_len, emin);
    CD_HIP(hipGetLastError());
  });
}

}  // extern "C"
