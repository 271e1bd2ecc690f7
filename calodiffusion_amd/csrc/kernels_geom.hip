// HGCal geometry maps (include/calodiff.h, "HGCal geometry maps"): a dense (layers, rows, cols) map packed into per-layer CSR (and,
// for the sparse decode, the column-major view of its entries > 1e-6), the product with a batch of showers, and
// generate_sparse_mat's sampled decode in two gather passes, and the HGCal forward pre-processing, which applies the packed encoder
// inside its own launch (cd_preprocess_hgcal).  Kernels and their C ABI; nothing here touches a plan.
#include "energy_map.h"
#include "philox.h"
#include "guarded.h"
#include "kernels_geom.h"
#include "geom_csr_check.h"

#include <climits>
#include <type_traits>

namespace cd {

constexpr float SPARSE_EPS = 1e-6f;  // generate_sparse_mat's eps (HGCal_utils.py:371)

// ---- packing: count, exclusive scan, fill --------------------------------------------------------------------------
// One wave per row: 64 consecutive columns per step, the kept ones numbered by the ballot's prefix count, so a row's entries
// come out in ascending column order.  fill == false: the row's count goes to ptr[row]; true: ptr is the scanned array.
// `pat` decides which entries are kept (the dense map itself, or a trainable map's mask); ent_row (nullable): the row of every entry.
template <bool FILL>
__global__ void __launch_bounds__(256) geom_pack_rows_kernel(const float* __restrict__ dense, const float* __restrict__ pat,
                                                             int n_rows, int cols, int* ptr, int* __restrict__ col_idx,
                                                             float* __restrict__ val, int* __restrict__ ent_row) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_rows) return;  // whole waves leave together
  const float* d = dense + (int64_t)row * cols;
  const float* m = pat + (int64_t)row * cols;
  int n = FILL ? ptr[row] : 0;
  for (int j0 = 0; j0 < cols; j0 += 64) {
    const int j = j0 + lane;
    const bool keep = j < cols && m[j] != 0.f;
    const unsigned long long mk = __ballot(keep);
    if (FILL && keep) {
      const int p = n + __popcll(mk & ((1ull << lane) - 1ull));
      col_idx[p] = j;
      val[p] = d[j];
      if (ent_row) ent_row[p] = row;
    }
    n += __popcll(mk);
  }
  if (!FILL && lane == 0) ptr[row] = n;
}

// One thread per (layer, column): the entries > SPARSE_EPS of the column in ascending row order (reads coalesce across columns)
template <bool FILL>
__global__ void __launch_bounds__(256) geom_pack_cols_kernel(const float* __restrict__ dense, int layers, int rows, int cols,
                                                             int* ptr, int* __restrict__ row_idx, float* __restrict__ cval) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= layers * cols) return;
  const int l = c / cols, j = c - l * cols;
  const float* d = dense + (int64_t)l * rows * cols + j;
  int n = FILL ? ptr[c] : 0;
  for (int i = 0; i < rows; ++i) {
    const float v = d[(int64_t)i * cols];
    if (v > SPARSE_EPS) {
      if (FILL) {
        row_idx[n] = i;
        cval[n] = v;
      }
      ++n;
    }
  }
  if (!FILL) ptr[c] = n;
}

// p[0 .. n) counts -> exclusive prefix sums in place, p[n] = total.  One workgroup: thread t owns a contiguous chunk.
__global__ void __launch_bounds__(1024) geom_scan_kernel(int* p, int n) {
  __shared__ int part[1024];
  const int t = threadIdx.x;
  const int chunk = (n + 1023) / 1024;
  const int lo = t * chunk < n ? t * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
  int s = 0;
  for (int i = lo; i < hi; ++i) s += p[i];
  part[t] = s;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int add = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  int run = part[t] - s;
  for (int i = lo; i < hi; ++i) {
    const int v = p[i];
    p[i] = run;
    run += v;
  }
  if (t == 1023) p[n] = part[1023];
}

// ---- y[r, l, i] = sum_j M[l, i, j] x[r, l, j] ------------------------------------------------------------------------
// A lane per row of a layer.  mode 0: plain; 1: the input is x * scale + shift; 2: the output is (y - shift) / scale.
__global__ void __launch_bounds__(256) geom_apply_kernel(const int* __restrict__ row_ptr, const int* __restrict__ col_idx,
                                                         const float* __restrict__ val, const float* __restrict__ x,
                                                         float* __restrict__ y, int layers, int rows, int cols, int batch_rows,
                                                         float scale, float shift, int mode) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  for (int l = blockIdx.y; l < layers; l += gridDim.y) {
    const int lo = row_ptr[l * rows + i], hi = row_ptr[l * rows + i + 1];
    for (int r = blockIdx.z; r < batch_rows; r += gridDim.z) {
      const float* xr = x + ((int64_t)r * layers + l) * cols;
      float acc = 0.f;
      for (int p = lo; p < hi; ++p) {
        float xv = xr[col_idx[p]];
        if (mode == 1) xv = __fadd_rn(__fmul_rn(xv, scale), shift);
        acc = fmaf(val[p], xv, acc);
      }
      if (mode == 2) acc = __fdiv_rn(__fsub_rn(acc, shift), scale);
      y[((int64_t)r * layers + l) * rows + i] = acc;
    }
  }
}

// ---- sampled decode ------------------------------------------------------------------------------------------------
// u + m of entry (b, l, n, e), the same instruction sequence in both passes (the product by 2^-24 inside philox_uniform is exact)
__device__ __forceinline__ float sparse_r(const float* __restrict__ rand, uint64_t seed, uint64_t offset, int64_t dense_index,
                                          float m) {
  const float u = rand ? rand[dense_index] : philox_uniform(offset + (uint64_t)dense_index, seed);
  return __fadd_rn(u, m);
}

// pass A: a thread per (b, l, e) -> count_ws[(b L + l) cols + e] = {argmax n (-1: empty column), selected entries}
__global__ void __launch_bounds__(256) geom_sparse_select_kernel(const int* __restrict__ col_ptr, const int* __restrict__ row_idx,
                                                                 const float* __restrict__ cval, int2* __restrict__ count_ws,
                                                                 int layers, int rows, int cols, int n_b,
                                                                 const float* __restrict__ rand, uint64_t seed, uint64_t offset) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (int64_t)n_b * layers * cols) return;
  const int c = (int)(g % ((int64_t)layers * cols));  // l cols + e
  const int64_t bl = g / cols;                        // b L + l
  const int e = c % cols;
  int best = -1, above = 0;
  float rbest = 0.f;
  bool best_above = false;
  for (int p = col_ptr[c]; p < col_ptr[c + 1]; ++p) {
    const int n = row_idx[p];
    const float r = sparse_r(rand, seed, offset, (bl * rows + n) * cols + e, cval[p]);
    const bool ab = r > 1.0f;
    above += ab ? 1 : 0;
    if (best < 0 || r > rbest) {
      best = n;
      rbest = r;
      best_above = ab;
    }
  }
  count_ws[g] = make_int2(best, above + ((best >= 0 && !best_above) ? 1 : 0));
}

// pass B: a thread per (b, c, l, n) gathers its row
__global__ void __launch_bounds__(256) geom_sparse_gather_kernel(const int* __restrict__ row_ptr, const int* __restrict__ col_idx,
                                                                 const float* __restrict__ val, const int2* __restrict__ count_ws,
                                                                 const float* __restrict__ x, float* __restrict__ y, int layers,
                                                                 int rows, int cols, int batch, int channels, int per_batch,
                                                                 const float* __restrict__ rand, uint64_t seed, uint64_t offset) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= rows) return;
  for (int l = blockIdx.y; l < layers; l += gridDim.y) {
    const int lo = row_ptr[l * rows + n], hi = row_ptr[l * rows + n + 1];
    for (int bc = blockIdx.z; bc < batch * channels; bc += gridDim.z) {
      const int b = bc / channels;
      const int64_t bl = (int64_t)(per_batch ? 0 : b) * layers + l;  // the shower whose selection this one uses
      const float* xr = x + ((int64_t)bc * layers + l) * cols;
      float acc = 0.f;
      for (int p = lo; p < hi; ++p) {
        const float m = val[p];
        if (!(m > SPARSE_EPS)) continue;
        const int e = col_idx[p];
        const int2 sel = count_ws[bl * cols + e];
        if (sel.x == n || sparse_r(rand, seed, offset, (bl * rows + n) * cols + e, m) > 1.0f)
          acc = __fadd_rn(acc, __fdiv_rn(xr[e], (float)sel.y));
      }
      y[((int64_t)bc * layers + l) * rows + n] = acc;
    }
  }
}

// ---- HGCal forward pre-processing: cells -> training batch -----------------------------------------------------------
// preprocess_hgcal_shower and the loader around it (calodiffusion/utils/HGCal_utils.py:20-86, 125-162), one workgroup per shower
// so that a row has the same bits in any batch or shard.  FUSED: the shower arrives as raw cells; a layer's cell row is staged
// in LDS (coalesced reads, the next layer's in flight in registers meanwhile), multiplied by shower_scale, and a thread per grid
// row forms the CSR row sum exactly as geom_apply_kernel does (ascending columns, the same fmaf chain, the same (y - mean) / std);
// the grid never leaves LDS.  Otherwise the shower is already on the grid and is kept in LDS when it fits (`cached`), re-read
// when it does not.  From there, as the reference forms the values:
//   q = grid / (max_deposit e)                       float32
//   'layer' maps (the reference's arrays are masked arrays there, whose arithmetic with python scalars is float64):
//     layer sums and the total                       float32 in the reference; here summed in fp64 in a fixed order (a wave per
//                                                    layer, lane-strided, xor butterfly; the total over the layers in layer
//                                                    order) and rounded to float32 once
//     layers / total                                 float32 quotient; from here on float64: logit, both normalisations, and the
//                                                    logit and normalisation of every voxel, rounded to float32 at the end
//   'logit-norm'                                     everything float32
// logit is np.ma.log(o / (1 - o)).filled(0): 0 wherever the argument is not positive or the logarithm not finite (and where
// layers / total is not finite: a total of 0), BEFORE the normalisation.
namespace {
constexpr int kHgThreads = 512;
constexpr int kHgStageRegs = 4;                          // staged cells of a layer per thread
constexpr int kHgMaxCells = kHgThreads * kHgStageRegs;   // fused form: cells per layer (8 KB of staging)
constexpr size_t kHgGridBytes = 48 * 1024;               // grid of one shower in LDS up to this size
constexpr int kHgFusedMaxLayers = 512;                   // fused form: 4 KB of layer sums; 60 KB of LDS in all
constexpr int kHgMaxLayers = 4096;
constexpr int kHgMaxGenCols = 8;

struct PreHgcalArgs {
  const int* row_ptr;  // the packed encoder (fused form only)
  const int* col_idx;
  const float* val;
  const float* showers;
  int64_t row_stride;
  const float* gen_info;
  float* out;
  float* layerE;
  float* e_out;
  int32_t* status;
  int layers, cells, grid, gen_cols, layer_mode, embed_affine;
  double logit_mean, logit_std, totalE_mean, totalE_std, layers_mean, layers_std;
  float embed_mean, embed_std, max_deposit, scale;
  double emin[kHgMaxGenCols], emax[kHgMaxGenCols];
};

__device__ __forceinline__ double hg_logit64(double x) {
#pragma clang fp contract(off)
  const double o = 1e-8 + (1.0 - 2.0 * 1e-8) * x;
  const double r = o / (1.0 - o);
  const double lg = log(r);
  return (r > 0.0 && isfinite(lg)) ? lg : 0.0;
}
__device__ __forceinline__ float hg_logit32(float x) {
#pragma clang fp contract(off)
  const float o = 1e-8f + x;  // numpy rounds 1 - 2e-8 to the array's float32: 1
  const float r = o / (1.f - o);
  const float lg = logf(r);
  return (r > 0.f && isfinite(lg)) ? lg : 0.f;
}
}  // namespace

template <bool FUSED>
__global__ void __launch_bounds__(kHgThreads) preprocess_hgcal_kernel(PreHgcalArgs a, int cached) {
  extern __shared__ double hg_smem[];  // layer sums (padded to 16 bytes), q of the shower when cached, a cell row when FUSED
  const int b = blockIdx.x, tid = threadIdx.x;
  const int L = a.layers, E = a.grid, NV = L * E;
  const float e = a.gen_info[(size_t)b * a.gen_cols];
  if (!(e > 0.f) || isinf(e)) {  // uniform over the workgroup
    if (tid == 0) atomicMax(a.status, b + 1);
    return;
  }
  // np.array(emin) is float64: a double computation rounded once (HGCal_utils.py:131-132, 158)
  if (tid < a.gen_cols)
    a.e_out[(size_t)b * a.gen_cols + tid] = energy_to_cond_hgcal(a.gen_info[(size_t)b * a.gen_cols + tid], a.emin[tid], a.emax[tid]);
  double* lsum = hg_smem;
  float* q_lds = (float*)(hg_smem + ((L + 1) & ~1));
  const float denom = __fmul_rn(a.max_deposit, e);
  const float* in = a.showers + (size_t)b * L * a.row_stride;
  float* out = a.out + (size_t)b * NV;

  if (FUSED) {
    float* stage = q_lds + NV;
    float r[kHgStageRegs];
#pragma unroll
    for (int k = 0; k < kHgStageRegs; ++k) {
      const int j = tid + k * kHgThreads;
      r[k] = j < a.cells ? in[j] : 0.f;
    }
    for (int l = 0; l < L; ++l) {
#pragma unroll
      for (int k = 0; k < kHgStageRegs; ++k) {
        const int j = tid + k * kHgThreads;
        if (j < a.cells) stage[j] = __fmul_rn(r[k], a.scale);
      }
      __syncthreads();
      if (l + 1 < L) {
        const float* nx = in + (size_t)(l + 1) * a.row_stride;
#pragma unroll
        for (int k = 0; k < kHgStageRegs; ++k) {
          const int j = tid + k * kHgThreads;
          r[k] = j < a.cells ? nx[j] : 0.f;
        }
      }
      for (int i = tid; i < E; i += kHgThreads) {
        const int lo = a.row_ptr[l * E + i], hi = a.row_ptr[l * E + i + 1];
        float acc = 0.f;
        for (int p = lo; p < hi; ++p) acc = fmaf(a.val[p], stage[a.col_idx[p]], acc);
        if (a.embed_affine) acc = __fdiv_rn(__fsub_rn(acc, a.embed_mean), a.embed_std);
        q_lds[l * E + i] = __fdiv_rn(acc, denom);
      }
      __syncthreads();  // the row is consumed before the next one is staged; after the last, q is complete
    }
  }

  if (a.layer_mode) {
    const int wave = tid >> 6, lane = tid & 63;
    for (int z = wave; z < L; z += kHgThreads / 64) {
      double acc = 0.0;
      for (int i = lane; i < E; i += 64) {
        float q;
        if (FUSED) {
          q = q_lds[z * E + i];
        } else {
          q = __fdiv_rn(in[z * E + i], denom);
          if (cached) q_lds[z * E + i] = q;
        }
        acc += (double)q;
      }
      for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
      if (lane == 0) lsum[z] = acc;
    }
    __syncthreads();
    double total = 0.0;
    for (int z = 0; z < L; ++z) total += lsum[z];  // every thread, layer order
    const float total32 = (float)total;
    float* le = a.layerE + (size_t)b * (L + 1);
    if (tid == 0) le[0] = (float)(((double)total32 - a.totalE_mean) / a.totalE_std);
    for (int z = tid; z < L; z += kHgThreads) {
      const float share = __fdiv_rn((float)lsum[z], total32);  // np.ma.divide masks it where it is not finite (total == 0)
      const double lg = isfinite(share) ? hg_logit64((double)share) : 0.0;
      le[1 + z] = (float)((lg - a.layers_mean) / a.layers_std);
    }
    for (int i = tid; i < NV; i += kHgThreads) {
      const float q = (FUSED || cached) ? q_lds[i] : __fdiv_rn(in[i], denom);
      out[i] = (float)((hg_logit64((double)q) - a.logit_mean) / a.logit_std);
    }
  } else {
    const float mean = (float)a.logit_mean, std = (float)a.logit_std;
    for (int i = tid; i < NV; i += kHgThreads) {
      const float q = FUSED ? q_lds[i] : __fdiv_rn(in[i], denom);
      out[i] = __fdiv_rn(__fsub_rn(hg_logit32(q), mean), std);
    }
  }
}

// The transposed view of the packed entries: one thread per (layer, column) walks the pattern down the rows and, in the fill pass,
// finds each kept entry's place in its CSR row (ascending columns: a binary search).  Rows come out ascending within a column.
template <bool FILL>
__global__ void __launch_bounds__(256) geom_pack_transposed_kernel(const float* __restrict__ pat, int layers, int rows, int cols,
                                                                   const int* __restrict__ row_ptr, const int* __restrict__ col_idx,
                                                                   int* ptr, int* __restrict__ t_row, int* __restrict__ t_pos) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= layers * cols) return;
  const int l = c / cols, j = c - l * cols;
  const float* m = pat + (int64_t)l * rows * cols + j;
  int n = FILL ? ptr[c] : 0;
  for (int i = 0; i < rows; ++i) {
    if (m[(int64_t)i * cols] == 0.f) continue;
    if (FILL) {
      int lo = row_ptr[l * rows + i], hi = row_ptr[l * rows + i + 1] - 1;
      while (lo < hi) {  // (the entry is there: both passes read one pattern)
        const int mid = (lo + hi) >> 1;
        if (col_idx[mid] < j) lo = mid + 1;
        else hi = mid;
      }
      t_row[n] = i;
      t_pos[n] = lo;
    }
    ++n;
  }
  if (!FILL) ptr[c] = n;
}

// val[p] = dense[row of p, column of p]: a trainable map's values from its live parameter (cd_geom_refresh)
__global__ void __launch_bounds__(256) geom_refresh_kernel(const float* __restrict__ dense, const int* __restrict__ ent_row,
                                                           const int* __restrict__ col_idx, float* __restrict__ val, int nnz, int cols) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p < nnz) val[p] = dense[(int64_t)ent_row[p] * cols + col_idx[p]];
}

enum GeomPack { kPackRows, kPackColumns, kPackTransposed };

// counts, scan, fill.  Returns the number of entries.  kPackRows fills m->row_ptr / col_idx / val / ent_row, kPackColumns the column
// view of the entries > SPARSE_EPS, kPackTransposed the transposed view of the rows' entries (after kPackRows).
static int pack(CdGeomMap* m, GeomPack kind, const float* dense, const float* pat, hipStream_t s) {
  const int layers = m->layers, rows = m->rows, cols = m->cols;
  const int n_lines = layers * (kind == kPackRows ? rows : cols);
  int* ptr = nullptr;
  CD_HIP(hipMalloc(&ptr, sizeof(int) * ((size_t)n_lines + 1)));
  (kind == kPackRows ? m->row_ptr : kind == kPackColumns ? m->col_ptr : m->t_ptr) = ptr;
  const dim3 grid_rows((unsigned)((n_lines + 3) / 4)), grid_cols((unsigned)((n_lines + 255) / 256));
  auto launch = [&](auto fill) {
    constexpr bool F = decltype(fill)::value;
    if (kind == kPackColumns)
      hipLaunchKernelGGL(geom_pack_cols_kernel<F>, grid_cols, dim3(256), 0, s, dense, layers, rows, cols, ptr, m->row_idx, m->cval);
    else if (kind == kPackRows)
      hipLaunchKernelGGL(geom_pack_rows_kernel<F>, grid_rows, dim3(256), 0, s, dense, pat, n_lines, cols, ptr, m->col_idx, m->val, m->ent_row);
    else
      hipLaunchKernelGGL(geom_pack_transposed_kernel<F>, grid_cols, dim3(256), 0, s, pat, layers, rows, cols, m->row_ptr, m->col_idx, ptr,
                         m->t_row, m->t_pos);
    CD_HIP(hipGetLastError());
  };
  launch(std::false_type{});
  hipLaunchKernelGGL(geom_scan_kernel, dim3(1), dim3(1024), 0, s, ptr, n_lines);
  CD_HIP(hipGetLastError());
  int nnz = 0;
  CD_HIP(hipMemcpyAsync(&nnz, ptr + n_lines, sizeof(int), hipMemcpyDeviceToHost, s));
  CD_HIP(hipStreamSynchronize(s));
  const size_t n = (size_t)(nnz > 0 ? nnz : 1);
  if (kind == kPackRows) {
    CD_HIP(hipMalloc(&m->col_idx, sizeof(int) * n));
    CD_HIP(hipMalloc(&m->val, sizeof(float) * n));
    CD_HIP(hipMalloc(&m->ent_row, sizeof(int) * n));
  } else if (kind == kPackColumns) {
    CD_HIP(hipMalloc(&m->row_idx, sizeof(int) * n));
    CD_HIP(hipMalloc(&m->cval, sizeof(float) * n));
  } else {
    CD_HIP(hipMalloc(&m->t_row, sizeof(int) * n));
    CD_HIP(hipMalloc(&m->t_pos, sizeof(int) * n));
  }
  launch(std::true_type{});
  return nnz;
}

static void geom_create(const float* dense, const float* mask, int layers, int rows, int cols, int flags, CdGeomMap** out,
                        hipStream_t s) {
  CD_REQUIRE(dense && out && layers > 0 && rows > 0 && cols > 0, "bad argument");
  CD_REQUIRE((flags & ~(CD_GEOM_COLUMNS | CD_GEOM_TRANSPOSED)) == 0, "cd_geom_create_ex: unknown flag");
  CD_REQUIRE(!(mask && (flags & CD_GEOM_COLUMNS)),
             "cd_geom_create_ex: no column view over a mask (the sampled decode's view holds values, which a refresh would leave stale)");
  CD_REQUIRE((int64_t)layers * rows * cols <= INT_MAX && (int64_t)layers * (rows > cols ? rows : cols) <= (1 << 30),
             "cd_geom_create: layers * rows * cols must stay below 2^31 (and layers * max(rows, cols) within 2^30)");
  struct Owner {
    CdGeomMap* m;
    ~Owner() { delete m; }
  } own{new CdGeomMap};
  CdGeomMap* m = own.m;
  m->layers = layers; m->rows = rows; m->cols = cols; m->masked = mask != nullptr;
  m->nnz = pack(m, kPackRows, dense, mask ? mask : dense, s);
  if (flags & CD_GEOM_COLUMNS) pack(m, kPackColumns, dense, nullptr, s);
  if (flags & CD_GEOM_TRANSPOSED) pack(m, kPackTransposed, dense, mask ? mask : dense, s);
  CD_HIP(hipStreamSynchronize(s));  // the caller may free `dense` and `mask` when this returns
  *out = m;
  own.m = nullptr;
}

// ---- a packed map from its sparse entries (cd_geom_create_csr) -------------------------------------------------------
// The CSR arrays are the caller's, uploaded as they are.  ent_row: a thread per line writes its own number over its entries.
__global__ void __launch_bounds__(256) geom_csr_ent_row_kernel(const int* __restrict__ row_ptr, int n_lines, int* __restrict__ ent_row) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_lines) return;
  for (int p = row_ptr[r]; p < row_ptr[r + 1]; ++p) ent_row[p] = r;
}

// The two views by column, without the dense tensor: a thread per entry counts its (layer, column) line (integer atomics), the
// scan turns counts into line starts, a thread per entry takes a slot of its line (in whatever order the threads arrive) and a
// thread per line sorts its slots by CSR position -- a line holds at most one entry of a row and positions ascend with the
// rows, so the sorted line is rows ascending and no longer depends on the order of arrival.  positive_only: the entries
// > SPARSE_EPS (the sampled decode's view); otherwise all of them (the transposed view).
__device__ __forceinline__ bool csr_kept(const float* __restrict__ val, int p, int positive_only) {
  return !positive_only || val[p] > SPARSE_EPS;
}
__device__ __forceinline__ int csr_line(const int* __restrict__ ent_row, const int* __restrict__ col_idx, int p, int rows, int cols) {
  return (ent_row[p] / rows) * cols + col_idx[p];
}
template <bool FILL>
__global__ void __launch_bounds__(256) geom_csr_by_column_kernel(const int* __restrict__ ent_row, const int* __restrict__ col_idx,
                                                                 const float* __restrict__ val, int nnz, int rows, int cols,
                                                                 int positive_only, int* cursor, int* __restrict__ slot) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= nnz || !csr_kept(val, p, positive_only)) return;
  const int at = atomicAdd(&cursor[csr_line(ent_row, col_idx, p, rows, cols)], 1);
  if (FILL) slot[at] = p;
}
// ptr: the scanned line starts.  out_row: the row within the layer; out_pos (transposed view) or out_val (column view).
__global__ void __launch_bounds__(256) geom_csr_sort_lines_kernel(const int* __restrict__ ptr, int n_lines, int* __restrict__ slot,
                                                                  const int* __restrict__ ent_row, const float* __restrict__ val,
                                                                  int rows, int* __restrict__ out_row, int* __restrict__ out_pos,
                                                                  float* __restrict__ out_val) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n_lines) return;
  const int lo = ptr[c], hi = ptr[c + 1];
  for (int i = lo + 1; i < hi; ++i) {  // insertion sort: a line holds a handful of entries
    const int key = slot[i];
    int j = i - 1;
    for (; j >= lo && slot[j] > key; --j) slot[j + 1] = slot[j];
    slot[j + 1] = key;
  }
  for (int i = lo; i < hi; ++i) {
    const int p = slot[i];
    out_row[i] = ent_row[p] % rows;
    if (out_pos) out_pos[i] = p;
    if (out_val) out_val[i] = val[p];
  }
}

struct DeviceInts {  // scratch of one view's build
  int* p = nullptr;
  ~DeviceInts() {
    if (p) (void)hipFree(p);
  }
};

// kPackColumns or kPackTransposed from the uploaded CSR arrays (and ent_row)
static void pack_csr_view(CdGeomMap* m, GeomPack kind, hipStream_t s) {
  const int n_lines = m->layers * m->cols, nnz = m->nnz, positive_only = kind == kPackColumns;
  int* ptr = nullptr;
  CD_HIP(hipMalloc(&ptr, sizeof(int) * ((size_t)n_lines + 1)));
  (kind == kPackColumns ? m->col_ptr : m->t_ptr) = ptr;
  CD_HIP(hipMemsetAsync(ptr, 0, sizeof(int) * ((size_t)n_lines + 1), s));
  const dim3 per_entry((unsigned)((nnz + 255) / 256)), per_line((unsigned)((n_lines + 255) / 256));
  if (nnz > 0) {
    hipLaunchKernelGGL(geom_csr_by_column_kernel<false>, per_entry, dim3(256), 0, s, m->ent_row, m->col_idx, m->val, nnz, m->rows, m->cols,
                       positive_only, ptr, (int*)nullptr);
    CD_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(geom_scan_kernel, dim3(1), dim3(1024), 0, s, ptr, n_lines);
  CD_HIP(hipGetLastError());
  int kept = 0;
  CD_HIP(hipMemcpyAsync(&kept, ptr + n_lines, sizeof(int), hipMemcpyDeviceToHost, s));
  CD_HIP(hipStreamSynchronize(s));
  const size_t n = (size_t)(kept > 0 ? kept : 1);
  if (kind == kPackColumns) {
    CD_HIP(hipMalloc(&m->row_idx, sizeof(int) * n));
    CD_HIP(hipMalloc(&m->cval, sizeof(float) * n));
  } else {
    CD_HIP(hipMalloc(&m->t_row, sizeof(int) * n));
    CD_HIP(hipMalloc(&m->t_pos, sizeof(int) * n));
  }
  if (kept == 0) return;
  DeviceInts cursor, slot;
  CD_HIP(hipMalloc(&cursor.p, sizeof(int) * (size_t)n_lines));
  CD_HIP(hipMalloc(&slot.p, sizeof(int) * n));
  CD_HIP(hipMemcpyAsync(cursor.p, ptr, sizeof(int) * (size_t)n_lines, hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(geom_csr_by_column_kernel<true>, per_entry, dim3(256), 0, s, m->ent_row, m->col_idx, m->val, nnz, m->rows, m->cols,
                     positive_only, cursor.p, slot.p);
  CD_HIP(hipGetLastError());
  hipLaunchKernelGGL(geom_csr_sort_lines_kernel, per_line, dim3(256), 0, s, ptr, n_lines, slot.p, m->ent_row, m->val, m->rows,
                     kind == kPackColumns ? m->row_idx : m->t_row, kind == kPackColumns ? (int*)nullptr : m->t_pos,
                     kind == kPackColumns ? m->cval : (float*)nullptr);
  CD_HIP(hipGetLastError());
  CD_HIP(hipStreamSynchronize(s));  // the scratch goes
}

static void geom_create_csr(const int32_t* row_ptr, const int32_t* col_idx, const float* val, int layers, int rows, int cols, int flags,
                            CdGeomMap** out, hipStream_t s) {
  CD_REQUIRE(row_ptr && out && layers > 0 && rows > 0 && cols > 0, "bad argument");
  CD_REQUIRE((flags & ~(CD_GEOM_COLUMNS | CD_GEOM_TRANSPOSED)) == 0, "cd_geom_create_csr: unknown flag");
  CD_REQUIRE((int64_t)layers * (rows > cols ? rows : cols) <= cdgeom::kMaxLines, "cd_geom_create_csr: layers * max(rows, cols) must stay within 2^30");
  const int n_lines = layers * rows;
  const int nnz = row_ptr[n_lines];
  CD_REQUIRE(nnz >= 0 && (nnz == 0 || (col_idx && val)), "cd_geom_create_csr: col_idx and val are required for a map with entries");
  std::string err;
  if (!cdgeom::csr_valid((const unsigned char*)row_ptr, (const unsigned char*)col_idx, (const unsigned char*)val, layers, rows, cols, nnz, &err))
    throw Fail{CD_EINVAL, "cd_geom_create_csr: " + err};
  struct Owner {
    CdGeomMap* m;
    ~Owner() { delete m; }
  } own{new CdGeomMap};
  CdGeomMap* m = own.m;
  m->layers = layers; m->rows = rows; m->cols = cols; m->nnz = nnz;
  const size_t n = (size_t)(nnz > 0 ? nnz : 1);
  bool zeros = false;  // a pattern with zeros is a mask's (cd_geom_create_ex's `masked`)
  for (int p = 0; p < nnz && !zeros; ++p) zeros = val[p] == 0.f;
  m->masked = zeros;
  CD_HIP(hipMalloc(&m->row_ptr, sizeof(int) * ((size_t)n_lines + 1)));
  CD_HIP(hipMalloc(&m->col_idx, sizeof(int) * n));
  CD_HIP(hipMalloc(&m->val, sizeof(float) * n));
  CD_HIP(hipMalloc(&m->ent_row, sizeof(int) * n));
  CD_HIP(hipMemcpyAsync(m->row_ptr, row_ptr, sizeof(int) * ((size_t)n_lines + 1), hipMemcpyHostToDevice, s));
  if (nnz > 0) {
    CD_HIP(hipMemcpyAsync(m->col_idx, col_idx, sizeof(int) * n, hipMemcpyHostToDevice, s));
    CD_HIP(hipMemcpyAsync(m->val, val, sizeof(float) * n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(geom_csr_ent_row_kernel, dim3((unsigned)((n_lines + 255) / 256)), dim3(256), 0, s, m->row_ptr, n_lines, m->ent_row);
    CD_HIP(hipGetLastError());
  }
  if (flags & CD_GEOM_COLUMNS) pack_csr_view(m, kPackColumns, s);
  if (flags & CD_GEOM_TRANSPOSED) pack_csr_view(m, kPackTransposed, s);
  CD_HIP(hipStreamSynchronize(s));  // the caller may free its arrays when this returns
  *out = m;
  own.m = nullptr;
}

// grid of the two per-row kernels: x covers the rows, y the layers, z the batch rows (both strided past the grid limit)
static dim3 row_grid(const CdGeomMap* m, int64_t batch_rows) {
  return dim3((unsigned)((m->rows + 255) / 256), (unsigned)(m->layers < 65535 ? m->layers : 65535),
              (unsigned)(batch_rows < 65535 ? batch_rows : 65535));
}

}  // namespace cd

extern "C" {

int cd_geom_create(const float* dense_dev, int layers, int rows, int cols, int want_columns, CdGeomMap** out, void* stream) {
  return guarded([&] { geom_create(dense_dev, nullptr, layers, rows, cols, want_columns ? CD_GEOM_COLUMNS : 0, out, (hipStream_t)stream); });
}

int cd_geom_create_ex(const float* dense_dev, const float* mask_dev, int layers, int rows, int cols, int flags, CdGeomMap** out,
                      void* stream) {
  return guarded([&] { geom_create(dense_dev, mask_dev, layers, rows, cols, flags, out, (hipStream_t)stream); });
}

int cd_geom_create_csr(const int32_t* row_ptr, const int32_t* col_idx, const float* val, int layers, int rows, int cols, int flags,
                       CdGeomMap** out, void* stream) {
  return guarded([&] { geom_create_csr(row_ptr, col_idx, val, layers, rows, cols, flags, out, (hipStream_t)stream); });
}

int cd_geom_refresh(CdGeomMap* map, const float* dense_dev, void* stream) {
  return guarded([&] {
    CD_REQUIRE(map && dense_dev, "bad argument");
    if (map->nnz > 0) {
      hipLaunchKernelGGL(geom_refresh_kernel, dim3((unsigned)((map->nnz + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dense_dev,
                         map->ent_row, map->col_idx, map->val, map->nnz, map->cols);
      CD_HIP(hipGetLastError());
    }
  });
}

int cd_geom_destroy(CdGeomMap* map) {
  return guarded([&] { delete map; });
}

int cd_geom_apply(const CdGeomMap* map, const float* x, float* y, int batch_rows, float scale, float shift, int affine_first,
                  void* stream) {
  return guarded([&] {
    CD_REQUIRE(map && x && y && batch_rows > 0, "bad argument");
    CD_REQUIRE(scale != 0.f, "cd_geom_apply: scale (embed_std) must not be 0");
    const int mode = (scale == 1.f && shift == 0.f) ? 0 : (affine_first ? 1 : 2);
    hipLaunchKernelGGL(geom_apply_kernel, row_grid(map, batch_rows), dim3(256), 0, (hipStream_t)stream, map->row_ptr, map->col_idx,
                       map->val, x, y, map->layers, map->rows, map->cols, batch_rows, scale, shift, mode);
    CD_HIP(hipGetLastError());
  });
}

int cd_geom_sparse_workspace_bytes(const CdGeomMap* map, int batch, size_t* bytes) {
  return guarded([&] {
    CD_REQUIRE(map && bytes && batch > 0, "bad argument");
    *bytes = sizeof(int2) * (size_t)batch * (size_t)map->layers * (size_t)map->cols;
  });
}

int cd_geom_decode_sparse(const CdGeomMap* map, const float* x, float* y, int batch, int channels, int per_batch,
                          const float* rand, uint64_t seed, uint64_t offset, void* count_ws, void* stream) {
  return guarded([&] {
    CD_REQUIRE(map && x && y && count_ws && batch > 0 && channels > 0, "bad argument");
    CD_REQUIRE(map->col_ptr, "cd_geom_decode_sparse: the map was created without its column view (want_columns)");
    CD_REQUIRE((int64_t)batch * channels <= INT_MAX, "cd_geom_decode_sparse: batch * channels must stay below 2^31");
    hipStream_t s = (hipStream_t)stream;
    const int n_b = per_batch ? 1 : batch;
    const int64_t items = (int64_t)n_b * map->layers * map->cols;
    CD_REQUIRE((items + 255) / 256 <= INT_MAX, "cd_geom_decode_sparse: batch too large");
    hipLaunchKernelGGL(geom_sparse_select_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, map->col_ptr, map->row_idx,
                       map->cval, (int2*)count_ws, map->layers, map->rows, map->cols, n_b, rand, seed, offset);
    CD_HIP(hipGetLastError());
    hipLaunchKernelGGL(geom_sparse_gather_kernel, row_grid(map, (int64_t)batch * channels), dim3(256), 0, s, map->row_ptr,
                       map->col_idx, map->val, (const int2*)count_ws, x, y, map->layers, map->rows, map->cols, batch, channels,
                       per_batch ? 1 : 0, rand, seed, offset);
    CD_HIP(hipGetLastError());
  });
}

int cd_preprocess_hgcal(const CdGeomMap* enc, const float* showers, int64_t row_stride, const float* gen_info, int gen_cols,
                        float* out, float* layerE, float* e_out, int32_t* status, int batch, int layers, int cells, int grid,
                        const double consts[6], float embed_mean, float embed_std, float max_deposit, const double* emin,
                        const double* emax, float shower_scale, void* stream) {
  return guarded([&] {
    CD_REQUIRE(showers && gen_info && out && e_out && status && consts && emin && emax && batch > 0, "bad argument");
    CD_REQUIRE(layers > 0 && layers <= kHgMaxLayers && cells > 0 && grid > 0 && (int64_t)layers * grid <= ((int64_t)1 << 28) &&
                   row_stride >= cells,
               "cd_preprocess_hgcal: 1..4096 layers, at most 2^28 grid values per shower, row_stride >= cells");
    CD_REQUIRE(gen_cols >= 1 && gen_cols <= kHgMaxGenCols, "cd_preprocess_hgcal: gen_info has 1..8 columns");
    for (int k = 0; k < gen_cols; ++k) CD_REQUIRE(emax[k] > emin[k], "cd_preprocess_hgcal: emax > emin in every column");
    CD_REQUIRE(max_deposit > 0.f && consts[1] != 0.0 && consts[3] != 0.0 && consts[5] != 0.0,
               "cd_preprocess_hgcal: max_deposit must be positive and the three std constants non-zero");
    PreHgcalArgs a{};
    a.showers = showers; a.row_stride = row_stride; a.gen_info = gen_info; a.out = out; a.layerE = layerE; a.e_out = e_out;
    a.status = status; a.layers = layers; a.cells = cells; a.grid = grid; a.gen_cols = gen_cols; a.layer_mode = layerE ? 1 : 0;
    a.logit_mean = consts[0]; a.logit_std = consts[1]; a.totalE_mean = consts[2]; a.totalE_std = consts[3];
    a.layers_mean = consts[4]; a.layers_std = consts[5]; a.max_deposit = max_deposit;
    for (int k = 0; k < gen_cols; ++k) {
      a.emin[k] = emin[k];
      a.emax[k] = emax[k];
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t sums = sizeof(double) * (size_t)((layers + 1) & ~1), grid_bytes = sizeof(float) * (size_t)layers * grid;
    if (enc) {
      CD_REQUIRE(enc->layers == layers && enc->rows == grid && enc->cols == cells,
                 "cd_preprocess_hgcal: the map is not (layers, grid, cells)");
      CD_REQUIRE(embed_std != 0.f && shower_scale > 0.f, "cd_preprocess_hgcal: embed_std must not be 0, shower_scale positive");
      CD_REQUIRE(grid_bytes <= kHgGridBytes && cells <= kHgMaxCells && layers <= kHgFusedMaxLayers,
                 "cd_preprocess_hgcal: the fused form keeps the grid of a shower on chip: layers * grid * 4 bytes <= 48 KB, "
                 "cells <= 2048, layers <= 512; beyond that apply the map first (cd_geom_apply) and pass enc = NULL");
      a.row_ptr = enc->row_ptr; a.col_idx = enc->col_idx; a.val = enc->val;
      a.embed_mean = embed_mean; a.embed_std = embed_std; a.scale = shower_scale;
      a.embed_affine = !(embed_std == 1.f && embed_mean == 0.f);  // cd_geom_apply's choice of the plain product
      CD_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
      hipLaunchKernelGGL(preprocess_hgcal_kernel<true>, dim3((unsigned)batch), dim3(kHgThreads),
                         sums + grid_bytes + sizeof(float) * (size_t)cells, s, a, 1);
    } else {
      CD_REQUIRE(cells == grid && row_stride == grid,
                 "cd_preprocess_hgcal: without a map the showers are (batch, layers, grid): cells = row_stride = grid");
      const int cached = a.layer_mode && grid_bytes <= kHgGridBytes && sums + grid_bytes <= 60 * 1024;
      CD_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
      hipLaunchKernelGGL(preprocess_hgcal_kernel<false>, dim3((unsigned)batch), dim3(kHgThreads), sums + (cached ? grid_bytes : 0),
                         s, a, cached);
    }
    CD_HIP(hipGetLastError());
  });
}

}  // extern "C"
