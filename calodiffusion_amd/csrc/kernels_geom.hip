// HGCal geometry maps (include/calodiff.h, "HGCal geometry maps"): a dense (layers, rows, cols) map packed into per-layer CSR (and,
// for the sparse decode, the column-major view of its entries > 1e-6), the product with a batch of showers, and
// generate_sparse_mat's sampled decode in two gather passes.  Kernels and their C ABI; nothing here touches a plan.
#include "philox.h"
#include "plan_internal.h"

#include <climits>

// row_ptr / col_ptr run over all layers: row i of layer l holds entries [row_ptr[l rows + i], row_ptr[l rows + i + 1])
struct CdGeomMap {
  int layers = 0, rows = 0, cols = 0;
  int* row_ptr = nullptr;  // layers * rows + 1
  int* col_idx = nullptr;  // nnz, ascending within a row
  float* val = nullptr;
  int* col_ptr = nullptr;  // layers * cols + 1, or null: no column view
  int* row_idx = nullptr;  // entries > SPARSE_EPS, ascending within a column
  float* cval = nullptr;
  ~CdGeomMap() {
    for (void* p : {(void*)row_ptr, (void*)col_idx, (void*)val, (void*)col_ptr, (void*)row_idx, (void*)cval})
      if (p) (void)hipFree(p);
  }
};

namespace cd {

constexpr float SPARSE_EPS = 1e-6f;  // generate_sparse_mat's eps (HGCal_utils.py:371)

// ---- packing: count, exclusive scan, fill --------------------------------------------------------------------------
// One wave per row: 64 consecutive columns per step, the kept ones numbered by the ballot's prefix count, so a row's entries
// come out in ascending column order.  fill == false: the row's count goes to ptr[row]; true: ptr is the scanned array.
template <bool FILL>
__global__ void __launch_bounds__(256) geom_pack_rows_kernel(const float* __restrict__ dense, int n_rows, int cols, int* ptr,
                                                             int* __restrict__ col_idx, float* __restrict__ val) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_rows) return;  // whole waves leave together
  const float* d = dense + (int64_t)row * cols;
  int n = FILL ? ptr[row] : 0;
  for (int j0 = 0; j0 < cols; j0 += 64) {
    const int j = j0 + lane;
    const float v = j < cols ? d[j] : 0.f;
    const bool keep = v != 0.f;
    const unsigned long long mk = __ballot(keep);
    if (FILL && keep) {
      const int p = n + __popcll(mk & ((1ull << lane) - 1ull));
      col_idx[p] = j;
      val[p] = v;
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

static void pack(const float* dense, int n_lines, bool columns, int layers, int rows, int cols, int** ptr_out, int** idx_out,
                 float** val_out, hipStream_t s) {
  int* ptr = nullptr;
  CD_HIP(hipMalloc(&ptr, sizeof(int) * ((size_t)n_lines + 1)));
  *ptr_out = ptr;
  const dim3 grid_rows((unsigned)((n_lines + 3) / 4)), grid_cols((unsigned)((n_lines + 255) / 256));
  if (columns) hipLaunchKernelGGL(geom_pack_cols_kernel<false>, grid_cols, dim3(256), 0, s, dense, layers, rows, cols, ptr, nullptr, nullptr);
  else hipLaunchKernelGGL(geom_pack_rows_kernel<false>, grid_rows, dim3(256), 0, s, dense, n_lines, cols, ptr, nullptr, nullptr);
  CD_HIP(hipGetLastError());
  hipLaunchKernelGGL(geom_scan_kernel, dim3(1), dim3(1024), 0, s, ptr, n_lines);
  CD_HIP(hipGetLastError());
  int nnz = 0;
  CD_HIP(hipMemcpyAsync(&nnz, ptr + n_lines, sizeof(int), hipMemcpyDeviceToHost, s));
  CD_HIP(hipStreamSynchronize(s));
  CD_HIP(hipMalloc(idx_out, sizeof(int) * (size_t)(nnz > 0 ? nnz : 1)));
  CD_HIP(hipMalloc(val_out, sizeof(float) * (size_t)(nnz > 0 ? nnz : 1)));
  if (columns) hipLaunchKernelGGL(geom_pack_cols_kernel<true>, grid_cols, dim3(256), 0, s, dense, layers, rows, cols, ptr, *idx_out, *val_out);
  else hipLaunchKernelGGL(geom_pack_rows_kernel<true>, grid_rows, dim3(256), 0, s, dense, n_lines, cols, ptr, *idx_out, *val_out);
  CD_HIP(hipGetLastError());
}

// grid of the two per-row kernels: x covers the rows, y the layers, z the batch rows (both strided past the grid limit)
static dim3 row_grid(const CdGeomMap* m, int64_t batch_rows) {
  return dim3((unsigned)((m->rows + 255) / 256), (unsigned)(m->layers < 65535 ? m->layers : 65535),
              (unsigned)(batch_rows < 65535 ? batch_rows : 65535));
}

}  // namespace cd

extern "C" {

int cd_geom_create(const float* dense_dev, int layers, int rows, int cols, int want_columns, CdGeomMap** out, void* stream) {
  return guarded([&] {
    CD_REQUIRE(dense_dev && out && layers > 0 && rows > 0 && cols > 0, "bad argument");
    CD_REQUIRE((int64_t)layers * rows * cols <= INT_MAX && (int64_t)layers * (rows > cols ? rows : cols) <= (1 << 30),
               "cd_geom_create: layers * rows * cols must stay below 2^31 (and layers * max(rows, cols) within 2^30)");
    hipStream_t s = (hipStream_t)stream;
    struct Owner {
      CdGeomMap* m;
      ~Owner() { delete m; }
    } own{new CdGeomMap};
    CdGeomMap* m = own.m;
    m->layers = layers; m->rows = rows; m->cols = cols;
    pack(dense_dev, layers * rows, false, layers, rows, cols, &m->row_ptr, &m->col_idx, &m->val, s);
    if (want_columns) pack(dense_dev, layers * cols, true, layers, rows, cols, &m->col_ptr, &m->row_idx, &m->cval, s);
    CD_HIP(hipStreamSynchronize(s));  // the caller may free `dense_dev` when this returns
    *out = m;
    own.m = nullptr;
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

}  // extern "C"
