// Dataset-1 radial maps (include/calodiff.h, "Dataset-1 radial maps"): GeomConverter / NNConverter of the reference
// (calodiffusion/utils/utils.py:576-784) as four launches -- enc, dec and the vector-Jacobian product of each -- over per-layer
// matrices that are live parameters.  Kernels and their C ABI; nothing here touches a plan.
//
// Two row programs serve the four operations, because a VJP with respect to the input is the other direction's product with the
// transposed matrix:
//   expand    flat (V) -> grid (L, A, R)   enc with W_i;  dec_vjp's dg with D_i^T
//   collapse  grid (L, A, R) -> flat (V)   dec with D_i;  enc_vjp's dx with W_i^T (and enc's division by A)
// A workgroup stages the layer table and every matrix of its direction in LDS once, k-major (the reduction index is the slow
// one), so that the lanes of a wave, which run along the output's fast index, read consecutive banks; it then walks showers
// blockIdx.x, blockIdx.x + row_blocks, ...: the shower is staged in LDS by coalesced reads and each thread forms whole output
// elements, an fmaf chain in ascending reduction index.  A result row never sees another row.
// The weight gradients ride in the same launch, in the workgroups after the row ones: a workgroup owns kRadTile consecutive
// elements of the concatenated gradient, its kRadSlices thread groups walk the showers b = slice, slice + kRadSlices, ... each in
// ascending (b, a), and a fixed tree over the slices in LDS finishes the element.  No atomics, no workspace.
#include "plan_internal.h"

#include <vector>

struct CdRadialMap {
  int layers = 0, A = 0, R = 0, V = 0, wtotal = 0;
  int4* lay = nullptr;  // device, per layer {bound, alpha, rin, float offset of its matrix}
  int* vlay = nullptr;  // device, layer of every voxel
  ~CdRadialMap() {
    if (lay) (void)hipFree(lay);
    if (vlay) (void)hipFree(vlay);
  }
};

namespace cd {
namespace {

constexpr int kRadThreads = 256;
constexpr int kRadMaxLayers = 64;     // 1 KB of layer table
constexpr int kRadMaxWeights = 8192;  // floats of one direction's matrices in LDS: 32 KB
constexpr int kRadMaxRow = 6144;      // floats of one staged shower, flat or on the grid: 24 KB
constexpr int kRadMaxRowBlocks = 1024;
constexpr int kRadTile = 32, kRadSlices = kRadThreads / kRadTile;  // weight gradient: elements per workgroup, batch slices
static_assert(kRadSlices == 8, "the tree below sums eight slices");

struct RadialArgs {
  const int4* lay;
  const int* vlay;
  const float* w;      // the matrices of this direction, concatenated
  const float* in;     // rows the row program reads
  float* out;          // rows it writes
  const float* other;  // weight gradient: the forward's input (`in` is then the cotangent)
  float* dw;           // weight gradient or null
  int L, A, R, V, wtotal, batch, row_blocks;
};

// lay_s[L] (16 bytes each), then the matrices (wtotal floats rounded up to 4) or the weight gradient's partial sums, then a row
__device__ __forceinline__ float* rad_weights(char* smem, int L) { return (float*)(smem + sizeof(int4) * (size_t)L); }
__device__ __forceinline__ float* rad_row(char* smem, int L, int wtotal) { return rad_weights(smem, L) + ((wtotal + 3) & ~3); }

__device__ __forceinline__ void rad_stage_layers(const RadialArgs& a, int4* lay_s) {
  for (int i = threadIdx.x; i < a.L; i += kRadThreads) lay_s[i] = a.lay[i];
}

// The matrices into LDS.  TRANSPOSE: a layer's (rows, cols) row-major matrix lands column-major; otherwise a straight copy.
// ROWS_ARE_R: the source is W_i (R, rin), else D_i (rin, R).  Reads of `w` are consecutive either way.
template <bool TRANSPOSE, bool ROWS_ARE_R>
__device__ __forceinline__ void rad_stage_weights(const RadialArgs& a, const int4* lay_s, float* wt) {
  if (!TRANSPOSE) {
    for (int e = threadIdx.x; e < a.wtotal; e += kRadThreads) wt[e] = a.w[e];
    return;
  }
  for (int i = 0; i < a.L; ++i) {
    const int4 ly = lay_s[i];
    const int rows = ROWS_ARE_R ? a.R : ly.z, cols = ROWS_ARE_R ? ly.z : a.R;
    for (int e = threadIdx.x; e < rows * cols; e += kRadThreads) {
      const int r = e / cols, c = e - r * cols;
      wt[ly.w + c * rows + r] = a.w[ly.w + e];
    }
  }
}

// One element of the concatenated weight gradient per thread of a slice.  ENC: dW_i[r, j] from gy (`in`, grid rows) and x
// (`other`, flat rows); otherwise dD_i[j, r] from gx (`in`, flat rows) and g (`other`, grid rows).
template <bool ENC>
__device__ __forceinline__ void rad_weight_grad(const RadialArgs& a, const int4* lay_s, float* part, int tile) {
  const int lane = threadIdx.x & (kRadTile - 1), slice = threadIdx.x / kRadTile;
  const int e = tile * kRadTile + lane;
  float acc = 0.f;
  if (e < a.wtotal) {
    int i = 0;
    while (i + 1 < a.L && lay_s[i + 1].w <= e) ++i;
    const int4 ly = lay_s[i];
    const int local = e - ly.w;
    const int r = ENC ? local / ly.z : local % a.R, j = ENC ? local % ly.z : local / a.R;
    const int LAR = a.L * a.A * a.R;
    const float* flat = (ENC ? a.other : a.in) + ly.x + j;                  // + b V + a rin
    const float* grid = (ENC ? a.in : a.other) + (size_t)i * a.A * a.R + r;  // + b LAR + a R
    if (ly.y == a.A) {
      for (int b = slice; b < a.batch; b += kRadSlices) {
        const float* fb = flat + (size_t)b * a.V;
        const float* gb = grid + (size_t)b * LAR;
        for (int aa = 0; aa < a.A; ++aa) acc = fmaf(gb[aa * a.R], fb[aa * ly.z], acc);
      }
    } else {  // alpha 1: the grid side is summed over a first (enc: and divided by A, as the forward divides)
      for (int b = slice; b < a.batch; b += kRadSlices) {
        const float* gb = grid + (size_t)b * LAR;
        float s = 0.f;
        for (int aa = 0; aa < a.A; ++aa) s = __fadd_rn(s, gb[aa * a.R]);
        if (ENC) s = __fdiv_rn(s, (float)a.A);
        acc = fmaf(s, flat[(size_t)b * a.V], acc);
      }
    }
  }
  part[slice * kRadTile + lane] = acc;
  __syncthreads();
  if (slice == 0 && e < a.wtotal) {
    const float* p = part + lane;
    const float s01 = __fadd_rn(p[0], p[kRadTile]), s23 = __fadd_rn(p[2 * kRadTile], p[3 * kRadTile]);
    const float s45 = __fadd_rn(p[4 * kRadTile], p[5 * kRadTile]), s67 = __fadd_rn(p[6 * kRadTile], p[7 * kRadTile]);
    a.dw[e] = __fadd_rn(__fadd_rn(s01, s23), __fadd_rn(s45, s67));
  }
}

}  // namespace

// flat -> grid.  ENC: enc (W_i given as (R, rin), the alpha-1 layers divided by A); otherwise dec_vjp's dg (D_i given as (rin, R),
// which is the k-major layout already) and, in the workgroups past row_blocks, dD.
template <bool ENC>
__global__ void __launch_bounds__(kRadThreads) radial_expand_kernel(RadialArgs a) {
  extern __shared__ __attribute__((aligned(16))) char rad_smem[];
  int4* lay_s = (int4*)rad_smem;
  float* wt = rad_weights(rad_smem, a.L);  // [woff_i + j R + r]
  rad_stage_layers(a, lay_s);
  __syncthreads();
  if ((int)blockIdx.x >= a.row_blocks) {  // uniform over the workgroup
    if (!ENC) rad_weight_grad<false>(a, lay_s, wt, (int)blockIdx.x - a.row_blocks);
    return;
  }
  float* row = rad_row(rad_smem, a.L, a.wtotal);
  rad_stage_weights<ENC, true>(a, lay_s, wt);
  const int AR = a.A * a.R, LAR = a.L * AR;
  for (int b = blockIdx.x; b < a.batch; b += a.row_blocks) {
    const float* in = a.in + (size_t)b * a.V;
    for (int v = threadIdx.x; v < a.V; v += kRadThreads) row[v] = in[v];
    __syncthreads();  // (the first pass: the matrices too)
    float* out = a.out + (size_t)b * LAR;
    for (int o = threadIdx.x; o < LAR; o += kRadThreads) {
      const int i = o / AR, rem = o - i * AR, aa = rem / a.R, r = rem - aa * a.R;
      const int4 ly = lay_s[i];
      const bool one = ly.y != a.A;
      const float* xr = row + ly.x + (one ? 0 : aa * ly.z);
      const float* wk = wt + ly.w + r;
      float acc = 0.f;
      for (int j = 0; j < ly.z; ++j) acc = fmaf(wk[j * a.R], xr[j], acc);
      if (ENC && one) acc = __fdiv_rn(acc, (float)a.A);
      out[o] = acc;
    }
    __syncthreads();  // the row is consumed before the next one is staged
  }
}

// grid -> flat.  DEC: dec (D_i given as (rin, R)); otherwise enc_vjp's dx (W_i given as (R, rin), the k-major layout already,
// the alpha-1 layers divided by A) and, in the workgroups past row_blocks, dW.
template <bool DEC>
__global__ void __launch_bounds__(kRadThreads) radial_collapse_kernel(RadialArgs a) {
  extern __shared__ __attribute__((aligned(16))) char rad_smem[];
  int4* lay_s = (int4*)rad_smem;
  float* wt = rad_weights(rad_smem, a.L);  // [woff_i + r rin + j]
  rad_stage_layers(a, lay_s);
  __syncthreads();
  if ((int)blockIdx.x >= a.row_blocks) {
    if (!DEC) rad_weight_grad<true>(a, lay_s, wt, (int)blockIdx.x - a.row_blocks);
    return;
  }
  float* row = rad_row(rad_smem, a.L, a.wtotal);
  rad_stage_weights<DEC, false>(a, lay_s, wt);
  const int AR = a.A * a.R, LAR = a.L * AR;
  for (int b = blockIdx.x; b < a.batch; b += a.row_blocks) {
    const float* in = a.in + (size_t)b * LAR;
    for (int o = threadIdx.x; o < LAR; o += kRadThreads) row[o] = in[o];
    __syncthreads();
    float* out = a.out + (size_t)b * a.V;
    for (int v = threadIdx.x; v < a.V; v += kRadThreads) {
      const int i = a.vlay[v];
      const int4 ly = lay_s[i];
      const bool one = ly.y != a.A;
      const int rem = v - ly.x, aa = one ? 0 : rem / ly.z, j = rem - aa * ly.z;
      const float* mk = wt + ly.w + j;
      const float* g = row + i * AR + aa * a.R;
      float res = 0.f;
      for (int s = 0; s < (one ? a.A : 1); ++s, g += a.R) {  // alpha 1: the sum over a, ascending
        float acc = 0.f;
        for (int r = 0; r < a.R; ++r) acc = fmaf(mk[r * ly.z], g[r], acc);
        res = one ? __fadd_rn(res, acc) : acc;
      }
      if (!DEC && one) res = __fdiv_rn(res, (float)a.A);
      out[v] = res;
    }
    __syncthreads();
  }
}

namespace {

enum RadialOp { kEnc, kDec, kEncVjp, kDecVjp };

void radial_launch(RadialOp op, const CdRadialMap* m, const float* w, const float* in, float* out, const float* other, float* dw,
                   int batch, hipStream_t s) {
  RadialArgs a{};
  a.lay = m->lay; a.vlay = m->vlay; a.w = w; a.in = in; a.out = out; a.other = other; a.dw = dw;
  a.L = m->layers; a.A = m->A; a.R = m->R; a.V = m->V; a.wtotal = m->wtotal; a.batch = batch;
  a.row_blocks = batch < kRadMaxRowBlocks ? batch : kRadMaxRowBlocks;
  const int LAR = m->layers * m->A * m->R;
  const size_t table = sizeof(int4) * (size_t)m->layers;
  size_t smem = table + sizeof(float) * (size_t)(((m->wtotal + 3) & ~3) + (m->V > LAR ? m->V : LAR));
  const size_t wg = table + sizeof(float) * kRadThreads;
  if (dw && smem < wg) smem = wg;
  const dim3 grid((unsigned)(a.row_blocks + (dw ? (m->wtotal + kRadTile - 1) / kRadTile : 0)));
  switch (op) {
    case kEnc: hipLaunchKernelGGL(radial_expand_kernel<true>, grid, dim3(kRadThreads), smem, s, a); break;
    case kDec: hipLaunchKernelGGL(radial_collapse_kernel<true>, grid, dim3(kRadThreads), smem, s, a); break;
    case kEncVjp: hipLaunchKernelGGL(radial_collapse_kernel<false>, grid, dim3(kRadThreads), smem, s, a); break;
    case kDecVjp: hipLaunchKernelGGL(radial_expand_kernel<false>, grid, dim3(kRadThreads), smem, s, a); break;
  }
  CD_HIP(hipGetLastError());
}

}  // namespace
}  // namespace cd

extern "C" {

int cd_radial_create(int layers, const int32_t* bound, const int32_t* alpha, const int32_t* rin, int alpha_out, int r_out,
                     CdRadialMap** out, void* stream) {
  return guarded([&] {
    CD_REQUIRE(bound && alpha && rin && out, "cd_radial_create: bound, alpha, rin and out must not be null");
    CD_REQUIRE(layers > 0 && alpha_out > 0 && r_out > 0, "cd_radial_create: layers, alpha_out and r_out must be positive");
    CD_REQUIRE(layers <= kRadMaxLayers, "cd_radial_create: at most 64 layers");
    CD_REQUIRE(bound[0] == 0, "cd_radial_create: bound[0] must be 0");
    std::vector<int4> lay((size_t)layers);
    int64_t wtotal = 0;
    for (int i = 0; i < layers; ++i)
      CD_REQUIRE(bound[i + 1] > bound[i], "cd_radial_create: bound must be strictly increasing (layer " + std::to_string(i) + ")");
    for (int i = 0; i < layers; ++i) {
      const std::string at = " (layer " + std::to_string(i) + ")";
      CD_REQUIRE(alpha[i] == 1 || alpha[i] == alpha_out,
                 "cd_radial_create: alpha must be 1 or alpha_out = " + std::to_string(alpha_out) + ", got " +
                     std::to_string(alpha[i]) + at);
      CD_REQUIRE(rin[i] > 0, "cd_radial_create: rin must be positive" + at);
      CD_REQUIRE((int64_t)bound[i + 1] - bound[i] == (int64_t)alpha[i] * rin[i],
                 "cd_radial_create: the span bound[i+1] - bound[i] must equal alpha[i] * rin[i]" + at);
      CD_REQUIRE(wtotal <= kRadMaxWeights, "cd_radial_create: the matrices of one direction exceed 8192 floats (32 KB of LDS)");
      lay[(size_t)i] = make_int4(bound[i], alpha[i], rin[i], (int)wtotal);
      wtotal += (int64_t)rin[i] * r_out;
    }
    CD_REQUIRE(wtotal <= kRadMaxWeights, "cd_radial_create: the matrices of one direction exceed 8192 floats (32 KB of LDS)");
    const int V = bound[layers];
    CD_REQUIRE(V <= kRadMaxRow && (int64_t)layers * alpha_out * r_out <= kRadMaxRow,
               "cd_radial_create: a shower exceeds 6144 floats (24 KB of LDS), flat or as layers * alpha_out * r_out");
    std::vector<int> vlay((size_t)V);
    for (int i = 0; i < layers; ++i)
      for (int v = bound[i]; v < bound[i + 1]; ++v) vlay[(size_t)v] = i;
    hipStream_t s = (hipStream_t)stream;
    struct Owner {
      CdRadialMap* m;
      ~Owner() { delete m; }
    } own{new CdRadialMap};
    CdRadialMap* m = own.m;
    m->layers = layers; m->A = alpha_out; m->R = r_out; m->V = V; m->wtotal = (int)wtotal;
    CD_HIP(hipMalloc(&m->lay, sizeof(int4) * lay.size()));
    CD_HIP(hipMalloc(&m->vlay, sizeof(int) * vlay.size()));
    CD_HIP(hipMemcpyAsync(m->lay, lay.data(), sizeof(int4) * lay.size(), hipMemcpyHostToDevice, s));
    CD_HIP(hipMemcpyAsync(m->vlay, vlay.data(), sizeof(int) * vlay.size(), hipMemcpyHostToDevice, s));
    CD_HIP(hipStreamSynchronize(s));  // the host arrays above go out of scope
    *out = m;
    own.m = nullptr;
  });
}

int cd_radial_destroy(CdRadialMap* map) {
  return guarded([&] { delete map; });
}

int cd_radial_enc(const CdRadialMap* map, const float* w, const float* x, float* y, int batch, void* stream) {
  return guarded([&] {
    CD_REQUIRE(map && w && x && y, "cd_radial_enc: map, w, x and y must not be null");
    CD_REQUIRE(batch > 0, "cd_radial_enc: batch must be positive");
    radial_launch(kEnc, map, w, x, y, nullptr, nullptr, batch, (hipStream_t)stream);
  });
}

int cd_radial_dec(const CdRadialMap* map, const float* d, const float* g, float* x, int batch, void* stream) {
  return guarded([&] {
    CD_REQUIRE(map && d && g && x, "cd_radial_dec: map, d, g and x must not be null");
    CD_REQUIRE(batch > 0, "cd_radial_dec: batch must be positive");
    radial_launch(kDec, map, d, g, x, nullptr, nullptr, batch, (hipStream_t)stream);
  });
}

int cd_radial_enc_vjp(const CdRadialMap* map, const float* w, const float* x, const float* gy, float* dx, float* dw, int batch,
                      void* stream) {
  return guarded([&] {
    CD_REQUIRE(map && w && x && gy && dx, "cd_radial_enc_vjp: map, w, x, gy and dx must not be null");
    CD_REQUIRE(batch > 0, "cd_radial_enc_vjp: batch must be positive");
    radial_launch(kEncVjp, map, w, gy, dx, x, dw, batch, (hipStream_t)stream);
  });
}

int cd_radial_dec_vjp(const CdRadialMap* map, const float* d, const float* g, const float* gx, float* dg, float* dd, int batch,
                      void* stream) {
  return guarded([&] {
    CD_REQUIRE(map && d && g && gx && dg, "cd_radial_dec_vjp: map, d, g, gx and dg must not be null");
    CD_REQUIRE(batch > 0, "cd_radial_dec_vjp: batch must be positive");
    radial_launch(kDecVjp, map, d, gx, dg, g, dd, batch, (hipStream_t)stream);
  });
}

}  // extern "C"
