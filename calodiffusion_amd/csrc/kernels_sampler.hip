// What the sampler loops launch around the network (sampler.hip): step scalars, Philox noise and the step-program ops.
#include "kernels_sampler.h"
#include "philox.h"

namespace cd {

// ------------------------------------------------------------------------------------------------------------
// Sampler loop helpers (DDim.__call__, models/sample.py:72-107).  Per-step scalars live in device memory so that one
// captured step graph can be replayed for every iteration.
//   stepvals = {sigma, sigma_prev*[t>0], ddim_sigma, denom}
// ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) load_step_kernel(const float* __restrict__ table, int* counter, float* stepvals, float* sigma_b,
                                                         int batch, StepChunk ch) {
  const int step = *counter;
  const float* row = table + (size_t)step * 4;
  const int tid = threadIdx.x;
  if (tid < 4) stepvals[tid] = row[tid];
  const float sg = row[0];
  for (int i = tid; i < batch; i += blockDim.x) sigma_b[i] = sg;
  if (ch.chunk_steps) {  // this step's embeddings and scalings out of the chunk computed ahead (one workgroup: ~150 KB from L2)
    const int slot = step % ch.chunk_steps;
    const f32x4* es = (const f32x4*)(ch.emb_src + (size_t)slot * ch.emb_floats);
    f32x4* ed = (f32x4*)ch.emb_dst;
    const f32x4* ss = (const f32x4*)(ch.scal_src + (size_t)slot * ch.scal_floats);
    f32x4* sd = (f32x4*)ch.scal_dst;
    if (ch.emb_cond) {  // separable form: the step's time row + every sample's condition row
      const int rq = ch.emb_floats / 4;
      const f32x4* ec = (const f32x4*)ch.emb_cond;
      for (int i = tid; i < batch * rq; i += blockDim.x) ed[i] = es[i % rq] + ec[i];
      for (int i = tid; i < batch; i += blockDim.x) sd[i] = ss[0];
    } else {
      for (int i = tid; i < ch.emb_floats / 4; i += blockDim.x) ed[i] = es[i];
      for (int i = tid; i < ch.scal_floats / 4; i += blockDim.x) sd[i] = ss[i];
    }
  }
  __syncthreads();
  if (tid == 0) *counter = step + 1;
}
void launch_load_step(const float* table, int* counter, float* stepvals, float* sigma_b, int batch, hipStream_t s,
                      const StepChunk* chunk) {
  StepChunk ch;
  if (chunk) {
    ch = *chunk;
    CD_REQUIRE(ch.emb_floats % 4 == 0 && ch.scal_floats % 4 == 0, "internal: step chunk rows must be whole float4s");
  }
  hipLaunchKernelGGL(load_step_kernel, dim3(1), dim3(chunk ? 1024 : 256), 0, s, table, counter, stepvals, sigma_b, batch, ch);
  CD_HIP(hipGetLastError());
}

// y = x * (*scale)   (x = start * sigma_start, sample.py:66)
__global__ void scale_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ sc, int64_t n) {
  const float f = sc[0];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] = x[i] * f;
}
void launch_scale(const float* x, float* y, const float* sc, int64_t n, hipStream_t s) {
  int64_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(scale_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, y, sc, n);
  CD_HIP(hipGetLastError());
}

__global__ void scale_imm_kernel(const float* __restrict__ x, float* __restrict__ y, float f, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] = x[i] * f;
}
void launch_scale_imm(const float* x, float* y, float scale, int64_t n, hipStream_t s) {
  int64_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(scale_imm_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, y, scale, n);
  CD_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------------------
// Unit normals of the device Philox stream (philox.h).
// ------------------------------------------------------------------------------------------------------------
// dev (optional): {seed, base offset, stride} in device memory and the sampler's step counter -- the stream position then is
// base + ((step - 1) * per_step + index) * stride, so that one captured step graph serves every step and every trajectory of a
// stochastic sampler
__global__ void __launch_bounds__(256) randn_kernel(float* __restrict__ out, int64_t n, uint64_t seed, uint64_t offset,
                                                    const uint64_t* __restrict__ dev, const int* __restrict__ step_counter,
                                                    int per_step, int index) {
  if (dev) {
    seed = dev[0];
    offset = dev[1] + ((uint64_t)(*step_counter - 1) * (uint64_t)per_step + (uint64_t)index) * dev[2];
  }
  const uint64_t first = offset >> 2, last = (offset + (uint64_t)n + 3) >> 2;  // counter range [first, last)
  for (uint64_t ctr = first + (uint64_t)blockIdx.x * 256 + threadIdx.x; ctr < last; ctr += (uint64_t)gridDim.x * 256) {
    float z[4];
    philox_normals4(ctr, seed, z);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint64_t g = ctr * 4 + e;
      if (g >= offset && g < offset + (uint64_t)n) out[g - offset] = z[e];
    }
  }
}
void launch_randn(float* out, int64_t n, uint64_t seed, uint64_t offset, hipStream_t s) {
  if (n <= 0) return;
  prof::Scope scope("randn", s, 0, 4.0 * n);  // (a one-workgroup draw doubles as the profiler's own per-launch overhead: bench.py)
  int64_t blocks = (n / 4 + 256) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(randn_kernel, dim3((unsigned)blocks), dim3(256), 0, s, out, n, seed, offset, (const uint64_t*)nullptr,
                     (const int*)nullptr, 1, 0);
  CD_HIP(hipGetLastError());
}
void launch_randn_step(float* out, int64_t n, const uint64_t* seed_offset_stride_dev, const int* step_counter, hipStream_t s,
                       int per_step, int index) {
  if (n <= 0) return;
  int64_t blocks = (n / 4 + 256) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(randn_kernel, dim3((unsigned)blocks), dim3(256), 0, s, out, n, (uint64_t)0, (uint64_t)0,
                     seed_offset_stride_dev, step_counter, per_step, index);
  CD_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------------------
// Generic sampler programs (cd_sampler_run): every per-step scalar is a column of row (*counter - 1) of a device table, so a
// step whose op list does not change is one captured graph replayed for the whole trajectory.
// ------------------------------------------------------------------------------------------------------------
__global__ void or_word_kernel(int* word, int bits) { atomicOr(word, bits); }
void launch_or_word(int* word, int bits, hipStream_t s) {
  hipLaunchKernelGGL(or_word_kernel, dim3(1), dim3(1), 0, s, word, bits);
  CD_HIP(hipGetLastError());
}
__global__ void step_advance_kernel(int* counter) { *counter = *counter + 1; }
void launch_step_advance(int* counter, hipStream_t s) {
  hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, s, counter);
  CD_HIP(hipGetLastError());
}
__global__ void fill_from_table_kernel(float* __restrict__ dst, int count, const float* __restrict__ table, int ncol, int col,
                                       const int* __restrict__ counter) {
  const float v = table[(size_t)(*counter - 1) * ncol + col];
  for (int i = threadIdx.x; i < count; i += blockDim.x) dst[i] = v;
}
void launch_fill_from_table(float* dst, int count, const float* table, int ncol, int col, const int* step_counter, hipStream_t s) {
  hipLaunchKernelGGL(fill_from_table_kernel, dim3(1), dim3(256), 0, s, dst, count, table, ncol, col, step_counter);
  CD_HIP(hipGetLastError());
}
// CD_SOP_DENOISE_PS: dst[b] = table[row][col + b], a sigma per sample
__global__ void fill_row_from_table_kernel(float* __restrict__ dst, int count, const float* __restrict__ table, int ncol, int col,
                                           const int* __restrict__ counter) {
  const float* row = table + (size_t)(*counter - 1) * ncol + col;
  for (int i = threadIdx.x; i < count; i += blockDim.x) dst[i] = row[i];
}
void launch_fill_row_from_table(float* dst, int count, const float* table, int ncol, int col, const int* step_counter,
                                hipStream_t s) {
  hipLaunchKernelGGL(fill_row_from_table_kernel, dim3(1), dim3(256), 0, s, dst, count, table, ncol, col, step_counter);
  CD_HIP(hipGetLastError());
}
struct LincombSrc { const float* p[6]; };
__global__ void __launch_bounds__(256) lincomb_kernel(float* out, LincombSrc src, int nsrc, const float* __restrict__ table,
                                                      int ncol, int col, const int* __restrict__ counter, int64_t n) {
  float c[6];
  const float* row = table + (size_t)(*counter - 1) * ncol + col;
#pragma unroll
  for (int k = 0; k < 6; ++k) c[k] = k < nsrc ? row[k] : 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float acc = c[0] * src.p[0][i];
#pragma unroll
    for (int k = 1; k < 6; ++k)
      if (k < nsrc) acc += c[k] * src.p[k][i];
    out[i] = acc;
  }
}
// The same in the operation order of a chain of torch elementwise kernels (CD_SOP_LINDIV): every product and every sum is
// rounded to fp32 on its own (no contraction into fused multiply-adds), the terms are added left to right and the result is
// divided (IEEE, correctly rounded) by the coefficient that follows the terms.  DPM-Solver's second- and third-order steps
// amplify the rounding of their intermediate states by sigma_max / sigma_mid (utils/sampling.py:419-456), so matching the
// reference there means rounding where it rounds.
__global__ void __launch_bounds__(256) lincomb_div_kernel(float* out, LincombSrc src, int nsrc, const float* __restrict__ table,
                                                          int ncol, int col, const int* __restrict__ counter, int64_t n) {
#pragma clang fp contract(off)
  float c[6];
  const float* row = table + (size_t)(*counter - 1) * ncol + col;
#pragma unroll
  for (int k = 0; k < 6; ++k) c[k] = k < nsrc ? row[k] : 0.f;
  const float div = row[nsrc];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    // (plain operators: the pragma above governs them, while the __f*_rn helpers of the HIP headers carry the contraction
    // flags of the translation unit and come out as v_fmac)
    float acc = c[0] * src.p[0][i];
#pragma unroll
    for (int k = 1; k < 6; ++k)
      if (k < nsrc) {
        const float prod = c[k] * src.p[k][i];
        acc = acc + prod;
      }
    out[i] = acc / div;
  }
}
void launch_lincomb(float* out, const float* const* src, int nsrc, const float* table, int ncol, int col, const int* step_counter,
                    int64_t n, bool div, hipStream_t s) {
  CD_REQUIRE(nsrc >= 1 && nsrc <= 6, "lincomb: 1..6 terms");
  LincombSrc ls{};
  for (int k = 0; k < 6; ++k) ls.p[k] = src[k < nsrc ? k : 0];
  int64_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(div ? lincomb_div_kernel : lincomb_kernel, dim3((unsigned)blocks), dim3(256), 0, s, out, ls, nsrc, table, ncol,
                     col, step_counter, n);
  CD_HIP(hipGetLastError());
}
__global__ void __launch_bounds__(256) record_step_kernel(float* __restrict__ traj, const float* __restrict__ src,
                                                          const int* __restrict__ counter, int64_t n) {
  float* dst = traj + (size_t)(*counter - 1) * n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] = src[i];
}
void launch_record_step(float* traj, const float* src, const int* step_counter, int64_t n, hipStream_t s) {
  int64_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(record_step_kernel, dim3((unsigned)blocks), dim3(256), 0, s, traj, src, step_counter, n);
  CD_HIP(hipGetLastError());
}

}  // namespace cd
