// Elementwise pieces of the linear attention's backward: the channel softmax of q and its backward, the backward of k's voxel
// softmax, and the per-sample 32x32 weight images of the context (plain / transposed).  The contractions themselves run on the
// pointwise conv and the per-sample 1x1 weight gradient (train.hip: attn_block_bwd).  Forward: kernels_attn_unfused.hip; reference
// LinearAttention.forward, models.py:301-318.
#include "kernels_bwd.h"

namespace cd {

// qs[n][d] = softmax over the 32 channels of q (q = channels [0,32) of the (B, n, 96) qkv tensor); one thread per voxel
// Eight lanes per row (a quad of the 32 channels each: a wave's load is 8 rows x 128 contiguous bytes), the row's max / sum by
// three xor shuffles, four rows per lane in flight.  (Round 4: one THREAD per row read its 128 bytes as eight 16-byte loads
// 384 bytes apart from its neighbours' -- every instruction touched 64 cache lines: 2.7 TB/s at level 0.)
__global__ void __launch_bounds__(256) softmax32_kernel(const float* __restrict__ qkv, float* __restrict__ qs, int64_t rows) {
  const int q = threadIdx.x & 7;
  const int64_t r0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 3;       // 32 rows per block and trip
  const int64_t stride = (int64_t)gridDim.x * 32;
  for (int64_t r = r0; r < rows; r += 4 * stride) {
    f32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t ru = r + u * stride;
      v[u] = *(const f32x4*)(qkv + (size_t)(ru < rows ? ru : rows - 1) * 96 + q * 4);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float m = fmaxf(fmaxf(v[u][0], v[u][1]), fmaxf(v[u][2], v[u][3]));
#pragma unroll
      for (int o = 1; o < 8; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
      float ssum = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[u][e] = expf(v[u][e] - m);
        ssum += v[u][e];
      }
#pragma unroll
      for (int o = 1; o < 8; o <<= 1) ssum += __shfl_xor(ssum, o, 64);
      const int64_t ru = r + u * stride;
      if (ru < rows) *(f32x4*)(qs + (size_t)ru * 32 + q * 4) = v[u] * (1.f / ssum);
    }
  }
}
void launch_softmax32(const float* qkv, float* qs, int64_t rows, hipStream_t s) {
  int64_t blocks = (rows + 127) / 128;  // four rows per lane
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(softmax32_kernel, dim3((unsigned)blocks), dim3(256), 0, s, qkv, qs, rows);
  CD_HIP(hipGetLastError());
}

// dq[n][d] = qs*(dqs - sum_d' qs*dqs)  written into channels [0,32) of dqkv (row stride 96); same lane layout
__global__ void __launch_bounds__(256) softmax32_bwd_kernel(const float* __restrict__ qs, const float* __restrict__ dqs,
                                                            float* __restrict__ dqkv, int64_t rows) {
  const int q = threadIdx.x & 7;
  const int64_t r0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 3;
  const int64_t stride = (int64_t)gridDim.x * 32;
  for (int64_t r = r0; r < rows; r += 4 * stride) {
    f32x4 av[4], gv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t ru = r + u * stride;
      const size_t o = (size_t)(ru < rows ? ru : rows - 1) * 32 + q * 4;
      av[u] = *(const f32x4*)(qs + o);
      gv[u] = *(const f32x4*)(dqs + o);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float dot = (av[u][0] * gv[u][0] + av[u][1] * gv[u][1]) + (av[u][2] * gv[u][2] + av[u][3] * gv[u][3]);
#pragma unroll
      for (int o = 1; o < 8; o <<= 1) dot += __shfl_xor(dot, o, 64);
      const int64_t ru = r + u * stride;
      if (ru < rows) *(f32x4*)(dqkv + (size_t)ru * 96 + q * 4) = av[u] * (gv[u] - dot);
    }
  }
}
void launch_softmax32_bwd(const float* qs, const float* dqs, float* dqkv, int64_t rows, hipStream_t s) {
  int64_t blocks = (rows + 127) / 128;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(softmax32_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, s, qs, dqs, dqkv, rows);
  CD_HIP(hipGetLastError());
}

// dk[n][d] = ks*(dks - r[d]),  ks = exp(k - M[d])/S[d],  r[d] = dscale * sum_e dctx[d][e]*ctx[d][e];  written to dqkv channels [32,64)
// kstat[b][d] = {M, 1/S};  ctx, dctx: [b][32][32] (row d, col e), both WITHOUT the q scale.
__global__ void __launch_bounds__(256) ksoftmax_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ dks,
                                                           const float* __restrict__ kstat, const float* __restrict__ ctx,
                                                           const float* __restrict__ dctx, float dscale, float* __restrict__ dqkv,
                                                           int64_t vox) {
  __shared__ float sR[32], sM[32], sI[32];
  const int b = blockIdx.y, tid = threadIdx.x;
  if (tid < 32) {
    float r = 0.f;
    for (int e = 0; e < 32; ++e) r += dctx[((size_t)b * 32 + tid) * 32 + e] * ctx[((size_t)b * 32 + tid) * 32 + e];
    sR[tid] = r * dscale;
    sM[tid] = kstat[((size_t)b * 32 + tid) * 2];
    sI[tid] = kstat[((size_t)b * 32 + tid) * 2 + 1];
  }
  __syncthreads();
  const int64_t total = vox * 8;  // float4 items
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t n = i >> 3;
    const int c = (int)(i & 7) * 4;
    const f32x4 kv = *(const f32x4*)(qkv + ((size_t)b * vox + n) * 96 + 32 + c);
    const f32x4 g = *(const f32x4*)(dks + ((size_t)b * vox + n) * 32 + c);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = expf(kv[e] - sM[c + e]) * sI[c + e] * (g[e] - sR[c + e]);
    *(f32x4*)(dqkv + ((size_t)b * vox + n) * 96 + 32 + c) = o;
  }
}
void launch_ksoftmax_bwd(const float* qkv, const float* dks, const float* kstat, const float* ctx, const float* dctx, float dscale,
                         float* dqkv, int batch, int64_t vox, hipStream_t s) {
  int64_t bx = (vox * 8 + 255) / 256;
  if (bx > 256) bx = 256;
  hipLaunchKernelGGL(ksoftmax_bwd_kernel, dim3((unsigned)bx, batch), dim3(256), 0, s, qkv, dks, kstat, ctx, dctx, dscale, dqkv, vox);
  CD_HIP(hipGetLastError());
}

// per-sample 32x32 matrix -> packed 1x1 MFMA weights:  W[co][ci] = scale * (transpose ? m[co][ci] : m[ci][co])
__global__ void pack_sample32_kernel(const float* __restrict__ m, float* __restrict__ wpk, int transpose, float scale) {
  const int b = blockIdx.x;
  for (int i = threadIdx.x; i < 1024; i += blockDim.x) {
    const int e4 = i & 3, lane = (i >> 2) & 63, q = (i >> 8) & 3;
    const int co = lane & 31, ci = (lane >> 5) * 16 + q * 4 + e4;
    wpk[(size_t)b * 1024 + i] = scale * (transpose ? m[((size_t)b * 32 + co) * 32 + ci] : m[((size_t)b * 32 + ci) * 32 + co]);
  }
}
void launch_pack_sample32(const float* m, float* wpk, int batch, bool transpose, float scale, hipStream_t s) {
  hipLaunchKernelGGL(pack_sample32_kernel, dim3(batch), dim3(256), 0, s, m, wpk, transpose ? 1 : 0, scale);
  CD_HIP(hipGetLastError());
}
// both images of the same matrices in one launch: wpk_plain (transpose = false) and wpk_tr (transpose = true)
__global__ void pack_sample32_pair_kernel(const float* __restrict__ m, float* __restrict__ wpk_plain, float* __restrict__ wpk_tr,
                                          float scale) {
  const int b = blockIdx.x, tr = blockIdx.y;
  float* wpk = tr ? wpk_tr : wpk_plain;
  for (int i = threadIdx.x; i < 1024; i += blockDim.x) {
    const int e4 = i & 3, lane = (i >> 2) & 63, q = (i >> 8) & 3;
    const int co = lane & 31, ci = (lane >> 5) * 16 + q * 4 + e4;
    wpk[(size_t)b * 1024 + i] = scale * (tr ? m[((size_t)b * 32 + co) * 32 + ci] : m[((size_t)b * 32 + ci) * 32 + co]);
  }
}
void launch_pack_sample32_pair(const float* m, float* wpk_plain, float* wpk_tr, int batch, float scale, hipStream_t s) {
  hipLaunchKernelGGL(pack_sample32_pair_kernel, dim3(batch, 2), dim3(256), 0, s, m, wpk_plain, wpk_tr, scale);
  CD_HIP(hipGetLastError());
}

}  // namespace cd
