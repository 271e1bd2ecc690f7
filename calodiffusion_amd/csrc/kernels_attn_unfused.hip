// Unfused linear-attention kernels (HBM-bound passes) for channels-last fp32 activations on gfx950: the form on the f32-input
// MFMA that the full-range precisions and the training tape take.  The fused forms of the sampling path: kernels_attn.hip.
// Reference semantics: LinearAttention.forward (calodiffusion/models/models.py:301-318).
#include "kernels_attn.h"
#include "conv_internal.h"

namespace cd {

// ------------------------------------------------------------------------------------------------------------
// Linear attention (heads = 1, dim_head = 32).  qkv is channels-last (B, n, 96): q = [0,32), k = [32,64), v = [64,96).
//   k <- softmax over the n voxels (per channel d);  context[d][e] = sum_n k[d,n] v[e,n]      (models.py:309,312)
//   q <- softmax over the 32 channels (per voxel) * 32^-1/2;  out[e,n] = sum_d context[d][e] q[d,n]   (:308,311,314)
// Pass 1 (this kernel): per (sample, voxel range) a local max m[d], local sum s[d] = sum exp(k - m) and the
// un-normalised context partial ctx[d][e] = sum exp(k[n][d] - m[d]) v[n][e] on the matrix cores (K = voxels).
// Pass 2 (attn_combine_kernel): merge the partials log-sum-exp style and fold the result into the to_out 1x1 conv:
//   W'[c][d] = scale * sum_e W_out[c][e] context[d][e], written in packed MFMA layout as per-sample weights.
// Pass 3 is the pointwise kernel with the softmax-32 A prologue and per-sample weights.
// ------------------------------------------------------------------------------------------------------------
int attn_nsplit_for(int64_t vox, int batch) {
  int64_t want = (1024 + batch - 1) / batch;
  int64_t cap = (vox + 511) / 512;  // >= 128 voxels per wave
  int64_t n = want < cap ? want : cap;
  if (n < 1) n = 1;
  if (n > 128) n = 128;
  return (int)n;
}
size_t attn_partial_floats(int batch, int nsplit) { return (size_t)batch * nsplit * (64 + 1024); }

__global__ void __launch_bounds__(256) attn_context_kernel(const float* __restrict__ qkv, float* __restrict__ partials,
                                                           int64_t vox, int nsplit) {
  __shared__ float sMax[4][32];
  __shared__ float sSum[8][32];
  __shared__ float sCtx[4][1024];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, col = lane & 31;
  const int split = blockIdx.x, b = blockIdx.y;
  const int64_t per = (((vox + nsplit - 1) / nsplit) + 1) & ~(int64_t)1;  // even
  const int64_t v0 = split * per;
  const int64_t v1 = (v0 + per < vox) ? v0 + per : vox;
  const float* base = qkv + (size_t)b * vox * 96;

  // local max of k over this block's voxels, per channel.  Both sweeps below fetch eight voxels per trip (round 4: one voxel per
  // trip was a memory round trip per 256 bytes and wave -- 40 us at Dataset-2's level 0 for 53 MB, with the training step's seven
  // attention blocks 0.17 ms of pure latency); indices past the block are clamped and their values masked.
  float m = -3.0e38f;
  for (int64_t n = v0 + 2 * wave + half; n < v1; n += 64) {
    float kv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int64_t nu = n + 8 * u;
      kv[u] = base[(size_t)(nu < v1 ? nu : v1 - 1) * 96 + 32 + col];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) m = fmaxf(m, kv[u]);  // (a clamped index repeats a voxel of the block: harmless under max)
  }
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  if (half == 0) sMax[wave][col] = m;
  __syncthreads();
  m = fmaxf(fmaxf(sMax[0][col], sMax[1][col]), fmaxf(sMax[2][col], sMax[3][col]));

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float ssum = 0.f;
  // A[i = d][k = voxel half] = exp(k[n][d] - m[d]),  B[k][j = e] = v[n][e]
  // (the loop bound is wave-uniform: per is even and a wave's two halves take voxels n, n + 1 of a pair, both below v0 + per or
  // both not -- every lane of a wave runs the same MFMAs, in the same order as the one-voxel-per-trip form: bit-identical sums)
  for (int64_t n = v0 + 2 * wave + half; n < v0 + per; n += 64) {
    float kk[8], vv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int64_t nu = n + 8 * u;
      const size_t o = (size_t)(nu < v1 ? nu : v1 - 1) * 96;
      kk[u] = base[o + 32 + col];
      vv[u] = base[o + 64 + col];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int64_t nu = n + 8 * u;
      if (nu - half < v0 + per) {  // (wave-uniform: the pair's first voxel)
        const bool in = nu < v1;
        const float av = in ? expf(kk[u] - m) : 0.f;
        const float bv = in ? vv[u] : 0.f;
        ssum += av;
        acc = MFMA32(av, bv, acc);
      }
    }
  }
  sSum[wave * 2 + half][col] = ssum;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int d = (r & 3) + 8 * (r >> 2) + 4 * half;  // row = A index = channel d; column = e
    sCtx[wave][d * 32 + col] = acc[r];
  }
  __syncthreads();
  float* out = partials + ((size_t)b * nsplit + split) * (64 + 1024);
  if (tid < 32) {
    out[tid] = m;
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) t += sSum[i][tid];
    out[32 + tid] = t;
  }
  for (int i = tid; i < 1024; i += 256) out[64 + i] = (sCtx[0][i] + sCtx[1][i]) + (sCtx[2][i] + sCtx[3][i]);
}

void launch_attn_context(const float* qkv, float* partials, int batch, int64_t vox, int nsplit, hipStream_t s) {
  prof::Scope scope("attn_context", s, 2.0 * 32 * 32 * (double)vox * batch, 4.0 * batch * (double)vox * 96);
  hipLaunchKernelGGL(attn_context_kernel, dim3(nsplit, batch), dim3(256), 0, s, qkv, partials, vox, nsplit);
  CD_HIP(hipGetLastError());
}

__global__ void __launch_bounds__(256) attn_combine_kernel(const float* __restrict__ partials, int nsplit,
                                                           const float* __restrict__ w_out, int cout,
                                                           float* __restrict__ wpk_b, float scale, float* __restrict__ ctx_out,
                                                           float* __restrict__ kstat_out, int layout_T) {
  __shared__ float sM[32], sInv[32];
  __shared__ float sCtx[1024];
  const int tid = threadIdx.x, b = blockIdx.x;
  const float* p = partials + (size_t)b * nsplit * (64 + 1024);
  if (tid < 32) {
    float M = -3.0e38f;
    for (int i = 0; i < nsplit; ++i) M = fmaxf(M, p[(size_t)i * 1088 + tid]);
    float S = 0.f;
    for (int i = 0; i < nsplit; ++i) S += p[(size_t)i * 1088 + 32 + tid] * expf(p[(size_t)i * 1088 + tid] - M);
    sM[tid] = M;
    sInv[tid] = scale / S;
    if (kstat_out) {
      kstat_out[((size_t)b * 32 + tid) * 2] = M;
      kstat_out[((size_t)b * 32 + tid) * 2 + 1] = 1.f / S;
    }
  }
  __syncthreads();
  // rescaling factors of the partials, once per (partial, channel) instead of once per context entry (32 x fewer exponentials and
  // loads of the maxima in the loop below; same expression, same summation order: bit-identical)
  __shared__ float sF[128 * 32];  // nsplit <= 128 (attn_nsplit_for)
  for (int i = tid; i < nsplit * 32; i += 256) sF[i] = expf(p[(size_t)(i >> 5) * 1088 + (i & 31)] - sM[i & 31]);
  __syncthreads();
  for (int i = tid; i < 1024; i += 256) {
    const int d = i >> 5;
    float c = 0.f;
    int k = 0;
    for (; k + 4 <= nsplit; k += 4) {  // four partials' loads in flight
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = p[(size_t)(k + u) * 1088 + 64 + i];
#pragma unroll
      for (int u = 0; u < 4; ++u) c += v[u] * sF[(k + u) * 32 + d];
    }
    for (; k < nsplit; ++k) c += p[(size_t)k * 1088 + 64 + i] * sF[k * 32 + d];
    sCtx[i] = c * sInv[d];
    if (ctx_out) ctx_out[(size_t)b * 1024 + i] = sCtx[i] / scale;
  }
  __syncthreads();
  // W'[c][d] = sum_e W_out[c][e] * ctx[d][e]; packed: ((ct*4+q)*64 + h*32+j)*4+e4 with c = ct*32+j, d = h*16 + 4q + e4
  const int CT = (cout + 31) / 32;
  float* wo = wpk_b + (size_t)b * CT * 1024;
  for (int i = tid; i < CT * 1024; i += 256) {
    const int e4 = i & 3, lane = (i >> 2) & 63, q = (i >> 8) & 3, ct = i >> 10;
    // layout_T (attn_out_kernel): the k-slot order of an accumulator-register operand, d = row(r = 4q + e4, half)
    const int c = ct * 32 + (lane & 31);
    const int d = layout_T ? (e4 + 8 * q + 4 * (lane >> 5)) : (lane >> 5) * 16 + q * 4 + e4;
    float acc = 0.f;
    if (c < cout)
      for (int e = 0; e < 32; ++e) acc = fmaf(w_out[c * 32 + e], sCtx[d * 32 + e], acc);
    wo[i] = acc;
  }
}

void launch_attn_combine(const float* partials, int nsplit, const float* w_out, int cout, float* wpk_b, int batch,
                         float scale, hipStream_t s, float* ctx_out, float* kstat_out, bool layout_T) {
  prof::Scope scope("attn_combine", s, 0, 0);
  hipLaunchKernelGGL(attn_combine_kernel, dim3(batch), dim3(256), 0, s, partials, nsplit, w_out, cout, wpk_b, scale, ctx_out,
                     kstat_out, layout_T ? 1 : 0);
  CD_HIP(hipGetLastError());
}

// The launch sequence of the unfused form, the same on the sampling path (attn_block) and the training tape (attn_block_train)
void launch_attn_unfused(const float* x, int C, const float* coef, const float* wqkv, const float* w_out, const float* bias,
                         float* qkv, float* partials, int nsplit, float* wpk_b, float* y, float* ch_part, int batch, int64_t vox,
                         hipStream_t s, float* ctx_out, float* kstat_out) {
  {
    PointwiseArgs a;
    a.in0 = x; a.ld0 = C; a.c0 = C; a.wpk = wqkv; a.out = qkv; a.batch = batch; a.cout = 96; a.vox = vox;
    a.prologue = A_AFFINE; a.coef = coef;
    launch_pointwise(a, s);
  }
  launch_attn_context(qkv, partials, batch, vox, nsplit, s);
  launch_attn_combine(partials, nsplit, w_out, C, wpk_b, batch, kAttnScale, s, ctx_out, kstat_out);
  const int CT = (C + 31) / 32;
  PointwiseArgs a;
  a.in0 = qkv; a.ld0 = 96; a.off0 = 0; a.c0 = 32; a.wpk = wpk_b; a.w_batch_stride = (int64_t)CT * 1024; a.bias = bias;
  a.out = y; a.batch = batch; a.cout = C; a.vox = vox; a.prologue = A_SOFTMAX32; a.ch_part = ch_part;
  launch_pointwise(a, s);
}

}  // namespace cd
