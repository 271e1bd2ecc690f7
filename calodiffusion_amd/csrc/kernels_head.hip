// The output head with the EDM pre-conditioning and the samplers' fused update (backward: kernels_head_bwd.hip).
#include "kernels_embed_head.h"
#include "gn_defer.h"

namespace cd {

// ------------------------------------------------------------------------------------------------------------
// Head: final 1x1x1 conv 32 -> 1 (models.py:696) fused with the EDM output scaling (calodiffusion.py:161-167).
// 8 lanes per voxel, each a float4 of the 128-B channel vector.
// ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) head_kernel(HeadArgs a) {
  const int64_t total = (int64_t)a.batch * a.vox;
  const int sub = threadIdx.x & 7;
  const f32x4 w = *(const f32x4*)(a.w + sub * 4);
  const float bias = a.bias[0];
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 3; i < total; i += ((int64_t)gridDim.x * 256) >> 3) {
    const f32x4 h = *(const f32x4*)(a.h + (size_t)i * 32 + sub * 4);
    float p = (h[0] * w[0] + h[1] * w[1]) + (h[2] * w[2] + h[3] * w[3]);
    p += __shfl_xor(p, 1, 64);
    p += __shfl_xor(p, 2, 64);
    p += __shfl_xor(p, 4, 64);
    if (sub == 0) {
      float pred = p + bias;
      if (a.scal) {
        const int b = (int)(i / a.vox);
        const float xv = a.x[i];
        if (a.objective == 0) pred = a.scal[b * 4 + 1] * xv + a.scal[b * 4 + 2] * pred;
        else if (a.objective == 1) pred = xv - a.scal[b * 4 + 3] * pred;
      }
      a.out[i] = pred;
      if (a.upd_stepvals) {  // (DDim.__call__'s update: HeadArgs::upd_*)
        const float sigma = a.upd_stepvals[0], sprev = a.upd_stepvals[1], dsig = a.upd_stepvals[2], denom = a.upd_stepvals[3];
        const float eps = (a.x[i] - pred) / sigma;
        float r = pred + sprev * eps;
        if (a.upd_noise) r += dsig * a.upd_noise[i] / denom;
        a.upd_x_next[i] = r;
        if (a.upd_xs) a.upd_xs[i] = r;
        if (a.upd_x0s) a.upd_x0s[i] = pred;
      }
    }
  }
}

// the same with the final ResnetBlock's GroupNorm(8) + SiLU + shortcut folded in: workgroups belong to one sample (blockIdx.y)
__global__ void __launch_bounds__(256) head_gn_kernel(HeadArgs a) {
  __shared__ __attribute__((aligned(16))) float sCoef[32 * 4];
  __shared__ __attribute__((aligned(16))) char sDefer[32 * 16 + 64 * 8];
  const int b = blockIdx.y;
  gn_defer_to_lds(a.defer, b, sCoef, sDefer);
  const int sub = threadIdx.x & 7;
  const f32x4 w = *(const f32x4*)(a.w + sub * 4);
  const float bias = a.bias[0];
  f32x4 cf[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) cf[e] = *(const f32x4*)(sCoef + (sub * 4 + e) * 4);
  const int64_t per = (a.vox + gridDim.x - 1) / gridDim.x;
  const int64_t v0 = (int64_t)blockIdx.x * per, v1 = v0 + per < a.vox ? v0 + per : a.vox;
  // four voxels per trip: eight 16-byte loads in flight per thread (one voxel per trip streamed Dataset-3's 332 MB at 3.5 TB/s)
  for (int64_t vb = v0 + (threadIdx.x >> 3); vb < v1; vb += 128) {
    f32x4 h4[4], r4[4];
    float xv4[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t v = vb + 32 * k < v1 ? vb + 32 * k : vb;  // (past the end: a repeat of the first, not stored)
      const int64_t i = (int64_t)b * a.vox + v;
      h4[k] = *(const f32x4*)(a.h + (size_t)i * 32 + sub * 4);
      r4[k] = *(const f32x4*)(a.res + (size_t)i * 32 + sub * 4);
      xv4[k] = (a.scal && sub == 0) ? a.x[i] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t v = vb + 32 * k;
      const int64_t i = (int64_t)b * a.vox + v;
      f32x4 h = h4[k];
      const f32x4 r = r4[k];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float u = cf[e][0] * h[e] + cf[e][1];
        u = u * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(u * -1.4426950408889634f));  // (gn_apply's SiLU)
        h[e] = u + cf[e][2] + r[e];
      }
      float p = (h[0] * w[0] + h[1] * w[1]) + (h[2] * w[2] + h[3] * w[3]);
      p += __shfl_xor(p, 1, 64);
      p += __shfl_xor(p, 2, 64);
      p += __shfl_xor(p, 4, 64);
      if (sub == 0 && v < v1) {
        float pred = p + bias;
        const float xv = xv4[k];
        if (a.scal) {
          if (a.objective == 0) pred = a.scal[b * 4 + 1] * xv + a.scal[b * 4 + 2] * pred;
          else if (a.objective == 1) pred = xv - a.scal[b * 4 + 3] * pred;
        }
        a.out[i] = pred;
        if (a.upd_stepvals) {  // (DDim.__call__'s update: HeadArgs::upd_*)
          const float sigma = a.upd_stepvals[0], sprev = a.upd_stepvals[1], dsig = a.upd_stepvals[2], denom = a.upd_stepvals[3];
          const float eps = (a.x[i] - pred) / sigma;
          float r = pred + sprev * eps;
          if (a.upd_noise) r += dsig * a.upd_noise[i] / denom;
          a.upd_x_next[i] = r;
          if (a.upd_xs) a.upd_xs[i] = r;
          if (a.upd_x0s) a.upd_x0s[i] = pred;
        }
      }
    }
  }
}

void launch_head(const HeadArgs& a, hipStream_t s) {
  CD_REQUIRE(!a.upd_stepvals || (a.x && a.scal && a.upd_x_next), "head: the fused sampler update needs x, the scalings and x_next");
  if (a.defer.part) {
    CD_REQUIRE(a.defer.C == 32 && a.res, "head: the fused final block is 32 channels wide with an identity shortcut");
    prof::Scope scope("head_gn", s, 64.0 * a.batch * a.vox, 4.0 * a.batch * a.vox * 66);
    int per_sample = (int)((1024 + a.batch - 1) / a.batch);  // one round of ~1024 workgroups, each folds the GroupNorm once
    const int cap = (int)((a.vox + 255) / 256);
    if (per_sample > cap) per_sample = cap;
    if (per_sample < 1) per_sample = 1;
    hipLaunchKernelGGL(head_gn_kernel, dim3((unsigned)per_sample, (unsigned)a.batch), dim3(256), 0, s, a);
    CD_HIP(hipGetLastError());
    return;
  }
  const int64_t total = (int64_t)a.batch * a.vox;
  int64_t blocks = (total * 8 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  prof::Scope scope("head", s, 64.0 * total, 4.0 * total * 34);
  hipLaunchKernelGGL(head_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
  CD_HIP(hipGetLastError());
}

}  // namespace cd
