// Backward of the output head (forward: head_kernel in kernels_head.hip): fused with the loss gradient for the training step
// (head_loss_bwd_kernel; the loss types and objectives of models/loss.py) and from a caller's dL/dD for cd_denoise_vjp
// (head_vjp_kernel); head_grad_reduce_kernel sums the blocks' partial weight / bias gradients in a fixed order.
#include "kernels_bwd.h"
#include "kernels_loss.h"

namespace cd {

// ------------------------------------------------------------------------------------------------------------
// Head + loss backward (forward: head_kernel; loss.py:103-104,176):
//   L = sum_b w_b sum_v (x0 - data)^2 / (mean(w) * B * per),  x0 = c_skip*x + c_out*F,  F = sum_c Wh[c]*h[v][c] + bh
//   dF = 2 w_b (x0 - data) c_out[b] / (mean(w) B per);  dh[v][c] = dF*Wh[c];  dWh[c] = sum dF*h[v][c];  dbh = sum dF
// part: [blocks][33] partial sums (32 weights + bias)
// res_objective: the objective whose residual and weight the loss takes, the plan's own (== objective) in cd_train_step;
// kResidualOnOutput with `data` the given target in cd_train_step_target (x0 - target, weight 1; the chain stays objective's)
// ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) head_loss_bwd_kernel(const float* __restrict__ x0, const float* __restrict__ data,
                                                            const float* __restrict__ noise,
                                                            const float* __restrict__ scal, const float* __restrict__ h,
                                                            const float* __restrict__ wh, float* __restrict__ dh,
                                                            float* __restrict__ part, int batch, int64_t vox, int loss_type,
                                                            int objective, int res_objective) {
  __shared__ float sW[32];
  __shared__ float sAcc[8][33];
  __shared__ float sNorm;
  const int tid = threadIdx.x, sub = tid & 7, grp = tid >> 3;
  if (tid < 32) sW[tid] = wh[tid];
  if (tid == 0) sNorm = loss_grad_norm(scal, batch, vox, loss_type, res_objective);
  __syncthreads();
  const int64_t total = (int64_t)batch * vox;
  f32x4 aw = {0.f, 0.f, 0.f, 0.f};
  float ab = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 32 + grp; i < total; i += (int64_t)gridDim.x * 32) {
    const int b = (int)(i / vox);
    const float sg = scal[b * 4 + 3];
    // d pred / d F: c_out (hybrid), -sigma (noise_pred: out = x - sigma F and pred ~ out), 1 (mean_pred)
    const float chain = objective == 0 ? scal[b * 4 + 2] : (objective == 1 ? -sg : 1.0f);
    const float dF = loss_grad_dF(sNorm, x0[i], data[i], res_objective == 1 ? noise[i] : 0.f, sg, chain, loss_type, res_objective);
    const f32x4 hv = *(const f32x4*)(h + (size_t)i * 32 + sub * 4);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o[e] = dF * sW[sub * 4 + e];
      aw[e] += dF * hv[e];
    }
    *(f32x4*)(dh + (size_t)i * 32 + sub * 4) = o;
    if (sub == 0) ab += dF;
  }
  // reduce over the 32 voxel groups of the block: lanes with equal `sub` hold the same channels
#pragma unroll
  for (int o = 8; o < 64; o <<= 1) {
#pragma unroll
    for (int e = 0; e < 4; ++e) aw[e] += __shfl_xor(aw[e], o, 64);
    ab += __shfl_xor(ab, o, 64);
  }
  const int wave = tid >> 6, lane = tid & 63;
  if (lane < 8) {
#pragma unroll
    for (int e = 0; e < 4; ++e) sAcc[wave * 2][lane * 4 + e] = aw[e];
    if (lane == 0) sAcc[wave * 2][32] = ab;
  }
  __syncthreads();
  if (tid < 33) part[(size_t)blockIdx.x * 33 + tid] = sAcc[0][tid] + sAcc[2][tid] + sAcc[4][tid] + sAcc[6][tid];
}
// 7 slices of the partial rows per column, eight loads in flight, fixed-order tree (33 threads walking 1024 rows each was
// a 237 us serial chain)
__global__ void __launch_bounds__(256) head_grad_reduce_kernel(const float* __restrict__ part, int nblocks, float* __restrict__ dwh,
                                                               float* __restrict__ dbh) {
  __shared__ double sh[7][33];
  const int c = threadIdx.x % 33, sl = threadIdx.x / 33;
  if (sl < 7) {
    double s = 0.0;
    int k = sl;
    for (; k + 7 * 7 < nblocks; k += 7 * 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(k + 7 * u) * 33 + c];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += (double)v[u];
    }
    for (; k < nblocks; k += 7) s += (double)part[(size_t)k * 33 + c];
    sh[sl][c] = s;
  }
  __syncthreads();
  if (threadIdx.x < 33) {
    double s = 0.0;
    for (int i = 0; i < 7; ++i) s += sh[i][threadIdx.x];
    if (threadIdx.x < 32) dwh[threadIdx.x] = (float)s;
    else dbh[0] = (float)s;
  }
}
int head_bwd_blocks(int batch, int64_t vox) {
  int64_t n = ((int64_t)batch * vox + 255) / 256;
  return (int)(n > 1024 ? 1024 : (n < 1 ? 1 : n));
}
void launch_head_loss_bwd(const float* x0, const float* data, const float* noise, const float* scal, const float* h, const float* wh,
                          float* dh, float* part, float* dwh, float* dbh, int batch, int64_t vox, hipStream_t s, int loss_type,
                          int objective, int res_objective) {
  const int nb = head_bwd_blocks(batch, vox);
  hipLaunchKernelGGL(head_loss_bwd_kernel, dim3(nb), dim3(256), 0, s, x0, data, noise, scal, h, wh, dh, part, batch, vox, loss_type,
                     objective, res_objective < 0 ? objective : res_objective);
  hipLaunchKernelGGL(head_grad_reduce_kernel, dim3(1), dim3(256), 0, s, part, nb, dwh, dbh);
  CD_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------------------
// Head backward from a caller's gradient gy = dL/dD of the denoiser output (cd_denoise_vjp; D as in head_kernel):
//   dF = coef_b gy,  coef_b = c_out (hybrid), -sigma (noise_pred), 1 (mean_pred);  dh[v][c] = dF*Wh[c]
//   PARAMS: dWh[c] = sum dF*h[v][c], dbh = sum dF as [blocks][33] partials for head_grad_reduce_kernel
// ------------------------------------------------------------------------------------------------------------
template <bool PARAMS>
__global__ void __launch_bounds__(256) head_vjp_kernel(const float* __restrict__ gy, const float* __restrict__ scal,
                                                       const float* __restrict__ h, const float* __restrict__ wh, float* __restrict__ dh,
                                                       float* __restrict__ part, int batch, int64_t vox, int objective) {
  __shared__ float sW[32];
  __shared__ float sAcc[4][33];
  const int tid = threadIdx.x, sub = tid & 7, grp = tid >> 3;
  if (tid < 32) sW[tid] = wh[tid];
  __syncthreads();
  const int64_t total = (int64_t)batch * vox;
  f32x4 aw = {0.f, 0.f, 0.f, 0.f};
  float ab = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 32 + grp; i < total; i += (int64_t)gridDim.x * 32) {
    const int b = (int)(i / vox);
    const float chain = objective == 0 ? scal[b * 4 + 2] : (objective == 1 ? -scal[b * 4 + 3] : 1.0f);
    const float dF = chain * gy[i];
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = dF * sW[sub * 4 + e];
    *(f32x4*)(dh + (size_t)i * 32 + sub * 4) = o;
    if (PARAMS) {
      const f32x4 hv = *(const f32x4*)(h + (size_t)i * 32 + sub * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) aw[e] += dF * hv[e];
      if (sub == 0) ab += dF;
    }
  }
  if (!PARAMS) return;
#pragma unroll
  for (int o = 8; o < 64; o <<= 1) {
#pragma unroll
    for (int e = 0; e < 4; ++e) aw[e] += __shfl_xor(aw[e], o, 64);
    ab += __shfl_xor(ab, o, 64);
  }
  const int wave = tid >> 6, lane = tid & 63;
  if (lane < 8) {
#pragma unroll
    for (int e = 0; e < 4; ++e) sAcc[wave][lane * 4 + e] = aw[e];
    if (lane == 0) sAcc[wave][32] = ab;
  }
  __syncthreads();
  if (tid < 33) part[(size_t)blockIdx.x * 33 + tid] = sAcc[0][tid] + sAcc[1][tid] + sAcc[2][tid] + sAcc[3][tid];
}
void launch_head_vjp(const float* gy, const float* scal, const float* h, const float* wh, float* dh, float* part, float* dwh, float* dbh,
                     int batch, int64_t vox, int objective, hipStream_t s) {
  const int nb = head_bwd_blocks(batch, vox);
  if (part) {
    hipLaunchKernelGGL(head_vjp_kernel<true>, dim3(nb), dim3(256), 0, s, gy, scal, h, wh, dh, part, batch, vox, objective);
    hipLaunchKernelGGL(head_grad_reduce_kernel, dim3(1), dim3(256), 0, s, part, nb, dwh, dbh);
  } else {
    hipLaunchKernelGGL(head_vjp_kernel<false>, dim3(nb), dim3(256), 0, s, gy, scal, h, wh, dh, part, batch, vox, objective);
  }
  CD_HIP(hipGetLastError());
}

}  // namespace cd
