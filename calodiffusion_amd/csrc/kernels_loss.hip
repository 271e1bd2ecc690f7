// The training loss on the denoiser's output (its gradient: kernels_head_bwd.hip).
#include "kernels_loss.h"

namespace cd {

// ------------------------------------------------------------------------------------------------------------
// Training forward: x_noisy = data + sigma*noise (loss.py:169) and the weighted L2 reduction (loss.py:103-104,176)
// ------------------------------------------------------------------------------------------------------------
__global__ void axpy_sigma_kernel(const float* __restrict__ data, const float* __restrict__ noise,
                                  const float* __restrict__ sigma_b, float* __restrict__ out, int64_t per) {
  const int b = blockIdx.y;
  const float sg = sigma_b[b];
  const size_t base = (size_t)b * per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (int64_t)gridDim.x * 256)
    out[base + i] = data[base + i] + sg * noise[base + i];
}
void launch_axpy_sigma(const float* data, const float* noise, const float* sigma_b, float* out, int batch, int64_t per,
                       hipStream_t s) {
  int64_t bx = (per + 255) / 256;
  if (bx > 64) bx = 64;
  hipLaunchKernelGGL(axpy_sigma_kernel, dim3((unsigned)bx, batch), dim3(256), 0, s, data, noise, sigma_b, out, per);
  CD_HIP(hipGetLastError());
}

// per-sample sum of the element loss of Loss._loss (models/loss.py:97-116) in fp64, one block per sample: 0 'l2' and 2 'mse':
// d^2; 1 'l1': |d|; 3 'huber' = torch smooth_l1_loss, beta 1: d^2 / 2 below |d| = 1, |d| - 1/2 above
__global__ void __launch_bounds__(256) loss_partial_kernel(const float* __restrict__ x0, const float* __restrict__ data,
                                                           const float* __restrict__ noise, const float* __restrict__ sigma_b,
                                                           double* __restrict__ partial, int64_t per, int loss_type, int objective) {
  __shared__ double sh[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const size_t base = (size_t)b * per;
  const float sg = sigma_b[b];
  double acc = 0.0;
  for (int64_t i = tid; i < per; i += 256) {
    const float d = objective_residual(objective, x0[base + i], data[base + i], objective == 1 ? noise[base + i] : 0.f, sg);
    const float ad = fabsf(d);
    const float e = loss_type == 1 ? ad : (loss_type == 3 ? (ad < 1.f ? 0.5f * d * d : ad - 0.5f) : d * d);
    acc += (double)e;
  }
  sh[tid] = acc;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) sh[tid] += sh[tid + st];
    __syncthreads();
  }
  if (tid == 0) partial[b] = sh[0];
}
void launch_loss_partial(const float* x0, const float* data, const float* noise, const float* sigma_b, double* partial, int batch,
                         int64_t per, hipStream_t s, int loss_type, int objective) {
  hipLaunchKernelGGL(loss_partial_kernel, dim3(batch), dim3(256), 0, s, x0, data, noise, sigma_b, partial, per, loss_type, objective);
  CD_HIP(hipGetLastError());
}
// loss = sum_b w_b * partial[b] / (mean_b(w_b) * B * per)
// (only 'l2' carries the weight; the torch.nn.functional losses of the other types are plain means, loss.py:106-111)
__global__ void loss_final_kernel(const double* __restrict__ partial, const float* __restrict__ sigma_b, double* loss,
                                  int batch, int64_t per, int loss_type, int objective) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double num = 0.0, wsum = 0.0;
    for (int b = 0; b < batch; ++b) {
      const float w = objective_weight(objective, loss_type, sigma_b[b]);
      num += (double)w * partial[b];
      wsum += (double)w;
    }
    loss[0] = num / ((wsum / batch) * (double)batch * (double)per);
  }
}
void launch_loss_final(const double* partial, const float* sigma_b, double* loss, int batch, int64_t per, hipStream_t s,
                       int loss_type, int objective) {
  hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(64), 0, s, partial, sigma_b, loss, batch, per, loss_type, objective);
  CD_HIP(hipGetLastError());
}

}  // namespace cd
