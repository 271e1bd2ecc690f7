// Fused Adam (cd_adam_step).
#include "guarded.h"

#include <cmath>

namespace cd {

// ------------------------------------------------------------------------------------------------------------
// Adam step over many parameter tensors in one launch per 48 tensors (torch.optim.Adam as the reference's training loop
// builds it, train/train.py:144: no amsgrad, optional L2 weight decay), same element-wise formulas and operation order as
// torch's implementation:  m <- m + (1-b1)(g - m);  v <- b2 v + (1-b2) g g;  p <- p - (lr/bc1) m / (sqrt(v)/sqrt(bc2) + eps).
// ------------------------------------------------------------------------------------------------------------
struct AdamChunk {  // up to 48 tensors per launch (kernel-argument table)
  float* p[48];
  const float* g[48];
  float* m[48];
  float* v[48];
  int64_t n[48];
};
__global__ void __launch_bounds__(256) adam_kernel(AdamChunk c, float w1, float beta2, float w2, float eps, float weight_decay,
                                                   float step_size, float bc2_sqrt) {
  const int t = blockIdx.y;
  float* __restrict__ p = c.p[t];
  const float* __restrict__ g = c.g[t];
  float* __restrict__ m = c.m[t];
  float* __restrict__ v = c.v[t];
  const int64_t n = c.n[t];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float gi = g[i];
    const float pi = p[i];
    if (weight_decay != 0.f) gi = gi + weight_decay * pi;
    const float mi = m[i] + w1 * (gi - m[i]);
    const float vi = v[i] * beta2 + w2 * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] = pi - step_size * (mi / denom);
  }
}

static void launch_adam(const AdamChunk& c, int ntensors, int64_t max_numel, double lr, double beta1, double beta2, float eps,
                        float weight_decay, int step, hipStream_t s) {
  const double bc1 = 1.0 - std::pow(beta1, step), bc2 = 1.0 - std::pow(beta2, step);
  const float step_size = (float)(lr / bc1), bc2_sqrt = (float)std::sqrt(bc2);
  int64_t bx = (max_numel + 256 * 4 - 1) / (256 * 4);
  if (bx < 1) bx = 1;
  if (bx > 1024) bx = 1024;
  // 1 - beta in double like torch (python floats), then rounded once to fp32
  const float w1 = (float)(1.0 - beta1), w2 = (float)(1.0 - beta2);
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)bx, (unsigned)ntensors), dim3(256), 0, s, c, w1, (float)beta2, w2, eps, weight_decay, step_size,
                     bc2_sqrt);
  CD_HIP(hipGetLastError());
}

}  // namespace cd

extern "C" int cd_adam_step(int n, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                            const int64_t* numel, double lr, double beta1, double beta2, float eps, float weight_decay, int step,
                            void* stream) {
  return guarded([&] {
    CD_REQUIRE(n >= 0 && (n == 0 || (params && grads && exp_avg && exp_avg_sq && numel)) && step >= 1, "bad argument");
    for (int i0 = 0; i0 < n; i0 += 48) {
      AdamChunk c{};
      const int k = n - i0 < 48 ? n - i0 : 48;
      int64_t mx = 0;
      for (int j = 0; j < k; ++j) {
        c.p[j] = params[i0 + j]; c.g[j] = grads[i0 + j]; c.m[j] = exp_avg[i0 + j]; c.v[j] = exp_avg_sq[i0 + j]; c.n[j] = numel[i0 + j];
        CD_REQUIRE(c.p[j] && c.g[j] && c.m[j] && c.v[j] && c.n[j] >= 0, "adam: null tensor pointer");
        if (c.n[j] > mx) mx = c.n[j];
      }
      launch_adam(c, k, mx, lr, beta1, beta2, eps, weight_decay, step, (hipStream_t)stream);
    }
  });
}
