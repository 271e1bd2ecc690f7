// The training objectives of models/loss.py: the device helpers every kernel that evaluates them shares, and the loss launchers
// (kernels_loss.hip).
#pragma once
#include "cd_common.h"

namespace cd {

void launch_axpy_sigma(const float* data, const float* noise, const float* sigma_b, float* out, int batch, int64_t per,
                       hipStream_t s);
// The training objectives of models/loss.py on top of the denoiser's output `out` (calodiffusion.py:161-169), objective =
// CD_OBJ_*:  what the loss compares, its per-sample weight (used by 'l2' only) and d pred / d F for the backward pass
//   0 hybrid_weight (:163-179)  pred = out = c_skip x + c_out F        target = data    w = 1 + sigma^-2   dpred/dF = c_out
//   1 noise_pred    (:181-196)  pred = (data - (data - sigma out)) / sigma, out = x - sigma F   target = noise   w = 1   dpred/dF = -sigma
//   2 mean_pred     (:198-210)  pred = out = F                         target = data    w = sigma^-2       dpred/dF = 1
// (noise_pred's round trip through x0_pred is evaluated as written, product / difference / quotient each rounded on its own)
__device__ __forceinline__ float objective_residual(int objective, float out, float data, float noise, float sigma) {
#pragma clang fp contract(off)
  if (objective == 1) {
    const float so = sigma * out;
    const float x0p = data - so;
    const float num = data - x0p;
    const float pred = num / sigma;
    return pred - noise;
  }
  return out - data;
}
__device__ __forceinline__ float objective_weight(int objective, int loss_type, float sg) {
  if (loss_type != 0 || objective == 1) return 1.0f;
  return objective == 0 ? 1.0f + 1.0f / (sg * sg) : 1.0f / (sg * sg);
}
// A given target (cd_train_step_target: consistency distillation): the residual is out - target and the weight 1 whatever the plan's
// objective.  That is what objective 0 evaluates for every loss type but 'l2' when `data` holds the target, so the kernels take the
// target where they take data and this value as the objective of the residual; d pred / d F stays the plan's own (c_out, -sigma, 1).
constexpr int kResidualOnOutput = 0;
// d loss / d x0 = norm * w_b * f'(d):  l2: 2 w d / (mean(w) N);  mse: 2 d / N;  l1: sign(d) / N;  huber: clamp(d, -1, 1) / N
// (scal: (batch, 4), sigma in column 3; one thread of a workgroup evaluates the norm)
__device__ __forceinline__ float loss_grad_norm(const float* scal, int batch, int64_t per, int loss_type, int objective) {
  double wsum = 0.0;
  for (int b = 0; b < batch; ++b) {
    wsum += (double)objective_weight(objective, 0, scal[b * 4 + 3]);
  }
  return loss_type == 0 ? (float)(2.0 / ((wsum / batch) * (double)batch * (double)per))
                        : (float)((loss_type == 2 ? 2.0 : 1.0) / ((double)batch * (double)per));
}
// ... times d pred / d F (`chain`): the gradient at the network's output F
__device__ __forceinline__ float loss_grad_dF(float norm, float x0, float data, float noise, float sg, float chain, int loss_type,
                                              int objective) {
  const float dd = objective_residual(objective, x0, data, noise, sg);
  const float fp = loss_type == 1 ? (dd > 0.f ? 1.f : (dd < 0.f ? -1.f : 0.f))
                                  : (loss_type == 3 ? fminf(fmaxf(dd, -1.f), 1.f) : dd);
  return norm * objective_weight(objective, loss_type, sg) * fp * chain;
}

void launch_loss_partial(const float* x0, const float* data, const float* noise, const float* sigma_b, double* partial, int batch,
                         int64_t per, hipStream_t s, int loss_type = 0, int objective = 0);
void launch_loss_final(const double* partial, const float* sigma_b, double* loss, int batch, int64_t per, hipStream_t s,
                       int loss_type = 0, int objective = 0);

}  // namespace cd
