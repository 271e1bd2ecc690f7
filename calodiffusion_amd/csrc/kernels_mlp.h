// LayerDiffusion's layer-energy MLP: forward, sampler programs (kernels_mlp.hip) and the training step (kernels_mlp_train.hip).
#pragma once
#include "cd_common.h"

struct CdSamplerOp;  // include/calodiff.h

namespace cd {

struct LinearWgradJob;  // kernels_bwd.h

// LayerDiffusion's layer-energy MLP: raw forward (mode 0), EDM denoise (mode 1) or a whole sampler trajectory (mode 2)
struct LayerMlpArgs {
  const float* w[64];    // (weight, bias) per Linear in the reference ResNet's state_dict order
  int dim_in, hidden, cond_emb, cond_size, n_res, time_kind, objective, mode, batch, n_steps;
  float sigma_data;
  const float* x;        // (B, dim_in): input / start noise
  const float* cond;     // (B, cond_size)
  const float* tsig;     // (B): time (mode 0) or sigma (mode 1)
  const float* table;    // device (n_steps, 4) step table (mode 2)
  const float* noise;    // (n_steps, B, dim_in) or null
  float* out;            // (B, dim_in)
  float* xs;             // (n_steps, B, dim_in) or null
  float* x0s;
};
void launch_layer_mlp(const LayerMlpArgs& a, hipStream_t s);

// a sampler step program (CdSamplerOp lists, include/calodiff.h) on the layer MLP, the whole trajectory in one launch
// (cd_layer_sampler_run); ops / op_begin / coefs are device arrays the host has validated
struct LayerProgArgs {
  const float* w[64];
  int dim_in, hidden, cond_emb, cond_size, n_res, time_kind, objective, batch;
  float sigma_data;
  const float* start;        // (B, dim_in): buffer 0 = start * start_scale
  float start_scale;
  const float* cond;         // (B, cond_size)
  int n_bufs, n_steps, n_ops, n_coef;
  const ::CdSamplerOp* ops;  // n_ops entries
  const int32_t* op_begin;   // n_steps + 1 entries, or null: every step runs ops[0, n_ops)
  const float* coefs;        // (n_steps, n_coef)
  const float* step_noise;   // (RANDN ops executed, B, dim_in), or null: the Philox stream
  uint64_t seed, offset, stride;  // RANDN number k takes stream elements offset + k stride + b dim_in + i
  float* out;                // (B, dim_in)
  float* xs;                 // (n_steps, B, dim_in) or null
  float* x0s;
};
constexpr int LAYER_PROG_MAX_BUFS = 10;
// n_denoise: DENOISE ops the program executes (the profiler's algorithmic flops)
void launch_layer_program(const LayerProgArgs& a, int64_t n_denoise, hipStream_t s);

// training step of the layer-energy MLP (kernels_mlp_train.hip)
struct LayerTapeLayout {
  int xin, t_in, a1t, a2t, cin, a1c, a2c, g, hprev[8], h1[8], hfin;       // inputs of the Linear layers
  int dpred, dv[8], du[8], de[8], dh0, d3t, d2t, d1t, d3c, d2c, d1c;     // their output deltas
  int total;
};
LayerTapeLayout layer_tape_layout(int dim, int hidden, int cond_emb, int cond_size, int n_res);
struct LayerMlpTrainArgs {
  const float* w[64];
  int dim_in, hidden, cond_emb, cond_size, n_res, time_kind, batch;
  int loss_type = 0;  // CD_LOSS_* (Loss._loss, models/loss.py:97-116): 0 l2 (weighted), 1 l1, 2 mse, 3 huber
  int objective = 0;  // CD_OBJ_* (objective_residual / objective_weight, kernels_loss.h)
  float sigma_data;
  const float *data, *noise, *sigma, *cond;  // (B, dim), (B, dim), (B), (B, cond_size)
  LayerTapeLayout layout;
  float* tape;        // [B][layout.total]
  double* loss_part;  // [B]
  // weight / bias gradients: the kernel that writes the tape also writes linear_wgrad_kernel's job table (workspace)
  float* grads;
  LinearWgradJob* jobs;
  // cd_layer_denoise_vjp: the state x and the upstream gradient gy = dL/dD, both (B, dim); dx = dL/dx
  const float *x, *gy;
  float* dx;
};
size_t layer_train_workspace_bytes(const LayerMlpTrainArgs& a);
// loss and, with grads, every parameter gradient; grads == null: the forward and the loss only (cd_layer_loss)
void launch_layer_mlp_train(LayerMlpTrainArgs a, float* grads, double* loss_out, void* workspace, hipStream_t s);
size_t layer_vjp_workspace_bytes(const LayerMlpTrainArgs& a, bool with_param_grads);
// dx and, with grads, every parameter gradient from the caller's gy (cd_layer_denoise_vjp)
void launch_layer_mlp_vjp(LayerMlpTrainArgs a, float* grads, void* workspace, hipStream_t s);

}  // namespace cd
