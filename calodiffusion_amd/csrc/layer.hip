// Entry points of LayerDiffusion's layer-energy MLP: forward, denoise, sampler, sampler programs, training step, loss and VJP
// (kernels: kernels_mlp.hip, kernels_mlp_train.hip).
#include "guarded.h"
#include "kernels_mlp.h"
#include "kernels_sampler.h"

#include <vector>

namespace cd {

static void check_layer_desc(const CdLayerMlpDesc* d, int n_weights) {
  CD_REQUIRE(d->struct_size == sizeof(CdLayerMlpDesc), "CdLayerMlpDesc.struct_size does not match this library's calodiff.h");
  CD_REQUIRE(d->n_res >= 0 && d->n_res <= 8 && n_weights == 2 * (8 + 3 * d->n_res),
             "layer MLP: n_weights must be 2*(8 + 3*n_res) (time_mlp, cond_mlp, in_lay, blocks, out_lay)");
  CD_REQUIRE(d->time_embed_kind >= 0 && d->time_embed_kind <= 2 && d->objective >= 0 && d->objective <= 2, "bad descriptor");
}

// what LayerMlpArgs, LayerProgArgs and LayerMlpTrainArgs share: the checked descriptor's dims and the caller's weight pointers
// (weights null: an entry point that takes none, the workspace sizes)
template <typename Args>
static Args layer_args(const CdLayerMlpDesc* d, const float* const* weights, int n_weights, int batch) {
  CD_REQUIRE(d && batch > 0, "bad argument");
  check_layer_desc(d, weights ? n_weights : 2 * (8 + 3 * d->n_res));
  Args a{};
  for (int i = 0; weights && i < n_weights; ++i) {
    CD_REQUIRE(weights[i], "null weight pointer");
    a.w[i] = weights[i];
  }
  a.dim_in = d->dim_in; a.hidden = d->hidden; a.cond_emb = d->cond_emb; a.cond_size = d->cond_size; a.n_res = d->n_res;
  a.time_kind = d->time_embed_kind; a.objective = d->objective; a.batch = batch; a.sigma_data = d->sigma_data;
  return a;
}

static void layer_mlp_call(const CdLayerMlpDesc* d, const float* const* weights, int n_weights, int batch, int mode,
                           const float* x, const float* cond, const float* tsig, const float* table, int n_steps,
                           const float* noise, float* out, float* xs, float* x0s, void* stream) {
  CD_REQUIRE(d && weights && x && cond && out && batch > 0, "bad argument");
  LayerMlpArgs a = layer_args<LayerMlpArgs>(d, weights, n_weights, batch);
  a.mode = mode; a.n_steps = n_steps;
  a.x = x; a.cond = cond; a.tsig = tsig; a.table = table; a.noise = noise; a.out = out; a.xs = xs; a.x0s = x0s;
  launch_layer_mlp(a, (hipStream_t)stream);
}

static LayerMlpTrainArgs layer_train_args(const CdLayerMlpDesc* d, const float* const* weights, int n_weights, int batch) {
  LayerMlpTrainArgs a = layer_args<LayerMlpTrainArgs>(d, weights, n_weights, batch);
  a.layout = layer_tape_layout(a.dim_in, a.hidden, a.cond_emb, a.cond_size, a.n_res);
  return a;
}

// the training step (grads) or the loss alone (grads == null) of the descriptor's objective
static void layer_loss_call(const CdLayerMlpDesc* desc, const float* const* weights, int n_weights, int batch, const float* data,
                            const float* noise, const float* sigma, const float* cond, int loss_type, double* loss_out,
                            float* grads, void* workspace, size_t workspace_bytes, void* stream) {
  CD_REQUIRE(weights && data && noise && sigma && cond && loss_out && workspace, "bad argument");
  CD_REQUIRE(loss_type >= CD_LOSS_L2 && loss_type <= CD_LOSS_HUBER, "loss_type must be one of CD_LOSS_L2 / L1 / MSE / HUBER");
  LayerMlpTrainArgs a = layer_train_args(desc, weights, n_weights, batch);
  a.loss_type = loss_type;
  CD_REQUIRE(workspace_bytes >= layer_train_workspace_bytes(a), "workspace too small: call cd_layer_train_workspace_bytes");
  a.data = data; a.noise = noise; a.sigma = sigma; a.cond = cond;
  launch_layer_mlp_train(a, grads, loss_out, workspace, (hipStream_t)stream);
}

}  // namespace cd

extern "C" {

int cd_layer_forward(const CdLayerMlpDesc* desc, const float* const* weights, int n_weights, int batch, const float* x,
                     const float* cond, const float* time, float* out, void* stream) {
  return guarded([&] {
    CD_REQUIRE(time, "bad argument");
    layer_mlp_call(desc, weights, n_weights, batch, 0, x, cond, time, nullptr, 1, nullptr, out, nullptr, nullptr, stream);
  });
}
int cd_layer_denoise(const CdLayerMlpDesc* desc, const float* const* weights, int n_weights, int batch, const float* x,
                     const float* sigma, const float* cond, float* out, void* stream) {
  return guarded([&] {
    CD_REQUIRE(sigma, "bad argument");
    layer_mlp_call(desc, weights, n_weights, batch, 1, x, cond, sigma, nullptr, 1, nullptr, out, nullptr, nullptr, stream);
  });
}
int cd_layer_sample(const CdLayerMlpDesc* desc, const float* const* weights, int n_weights, int batch, const float* start,
                    const float* cond, const CdStep* steps_dev, int n_steps, const float* step_noise, float* x_out, float* xs,
                    float* x0s, void* stream) {
  return guarded([&] {
    CD_REQUIRE(steps_dev && n_steps > 0, "bad argument");
    layer_mlp_call(desc, weights, n_weights, batch, 2, start, cond, nullptr, (const float*)steps_dev, n_steps, step_noise,
                   x_out, xs, x0s, stream);
  });
}

int cd_layer_sampler_run(const CdLayerMlpDesc* desc, const float* const* weights, int n_weights, int batch, const float* start,
                         float start_scale, const float* cond, int n_bufs, int n_steps, const CdSamplerOp* ops_dev, int n_ops,
                         const int32_t* op_begin_dev, const float* coefs_dev, int n_coef, const float* step_noise, uint64_t seed,
                         uint64_t offset, uint64_t noise_stride, float* x_out, float* xs, float* x0s, void* stream) {
  return guarded([&] {
    CD_REQUIRE(desc && weights && start && cond && ops_dev && coefs_dev && x_out && batch > 0, "bad argument");
    LayerProgArgs a = layer_args<LayerProgArgs>(desc, weights, n_weights, batch);
    CD_REQUIRE(n_bufs >= 2 && n_bufs <= LAYER_PROG_MAX_BUFS && n_steps >= 1 && n_steps <= 1 << 20 && n_ops >= 1 && n_coef >= 1,
               "bad program size (2..10 buffers)");
    hipStream_t s = (hipStream_t)stream;
    // the program is checked on the host's copy of it
    std::vector<CdSamplerOp> ops((size_t)n_ops);
    std::vector<int32_t> begin(op_begin_dev ? (size_t)n_steps + 1 : 0);
    CD_HIP(hipMemcpyAsync(ops.data(), ops_dev, sizeof(CdSamplerOp) * ops.size(), hipMemcpyDeviceToHost, s));
    if (op_begin_dev) CD_HIP(hipMemcpyAsync(begin.data(), op_begin_dev, sizeof(int32_t) * begin.size(), hipMemcpyDeviceToHost, s));
    CD_HIP(hipStreamSynchronize(s));
    const int64_t n_denoise =
        validate_sampler_program(ops.data(), op_begin_dev ? begin.data() : nullptr, n_steps, n_ops, n_bufs, n_coef, batch).n_denoise;
    a.start = start; a.start_scale = start_scale; a.cond = cond;
    a.n_bufs = n_bufs; a.n_steps = n_steps; a.n_ops = n_ops; a.n_coef = n_coef;
    a.ops = ops_dev; a.op_begin = op_begin_dev; a.coefs = coefs_dev; a.step_noise = step_noise;
    a.seed = seed; a.offset = offset; a.stride = noise_stride ? noise_stride : (uint64_t)batch * (uint64_t)desc->dim_in;
    a.out = x_out; a.xs = xs; a.x0s = x0s;
    launch_layer_program(a, n_denoise, s);
  });
}

int cd_layer_train_workspace_bytes(const CdLayerMlpDesc* desc, int batch, size_t* bytes) {
  return guarded([&] {
    CD_REQUIRE(bytes, "bad argument");
    *bytes = layer_train_workspace_bytes(layer_train_args(desc, nullptr, 0, batch));
  });
}
int cd_layer_train_step(const CdLayerMlpDesc* desc, const float* const* weights, int n_weights, int batch, const float* data,
                        const float* noise, const float* sigma, const float* cond, double* loss_out, float* grads,
                        void* workspace, size_t workspace_bytes, void* stream) {
  return cd_layer_train_step_loss(desc, weights, n_weights, batch, data, noise, sigma, cond, CD_LOSS_L2, loss_out, grads, workspace,
                                  workspace_bytes, stream);
}
int cd_layer_train_step_loss(const CdLayerMlpDesc* desc, const float* const* weights, int n_weights, int batch, const float* data,
                             const float* noise, const float* sigma, const float* cond, int loss_type, double* loss_out,
                             float* grads, void* workspace, size_t workspace_bytes, void* stream) {
  return guarded([&] {
    CD_REQUIRE(grads, "bad argument");
    layer_loss_call(desc, weights, n_weights, batch, data, noise, sigma, cond, loss_type, loss_out, grads, workspace, workspace_bytes,
                    stream);
  });
}
int cd_layer_loss(const CdLayerMlpDesc* desc, const float* const* weights, int n_weights, int batch, const float* data,
                  const float* noise, const float* sigma, const float* cond, int loss_type, double* loss_out, void* workspace,
                  size_t workspace_bytes, void* stream) {
  return guarded([&] {
    layer_loss_call(desc, weights, n_weights, batch, data, noise, sigma, cond, loss_type, loss_out, nullptr, workspace,
                    workspace_bytes, stream);
  });
}

int cd_layer_vjp_workspace_bytes(const CdLayerMlpDesc* desc, int batch, int with_param_grads, size_t* bytes) {
  return guarded([&] {
    CD_REQUIRE(bytes, "bad argument");
    *bytes = layer_vjp_workspace_bytes(layer_train_args(desc, nullptr, 0, batch), with_param_grads != 0);
  });
}
int cd_layer_denoise_vjp(const CdLayerMlpDesc* desc, const float* const* weights, int n_weights, int batch, const float* x,
                         const float* sigma, const float* cond, const float* gy, float* dx, float* grads, void* workspace,
                         size_t workspace_bytes, void* stream) {
  return guarded([&] {
    CD_REQUIRE(weights && x && sigma && cond && gy && dx && workspace, "bad argument");
    LayerMlpTrainArgs a = layer_train_args(desc, weights, n_weights, batch);
    CD_REQUIRE(workspace_bytes >= layer_vjp_workspace_bytes(a, grads != nullptr),
               "workspace too small: call cd_layer_vjp_workspace_bytes");
    a.x = x; a.gy = gy; a.dx = dx; a.sigma = sigma; a.cond = cond;
    launch_layer_mlp_vjp(a, grads, workspace, (hipStream_t)stream);
  });
}

}  // extern "C"
