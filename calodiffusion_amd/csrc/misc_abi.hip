// Entry points outside the plan: the layer-energy MLP (forward, denoise, sampler, training step, loss, VJP), the fused Adam step, the
// reverse normalisation and its forward map, the convolution precision switch and the per-launch profiler.
#include "plan_internal.h"

#include <cstring>
#include <vector>

extern "C" {

int cd_adam_step(int n, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                 const int64_t* numel, double lr, double beta1, double beta2, float eps, float weight_decay, int step, void* stream) {
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

int cd_reverse_norm(const float* voxels, const float* energy, const float* layerE, float* out, int batch, const int32_t dims[3],
                    const float consts[6], float max_deposit, float ecut, void* stream) {
  return guarded([&] {
    CD_REQUIRE(voxels && energy && out && dims && consts && batch > 0, "bad argument");
    ReverseNormArgs a;
    a.voxels = voxels; a.energy = energy; a.layerE = layerE; a.out = out; a.batch = batch;
    a.D = dims[0]; a.H = dims[1]; a.W = dims[2]; a.layer_mode = layerE ? 1 : 0;
    a.logit_mean = consts[0]; a.logit_std = consts[1]; a.totalE_mean = consts[2]; a.totalE_std = consts[3];
    a.layers_mean = consts[4]; a.layers_std = consts[5]; a.max_deposit = max_deposit; a.ecut = ecut;
    launch_reverse_norm(a, (hipStream_t)stream);
  });
}

int cd_reverse_norm_staged(const float* voxels, const float* energy, const float* layerE, float* out, int batch,
                           const int32_t dims[3], const float consts[6], float max_deposit, float ecut, float alpha, float layer_eps,
                           int stage, void* stream) {
  return guarded([&] {
    CD_REQUIRE(voxels && out && dims && consts && batch > 0 && stage >= 0 && stage <= 2, "bad argument");
    CD_REQUIRE(stage == 1 || energy, "cd_reverse_norm_staged: stages 0 and 2 scale by the incident energies");
    ReverseNormArgs a;
    a.voxels = voxels; a.energy = energy; a.layerE = stage == 1 ? nullptr : layerE; a.out = out; a.batch = batch;
    a.D = dims[0]; a.H = dims[1]; a.W = dims[2]; a.layer_mode = a.layerE ? 1 : 0;
    a.logit_mean = consts[0]; a.logit_std = consts[1]; a.totalE_mean = consts[2]; a.totalE_std = consts[3];
    a.layers_mean = consts[4]; a.layers_std = consts[5]; a.max_deposit = max_deposit; a.ecut = ecut;
    a.stage = stage; a.alpha = alpha; a.layer_eps = layer_eps;
    launch_reverse_norm(a, (hipStream_t)stream);
  });
}

int cd_preprocess(const float* showers, const float* energy, float* out, float* layerE, float* e_out, int32_t* status, int batch,
                  const int32_t dims[3], const float consts[6], float max_deposit, float emin, float emax, int logE,
                  float shower_scale, void* stream) {
  return guarded([&] {
    CD_REQUIRE(showers && energy && out && e_out && status && dims && consts && batch > 0, "bad argument");
    CD_REQUIRE(dims[0] > 0 && dims[0] <= 4096 && dims[1] > 0 && dims[2] > 0 &&
                   (int64_t)dims[0] * dims[1] * dims[2] <= ((int64_t)1 << 28),
               "cd_preprocess: dims = {layers <= 4096, phi, r}, at most 2^28 voxels per shower");
    CD_REQUIRE(max_deposit > 0.f && shower_scale > 0.f && emax > emin && (!logE || emin > 0.f),
               "cd_preprocess: max_deposit and shower_scale must be positive, emax > emin (> 0 with logE)");
    PreprocessArgs a;
    a.showers = showers; a.energy = energy; a.out = out; a.layerE = layerE; a.e_out = e_out; a.status = status; a.batch = batch;
    a.D = dims[0]; a.H = dims[1]; a.W = dims[2]; a.layer_mode = layerE ? 1 : 0; a.logE = logE ? 1 : 0;
    a.logit_mean = consts[0]; a.logit_std = consts[1]; a.totalE_mean = consts[2]; a.totalE_std = consts[3];
    a.layers_mean = consts[4]; a.layers_std = consts[5]; a.max_deposit = max_deposit; a.emin = emin; a.emax = emax;
    a.scale = shower_scale;
    launch_preprocess(a, (hipStream_t)stream);
  });
}

static void layer_mlp_call(const CdLayerMlpDesc* d, const float* const* weights, int n_weights, int batch, int mode,
                           const float* x, const float* cond, const float* tsig, const float* table, int n_steps,
                           const float* noise, float* out, float* xs, float* x0s, void* stream) {
  CD_REQUIRE(d && weights && x && cond && out && batch > 0, "bad argument");
  CD_REQUIRE(d->struct_size == sizeof(CdLayerMlpDesc), "CdLayerMlpDesc.struct_size does not match this library's calodiff.h");
  CD_REQUIRE(d->n_res >= 0 && d->n_res <= 8 && n_weights == 2 * (8 + 3 * d->n_res),
             "layer MLP: n_weights must be 2*(8 + 3*n_res) (time_mlp, cond_mlp, in_lay, blocks, out_lay)");
  CD_REQUIRE(d->time_embed_kind >= 0 && d->time_embed_kind <= 2 && d->objective >= 0 && d->objective <= 2, "bad descriptor");
  LayerMlpArgs a{};
  for (int i = 0; i < n_weights; ++i) {
    CD_REQUIRE(weights[i], "null weight pointer");
    a.w[i] = weights[i];
  }
  a.dim_in = d->dim_in; a.hidden = d->hidden; a.cond_emb = d->cond_emb; a.cond_size = d->cond_size; a.n_res = d->n_res;
  a.time_kind = d->time_embed_kind; a.objective = d->objective; a.mode = mode; a.batch = batch; a.n_steps = n_steps;
  a.sigma_data = d->sigma_data;
  a.x = x; a.cond = cond; a.tsig = tsig; a.table = table; a.noise = noise; a.out = out; a.xs = xs; a.x0s = x0s;
  launch_layer_mlp(a, (hipStream_t)stream);
}

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
    const CdLayerMlpDesc* d = desc;
    CD_REQUIRE(d && weights && start && cond && ops_dev && coefs_dev && x_out && batch > 0, "bad argument");
    CD_REQUIRE(d->struct_size == sizeof(CdLayerMlpDesc), "CdLayerMlpDesc.struct_size does not match this library's calodiff.h");
    CD_REQUIRE(d->n_res >= 0 && d->n_res <= 8 && n_weights == 2 * (8 + 3 * d->n_res),
               "layer MLP: n_weights must be 2*(8 + 3*n_res) (time_mlp, cond_mlp, in_lay, blocks, out_lay)");
    CD_REQUIRE(d->time_embed_kind >= 0 && d->time_embed_kind <= 2 && d->objective >= 0 && d->objective <= 2, "bad descriptor");
    CD_REQUIRE(n_bufs >= 2 && n_bufs <= LAYER_PROG_MAX_BUFS && n_steps >= 1 && n_steps <= 1 << 20 && n_ops >= 1 && n_coef >= 1,
               "bad program size (2..10 buffers)");
    hipStream_t s = (hipStream_t)stream;
    // validate the program before anything is enqueued: an index out of range would address outside the on-chip buffers
    std::vector<CdSamplerOp> ops((size_t)n_ops);
    std::vector<int32_t> begin(op_begin_dev ? (size_t)n_steps + 1 : 0);
    CD_HIP(hipMemcpyAsync(ops.data(), ops_dev, sizeof(CdSamplerOp) * ops.size(), hipMemcpyDeviceToHost, s));
    if (op_begin_dev) CD_HIP(hipMemcpyAsync(begin.data(), op_begin_dev, sizeof(int32_t) * begin.size(), hipMemcpyDeviceToHost, s));
    CD_HIP(hipStreamSynchronize(s));
    if (op_begin_dev) {
      CD_REQUIRE(begin[0] == 0 && begin[n_steps] == n_ops, "op_begin must run from 0 to n_ops");
      for (int i = 0; i < n_steps; ++i) CD_REQUIRE(begin[i] <= begin[i + 1], "op_begin must be non-decreasing");
    }
    int64_t n_denoise = 0;
    for (int k = 0; k < n_ops; ++k) {
      const CdSamplerOp& o = ops[k];
      CD_REQUIRE(o.kind >= CD_SOP_LINCOMB && o.kind <= CD_SOP_DENOISE_PS, "sampler op: unknown kind");
      const bool lin = o.kind == CD_SOP_LINCOMB || o.kind == CD_SOP_LINDIV;
      const int ns = lin ? o.nsrc : (o.kind == CD_SOP_RANDN ? 0 : 1);
      CD_REQUIRE(ns >= 0 && ns <= 6 && (!lin || ns >= 1), "sampler op: 1..6 sources");
      for (int j = 0; j < ns; ++j) CD_REQUIRE(o.src[j] >= 0 && o.src[j] < n_bufs, "sampler op: source buffer out of range");
      if (o.kind == CD_SOP_RECORD) CD_REQUIRE(o.dst == 0 || o.dst == 1, "record op: dst is 0 (xs) or 1 (x0s)");
      else CD_REQUIRE(o.dst >= 0 && o.dst < n_bufs, "sampler op: destination buffer out of range");
      if (lin) CD_REQUIRE(o.col >= 0 && o.col + ns + (o.kind == CD_SOP_LINDIV ? 1 : 0) <= n_coef, "lincomb op: coefficient columns out of range");
      if (o.kind == CD_SOP_DENOISE || o.kind == CD_SOP_DENOISE_PS) {
        if (o.kind == CD_SOP_DENOISE) CD_REQUIRE(o.col >= 0 && o.col < n_coef, "denoise op: sigma column out of range");
        else CD_REQUIRE(o.col >= 0 && o.col + batch <= n_coef, "per-sample denoise op: sigma columns out of range (col + batch > n_coef)");
        CD_REQUIRE(o.dst != o.src[0], "denoise op: output must not alias its input");
        // DENOISE ops executed: once per step of a uniform program, once otherwise
        n_denoise += op_begin_dev ? 1 : n_steps;
      }
    }
    LayerProgArgs a{};
    for (int i = 0; i < n_weights; ++i) {
      CD_REQUIRE(weights[i], "null weight pointer");
      a.w[i] = weights[i];
    }
    a.dim_in = d->dim_in; a.hidden = d->hidden; a.cond_emb = d->cond_emb; a.cond_size = d->cond_size; a.n_res = d->n_res;
    a.time_kind = d->time_embed_kind; a.objective = d->objective; a.batch = batch; a.sigma_data = d->sigma_data;
    a.start = start; a.start_scale = start_scale; a.cond = cond;
    a.n_bufs = n_bufs; a.n_steps = n_steps; a.n_ops = n_ops; a.n_coef = n_coef;
    a.ops = ops_dev; a.op_begin = op_begin_dev; a.coefs = coefs_dev; a.step_noise = step_noise;
    a.seed = seed; a.offset = offset; a.stride = noise_stride ? noise_stride : (uint64_t)batch * (uint64_t)d->dim_in;
    a.out = x_out; a.xs = xs; a.x0s = x0s;
    launch_layer_program(a, n_denoise, s);
  });
}

static LayerMlpTrainArgs layer_train_args(const CdLayerMlpDesc* d, int batch) {
  CD_REQUIRE(d && batch > 0, "bad argument");
  CD_REQUIRE(d->struct_size == sizeof(CdLayerMlpDesc), "CdLayerMlpDesc.struct_size does not match this library's calodiff.h");
  CD_REQUIRE(d->n_res >= 0 && d->n_res <= 8 && d->time_embed_kind >= 0 && d->time_embed_kind <= 2 && d->objective >= 0 &&
                 d->objective <= 2,
             "bad descriptor");
  LayerMlpTrainArgs a{};
  a.dim_in = d->dim_in; a.hidden = d->hidden; a.cond_emb = d->cond_emb; a.cond_size = d->cond_size; a.n_res = d->n_res;
  a.time_kind = d->time_embed_kind; a.objective = d->objective; a.batch = batch; a.sigma_data = d->sigma_data;
  a.layout = layer_tape_layout(a.dim_in, a.hidden, a.cond_emb, a.cond_size, a.n_res);
  return a;
}
static void layer_train_weights(LayerMlpTrainArgs& a, const CdLayerMlpDesc* desc, const float* const* weights, int n_weights) {
  CD_REQUIRE(n_weights == 2 * (8 + 3 * desc->n_res), "layer MLP: n_weights must be 2*(8 + 3*n_res)");
  for (int i = 0; i < n_weights; ++i) {
    CD_REQUIRE(weights[i], "null weight pointer");
    a.w[i] = weights[i];
  }
}
int cd_layer_train_workspace_bytes(const CdLayerMlpDesc* desc, int batch, size_t* bytes) {
  return guarded([&] {
    CD_REQUIRE(bytes, "bad argument");
    *bytes = layer_train_workspace_bytes(layer_train_args(desc, batch));
  });
}
int cd_layer_train_step(const CdLayerMlpDesc* desc, const float* const* weights, int n_weights, int batch, const float* data,
                        const float* noise, const float* sigma, const float* cond, double* loss_out, float* grads,
                        void* workspace, size_t workspace_bytes, void* stream) {
  return cd_layer_train_step_loss(desc, weights, n_weights, batch, data, noise, sigma, cond, CD_LOSS_L2, loss_out, grads, workspace,
                                  workspace_bytes, stream);
}

// the training step (grads) or the loss alone (grads == null) of the descriptor's objective
static void layer_loss_call(const CdLayerMlpDesc* desc, const float* const* weights, int n_weights, int batch, const float* data,
                            const float* noise, const float* sigma, const float* cond, int loss_type, double* loss_out,
                            float* grads, void* workspace, size_t workspace_bytes, void* stream) {
  CD_REQUIRE(weights && data && noise && sigma && cond && loss_out && workspace, "bad argument");
  CD_REQUIRE(loss_type >= CD_LOSS_L2 && loss_type <= CD_LOSS_HUBER, "loss_type must be one of CD_LOSS_L2 / L1 / MSE / HUBER");
  LayerMlpTrainArgs a = layer_train_args(desc, batch);
  a.loss_type = loss_type;
  layer_train_weights(a, desc, weights, n_weights);
  CD_REQUIRE(workspace_bytes >= layer_train_workspace_bytes(a), "workspace too small: call cd_layer_train_workspace_bytes");
  a.data = data; a.noise = noise; a.sigma = sigma; a.cond = cond;
  launch_layer_mlp_train(a, grads, loss_out, workspace, (hipStream_t)stream);
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
    *bytes = layer_vjp_workspace_bytes(layer_train_args(desc, batch), with_param_grads != 0);
  });
}
int cd_layer_denoise_vjp(const CdLayerMlpDesc* desc, const float* const* weights, int n_weights, int batch, const float* x,
                         const float* sigma, const float* cond, const float* gy, float* dx, float* grads, void* workspace,
                         size_t workspace_bytes, void* stream) {
  return guarded([&] {
    CD_REQUIRE(weights && x && sigma && cond && gy && dx && workspace, "bad argument");
    LayerMlpTrainArgs a = layer_train_args(desc, batch);
    layer_train_weights(a, desc, weights, n_weights);
    CD_REQUIRE(workspace_bytes >= layer_vjp_workspace_bytes(a, grads != nullptr),
               "workspace too small: call cd_layer_vjp_workspace_bytes");
    a.x = x; a.gy = gy; a.dx = dx; a.sigma = sigma; a.cond = cond;
    launch_layer_mlp_vjp(a, grads, workspace, (hipStream_t)stream);
  });
}

int cd_set_conv_precision(const char* mode) {
  return guarded([&] {
    CD_REQUIRE(mode, "null argument");
    if (!std::strcmp(mode, "f16x2")) set_conv_precision(PREC_F16X2);
    else if (!std::strcmp(mode, "bf16x3")) set_conv_precision(PREC_BF16X3);
    else if (!std::strcmp(mode, "f32")) set_conv_precision(PREC_F32);
    else throw Fail{CD_EINVAL, std::string("unknown convolution precision '") + mode + "' (f16x2, bf16x3, f32)"};
  });
}
const char* cd_get_conv_precision(void) {
  static const char* names[3] = {"f16x2", "bf16x3", "f32"};
  return names[conv_precision()];
}

int cd_profile_begin(void) {
  return guarded([&] { prof::begin(); });
}
int cd_profile_end(char* json, int cap) {
  return guarded([&] {
    CD_REQUIRE(json && cap > 2, "bad argument");
    if (prof::end(json, cap) < 0) throw Fail{CD_EINVAL, "profile buffer too small"};
  });
}

}  // extern "C"
