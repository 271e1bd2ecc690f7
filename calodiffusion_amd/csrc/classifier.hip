// Classifier two-sample test, host side (include/calodiff.h, "classifier two-sample test"): the entry points that chain the
// kernels of kernels_classifier.hip into the reference's evaluation pass, training step and epoch
// (calodiffusion/tests/hgcal_metrics.py:45-123, 185-209).
#include "guarded.h"
#include "kernels_classifier.h"

#include <cmath>
#include <vector>

namespace cd {
namespace {

struct ClsNet {
  int d, h, layers;  // layers = num_layer + 1 Linear -> LeakyReLU -> Dropout blocks, then the output layer
  float slope, p;
  int tensors() const { return 2 * layers + 2; }
  // parameter order: inputlayer.weight, .bias, outputlayer.weight, .bias, then weight and bias of every hidden Linear
  int w_of(int l) const { return l == 0 ? 0 : 2 + 2 * l; }
  int b_of(int l) const { return w_of(l) + 1; }
  int in_of(int l) const { return l == 0 ? d : h; }
  int64_t numel(int tensor) const {
    if (tensor == 0) return (int64_t)h * d;
    if (tensor == 2) return h;
    if (tensor == 3) return 1;
    return tensor % 2 ? h : (int64_t)h * h;
  }
  int64_t offset(int tensor) const {
    int64_t o = 0;
    for (int i = 0; i < tensor; ++i) o += numel(i);
    return o;
  }
};

ClsNet net_of(const CdClassifierDesc* desc, const char* who) {
  const std::string w(who);
  CD_REQUIRE(desc, w + ": desc must not be null");
  CD_REQUIRE(desc->struct_size == sizeof(CdClassifierDesc), w + ": desc->struct_size is " + std::to_string(desc->struct_size) + ", this library's CdClassifierDesc has " +
                                                                std::to_string(sizeof(CdClassifierDesc)) + " bytes");
  CD_REQUIRE(desc->input_dim >= 1 && desc->input_dim <= CD_CLS_MAX_DIM && desc->hidden >= 1 && desc->hidden <= CD_CLS_MAX_DIM,
             w + ": input_dim and hidden must be in [1, " + std::to_string(CD_CLS_MAX_DIM) + "], got " + std::to_string(desc->input_dim) + " and " +
                 std::to_string(desc->hidden));
  CD_REQUIRE(desc->num_layer >= 0 && desc->num_layer <= CD_CLS_MAX_LAYERS,
             w + ": num_layer must be in [0, " + std::to_string(CD_CLS_MAX_LAYERS) + "], got " + std::to_string(desc->num_layer));
  CD_REQUIRE(desc->negative_slope >= 0.f && std::isfinite(desc->negative_slope),
             w + ": negative_slope must be finite and not negative (the backward pass reads the activation's derivative off its output)");
  CD_REQUIRE(desc->dropout_p >= 0.f && desc->dropout_p < 1.f, w + ": dropout_p must be in [0, 1)");
  return ClsNet{desc->input_dim, desc->hidden, desc->num_layer + 1, desc->negative_slope, desc->dropout_p};
}

// the workspace of `rows` rows, in floats
struct ClsSpace {
  float *xb, *yb, *z, *dz, *g, *dy;
  float* act[CD_CLS_MAX_LAYERS + 1];
  size_t bytes;
};

ClsSpace carve(const ClsNet& n, int rows, void* base) {
  ClsSpace sp{};
  size_t at = 0;
  auto take = [&](size_t floats) {
    float* p = base ? reinterpret_cast<float*>(static_cast<char*>(base) + at) : nullptr;
    at += (floats * sizeof(float) + 255) & ~(size_t)255;
    return p;
  };
  sp.xb = take((size_t)rows * n.d);
  sp.yb = take(rows);
  sp.z = take(rows);
  sp.dz = take(rows);
  sp.g = take((size_t)rows * n.h);
  sp.dy = take((size_t)rows * n.h);
  for (int l = 0; l < n.layers; ++l) sp.act[l] = take((size_t)rows * n.h);
  sp.bytes = at;
  return sp;
}

ClsSpace space_of(const ClsNet& n, int rows, void* workspace, size_t workspace_bytes, const char* who) {
  CD_REQUIRE(workspace && ((uintptr_t)workspace & 255) == 0, std::string(who) + ": workspace must not be null and must be 256-byte aligned");
  const ClsSpace sp = carve(n, rows, workspace);
  CD_REQUIRE(workspace_bytes >= sp.bytes, std::string(who) + ": workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(rows) +
                                              " rows need " + std::to_string(sp.bytes) + " (cd_classifier_workspace_bytes)");
  return sp;
}

void require_weights(const ClsNet& n, const float* const* weights, const char* who) {
  CD_REQUIRE(weights, std::string(who) + ": weights must not be null");
  for (int i = 0; i < n.tensors(); ++i) CD_REQUIRE(weights[i], std::string(who) + ": weights[" + std::to_string(i) + "] is null");
}

// eval mode over `count` rows (count <= the rows `sp` was carved for): logits [count]
void forward_rows(const ClsNet& n, const float* const* w, const float* x, int count, const ClsSpace& sp, float* logits, hipStream_t s) {
  const ClsDropout none{};
  const float* in = x;
  for (int l = 0; l < n.layers; ++l) {
    float* out = l % 2 ? sp.dy : sp.g;
    launch_cls_linear(in, w[n.w_of(l)], w[n.b_of(l)], out, count, n.in_of(l), n.h, 1, n.slope, none, s);
    in = out;
  }
  launch_cls_rowdot(in, w[2], w[3], logits, count, n.h, s);
}

struct ClsAdam {
  float *m, *v;
  double lr, beta1, beta2;
  float eps;
};

// one training step on the rows idx[0 .. batch): gradients into `grads`, the loss into *loss; Adam with step number adam_step (>= 1) if `adam`
void train_one(const ClsNet& n, float* const* w, const float* x, const float* labels, int64_t rows_total, const int32_t* idx, int batch,
               uint64_t seed, uint64_t step, float* grads, double* loss, const ClsAdam* adam, int adam_step, const ClsSpace& sp, hipStream_t s) {
  launch_cls_gather(x, labels, rows_total, idx, batch, n.d, sp.xb, sp.yb, s);
  const float* in = sp.xb;
  for (int l = 0; l < n.layers; ++l) {
    launch_cls_linear(in, w[n.w_of(l)], w[n.b_of(l)], sp.act[l], batch, n.in_of(l), n.h, 1, n.slope, cls_dropout(n.p, seed, step, l), s);
    in = sp.act[l];
  }
  launch_cls_rowdot(in, w[2], w[3], sp.z, batch, n.h, s);
  launch_cls_loss(sp.z, sp.yb, batch, loss, sp.dz, grads + n.offset(3), s);
  for (int l = n.layers - 1; l >= 0; --l) {
    const bool last = l == n.layers - 1;
    launch_cls_gate(last ? nullptr : sp.dy, sp.dz, w[2], last ? grads + n.offset(2) : nullptr, sp.act[l], nullptr, 1, n.slope,
                    cls_dropout(n.p, seed, step, l), sp.g, grads + n.offset(n.b_of(l)), batch, n.h, s);
    launch_cls_wgrad(sp.g, l == 0 ? sp.xb : sp.act[l - 1], grads + n.offset(n.w_of(l)), batch, n.in_of(l), n.h, s);
    if (l > 0) launch_cls_dgrad(sp.g, w[n.w_of(l)], sp.dy, batch, n.h, n.h, s);
  }
  if (adam) {
    const int nt = n.tensors();
    std::vector<float*> p(nt), m(nt), v(nt);
    std::vector<const float*> g(nt);
    std::vector<int64_t> numel(nt);
    for (int i = 0; i < nt; ++i) {
      const int64_t o = n.offset(i);
      p[i] = w[i]; g[i] = grads + o; m[i] = adam->m + o; v[i] = adam->v + o; numel[i] = n.numel(i);
    }
    const int rc = cd_adam_step(nt, p.data(), g.data(), m.data(), v.data(), numel.data(), adam->lr, adam->beta1, adam->beta2, adam->eps, 0.f,
                                adam_step, (void*)s);
    if (rc != CD_OK) throw Fail{rc, std::string("cd_adam_step: ") + cd_last_error()};
  }
}

void require_train_io(const char* who, const float* x, const float* labels, int64_t rows_total, const int32_t* idx, const float* grads) {
  CD_REQUIRE(x && labels && idx && grads, std::string(who) + ": x, labels, the index list and grads must not be null");
  CD_REQUIRE(rows_total >= 1, std::string(who) + ": rows_total must be positive, got " + std::to_string(rows_total));
}

}  // namespace
}  // namespace cd

extern "C" {

int cd_classifier_num_params(const CdClassifierDesc* desc, int64_t* numel) {
  return guarded([&] {
    const ClsNet n = net_of(desc, "cd_classifier_num_params");
    CD_REQUIRE(numel, "cd_classifier_num_params: numel must not be null");
    *numel = n.offset(n.tensors());
  });
}

int cd_classifier_workspace_bytes(const CdClassifierDesc* desc, int max_rows_per_call, size_t* bytes) {
  return guarded([&] {
    const ClsNet n = net_of(desc, "cd_classifier_workspace_bytes");
    CD_REQUIRE(bytes, "cd_classifier_workspace_bytes: bytes must not be null");
    CD_REQUIRE(max_rows_per_call >= 1 && max_rows_per_call <= CD_CLS_MAX_ROWS_PER_CALL,
               "cd_classifier_workspace_bytes: max_rows_per_call must be in [1, " + std::to_string(CD_CLS_MAX_ROWS_PER_CALL) + "], got " +
                   std::to_string(max_rows_per_call));
    *bytes = carve(n, max_rows_per_call, nullptr).bytes;
  });
}

int cd_classifier_forward(const CdClassifierDesc* desc, const float* const* weights, const float* x, int64_t rows_total, const int32_t* idx,
                          int64_t count, float* logits, int max_rows_per_call, void* workspace, size_t workspace_bytes, void* stream) {
  return guarded([&] {
    const ClsNet n = net_of(desc, "cd_classifier_forward");
    require_weights(n, weights, "cd_classifier_forward");
    CD_REQUIRE(x && logits, "cd_classifier_forward: x and logits must not be null");
    CD_REQUIRE(rows_total >= 1 && count >= 0 && (idx || count <= rows_total),
               "cd_classifier_forward: needs rows_total >= 1 and, without an index list, 0 <= count <= rows_total; got " + std::to_string(rows_total) +
                   " and " + std::to_string(count));
    CD_REQUIRE(max_rows_per_call >= 1 && max_rows_per_call <= CD_CLS_MAX_ROWS_PER_CALL,
               "cd_classifier_forward: max_rows_per_call must be in [1, " + std::to_string(CD_CLS_MAX_ROWS_PER_CALL) + "]");
    const ClsSpace sp = space_of(n, max_rows_per_call, workspace, workspace_bytes, "cd_classifier_forward");
    hipStream_t s = (hipStream_t)stream;
    for (int64_t lo = 0; lo < count; lo += max_rows_per_call) {
      const int part = (int)(count - lo < max_rows_per_call ? count - lo : max_rows_per_call);
      const float* in = x + lo * n.d;
      if (idx) {
        launch_cls_gather(x, nullptr, rows_total, idx + lo, part, n.d, sp.xb, nullptr, s);
        in = sp.xb;
      }
      forward_rows(n, weights, in, part, sp, logits + lo, s);
    }
  });
}

int cd_classifier_train_step(const CdClassifierDesc* desc, float* const* weights, const float* x, const float* labels, int64_t rows_total,
                             const int32_t* batch_idx, int batch, uint64_t seed, uint64_t step, float* grads, double* loss, int apply_adam,
                             float* exp_avg, float* exp_avg_sq, double lr, double beta1, double beta2, float eps, int adam_step, void* workspace,
                             size_t workspace_bytes, void* stream) {
  return guarded([&] {
    const ClsNet n = net_of(desc, "cd_classifier_train_step");
    require_weights(n, weights, "cd_classifier_train_step");
    require_train_io("cd_classifier_train_step", x, labels, rows_total, batch_idx, grads);
    CD_REQUIRE(loss, "cd_classifier_train_step: loss must not be null");
    CD_REQUIRE(batch >= 1 && batch <= CD_CLS_MAX_BATCH,
               "cd_classifier_train_step: batch must be in [1, " + std::to_string(CD_CLS_MAX_BATCH) + "], got " + std::to_string(batch));
    CD_REQUIRE(!apply_adam || (exp_avg && exp_avg_sq && adam_step >= 1), "cd_classifier_train_step: Adam needs exp_avg, exp_avg_sq and adam_step >= 1");
    const ClsSpace sp = space_of(n, batch, workspace, workspace_bytes, "cd_classifier_train_step");
    const ClsAdam adam{exp_avg, exp_avg_sq, lr, beta1, beta2, eps};
    train_one(n, weights, x, labels, rows_total, batch_idx, batch, seed, step, grads, loss, apply_adam ? &adam : nullptr, adam_step, sp,
              (hipStream_t)stream);
  });
}

int cd_classifier_train_epoch(const CdClassifierDesc* desc, float* const* weights, const float* x, const float* labels, int64_t rows_total,
                              const int32_t* perm, int64_t n_train, int batch_size, uint64_t seed, uint64_t first_step, float* grads,
                              float* exp_avg, float* exp_avg_sq, double lr, double beta1, double beta2, float eps, double* losses, void* workspace,
                              size_t workspace_bytes, void* stream) {
  return guarded([&] {
    const ClsNet n = net_of(desc, "cd_classifier_train_epoch");
    require_weights(n, weights, "cd_classifier_train_epoch");
    require_train_io("cd_classifier_train_epoch", x, labels, rows_total, perm, grads);
    CD_REQUIRE(losses && exp_avg && exp_avg_sq, "cd_classifier_train_epoch: losses, exp_avg and exp_avg_sq must not be null");
    CD_REQUIRE(n_train >= 1, "cd_classifier_train_epoch: n_train must be positive, got " + std::to_string(n_train));
    CD_REQUIRE(batch_size >= 1 && batch_size <= CD_CLS_MAX_BATCH,
               "cd_classifier_train_epoch: batch_size must be in [1, " + std::to_string(CD_CLS_MAX_BATCH) + "], got " + std::to_string(batch_size));
    const int64_t steps = (n_train + batch_size - 1) / batch_size;
    CD_REQUIRE(first_step + (uint64_t)steps < (uint64_t)INT32_MAX, "cd_classifier_train_epoch: the Adam step number must stay below 2^31 - 1");
    const ClsSpace sp = space_of(n, batch_size, workspace, workspace_bytes, "cd_classifier_train_epoch");
    const ClsAdam adam{exp_avg, exp_avg_sq, lr, beta1, beta2, eps};
    for (int64_t k = 0; k < steps; ++k) {
      const int64_t lo = k * batch_size;
      const int batch = (int)(n_train - lo < batch_size ? n_train - lo : batch_size);  // the last batch is ragged
      train_one(n, weights, x, labels, rows_total, perm + lo, batch, seed, first_step + (uint64_t)k, grads, losses + k, &adam,
                (int)(first_step + (uint64_t)k + 1), sp, (hipStream_t)stream);
    }
  });
}

int cd_classifier_dropout_mask(uint64_t seed, uint64_t step, int layer, float dropout_p, int rows, int n, uint8_t* mask, void* stream) {
  return guarded([&] {
    CD_REQUIRE(mask && rows >= 1 && n >= 1 && layer >= 0, "cd_classifier_dropout_mask: needs a mask, rows >= 1, n >= 1 and layer >= 0");
    CD_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "cd_classifier_dropout_mask: dropout_p must be in [0, 1)");
    launch_cls_mask(cls_dropout(dropout_p, seed, step, layer), rows, n, mask, (hipStream_t)stream);
  });
}

int cd_op_linear_act(const float* x, const float* w, const float* bias, float* y, int rows, int n_in, int n_out, int act, float negative_slope,
                     float dropout_p, uint64_t seed, uint64_t step, int layer, void* stream) {
  return guarded([&] {
    CD_REQUIRE(x && w && y, "cd_op_linear_act: x, w and y must not be null");
    CD_REQUIRE(rows >= 1 && rows <= CD_CLS_MAX_ROWS_PER_CALL && n_in >= 1 && n_in <= CD_CLS_MAX_DIM && n_out >= 1 && n_out <= CD_CLS_MAX_DIM,
               "cd_op_linear_act: needs 1 <= rows <= " + std::to_string(CD_CLS_MAX_ROWS_PER_CALL) + " and n_in, n_out in [1, " +
                   std::to_string(CD_CLS_MAX_DIM) + "]");
    CD_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f && layer >= 0, "cd_op_linear_act: dropout_p must be in [0, 1) and layer >= 0");
    launch_cls_linear(x, w, bias, y, rows, n_in, n_out, act, negative_slope, cls_dropout(dropout_p, seed, step, layer), (hipStream_t)stream);
  });
}

int cd_op_linear_act_backward(const float* x, const float* w, const float* y, const float* dy, const uint8_t* mask, float keep_scale, int act,
                              float negative_slope, float* dx, float* dw, float* db, int rows, int n_in, int n_out, void* workspace,
                              size_t workspace_bytes, void* stream) {
  return guarded([&] {
    CD_REQUIRE(x && w && y && dy && dw && db && workspace, "cd_op_linear_act_backward: x, w, y, dy, dw, db and workspace must not be null");
    CD_REQUIRE(rows >= 1 && rows <= CD_CLS_MAX_BATCH && n_in >= 1 && n_in <= CD_CLS_MAX_DIM && n_out >= 1 && n_out <= CD_CLS_MAX_DIM,
               "cd_op_linear_act_backward: needs 1 <= rows <= " + std::to_string(CD_CLS_MAX_BATCH) + " and n_in, n_out in [1, " +
                   std::to_string(CD_CLS_MAX_DIM) + "]");
    CD_REQUIRE(negative_slope >= 0.f, "cd_op_linear_act_backward: negative_slope must not be negative");
    const size_t need = (size_t)rows * n_out * sizeof(float);
    CD_REQUIRE(((uintptr_t)workspace & 15) == 0 && workspace_bytes >= need,
               "cd_op_linear_act_backward: needs a 16-byte aligned workspace of rows * n_out * 4 = " + std::to_string(need) + " bytes");
    hipStream_t s = (hipStream_t)stream;
    float* g = static_cast<float*>(workspace);
    ClsDropout drop{};
    drop.scale = mask ? keep_scale : 1.f;
    launch_cls_gate(dy, nullptr, nullptr, nullptr, y, mask, act, negative_slope, drop, g, db, rows, n_out, s);
    launch_cls_wgrad(g, x, dw, rows, n_in, n_out, s);
    if (dx) launch_cls_dgrad(g, w, dx, rows, n_in, n_out, s);
  });
}

}  // extern "C"
