// Backward: everything but the convolutions' weight gradients (kernels_{conv,gn,attn,head,init,embed}_bwd.hip).
#pragma once
#include "cd_common.h"
#include "kernels_conv.h"
#include "kernels_embed_head.h"

namespace cd {

void launch_strided_dgrad_naive(const float* dy, const float* w, float* dx, int batch, int cin, int cout, Dims3 din, Dims3 dout,
                                int kd, int sz, hipStream_t s);
void launch_softmax32(const float* qkv, float* qs, int64_t rows, hipStream_t s);
void launch_softmax32_bwd(const float* qs, const float* dqs, float* dqkv, int64_t rows, hipStream_t s);
void launch_ksoftmax_bwd(const float* qkv, const float* dks, const float* kstat, const float* ctx, const float* dctx, float dscale,
                         float* dqkv, int batch, int64_t vox, hipStream_t s);
void launch_pack_sample32(const float* m, float* wpk, int batch, bool transpose, float scale, hipStream_t s);
void launch_pack_sample32_pair(const float* m, float* wpk_plain, float* wpk_tr, int batch, float scale, hipStream_t s);
int head_bwd_blocks(int batch, int64_t vox);
// loss_type (here and below): CD_LOSS_* of calodiff.h -- 0 l2 (hybrid weight), 1 l1, 2 mse, 3 huber (models/loss.py:97-116)
// objective: CD_OBJ_* (objective_residual / objective_weight, kernels_loss.h); noise is only read for noise_pred
void launch_head_loss_bwd(const float* x0, const float* data, const float* noise, const float* scal, const float* h, const float* wh,
                          float* dh, float* part, float* dwh, float* dbh, int batch, int64_t vox, hipStream_t s, int loss_type = 0,
                          int objective = 0, int res_objective = -1 /* the objective's own */);
// the head's backward from the caller's dL/dD (cd_denoise_vjp): dh always; dWh / dbh only when part != null
void launch_head_vjp(const float* gy, const float* scal, const float* h, const float* wh, float* dh, float* part, float* dwh, float* dbh,
                     int batch, int64_t vox, int objective, hipStream_t s);
// input gradient of the init conv's data channel with the EDM preconditioning: g (B, vox, c0) channels-last, w_raw torch layout
// (c0, cin, 3, 3, 3), scal the (B, 4) scalings {c_in, c_skip, c_out, sigma}; dx, gy (B, 1, D, H, W)
void launch_init_dgrad(const float* g, const float* w_raw, int cin, int c0, const float* gy, const float* scal, int objective, float* dx,
                       int batch, Dims3 dims, hipStream_t s);
struct LinearWgradJob {
  const float* delta;  // (B, delta_ld) rows, nout used
  const float* in;     // (B, in_ld) rows, nin used
  float* dw;           // (nout, nin)
  float* db;           // (nout)
  int nout, nin, delta_ld, in_ld;
};
void launch_linear_wgrad(const LinearWgradJob* jobs_dev, int njobs, int max_elems, int batch, hipStream_t s);
void launch_fold_phi(const float* src, float* dst, int batch, Dims3 d, int C, hipStream_t s);
void launch_add_slices(const float* a, int lda, int aoff, const float* b, int ldb, int boff, float* out, int channels,
                       int64_t rows, hipStream_t s);
void launch_bias_grad(const float* part, int units, int batch, int channels, float* db, bool accumulate, hipStream_t s);
size_t gn_backward_scratch_floats(int batch, int channels, int64_t vox);
// backward of y = act(scale*h + shift) + add: dh, dgamma, dbeta (accumulated if asked), dadd[b][c] (optional)
// Deferred batch reduction of the GroupNorm parameter gradients: one job per layer, passed to the kernel by value
struct GnParamJob {
  const float* sums_bc;  // [batch][channels][4] = {dbeta, dgamma, conv-bias, sum dy} contributions per sample
  float *dgamma, *dbeta, *dbias, *dsumdy;
  int batch, channels;
};
struct GnParamJobs {
  static constexpr int kMax = 64;
  GnParamJob job[kMax];
  int n = 0;
};
struct GnParamQueue {
  GnParamJobs jobs;
  float* sums = nullptr;       // region of the jobs' per-sample sums, kept by the caller until the flush: [sums, sums_end)
  float* sums_end = nullptr;
  float* next_sums = nullptr;  // bump pointer into it (back to `sums` after a flush)
  bool discard = false;        // input gradients only (cd_denoise_vjp without grads): the jobs are never run, a full queue rewinds
};
void launch_gn_param_jobs(const GnParamJobs& jobs, hipStream_t s);
void launch_gn_backward(const float* dy, const float* h, const float* coef, const float* stat, const float* gamma, float* dh,
                        float* dgamma, float* dbeta, float* dadd, int dadd_ld, int batch, int channels, int64_t vox, int groups,
                        int silu, float* scratch, bool accumulate_params, hipStream_t s,
                        // (optional, round 4) the bias gradient of the conv that produced h, and sum_{b,v} dy per channel (the bias
                        // gradient of a conv that adds into y): both fall out of the statistics pass, see kernels_gn_bwd.hip
                        float* dbias = nullptr, float* dsumdy = nullptr,
                        // (optional) queue the batch reduction of the parameter gradients instead of launching it (training step)
                        GnParamQueue* queue = nullptr,
                        // (optional) a zeroed device word that receives max |dh| (bit pattern): the conv gradients that consume dh
                        // rescale by it (WgradAux::gmax, ConvFusion::in_absmax) without a pass of their own
                        unsigned* dh_absmax = nullptr);

size_t init_wgrad_partial_floats(int batch, int64_t vox, int cin, int cout);
void launch_init_wgrad(const InitConvArgs& a, const float* g, float* part, float* dw, hipStream_t s);
// the same through the general weight-gradient kernels (padded 32-channel input); scratch: init_wgrad_mfma_floats floats
size_t init_wgrad_mfma_floats(int batch, int64_t vox, int cout);
void launch_init_wgrad_mfma(const InitConvArgs& a, const float* g, float* scratch, float* dw, hipStream_t s, AbsmaxWords* words);
// per-sample record the embedding backward leaves for the Linear weight gradients
struct EmbedTapeLayout {
  int t_in, a1t, a2t, a1c, a2c, sc;      // inputs of the Linears (time: 1, q, half; cond: cond(copied), hidden, half; proj: 2*half)
  int cond_in;
  int d1t, d2t, d3t, d1c, d2c, d3c;      // deltas at the Linear outputs
  int total;
};
__host__ __device__ inline EmbedTapeLayout embed_tape_layout(int cond_size, int hidden, int half) {
  EmbedTapeLayout L;
  int o = 0;
  const int q = half / 2;
  L.t_in = o; o += 1;
  L.a1t = o; o += q;
  L.a2t = o; o += half;
  L.cond_in = o; o += cond_size;
  L.a1c = o; o += hidden;
  L.a2c = o; o += half;
  L.sc = o; o += 2 * half;
  L.d1t = o; o += q;
  L.d2t = o; o += half;
  L.d3t = o; o += half;
  L.d1c = o; o += hidden;
  L.d2c = o; o += half;
  L.d3c = o; o += half;
  L.total = (o + 3) & ~3;
  return L;
}

size_t embed_tape_floats(int cond_size, int hidden, int half);
void launch_embed_bwd(const EmbedArgs& a, const float* demb, float* tape, hipStream_t s);

}  // namespace cd
