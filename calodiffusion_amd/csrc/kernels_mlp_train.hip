// Layer-energy model of LayerDiffusion (the conditional residual MLP "ResNet", reference calodiffusion/models/models.py:373-457)
// with a gradient: its training step (LayerDiffusion.compute_loss in the layer state, models/layerdiffusion.py:52-57, for the
// three objectives of models/loss.py:163-210 and every reduction of Loss._loss, :97-116), the same loss without a backward, and
// the vector-Jacobian product of cd_layer_denoise (calodiffusion.py:154-169 under autograd):
//   x = data + sigma * noise;  D = denoise(x): hybrid c_skip x + c_out F(c_in x, cond, t(sigma)), noise_pred x - sigma F, mean_pred F
//   training: L = sum_b w_b sum_i (pred - target)^2 / (mean(w) B D), seeded with dL/dF;   VJP: seeded with (dD/dF) gy
// One workgroup per sample runs the forward with every pre-activation in LDS, then the explicit chain rule back to the per-layer
// output deltas (for the VJP on through in_lay to dx) in the same launch.  With parameter gradients, inputs and deltas of the
// 20 Linear layers go to a per-sample tape in HBM and linear_wgrad_kernel (kernels_embed_bwd.hip) forms all weight / bias gradients
// (sums over the batch, fixed order => deterministic) in one more launch; its job table is written by the taping kernel itself,
// so nothing here copies from the host or synchronises.  Forward and backward are device functions shared by the kernels.
#include "kernels_mlp.h"
#include "kernels_bwd.h"
#include "kernels_loss.h"

#include <algorithm>
#include <cmath>

namespace cd {

namespace {

__device__ __forceinline__ float tm_gelu(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }
__device__ __forceinline__ float tm_gelu_grad(float x) {
  return 0.5f * (1.f + erff(x * 0.70710678118654752440f)) + x * 0.3989422804014327f * expf(-0.5f * x * x);
}

// pre[j] = bias[j] + sum_k w[j][k] in[k]; a wave owns 8 rows at a time (8 weight rows in flight)
__device__ void tm_dense(const float* __restrict__ w, const float* __restrict__ bias, const float* in, float* pre, int nin,
                         int nout) {
  constexpr int R = 8;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int j0 = wave * R; j0 < nout; j0 += nw * R) {
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
    for (int k = lane; k < nin; k += 64) {
      const float xv = in[k];
      float wv[R];
#pragma unroll
      for (int r = 0; r < R; ++r) wv[r] = w[(size_t)min(j0 + r, nout - 1) * nin + k];
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = fmaf(wv[r], xv, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc[r] += __shfl_xor(acc[r], o, 64);
    }
    if (lane < R && j0 + lane < nout) {
      float v = 0.f;
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (lane == r) v = acc[r];
      pre[j0 + lane] = v + bias[j0 + lane];
    }
  }
  __syncthreads();
}
// din[k] = sum_j w[j][k] dout[j]   (thread per k: coalesced rows, 8 in flight)
__device__ void tm_dense_T(const float* __restrict__ w, const float* dout, float* din, int nin, int nout) {
  for (int k = threadIdx.x; k < nin; k += blockDim.x) {
    float acc = 0.f;
    int j = 0;
    for (; j + 8 <= nout; j += 8) {
      float wv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) wv[u] = w[(size_t)(j + u) * nin + k];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = fmaf(wv[u], dout[j + u], acc);
    }
    for (; j < nout; ++j) acc = fmaf(w[(size_t)j * nin + k], dout[j], acc);
    din[k] = acc;
  }
  __syncthreads();
}

constexpr int TM_MAXV = 256, TM_MAXH = 512, TM_MAXR = 8;

// one workgroup's LDS: the vectors of one sample, every pre-activation of its forward included (54 KiB)
struct LayerSm {
  float xs_[TM_MAXV], x0s[TM_MAXV], vecA[TM_MAXV], vecB[TM_MAXV], cat[TM_MAXV], gcat[TM_MAXV];
  float p1t[TM_MAXV], p2t[TM_MAXV], p1c[TM_MAXV], p2c[TM_MAXV], dg[TM_MAXV], dvec[TM_MAXV];
  float h[TM_MAXH], pu[TM_MAXR][TM_MAXH], pv[TM_MAXR][TM_MAXH], emb[TM_MAXH], tmp[TM_MAXH];
  float dh[TM_MAXH], dtmp[TM_MAXH];
};

// time embedding input and EDM scalings of one sample's sigma (calodiffusion.py:144-169)
struct LayerScal {
  float sigma, t_in, c_in, c_skip, c_out;
};
__device__ __forceinline__ LayerScal layer_scalings(const LayerMlpTrainArgs& a, int b) {
  LayerScal e;
  const float sigma = a.sigma[b], sd = a.sigma_data;
  const float s2 = sigma * sigma + sd * sd;
  e.sigma = sigma;
  e.c_in = 1.f / sqrtf(s2), e.c_skip = sd * sd / s2, e.c_out = sigma * sd / sqrtf(s2);
  e.t_in = a.time_kind == 0 ? 0.5f * logf(sigma) : a.time_kind == 1 ? sigma / sqrtf(1.f + sigma * sigma) : sigma;
  return e;
}

// Forward of sample b.  On entry sm.vecA[0:dim] holds the network input c_in x, published; on return sm.x0s[0:dim] holds the
// network output F, published, and cat / p1t / p2t / p1c / p2c / pu / pv the pre-activations the backward needs.  TAPE: the
// inputs of every Linear except in_lay's (the caller has it) go to the tape row T.
template <bool TAPE>
__device__ __forceinline__ void tm_forward(const LayerMlpTrainArgs& a, LayerSm& sm, int b, float t_in, float* T) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int dim = a.dim_in, Hd = a.hidden, half = a.cond_emb / 2, q = half / 2, R = a.n_res;
  const float* const* W = a.w;
  const LayerTapeLayout& L = a.layout;
  tm_dense(W[12], W[13], sm.vecA, sm.h, dim, Hd);  // in_lay
  // time branch
  if (tid == 0) {
    sm.vecA[0] = t_in;
    if (TAPE) T[L.t_in] = t_in;
  }
  __syncthreads();
  tm_dense(W[0], W[1], sm.vecA, sm.p1t, 1, q);
  for (int i = tid; i < q; i += nt) {
    sm.vecB[i] = tm_gelu(sm.p1t[i]);
    if (TAPE) T[L.a1t + i] = sm.vecB[i];
  }
  __syncthreads();
  tm_dense(W[2], W[3], sm.vecB, sm.p2t, q, half);
  for (int i = tid; i < half; i += nt) {
    sm.vecA[i] = tm_gelu(sm.p2t[i]);
    if (TAPE) T[L.a2t + i] = sm.vecA[i];
  }
  __syncthreads();
  tm_dense(W[4], W[5], sm.vecA, sm.cat + half, half, half);
  // cond branch
  for (int i = tid; i < a.cond_size; i += nt) {
    sm.vecA[i] = a.cond[(size_t)b * a.cond_size + i];
    if (TAPE) T[L.cin + i] = sm.vecA[i];
  }
  __syncthreads();
  tm_dense(W[6], W[7], sm.vecA, sm.p1c, a.cond_size, q);
  for (int i = tid; i < q; i += nt) {
    sm.vecB[i] = tm_gelu(sm.p1c[i]);
    if (TAPE) T[L.a1c + i] = sm.vecB[i];
  }
  __syncthreads();
  tm_dense(W[8], W[9], sm.vecB, sm.p2c, q, half);
  for (int i = tid; i < half; i += nt) {
    sm.vecA[i] = tm_gelu(sm.p2c[i]);
    if (TAPE) T[L.a2c + i] = sm.vecA[i];
  }
  __syncthreads();
  tm_dense(W[10], W[11], sm.vecA, sm.cat, half, half);
  for (int i = tid; i < 2 * half; i += nt) {
    sm.gcat[i] = tm_gelu(sm.cat[i]);
    if (TAPE) T[L.g + i] = sm.gcat[i];
  }
  __syncthreads();
  for (int r = 0; r < R; ++r) {
    const float* const* Lw = W + 14 + 6 * r;
    if (TAPE)
      for (int i = tid; i < Hd; i += nt) T[L.hprev[r] + i] = sm.h[i];
    tm_dense(Lw[0], Lw[1], sm.gcat, sm.emb, 2 * half, Hd);  // embed = Linear(GELU(cond))
    tm_dense(Lw[2], Lw[3], sm.h, sm.pu[r], Hd, Hd);         // u = dense1(h)
    for (int i = tid; i < Hd; i += nt) {
      sm.tmp[i] = tm_gelu(sm.pu[r][i]) + sm.emb[i];
      if (TAPE) T[L.h1[r] + i] = sm.tmp[i];
    }
    __syncthreads();
    tm_dense(Lw[4], Lw[5], sm.tmp, sm.pv[r], Hd, Hd);       // v = dense2(h1)
    for (int i = tid; i < Hd; i += nt) sm.h[i] = tm_gelu(sm.pv[r][i]) + sm.h[i];
    __syncthreads();
  }
  if (TAPE)
    for (int i = tid; i < Hd; i += nt) T[L.hfin + i] = sm.h[i];
  tm_dense(W[14 + 6 * R], W[15 + 6 * R], sm.h, sm.x0s, Hd, dim);  // pred (out_lay)
}

// Backward of sample b from sm.dvec[0:dim] = dL/dF, published.  On return sm.dh[0:hidden] = dL/d(in_lay's output), published.
// TAPE: the output delta of every Linear except out_lay's (the caller has it) goes to the tape row T, which takes the walk on
// through the embedders into the time and cond branches; without it only the trunk is walked: sigma and cond are constants,
// and sm.dh comes out the same bits.
template <bool TAPE>
__device__ __forceinline__ void tm_backward(const LayerMlpTrainArgs& a, LayerSm& sm, float* T) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int dim = a.dim_in, Hd = a.hidden, half = a.cond_emb / 2, q = half / 2, R = a.n_res;
  const float* const* W = a.w;
  const LayerTapeLayout& L = a.layout;
  tm_dense_T(W[14 + 6 * R], sm.dvec, sm.dh, Hd, dim);  // d h_final
  if (TAPE) {
    for (int i = tid; i < 2 * half; i += nt) sm.dg[i] = 0.f;
    __syncthreads();
  }
  for (int r = R - 1; r >= 0; --r) {
    const float* const* Lw = W + 14 + 6 * r;
    for (int i = tid; i < Hd; i += nt) {  // dv
      sm.dtmp[i] = sm.dh[i] * tm_gelu_grad(sm.pv[r][i]);
      if (TAPE) T[L.dv[r] + i] = sm.dtmp[i];
    }
    __syncthreads();
    tm_dense_T(Lw[4], sm.dtmp, sm.tmp, Hd, Hd);  // d h1 (= d embed)
    for (int i = tid; i < Hd; i += nt) {
      if (TAPE) T[L.de[r] + i] = sm.tmp[i];
      sm.dtmp[i] = sm.tmp[i] * tm_gelu_grad(sm.pu[r][i]);  // du
      if (TAPE) T[L.du[r] + i] = sm.dtmp[i];
    }
    __syncthreads();
    if (TAPE) {
      tm_dense_T(Lw[0], sm.tmp, sm.emb, 2 * half, Hd);  // d g += We^T de
      for (int i = tid; i < 2 * half; i += nt) sm.dg[i] += sm.emb[i];
    }
    tm_dense_T(Lw[2], sm.dtmp, sm.tmp, Hd, Hd);            // W1^T du
    for (int i = tid; i < Hd; i += nt) sm.dh[i] += sm.tmp[i];  // residual + dense1 path
    __syncthreads();
  }
  if (!TAPE) return;
  for (int i = tid; i < Hd; i += nt) T[L.dh0 + i] = sm.dh[i];
  // d cat = d g * gelu'(cat): first half = cond branch output, second half = time branch output
  for (int i = tid; i < 2 * half; i += nt) sm.dg[i] *= tm_gelu_grad(sm.cat[i]);
  __syncthreads();
  for (int i = tid; i < half; i += nt) {
    T[L.d3c + i] = sm.dg[i];
    T[L.d3t + i] = sm.dg[half + i];
  }
  tm_dense_T(W[4], sm.dg + half, sm.vecA, half, half);  // time branch
  for (int i = tid; i < half; i += nt) {
    sm.vecA[i] *= tm_gelu_grad(sm.p2t[i]);
    T[L.d2t + i] = sm.vecA[i];
  }
  __syncthreads();
  tm_dense_T(W[2], sm.vecA, sm.vecB, q, half);
  for (int i = tid; i < q; i += nt) T[L.d1t + i] = sm.vecB[i] * tm_gelu_grad(sm.p1t[i]);
  __syncthreads();
  tm_dense_T(W[10], sm.dg, sm.vecA, half, half);  // cond branch
  for (int i = tid; i < half; i += nt) {
    sm.vecA[i] *= tm_gelu_grad(sm.p2c[i]);
    T[L.d2c + i] = sm.vecA[i];
  }
  __syncthreads();
  tm_dense_T(W[8], sm.vecA, sm.vecB, q, half);
  for (int i = tid; i < q; i += nt) T[L.d1c + i] = sm.vecB[i] * tm_gelu_grad(sm.p1c[i]);
}

// linear_wgrad_kernel's job table over the tape: one job per Linear in the order of the flat gradient buffer (state_dict order:
// weight, bias, weight, bias, ...).  Returns the number of jobs (8 + 3 n_res <= 32).
__host__ __device__ inline int layer_wgrad_jobs(const LayerMlpTrainArgs& a, LinearWgradJob* jobs) {
  const LayerTapeLayout& L = a.layout;
  const int half = a.cond_emb / 2, q = half / 2, Hd = a.hidden, D = a.dim_in;
  size_t goff = 0;
  int n = 0;
  auto add = [&](int delta_off, int in_off, int nout, int nin) {
    LinearWgradJob j;
    j.delta = a.tape + delta_off; j.in = a.tape + in_off; j.dw = a.grads + goff; j.db = a.grads + goff + (size_t)nout * nin;
    j.nout = nout; j.nin = nin; j.delta_ld = L.total; j.in_ld = L.total;
    goff += (size_t)nout * nin + nout;
    jobs[n++] = j;
  };
  add(L.d1t, L.t_in, q, 1); add(L.d2t, L.a1t, half, q); add(L.d3t, L.a2t, half, half);          // time_mlp.{1,3,5}
  add(L.d1c, L.cin, q, a.cond_size); add(L.d2c, L.a1c, half, q); add(L.d3c, L.a2c, half, half);  // cond_mlp.{0,2,4}
  add(L.dh0, L.xin, Hd, D);                                                                      // in_lay
  for (int r = 0; r < a.n_res; ++r) {
    add(L.de[r], L.g, Hd, 2 * half);     // embeder.1
    add(L.du[r], L.hprev[r], Hd, Hd);    // dense1.0
    add(L.dv[r], L.h1[r], Hd, Hd);       // dense2.0
  }
  add(L.dpred, L.hfin, D, Hd);           // out_lay
  return n;
}
constexpr int TM_MAXJOBS = 8 + 3 * TM_MAXR;

// d D / d F of the objective (calodiffusion.py:161-169)
__device__ __forceinline__ float objective_chain(int objective, const LayerScal& e) {
  return objective == 0 ? e.c_out : (objective == 1 ? -e.sigma : 1.0f);
}

}  // namespace

// tape row (floats) of one sample: inputs and output deltas of every Linear layer
LayerTapeLayout layer_tape_layout(int dim, int hidden, int cond_emb, int cond_size, int n_res) {
  LayerTapeLayout L;
  const int half = cond_emb / 2, q = half / 2;
  int o = 0;
  auto take = [&](int n) { const int at = o; o += (n + 3) & ~3; return at; };
  L.xin = take(dim); L.t_in = take(1); L.a1t = take(q); L.a2t = take(half); L.cin = take(cond_size); L.a1c = take(q);
  L.a2c = take(half); L.g = take(2 * half);
  for (int r = 0; r < n_res; ++r) { L.hprev[r] = take(hidden); L.h1[r] = take(hidden); }
  L.hfin = take(hidden);
  L.dpred = take(dim);
  for (int r = 0; r < n_res; ++r) { L.dv[r] = take(hidden); L.du[r] = take(hidden); L.de[r] = take(hidden); }
  L.dh0 = take(hidden);
  L.d3t = take(half); L.d2t = take(half); L.d1t = take(q); L.d3c = take(half); L.d2c = take(half); L.d1c = take(q);
  L.total = o;
  return L;
}

// BWD: the training step (tape + chain rule); without it the forward and the loss only, the same bits of the loss
template <bool BWD>
__global__ void __launch_bounds__(512) layer_mlp_train_kernel(LayerMlpTrainArgs a) {
  __shared__ __attribute__((aligned(16))) LayerSm sm;
  __shared__ double sred[8];
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int dim = a.dim_in;
  const LayerTapeLayout& L = a.layout;
  float* T = BWD ? a.tape + (size_t)b * L.total : nullptr;
  if (BWD && b == 0 && tid == 0) layer_wgrad_jobs(a, a.jobs);

  // ---- loss weights: hybrid w_b = 1 + sigma^-2, mean_pred sigma^-2, noise_pred 1; their mean over the batch in a fixed order
  // (every workgroup repeats it) ----------------------------------------------------------------------------------------------
  const int obj = a.objective;
  double wsum = 0.0;
  for (int n = 0; n < a.batch; ++n) wsum += (double)objective_weight(obj, 0, a.sigma[n]);
  const float wmean = (float)(wsum / a.batch);
  const LayerScal e = layer_scalings(a, b);
  const float sigma = e.sigma, c_in = e.c_in, c_skip = e.c_skip, c_out = e.c_out;
  const float wb = objective_weight(obj, 0, sigma);

  // ---- forward ------------------------------------------------------------------------------------------------------------
  for (int i = tid; i < dim; i += nt) {
    const float x = a.data[(size_t)b * dim + i] + sigma * a.noise[(size_t)b * dim + i];
    sm.xs_[i] = x;
    sm.vecA[i] = x * c_in;
    if (BWD) T[L.xin + i] = x * c_in;
  }
  __syncthreads();
  tm_forward<BWD>(a, sm, b, e.t_in, T);

  // ---- loss and d pred ----------------------------------------------------------------------------------------------------
  // the element losses of Loss._loss (models/loss.py:97-116) as in head_loss_bwd_kernel: only 'l2' carries the objective's weight;
  // the torch.nn.functional losses are plain means -- d loss / d pred = gscale f'(d): l2 2 w d / (mean(w) N), mse 2 d / N,
  // l1 sign(d) / N, huber (smooth_l1, beta 1) clamp(d, -1, 1) / N; d = pred - target by objective_residual's table
  const int lt = a.loss_type;
  const float gscale = lt == 0 ? 2.f * wb / (wmean * (float)a.batch * (float)dim) : (lt == 2 ? 2.f : 1.f) / ((float)a.batch * (float)dim);
  const float chain = objective_chain(obj, e);
  double lacc = 0.0;
  for (int i = tid; i < dim; i += nt) {
    float d;
    if (obj == 0) {
      const float x0 = c_skip * sm.xs_[i] + c_out * sm.x0s[i];
      d = x0 - a.data[(size_t)b * dim + i];
    } else {
      const float out = obj == 1 ? sm.xs_[i] - sigma * sm.x0s[i] : sm.x0s[i];
      d = objective_residual(obj, out, a.data[(size_t)b * dim + i], obj == 1 ? a.noise[(size_t)b * dim + i] : 0.f, sigma);
    }
    const float ad = fabsf(d);
    lacc += (double)(lt == 1 ? ad : (lt == 3 ? (ad < 1.f ? 0.5f * d * d : ad - 0.5f) : d * d));
    if (BWD) {
      const float fp = lt == 1 ? (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) : (lt == 3 ? fminf(fmaxf(d, -1.f), 1.f) : d);
      sm.dvec[i] = gscale * fp * chain;
      T[L.dpred + i] = sm.dvec[i];
    }
  }
  for (int o = 32; o > 0; o >>= 1) lacc += __shfl_xor(lacc, o, 64);
  if ((tid & 63) == 0) sred[tid >> 6] = lacc;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < (nt >> 6); ++i) s += sred[i];
    a.loss_part[b] = lt == 0 ? s * (double)wb : s;
  }

  // ---- backward -----------------------------------------------------------------------------------------------------------
  if (BWD) tm_backward<true>(a, sm, T);
}

// dx = dL/dx of D = denoise(x) from gy = dL/dD; TAPE: the tape for the parameter gradients as well
template <bool TAPE>
__global__ void __launch_bounds__(512) layer_mlp_vjp_kernel(LayerMlpTrainArgs a) {
  __shared__ __attribute__((aligned(16))) LayerSm sm;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int dim = a.dim_in;
  const LayerTapeLayout& L = a.layout;
  float* T = TAPE ? a.tape + (size_t)b * L.total : nullptr;
  if (TAPE && b == 0 && tid == 0) layer_wgrad_jobs(a, a.jobs);
  const LayerScal e = layer_scalings(a, b);
  for (int i = tid; i < dim; i += nt) {
    const float x = a.x[(size_t)b * dim + i];
    sm.vecA[i] = x * e.c_in;
    if (TAPE) T[L.xin + i] = x * e.c_in;
  }
  __syncthreads();
  tm_forward<TAPE>(a, sm, b, e.t_in, T);
  // seed: d F = (d D / d F) gy
  const float chain = objective_chain(a.objective, e);
  for (int i = tid; i < dim; i += nt) {
    sm.dvec[i] = chain * a.gy[(size_t)b * dim + i];
    if (TAPE) T[L.dpred + i] = sm.dvec[i];
  }
  __syncthreads();
  tm_backward<TAPE>(a, sm, T);
  // through in_lay and the pre-conditioning: dx = c_in W_in^T dh0 + (dD/dx at fixed F) gy.  (sm.x0s is free: F is not read again)
  tm_dense_T(a.w[12], sm.dh, sm.x0s, dim, a.hidden);
  const float direct = a.objective == 0 ? e.c_skip : (a.objective == 1 ? 1.0f : 0.0f);
  for (int i = tid; i < dim; i += nt) a.dx[(size_t)b * dim + i] = e.c_in * sm.x0s[i] + direct * a.gy[(size_t)b * dim + i];
}

__global__ void layer_loss_final_kernel(const double* __restrict__ part, const float* __restrict__ sigma, int batch, int dim,
                                        double* __restrict__ loss, int loss_type, int objective) {
  if (threadIdx.x || blockIdx.x) return;
  double s = 0.0, w = 0.0;
  for (int n = 0; n < batch; ++n) {
    s += part[n];
    w += (double)objective_weight(objective, 0, sigma[n]);
  }
  const float wmean = loss_type == 0 ? (float)(w / batch) : 1.0f;
  *loss = s / ((double)wmean * (double)batch * (double)dim);
}

namespace {

size_t tape_bytes(const LayerMlpTrainArgs& a) { return ((size_t)a.batch * a.layout.total * 4 + 255) / 256 * 256; }

void require_layer_limits(const LayerMlpTrainArgs& a) {
  CD_REQUIRE(a.dim_in >= 1 && a.dim_in <= TM_MAXV && a.cond_emb >= 4 && a.cond_emb <= TM_MAXV && (a.cond_emb & 3) == 0 &&
                 a.hidden >= 1 && a.hidden <= TM_MAXH && a.cond_size >= 1 && a.cond_size <= TM_MAXV && a.n_res >= 0 &&
                 a.n_res <= TM_MAXR,
             "layer MLP gradients: dim_in / cond_emb / cond_size up to 256, hidden up to 512, at most 8 residual blocks");
}

// multiply-adds of one forward per sample (the profiler's algorithmic work)
double tm_macs(const LayerMlpTrainArgs& a) {
  const double half = a.cond_emb / 2, q = half / 2;
  return q + q * half + half * half + (double)a.dim_in * a.hidden * 2 + a.n_res * ((double)a.cond_emb * a.hidden + 2.0 * a.hidden * a.hidden);
}

// weight / bias gradients of every Linear from the tape: one launch over the job table the taping kernel wrote
void launch_layer_wgrad(const LayerMlpTrainArgs& a, hipStream_t s) {
  LinearWgradJob jobs[TM_MAXJOBS];
  const int n = layer_wgrad_jobs(a, jobs);  // (the host's copy only sizes the grid)
  int max_elems = 1;
  for (int i = 0; i < n; ++i) max_elems = std::max(max_elems, jobs[i].nout * jobs[i].nin);
  const double macs = tm_macs(a);
  prof::Scope scope("linear_wgrad", s, 2.0 * macs * a.batch, 8.0 * (double)a.batch * a.layout.total);
  launch_linear_wgrad(a.jobs, n, max_elems, a.batch, s);
}

}  // namespace

size_t layer_train_workspace_bytes(const LayerMlpTrainArgs& a) {
  return tape_bytes(a) + (size_t)a.batch * 8 + 256 + 64 * sizeof(LinearWgradJob) + 256;
}
size_t layer_vjp_workspace_bytes(const LayerMlpTrainArgs& a, bool with_param_grads) {
  return with_param_grads ? tape_bytes(a) + 64 * sizeof(LinearWgradJob) : 256;
}

// grads: flat buffer with the parameters' numel in state_dict order (weight, bias, weight, bias, ...), or null: loss only
void launch_layer_mlp_train(LayerMlpTrainArgs a, float* grads, double* loss_out, void* workspace, hipStream_t s) {
  require_layer_limits(a);
  char* ws = (char*)workspace;
  a.tape = (float*)ws;
  ws += tape_bytes(a);
  a.loss_part = (double*)ws;
  ws += ((size_t)a.batch * 8 + 255) / 256 * 256;
  a.jobs = (LinearWgradJob*)ws;
  a.grads = grads;
  const double macs = tm_macs(a);
  {
    prof::Scope scope(grads ? "layer_mlp_train" : "layer_mlp_loss", s, (grads ? 4.0 : 2.0) * macs * a.batch, (grads ? 8.0 : 4.0) * macs);
    if (grads) hipLaunchKernelGGL(layer_mlp_train_kernel<true>, dim3(a.batch), dim3(512), 0, s, a);
    else hipLaunchKernelGGL(layer_mlp_train_kernel<false>, dim3(a.batch), dim3(512), 0, s, a);
    CD_HIP(hipGetLastError());
  }
  {
    prof::Scope scope("layer_loss_final", s, 0.0, 12.0 * a.batch);
    hipLaunchKernelGGL(layer_loss_final_kernel, dim3(1), dim3(64), 0, s, a.loss_part, a.sigma, a.batch, a.dim_in, loss_out, a.loss_type,
                       a.objective);
    CD_HIP(hipGetLastError());
  }
  if (grads) launch_layer_wgrad(a, s);
}

void launch_layer_mlp_vjp(LayerMlpTrainArgs a, float* grads, void* workspace, hipStream_t s) {
  require_layer_limits(a);
  a.tape = (float*)workspace;
  a.jobs = (LinearWgradJob*)((char*)workspace + tape_bytes(a));
  a.grads = grads;
  const double macs = tm_macs(a);
  {
    prof::Scope scope("layer_mlp_vjp", s, 4.0 * macs * a.batch, 8.0 * macs);
    if (grads) hipLaunchKernelGGL(layer_mlp_vjp_kernel<true>, dim3(a.batch), dim3(512), 0, s, a);
    else hipLaunchKernelGGL(layer_mlp_vjp_kernel<false>, dim3(a.batch), dim3(512), 0, s, a);
    CD_HIP(hipGetLastError());
  }
  if (grads) launch_layer_wgrad(a, s);
}

}  // namespace cd
