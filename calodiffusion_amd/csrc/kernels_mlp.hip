// Layer-energy model of LayerDiffusion: the conditional residual MLP ("ResNet", reference calodiffusion/models/models.py:373-457)
// with its EDM pre-conditioning (calodiffusion.py:154-169) and the whole DDim/DDPM/Euler trajectory (models/sample.py:40-110) in
// ONE launch.  A (B, D+1) vector per shower is tiny and the samples are independent, so one workgroup owns one sample and walks
// all sampler steps with the state in LDS: no per-step launches, no intermediate in HBM.  The ~0.7 M weights (2.7 MB) stream
// from L2 every step; a wave owns 8 output rows at a time so 8 independent 1-KiB row reads are in flight per wave
// (16 rows x 16 waves measured 3x slower: register pressure).
#include "kernels_mlp.h"
#include "philox.h"
#include "../../include/calodiff.h"

#include <cmath>

namespace cd {

namespace {

__device__ __forceinline__ float mlp_gelu(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }

constexpr int MLP_ROWS = 8;

// out[j] = act(bias[j] + sum_k w[j][k] in[k]) + (post ? post[j] : 0).  `out` may alias `post`, never `in`.
__device__ void mlp_dense(const float* __restrict__ w, const float* __restrict__ bias, const float* in, float* out,
                          const float* post, int nin, int nout, bool gelu) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const bool vec = (nin & 3) == 0;
  for (int j0 = wave * MLP_ROWS; j0 < nout; j0 += nw * MLP_ROWS) {
    float acc[MLP_ROWS];
#pragma unroll
    for (int r = 0; r < MLP_ROWS; ++r) acc[r] = 0.f;
    if (vec) {
      for (int k4 = lane; k4 * 4 < nin; k4 += 64) {
        const f32x4 xv = *(const f32x4*)(in + k4 * 4);
        f32x4 wv[MLP_ROWS];
#pragma unroll
        for (int r = 0; r < MLP_ROWS; ++r) {
          const int j = j0 + r < nout ? j0 + r : nout - 1;  // clamped: the load stays unconditional, the row is dropped below
          wv[r] = *(const f32x4*)(w + (size_t)j * nin + k4 * 4);
        }
#pragma unroll
        for (int r = 0; r < MLP_ROWS; ++r)
          acc[r] = fmaf(wv[r][3], xv[3], fmaf(wv[r][2], xv[2], fmaf(wv[r][1], xv[1], fmaf(wv[r][0], xv[0], acc[r]))));
      }
    } else {
      for (int k = lane; k < nin; k += 64) {
        const float xv = in[k];
#pragma unroll
        for (int r = 0; r < MLP_ROWS; ++r) {
          const int j = j0 + r < nout ? j0 + r : nout - 1;
          acc[r] = fmaf(w[(size_t)j * nin + k], xv, acc[r]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < MLP_ROWS; ++r) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc[r] += __shfl_xor(acc[r], o, 64);
    }
    if (lane < MLP_ROWS && j0 + lane < nout) {
      float v = 0.f;
#pragma unroll
      for (int r = 0; r < MLP_ROWS; ++r)
        if (lane == r) v = acc[r];
      v += bias[j0 + lane];
      if (gelu) v = mlp_gelu(v);
      if (post) v += post[j0 + lane];
      out[j0 + lane] = v;
    }
  }
  __syncthreads();
}

constexpr int MLP_MAXV = 256;  // dim_in, cond_emb
constexpr int MLP_MAXH = 512;  // hidden

// time embedding input and EDM scalings of sigma (calodiffusion.py:144-169)
struct EdmScal {
  float t_in, c_in, c_skip, c_out;
};
__device__ __forceinline__ EdmScal edm_scalings(float sigma, float sd, int time_kind) {
  EdmScal e;
  e.t_in = time_kind == 0 ? 0.5f * logf(sigma) : time_kind == 1 ? sigma / sqrtf(1.f + sigma * sigma) : sigma;
  const float s2 = sigma * sigma + sd * sd;
  e.c_in = 1.f / sqrtf(s2);
  e.c_skip = sd * sd / s2;
  e.c_out = sigma * sd / sqrtf(s2);
  return e;
}

// the objective's x0 from the state x and the network output p (0 hybrid, 1 noise_pred, 2 mean_pred)
__device__ __forceinline__ float edm_x0(int objective, float xv, float p, float sigma, const EdmScal& e) {
  float x0 = p;  // mean_pred
  if (objective == 0) x0 = e.c_skip * xv + e.c_out * p;
  else if (objective == 1) x0 = xv - sigma * p;
  return x0;
}

// cond branch (constant over a trajectory): Linear(cond_size, q) GELU Linear(q, half) GELU Linear(half, half) -> cat[0:half].
// tb0 holds the condition on entry; tb0 / tb1 are scratch.
__device__ __forceinline__ void mlp_cond_branch(const float* const* W, int cond_size, int q, int half, float* tb0, float* tb1,
                                                float* cat) {
  mlp_dense(W[6], W[7], tb0, tb1, nullptr, cond_size, q, true);
  mlp_dense(W[8], W[9], tb1, tb0, nullptr, q, half, true);
  mlp_dense(W[10], W[11], tb0, cat, nullptr, half, half, false);
}

// time branch and trunk: tb0[0] = the time input and xin = the network input, both published; cat[0:half] = the cond branch.
// -> pred (dim), published.
__device__ __forceinline__ void mlp_time_and_trunk(const float* const* W, int dim, int hidden, int q, int half, int n_res,
                                                   float* tb0, float* tb1, float* cat, float* gcat, const float* xin, float* h0,
                                                   float* h1, float* emb, float* pred) {
  const int tid = threadIdx.x;
  // time branch: Unflatten, Linear(1, q) GELU Linear(q, half) GELU Linear(half, half) -> cat[half:2 half]
  mlp_dense(W[0], W[1], tb0, tb1, nullptr, 1, q, true);
  mlp_dense(W[2], W[3], tb1, tb0, nullptr, q, half, true);
  mlp_dense(W[4], W[5], tb0, cat + half, nullptr, half, half, false);
  for (int i = tid; i < 2 * half; i += blockDim.x) gcat[i] = mlp_gelu(cat[i]);  // ResDense.embeder[0]
  mlp_dense(W[12], W[13], xin, h0, nullptr, dim, hidden, false);  // in_lay (its barrier also publishes gcat)
  for (int r = 0; r < n_res; ++r) {
    const float* const* L = W + 14 + 6 * r;
    mlp_dense(L[0], L[1], gcat, emb, nullptr, 2 * half, hidden, false);  // embed = Linear(GELU(cond))
    mlp_dense(L[2], L[3], h0, h1, emb, hidden, hidden, true);            // h = GELU(dense1(x)) + embed
    mlp_dense(L[4], L[5], h1, h0, h0, hidden, hidden, true);             // x = GELU(dense2(h)) + x
  }
  mlp_dense(W[14 + 6 * n_res], W[15 + 6 * n_res], h0, pred, nullptr, hidden, dim, false);  // out_lay
}

// multiply-adds of one forward per sample
double layer_mlp_macs(int dim_in, int hidden, int cond_emb, int n_res) {
  const double half = cond_emb / 2, q = half / 2;
  return q + q * half + half * half + (double)dim_in * hidden * 2 + n_res * ((double)cond_emb * hidden + 2.0 * hidden * hidden);
}

}  // namespace

__global__ void __launch_bounds__(512) layer_mlp_kernel(LayerMlpArgs a) {
  __shared__ __attribute__((aligned(16))) float xs_[MLP_MAXV], xin[MLP_MAXV], cat[MLP_MAXV], gcat[MLP_MAXV], pred[MLP_MAXV];
  __shared__ __attribute__((aligned(16))) float h0[MLP_MAXH], h1[MLP_MAXH], emb[MLP_MAXH], tb0[MLP_MAXV], tb1[MLP_MAXV];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int dim = a.dim_in, half = a.cond_emb / 2, q = half / 2;
  const float* const* W = a.w;
  // weight order = the reference module's state_dict order: time_mlp (3 Linear), cond_mlp (3), in_lay, per block
  // {embeder, dense1, dense2}, out_lay; each as (weight, bias)
  const float sd = a.sigma_data;

  float scale0 = 1.f;
  if (a.mode == 2) scale0 = a.table[0];  // x = start * sigma_start (sample.py:66)
  for (int i = tid; i < dim; i += blockDim.x) xs_[i] = a.x[(size_t)b * dim + i] * scale0;
  for (int i = tid; i < a.cond_size; i += blockDim.x) tb0[i] = a.cond[(size_t)b * a.cond_size + i];
  __syncthreads();
  mlp_cond_branch(W, a.cond_size, q, half, tb0, tb1, cat);

  const int n_steps = a.mode == 2 ? a.n_steps : 1;
  for (int step = 0; step < n_steps; ++step) {
    float sigma = 0.f;
    EdmScal e{0.f, 1.f, 0.f, 1.f};
    if (a.mode == 0) {
      e.t_in = a.tsig[b];  // raw forward: the caller has applied the time embedding (ResNet.forward, models.py:444)
    } else {
      sigma = a.mode == 2 ? a.table[(size_t)step * 4] : a.tsig[b];
      e = edm_scalings(sigma, sd, a.time_kind);
    }
    if (tid == 0) tb0[0] = e.t_in;
    for (int i = tid; i < dim; i += blockDim.x) xin[i] = xs_[i] * e.c_in;
    __syncthreads();
    mlp_time_and_trunk(W, dim, a.hidden, q, half, a.n_res, tb0, tb1, cat, gcat, xin, h0, h1, emb, pred);
    if (a.mode == 0) {
      for (int i = tid; i < dim; i += blockDim.x) a.out[(size_t)b * dim + i] = pred[i];
      return;
    }
    float sprev = 0.f, dsig = 0.f, denom = 1.f;
    if (a.mode == 2) {
      sprev = a.table[(size_t)step * 4 + 1];
      dsig = a.table[(size_t)step * 4 + 2];
      denom = a.table[(size_t)step * 4 + 3];
    }
    for (int i = tid; i < dim; i += blockDim.x) {
      const float xv = xs_[i];
      const float x0 = edm_x0(a.objective, xv, pred[i], sigma, e);
      if (a.mode == 1) {
        a.out[(size_t)b * dim + i] = x0;
      } else {
        const float eps = (xv - x0) / sigma;  // sample.py:90
        float r = x0 + sprev * eps;           // sample.py:104 (sigma_prev already carries the t > 0 mask)
        const size_t o = ((size_t)step * a.batch + b) * dim + i;
        if (a.noise) r += dsig * a.noise[o] / denom;
        xs_[i] = r;
        if (a.xs) a.xs[o] = r;
        if (a.x0s) a.x0s[o] = x0;
        if (step == n_steps - 1) a.out[(size_t)b * dim + i] = r;
      }
    }
    __syncthreads();
  }
}

namespace {

// LINDIV of cd_sampler_run (lincomb_div_kernel): every product and sum rounded on its own, then an IEEE division
__device__ __forceinline__ float prog_lindiv(const float* c, const float* const* src, int nsrc, float div, int i) {
#pragma clang fp contract(off)
  float acc = c[0] * src[0][i];
#pragma unroll
  for (int k = 1; k < 6; ++k)
    if (k < nsrc) {
      const float prod = c[k] * src[k][i];
      acc = acc + prod;
    }
  return acc / div;
}

}  // namespace

// A sampler step program (cd_sampler_run's ops, include/calodiff.h) on the layer MLP: one workgroup per sample walks every op of
// every step with the n_bufs state vectors in LDS; the element-wise ops give element i to thread i (dim_in <= 256 < 512).
__global__ void __launch_bounds__(512) layer_program_kernel(LayerProgArgs a) {
  __shared__ __attribute__((aligned(16))) float bufs[LAYER_PROG_MAX_BUFS * MLP_MAXV];
  __shared__ __attribute__((aligned(16))) float xin[MLP_MAXV], cat[MLP_MAXV], gcat[MLP_MAXV], pred[MLP_MAXV];
  __shared__ __attribute__((aligned(16))) float h0[MLP_MAXH], h1[MLP_MAXH], emb[MLP_MAXH], tb0[MLP_MAXV], tb1[MLP_MAXV];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int dim = a.dim_in, half = a.cond_emb / 2, q = half / 2;
  const float* const* W = a.w;
  const bool mine = tid < dim;  // this thread's element of the element-wise ops

  for (int i = tid; i < a.n_bufs * dim; i += blockDim.x) bufs[i] = i < dim ? a.start[(size_t)b * dim + i] * a.start_scale : 0.f;
  for (int i = tid; i < a.cond_size; i += blockDim.x) tb0[i] = a.cond[(size_t)b * a.cond_size + i];
  __syncthreads();
  mlp_cond_branch(W, a.cond_size, q, half, tb0, tb1, cat);

  uint64_t draw = 0;  // RANDN ops executed so far
  for (int step = 0; step < a.n_steps; ++step) {
    const float* row = a.coefs + (size_t)step * a.n_coef;
    const int k0 = a.op_begin ? a.op_begin[step] : 0, k1 = a.op_begin ? a.op_begin[step + 1] : a.n_ops;
    for (int k = k0; k < k1; ++k) {
      const CdSamplerOp o = a.ops[k];
      const float* s0 = bufs + o.src[0] * dim;
      switch (o.kind) {
        case CD_SOP_LINCOMB:
        case CD_SOP_LINDIV: {
          float c[6];
          const float* src[6];
#pragma unroll
          for (int j = 0; j < 6; ++j) {
            c[j] = j < o.nsrc ? row[o.col + j] : 0.f;
            src[j] = bufs + (j < o.nsrc ? o.src[j] : o.src[0]) * dim;
          }
          if (mine) {
            float v;
            if (o.kind == CD_SOP_LINDIV) {
              v = prog_lindiv(c, src, o.nsrc, row[o.col + o.nsrc], tid);
            } else {  // lincomb_kernel's order and contraction
              float acc = c[0] * src[0][tid];
#pragma unroll
              for (int j = 1; j < 6; ++j)
                if (j < o.nsrc) acc += c[j] * src[j][tid];
              v = acc;
            }
            bufs[o.dst * dim + tid] = v;
          }
          break;
        }
        case CD_SOP_DENOISE:
        case CD_SOP_DENOISE_PS: {  // (DENOISE_PS: this workgroup's shower at its own column)
          const float sigma = row[o.col + (o.kind == CD_SOP_DENOISE_PS ? b : 0)];
          const EdmScal e = edm_scalings(sigma, a.sigma_data, a.time_kind);
          if (tid == 0) tb0[0] = e.t_in;
          if (mine) xin[tid] = s0[tid] * e.c_in;
          __syncthreads();
          mlp_time_and_trunk(W, dim, a.hidden, q, half, a.n_res, tb0, tb1, cat, gcat, xin, h0, h1, emb, pred);
          if (mine) bufs[o.dst * dim + tid] = edm_x0(a.objective, s0[tid], pred[tid], sigma, e);
          break;
        }
        case CD_SOP_RANDN: {
          if (mine) {
            float z;
            if (a.step_noise) z = a.step_noise[(draw * a.batch + b) * dim + tid];
            else z = philox_normal(a.offset + draw * a.stride + (uint64_t)b * dim + tid, a.seed);
            bufs[o.dst * dim + tid] = z;
          }
          ++draw;
          break;
        }
        case CD_SOP_RECORD: {
          float* traj = o.dst == 0 ? a.xs : a.x0s;
          if (traj && mine) traj[((size_t)step * a.batch + b) * dim + tid] = s0[tid];
          break;
        }
        default:
          break;
      }
      __syncthreads();
    }
  }
  if (mine) a.out[(size_t)b * dim + tid] = bufs[tid];
}

void launch_layer_program(const LayerProgArgs& a, int64_t n_denoise, hipStream_t s) {
  CD_REQUIRE(a.dim_in >= 1 && a.dim_in <= MLP_MAXV && a.cond_emb >= 4 && a.cond_emb <= MLP_MAXV && (a.cond_emb & 3) == 0 &&
                 a.hidden >= 1 && a.hidden <= MLP_MAXH && a.cond_size >= 1 && a.cond_size <= MLP_MAXV && a.n_res >= 0 &&
                 a.n_res <= 8,
             "layer MLP: dim_in / cond_emb / cond_size up to 256, hidden up to 512, at most 8 residual blocks");
  CD_REQUIRE(a.n_bufs >= 1 && a.n_bufs <= LAYER_PROG_MAX_BUFS, "layer sampler program: 1..10 buffers");
  const double macs = layer_mlp_macs(a.dim_in, a.hidden, a.cond_emb, a.n_res);
  prof::Scope scope("layer_program", s, 2.0 * macs * a.batch * (double)n_denoise, 4.0 * macs);
  hipLaunchKernelGGL(layer_program_kernel, dim3(a.batch), dim3(512), 0, s, a);
  CD_HIP(hipGetLastError());
}

void launch_layer_mlp(const LayerMlpArgs& a, hipStream_t s) {
  CD_REQUIRE(a.dim_in >= 1 && a.dim_in <= MLP_MAXV && a.cond_emb >= 4 && a.cond_emb <= MLP_MAXV && (a.cond_emb & 3) == 0 &&
                 a.hidden >= 1 && a.hidden <= MLP_MAXH && a.cond_size >= 1 && a.cond_size <= MLP_MAXV && a.n_res >= 0 &&
                 a.n_res <= 8,
             "layer MLP: dim_in / cond_emb / cond_size up to 256, hidden up to 512, at most 8 residual blocks");
  // algorithmic work per sample and step: the dense layers' multiply-adds; the weights are the traffic (L2-resident)
  const double macs = layer_mlp_macs(a.dim_in, a.hidden, a.cond_emb, a.n_res);
  const int n_steps = a.mode == 2 ? a.n_steps : 1;
  prof::Scope scope("layer_mlp", s, 2.0 * macs * a.batch * n_steps, 4.0 * macs);
  hipLaunchKernelGGL(layer_mlp_kernel, dim3(a.batch), dim3(512), 0, s, a);
  CD_HIP(hipGetLastError());
}

}  // namespace cd
