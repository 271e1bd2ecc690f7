// Backward of the conditioning MLPs (time / energy embeddings and the ResnetBlock projections of CondUnet; forward: embed_kernel
// in kernels_embed.hip): embed_bwd_kernel leaves every Linear's input and output delta per sample on a tape, linear_wgrad_kernel
// forms the weight and bias gradients from it.
#include "kernels_bwd.h"

namespace cd {

// ------------------------------------------------------------------------------------------------------------
// Conditioning MLPs backward (forward: embed_kernel).  One block per sample recomputes the tiny forward, back-propagates
// demb (gradient of every ResnetBlock projection output) down to the first layers and leaves, per sample, each Linear's
// input activation and output delta in `tape`; linear_wgrad_kernel then forms dW = sum_b delta x input, db = sum_b delta.
// tape row layout per sample (floats): see EmbedTapeLayout.
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gelu_erf_b(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }
__device__ __forceinline__ float gelu_grad(float x) {
  return 0.5f * (1.f + erff(x * 0.70710678118654752440f)) + x * 0.3989422804014327f * expf(-0.5f * x * x);
}
// y = W x + b (pre-activation) for all outputs; block-cooperative (thread per output row, serial dot: tiny sizes)
__device__ void dense_pre(const float* __restrict__ w, const float* __restrict__ bias, const float* in, float* pre, int nin, int nout) {
  for (int j = threadIdx.x; j < nout; j += blockDim.x) {
    float acc = bias[j];
    for (int k = 0; k < nin; ++k) acc = fmaf(w[(size_t)j * nin + k], in[k], acc);
    pre[j] = acc;
  }
  __syncthreads();
}
// din[k] = sum_j W[j][k] * dout[j]
__device__ void dense_bwd_in(const float* __restrict__ w, const float* dout, float* din, int nin, int nout) {
  for (int k = threadIdx.x; k < nin; k += blockDim.x) {
    float acc = 0.f;
    for (int j = 0; j < nout; ++j) acc = fmaf(w[(size_t)j * nin + k], dout[j], acc);
    din[k] = acc;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(256) embed_bwd_kernel(EmbedArgs a, const float* __restrict__ demb, float* __restrict__ tape) {
  __shared__ float p1t[128], p2t[128], p1c[256], p2c[128], cat[256], sc[256], dcat[256], tmpA[256], tmpB[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int half = a.half, q = half / 2, hid = a.cond_hidden;
  const EmbedTapeLayout L = embed_tape_layout(a.cond_size, hid, half);
  float* T = tape + (size_t)b * L.total;
  const float tv = a.time_or_sigma[b];
  float t_in = tv;
  if (a.time_kind == 0) t_in = 0.5f * logf(tv);
  else if (a.time_kind == 1) t_in = tv / sqrtf(1.f + tv * tv);
  // ---- forward recompute (pre-activations kept) ----
  if (tid == 0) { tmpA[0] = t_in; T[L.t_in] = t_in; }
  __syncthreads();
  dense_pre(a.tw1, a.tb1, tmpA, p1t, 1, q);
  for (int i = tid; i < q; i += blockDim.x) { tmpB[i] = gelu_erf_b(p1t[i]); T[L.a1t + i] = tmpB[i]; }
  __syncthreads();
  dense_pre(a.tw2, a.tb2, tmpB, p2t, q, half);
  for (int i = tid; i < half; i += blockDim.x) { tmpA[i] = gelu_erf_b(p2t[i]); T[L.a2t + i] = tmpA[i]; }
  __syncthreads();
  dense_pre(a.tw3, a.tb3, tmpA, cat, half, half);
  for (int i = tid; i < a.cond_size; i += blockDim.x) { tmpA[i] = a.cond[(size_t)b * a.cond_size + i]; T[L.cond_in + i] = tmpA[i]; }
  __syncthreads();
  dense_pre(a.cw1, a.cb1, tmpA, p1c, a.cond_size, hid);
  for (int i = tid; i < hid; i += blockDim.x) { tmpB[i] = gelu_erf_b(p1c[i]); T[L.a1c + i] = tmpB[i]; }
  __syncthreads();
  dense_pre(a.cw2, a.cb2, tmpB, p2c, hid, half);
  for (int i = tid; i < half; i += blockDim.x) { tmpA[i] = gelu_erf_b(p2c[i]); T[L.a2c + i] = tmpA[i]; }
  __syncthreads();
  dense_pre(a.cw3, a.cb3, tmpA, cat + half, half, half);
  for (int i = tid; i < 2 * half; i += blockDim.x) {
    const float v = cat[i];
    sc[i] = v / (1.f + expf(-v));
    T[L.sc + i] = sc[i];
  }
  __syncthreads();
  // ---- backward: dsc = sum_l W_l^T demb_l ; dcat = dsc * silu'(cat) ----
  // (two thread groups take the even / odd projection layers, eight weight loads in flight each: one thread per k walking all
  // ~800 rows alone was a 200 us chain of L2 round trips)
  {
    const int nk = 2 * half, grp = tid / nk, k = tid - grp * nk, ngrp = blockDim.x / nk;  // nk <= 128 => ngrp >= 2
    float acc = 0.f;
    if (grp < 2) {
      for (int l = grp; l < a.n_layers; l += 2) {
        const EmbedLayer Ly = a.layers[l];
        const float* d = demb + (size_t)b * a.emb_ld + Ly.offset;
        const float* wk = Ly.w + k;
        int j = 0;
        for (; j + 8 <= Ly.cout; j += 8) {
          float wv[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) wv[u] = wk[(size_t)(j + u) * nk];
#pragma unroll
          for (int u = 0; u < 8; ++u) acc = fmaf(wv[u], d[j + u], acc);
        }
        for (; j < Ly.cout; ++j) acc = fmaf(wk[(size_t)j * nk], d[j], acc);
      }
      (grp == 0 ? tmpA : tmpB)[k] = acc;
    }
    (void)ngrp;
    __syncthreads();
    if (tid < nk) {
      const float v = cat[tid];
      const float sg = 1.f / (1.f + expf(-v));
      dcat[tid] = (tmpA[tid] + tmpB[tid]) * sg * (1.f + v * (1.f - sg));
    }
  }
  __syncthreads();
  // time branch: cat[0:half] = W3 a2t + b3
  for (int i = tid; i < half; i += blockDim.x) T[L.d3t + i] = dcat[i];
  dense_bwd_in(a.tw3, dcat, tmpA, half, half);                       // d a2t
  for (int i = tid; i < half; i += blockDim.x) { tmpA[i] *= gelu_grad(p2t[i]); T[L.d2t + i] = tmpA[i]; }
  __syncthreads();
  dense_bwd_in(a.tw2, tmpA, tmpB, q, half);                          // d a1t
  for (int i = tid; i < q; i += blockDim.x) { tmpB[i] *= gelu_grad(p1t[i]); T[L.d1t + i] = tmpB[i]; }
  __syncthreads();
  // cond branch: cat[half:] = W3c a2c + b3c
  for (int i = tid; i < half; i += blockDim.x) T[L.d3c + i] = dcat[half + i];
  dense_bwd_in(a.cw3, dcat + half, tmpA, half, half);
  for (int i = tid; i < half; i += blockDim.x) { tmpA[i] *= gelu_grad(p2c[i]); T[L.d2c + i] = tmpA[i]; }
  __syncthreads();
  dense_bwd_in(a.cw2, tmpA, tmpB, hid, half);
  for (int i = tid; i < hid; i += blockDim.x) { tmpB[i] *= gelu_grad(p1c[i]); T[L.d1c + i] = tmpB[i]; }
}
size_t embed_tape_floats(int cond_size, int hidden, int half) { return (size_t)embed_tape_layout(cond_size, hidden, half).total; }
void launch_embed_bwd(const EmbedArgs& a, const float* demb, float* tape, hipStream_t s) {
  hipLaunchKernelGGL(embed_bwd_kernel, dim3(a.batch), dim3(256), 0, s, a, demb, tape);
  CD_HIP(hipGetLastError());
}

// dW[j][k] = sum_b delta[b][j] * in[b][k],  db[j] = sum_b delta[b][j];  blockIdx.y = job
__global__ void linear_wgrad_kernel(const LinearWgradJob* __restrict__ jobs, int batch) {
  const LinearWgradJob J = jobs[blockIdx.y];
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < J.nout * J.nin) {
    const int j = idx / J.nin, k = idx % J.nin;
    float s = 0.f;
    for (int b = 0; b < batch; ++b) s = fmaf(J.delta[(size_t)b * J.delta_ld + j], J.in[(size_t)b * J.in_ld + k], s);
    J.dw[idx] = s;
  }
  if (idx < J.nout) {
    float s = 0.f;
    for (int b = 0; b < batch; ++b) s += J.delta[(size_t)b * J.delta_ld + idx];
    J.db[idx] = s;
  }
}
void launch_linear_wgrad(const LinearWgradJob* jobs_dev, int njobs, int max_elems, int batch, hipStream_t s) {
  hipLaunchKernelGGL(linear_wgrad_kernel, dim3((max_elems + 255) / 256, njobs), dim3(256), 0, s, jobs_dev, batch);
  CD_HIP(hipGetLastError());
}

}  // namespace cd
