// The conditioning MLPs of the U-Net (backward: kernels_embed_bwd.hip).
#include "kernels_embed_head.h"

namespace cd {

// ------------------------------------------------------------------------------------------------------------
// Conditioning: time MLP, cond MLP (exact-erf GELU), concat, and every ResnetBlock's SiLU->Linear(128, C) projection
// in ONE launch (20 nn.Linear calls per forward in the reference: models.py:176-180, 575-608, 704-707).
// Also derives the EDM scalings of Loss.get_scaling (loss.py:29-41) and the time embedding input
// (calodiffusion.py:144-152) from sigma.  One 128-thread block per sample.
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }

// out[j] = bias[j] + sum_k w[j][k] * in[k]: one wave per output row, lanes stride k (coalesced 256-B reads of the
// row-major torch weight), butterfly reduction.
__device__ __forceinline__ float wave_dot(const float* __restrict__ wr, const float* in, int nin, int lane) {
  float acc = 0.f;
  for (int k = lane; k < nin; k += 64) acc = fmaf(wr[k], in[k], acc);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  return acc;
}

// A wave owns 8 output rows at a time: their 8 weight-row loads are in flight together (one row per trip made every layer of
// the two small MLPs a chain of 8 L2 round trips per wave: 46 us for the whole kernel).
__device__ void dense(const float* __restrict__ w, const float* __restrict__ bias, const float* in, float* out, int nin,
                      int nout, bool gelu) {
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
      for (int r = 0; r < R; ++r) wv[r] = w[(size_t)min(j0 + r, nout - 1) * nin + k];  // clamped: rows past the end are dropped
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
      v += bias[j0 + lane];
      out[j0 + lane] = gelu ? gelu_erf(v) : v;
    }
  }
  __syncthreads();
}

__global__ void __launch_bounds__(512) embed_kernel(EmbedArgs a) {
  __shared__ float bufA[256], bufB[256], cat[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int bc = a.cond_rows ? b % a.cond_rows : b;  // row of `cond`
  const float tv = a.part == 2 ? 1.f
                   : a.part == 1 ? a.time_or_sigma[(size_t)b * a.time_stride]
                   : a.cond_rows ? a.time_or_sigma[(size_t)(b / a.cond_rows) * a.time_stride] : a.time_or_sigma[b];
  float t_in = tv;
  if (a.time_kind == 0) t_in = 0.5f * logf(tv);
  else if (a.time_kind == 1) t_in = tv / sqrtf(1.f + tv * tv);
  if (a.scal && a.part != 2 && tid == 0 && blockIdx.y == 0) {
    const float sd = a.sigma_data;
    const float s2 = tv * tv + sd * sd;
    a.scal[b * 4 + 0] = 1.f / sqrtf(s2);           // c_in
    a.scal[b * 4 + 1] = sd * sd / s2;              // c_skip
    a.scal[b * 4 + 2] = tv * sd / sqrtf(s2);       // c_out
    a.scal[b * 4 + 3] = tv;
  }
  const int half = a.half, q = half / 2;
  // SinusoidalPositionEmbeddings(q) (models.py:132-144): [sin(v f_i), cos(v f_i)], f_i = exp(-i ln(1e4) / (q/2 - 1))
  auto sinusoidal = [&](float v, float* dst) {
    const int hd = q / 2;
    const float step = (float)(9.210340371976184 / (double)(hd - 1));  // np.log(10000) / (half_dim - 1): a double, rounded to
                                                                       // fp32 when it multiplies the arange tensor
    for (int i = tid; i < hd; i += blockDim.x) {
      const float ang = v * expf((float)i * -step);
      dst[i] = sinf(ang);
      dst[hd + i] = cosf(ang);
    }
    __syncthreads();
  };
  // time branch: Linear(1, half/2) GELU | sinusoidal(half/2);  Linear(half/2, half) GELU Linear(half, half)
  if (a.part == 2) {  // condition row: the time half of `conditions` contributes nothing (SiLU(0) = 0)
    for (int i = tid; i < half; i += blockDim.x) cat[i] = 0.f;
    __syncthreads();
  } else {
    if (a.time_sin) {
      sinusoidal(t_in, bufB);
    } else {
      if (tid == 0) bufA[0] = t_in;
      __syncthreads();
      dense(a.tw1, a.tb1, bufA, bufB, 1, q, true);
    }
    dense(a.tw2, a.tb2, bufB, bufA, q, half, true);
    dense(a.tw3, a.tb3, bufA, cat, half, half, false);
  }
  // cond branch: Linear(cond_size, hidden) GELU | sinusoidal(half/2) of the scalar condition;  Linear(hidden, half) GELU
  // Linear(half, half)
  if (a.part == 1) {  // time row: no condition half
    for (int i = tid; i < half; i += blockDim.x) cat[half + i] = 0.f;
    __syncthreads();
  } else {
    if (a.cond_sin) {
      sinusoidal(a.cond[bc], bufB);
    } else {
      for (int i = tid; i < a.cond_size; i += blockDim.x) bufA[i] = a.cond[(size_t)bc * a.cond_size + i];
      __syncthreads();
      dense(a.cw1, a.cb1, bufA, bufB, a.cond_size, a.cond_hidden, true);
    }
    dense(a.cw2, a.cb2, bufB, bufA, a.cond_hidden, half, true);
    dense(a.cw3, a.cb3, bufA, cat + half, half, half, false);
  }
  // SiLU of conditions = cat(t, c)  (models.py:707; ResnetBlock.mlp[0])
  for (int i = tid; i < 2 * half; i += blockDim.x) {
    const float v = cat[i];
    bufA[i] = v / (1.f + expf(-v));
  }
  __syncthreads();
  // all ResnetBlock projections: a wave owns 4 output rows at a time so that 4 independent weight-row loads are in flight
  // gridDim.y workgroups per sample share the projection layers (each repeats the two small MLPs above: the projections'
  // ~700 weight rows are the latency chain of this kernel)
  const int nin = 2 * half;
  for (int l = blockIdx.y; l < a.n_layers; l += gridDim.y) {
    const EmbedLayer L = a.layers[l];
    for (int j0 = wave * 4; j0 < L.cout; j0 += nw * 4) {
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      for (int k = lane; k < nin; k += 64) {
        const float xv = bufA[k];
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (j0 + r < L.cout) acc[r] = fmaf(L.w[(size_t)(j0 + r) * nin + k], xv, acc[r]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[r] += __shfl_xor(acc[r], o, 64);
        if (lane == 0 && j0 + r < L.cout) a.emb[(size_t)b * a.emb_ld + L.offset + j0 + r] = a.part == 2 ? acc[r] : acc[r] + L.b[j0 + r];
      }
    }
  }
}

void launch_embed(const EmbedArgs& a, hipStream_t s) {
  CD_REQUIRE(a.half * 2 <= 256 && a.cond_hidden <= 256 && a.cond_size <= 256, "embedding widths above 256 unsupported");
  prof::Scope scope("embed", s, 0, 0);
  const int groups = a.n_layers >= 4 ? 4 : 1;
  CD_REQUIRE(!a.cond_rows || a.batch % a.cond_rows == 0, "internal: embedding chunk must be whole steps");
  hipLaunchKernelGGL(embed_kernel, dim3(a.batch, groups), dim3(512), 0, s, a);
  CD_HIP(hipGetLastError());
}

// out[b][j] = bias[j] + sum_k w[j][k] * silu(cond[b][k])   (ResnetBlock.mlp, models.py:176-180; block-level tests only)
__global__ void silu_linear_kernel(const float* __restrict__ cond, const float* __restrict__ w, const float* __restrict__ bias,
                                   float* __restrict__ out, int nin, int nout) {
  const int b = blockIdx.x;
  for (int j = threadIdx.x; j < nout; j += blockDim.x) {
    float acc = bias[j];
    for (int k = 0; k < nin; ++k) {
      const float v = cond[(size_t)b * nin + k];
      acc = fmaf(w[(size_t)j * nin + k], v / (1.f + expf(-v)), acc);
    }
    out[(size_t)b * nout + j] = acc;
  }
}
void launch_silu_linear(const float* cond, const float* w, const float* bias, float* out, int batch, int nin, int nout,
                        hipStream_t s) {
  hipLaunchKernelGGL(silu_linear_kernel, dim3(batch), dim3(128), 0, s, cond, w, bias, out, nin, nout);
  CD_HIP(hipGetLastError());
}

}  // namespace cd
