// GroupNorm(+SiLU)(+add) backward: the statistics pass, its finalize, the elementwise pass, the one-workgroup-per-sample form
// for small tensors, and the batch reduction of the parameter gradients (alone or as queued jobs).  Reference: torch autograd
// through the nn.GroupNorm + SiLU of Block / ResnetBlock (models.py:147-201) and the norms around LinearAttention
// (models.py:281-333); forward: kernels_gn.hip (launch_gn_finalize / launch_gn_apply).
#include "kernels_bwd.h"
#include "kernels_gn.h"
#include <cstdlib>

namespace cd {

// ------------------------------------------------------------------------------------------------------------
// GroupNorm(+SiLU)(+add) backward.   forward: z = scale*h + shift (scale = rstd*gamma, shift = beta - mean*scale),
// y = act(z) + add [+ residual].  Given dy:
//   dz = dy * act'(z);  dgamma[c] = sum dz*hhat;  dbeta[c] = sum dz;  dadd[b][c] = sum_v dy
//   dh = rstd * (dhhat - mean_g(dhhat) - hhat * mean_g(dhhat*hhat)),  dhhat = dz*gamma,  hhat = (h - mean)*rstd
// Pass 1 (gn_bwd_stats_kernel): per (b, split, c): {sum dz, sum dz*hhat, sum dy, sum (h - mean)}.  Pass 2 (gn_bwd_apply_kernel).
// `stat` = saved {mean, rstd} per (b, g).
// Two more parameter gradients fall out of those sums without another pass over a tensor (round 4: ch_stats + bias_grad were two
// launches and a re-read of dh / dy per convolution bias):
//   the bias of the convolution that PRODUCED h:  sum_v dh = A sum_v dz - rstd (vox m1 + rstd m2 sum_v (h - mean))
//       (dh = A dz + Bh h + C0 with A = rstd gamma, Bh = -rstd^2 m2, C0 = rstd (-m1 + mean rstd m2): gn_bwd_finalize_kernel)
//   the bias of a convolution that adds into y (a ResnetBlock's 1x1 shortcut):  sum_v dy.
// ------------------------------------------------------------------------------------------------------------
// (on the transcendental unit, like the forward's cd_fast_silu: ~3 ulp; libm's expf and a division were ~40 vector instructions
// per element in kernels that stream two tensors)
__device__ __forceinline__ float silu_grad(float z) {
  const float sg = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(z * -1.4426950408889634f));
  return sg * (1.f + z * (1.f - sg));
}

__global__ void __launch_bounds__(256) gn_bwd_stats_kernel(const float* __restrict__ dy, const float* __restrict__ h,
                                                           const float* __restrict__ coef, const float* __restrict__ stat,
                                                           float* __restrict__ part, int channels, int64_t vox, int groups,
                                                           int silu, int nsplit) {
  __shared__ double sP[256][4];
  const int tid = threadIdx.x;
  const int split = blockIdx.x, b = blockIdx.y;
  const int cols = channels >> 2, rows = 256 / cols;
  const int64_t per = (vox + nsplit - 1) / nsplit;
  const int64_t v0 = split * per, v1 = (v0 + per < vox) ? v0 + per : vox;
  const int colid = tid % cols, row = tid / cols;
  const int c = colid * 4, cpg = channels / groups;
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0, s2 = s0, s3 = s0;
  if (row < rows) {
    f32x4 cf[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) cf[e] = *(const f32x4*)(coef + ((size_t)b * channels + c + e) * 4);
    const float mean = stat[((size_t)b * groups + c / cpg) * 2], rstd = stat[((size_t)b * groups + c / cpg) * 2 + 1];
    const size_t sb = (size_t)b * vox * channels + c;
    // four voxels per trip: eight loads in flight (one pair per trip ran at 3.2 TB/s at level 0); the order of the additions into
    // a thread's sums is that of the plain loop
    int64_t v = v0 + row;
    for (; v + 3 * rows < v1; v += 4 * rows) {
      f32x4 g4[4], h4[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        g4[k] = *(const f32x4*)(dy + sb + (size_t)(v + k * rows) * channels);
        h4[k] = *(const f32x4*)(h + sb + (size_t)(v + k * rows) * channels);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float z = cf[e][0] * h4[k][e] + cf[e][1];
          const float dz = silu ? g4[k][e] * silu_grad(z) : g4[k][e];
          s0[e] += dz;
          s1[e] += dz * (h4[k][e] - mean) * rstd;
          s2[e] += g4[k][e];
          s3[e] += h4[k][e] - mean;
        }
    }
    for (; v < v1; v += rows) {
      const f32x4 g = *(const f32x4*)(dy + sb + (size_t)v * channels);
      const f32x4 hv = *(const f32x4*)(h + sb + (size_t)v * channels);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float z = cf[e][0] * hv[e] + cf[e][1];
        const float dz = silu ? g[e] * silu_grad(z) : g[e];
        s0[e] += dz;
        s1[e] += dz * (hv[e] - mean) * rstd;
        s2[e] += g[e];
        s3[e] += hv[e] - mean;
      }
    }
  }
  float* dst = part + (((size_t)b * nsplit + split) * channels) * 4;
  if (cols == 8 || cols == 16) {  // (32 and 64 channels; the scratch below is 8 KB = 4 waves x 16 quads x 16 doubles)
    // the threads of one channel quad are `cols` lanes apart: fp64 xor tree inside the wave, then the four waves through LDS (fixed
    // order).  The LDS-only form below serialised 4 x (barrier, `rows` fp64 loads by `cols` threads, barrier): ~6 us of a 15 us launch
    // whose workgroups stream 250 voxels each.
    double d[4][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      d[e][0] = (double)s0[e]; d[e][1] = (double)s1[e]; d[e][2] = (double)s2[e]; d[e][3] = (double)s3[e];
    }
    for (int m = cols; m < 64; m <<= 1) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int k = 0; k < 4; ++k) d[e][k] += __shfl_xor(d[e][k], m, 64);
    }
    const int lane = tid & 63, wave = tid >> 6;
    double* sW = &sP[0][0];  // [4 waves][cols][16]
    if (lane < cols) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int k = 0; k < 4; ++k) sW[(wave * cols + lane) * 16 + e * 4 + k] = d[e][k];
    }
    __syncthreads();
    for (int i = tid; i < cols * 4; i += 256) {  // (quad, element)
      const int q = i >> 2, e = i & 3;
      double a[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) a[k] = ((sW[(0 * cols + q) * 16 + e * 4 + k] + sW[(1 * cols + q) * 16 + e * 4 + k]) + sW[(2 * cols + q) * 16 + e * 4 + k]) + sW[(3 * cols + q) * 16 + e * 4 + k];
      *(f32x4*)(dst + (q * 4 + e) * 4) = f32x4{(float)a[0], (float)a[1], (float)a[2], (float)a[3]};
    }
    return;
  }
  for (int e = 0; e < 4; ++e) {
    sP[tid][0] = (double)s0[e]; sP[tid][1] = (double)s1[e]; sP[tid][2] = (double)s2[e]; sP[tid][3] = (double)s3[e];
    __syncthreads();
    if (tid < cols) {
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
      for (int r = 0; r < rows; ++r) {
        a0 += sP[r * cols + tid][0]; a1 += sP[r * cols + tid][1]; a2 += sP[r * cols + tid][2]; a3 += sP[r * cols + tid][3];
      }
      *(f32x4*)(dst + (tid * 4 + e) * 4) = f32x4{(float)a0, (float)a1, (float)a2, (float)a3};
    }
    __syncthreads();
  }
}

// one block per sample: reduces the partials; writes gcoef[b][c] = {gamma*rstd, m1, m2*rstd... } for the apply pass,
// accumulates dadd[b][c]; dgamma/dbeta are reduced over the batch by a second tiny kernel.
__global__ void __launch_bounds__(256) gn_bwd_finalize_kernel(const float* __restrict__ part, int nsplit, const float* __restrict__ gamma,
                                                              const float* __restrict__ stat, float* __restrict__ gcoef,
                                                              float* __restrict__ sums_bc, float* __restrict__ dadd, int dadd_ld,
                                                              int channels, int groups, int64_t vox) {
  __shared__ double s0[256], s1[256];
  __shared__ float m1[64], m2[64];
  const int b = blockIdx.x, c = threadIdx.x;
  const int cpg = channels / groups;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (c < channels) {
    const float* p = part + ((size_t)b * nsplit * channels + c) * 4;
    for (int u = 0; u < nsplit; ++u) {
      const f32x4 v = *(const f32x4*)(p + (size_t)u * channels * 4);
      a0 += (double)v[0]; a1 += (double)v[1]; a2 += (double)v[2]; a3 += (double)v[3];
    }
    s0[c] = a0 * (double)gamma[c];   // sum dhhat
    s1[c] = a1 * (double)gamma[c];   // sum dhhat*hhat
    sums_bc[((size_t)b * channels + c) * 4] = (float)a0;      // dbeta contribution of this sample
    sums_bc[((size_t)b * channels + c) * 4 + 1] = (float)a1;  // dgamma contribution
    sums_bc[((size_t)b * channels + c) * 4 + 3] = (float)a2;  // sum_v dy: bias of a conv that adds into y (the shortcut)
    if (dadd) dadd[(size_t)b * dadd_ld + c] = (float)a2;
  }
  __syncthreads();
  if (c < groups) {
    double t0 = 0.0, t1 = 0.0;
    for (int k = 0; k < cpg; ++k) { t0 += s0[c * cpg + k]; t1 += s1[c * cpg + k]; }
    const double cnt = (double)vox * cpg;
    m1[c] = (float)(t0 / cnt);
    m2[c] = (float)(t1 / cnt);
  }
  __syncthreads();
  if (c < channels) {
    const int g = c / cpg;
    const float mean = stat[((size_t)b * groups + g) * 2], rstd = stat[((size_t)b * groups + g) * 2 + 1];
    // dh = rstd*(gamma*dz - m1 - hhat*m2) = A*dz + Bh*h + C0 with hhat = (h-mean)*rstd
    f32x4 o;
    o[0] = rstd * gamma[c];                 // * dz
    o[1] = -rstd * rstd * m2[g];            // * h
    o[2] = rstd * (-m1[g] + mean * rstd * m2[g]);
    o[3] = 0.f;
    *(f32x4*)(gcoef + ((size_t)b * channels + c) * 4) = o;
    // sum_v dh of this sample and channel (the bias gradient of the conv that produced h), from the sums in hand
    sums_bc[((size_t)b * channels + c) * 4 + 2] =
        (float)((double)o[0] * a0 - (double)rstd * ((double)m1[g] * (double)vox + (double)rstd * (double)m2[g] * a3));
  }
}

__global__ void param_grad_from_samples_kernel(const float* __restrict__ sums_bc, int batch, int channels, float* __restrict__ dgamma,
                                               float* __restrict__ dbeta, int accumulate, float* __restrict__ dbias,
                                               float* __restrict__ dsumdy) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= channels) return;
  double g = 0.0, bt = 0.0, bs = 0.0, sy = 0.0;
  int n = 0;
  for (; n + 8 <= batch; n += 8) {  // eight samples' rows in flight (fixed summation order)
    f32x4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = *(const f32x4*)(sums_bc + ((size_t)(n + u) * channels + c) * 4);
#pragma unroll
    for (int u = 0; u < 8; ++u) { bt += (double)v[u][0]; g += (double)v[u][1]; bs += (double)v[u][2]; sy += (double)v[u][3]; }
  }
  for (; n < batch; ++n) {
    const f32x4 v = *(const f32x4*)(sums_bc + ((size_t)n * channels + c) * 4);
    bt += (double)v[0]; g += (double)v[1]; bs += (double)v[2]; sy += (double)v[3];
  }
  dgamma[c] = accumulate ? dgamma[c] + (float)g : (float)g;
  dbeta[c] = accumulate ? dbeta[c] + (float)bt : (float)bt;
  if (dbias) dbias[c] = (float)bs;
  if (dsumdy) dsumdy[c] = (float)sy;
}

// dh = gc0*dz + gc1*h + gc2 (+ dh_accum), dz = dy*act'(scale*h+shift)
// `fold` (round 4): the arithmetic of gn_bwd_finalize_kernel in the prologue of every workgroup of the sample, from the statistics
// partials (a few KB per sample) -- same operations in the same order, so the result equals the three-launch form bit for bit;
// the sample's first workgroup writes the per-sample sums for the parameter gradients.  One launch less per GroupNorm layer.
struct GnBwdFold {
  const float* part = nullptr;   // [B][nsplit][C][4] of gn_bwd_stats_kernel; null: gcoef is read from memory
  const float* gamma = nullptr;
  const float* stat = nullptr;
  float* sums_bc = nullptr;
  float* dadd = nullptr;
  int nsplit = 0, dadd_ld = 0, groups = 0;
};
__global__ void __launch_bounds__(256) gn_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ h,
                                                           const float* __restrict__ coef, const float* __restrict__ gcoef,
                                                           float* __restrict__ dh, int channels, int64_t vox, int silu,
                                                           int blocks_per_sample, unsigned* __restrict__ amax_out, GnBwdFold fold) {
  __shared__ float sAmax[4];
  __shared__ double fs0[256], fs1[256];
  __shared__ float fm1[64], fm2[64];
  __shared__ __attribute__((aligned(16))) float sGc[256][4];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / blocks_per_sample, blk = blockIdx.x % blocks_per_sample;
  if (fold.part) {
    const int cc = tid, cpg = channels / fold.groups;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (cc < channels) {
      const float* p = fold.part + ((size_t)b * fold.nsplit * channels + cc) * 4;
      int u = 0;
      for (; u + 8 <= fold.nsplit; u += 8) {  // eight partials in flight (same order of additions as the plain loop)
        f32x4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = *(const f32x4*)(p + (size_t)(u + k) * channels * 4);
#pragma unroll
        for (int k = 0; k < 8; ++k) { a0 += (double)v[k][0]; a1 += (double)v[k][1]; a2 += (double)v[k][2]; a3 += (double)v[k][3]; }
      }
      for (; u < fold.nsplit; ++u) {
        const f32x4 v = *(const f32x4*)(p + (size_t)u * channels * 4);
        a0 += (double)v[0]; a1 += (double)v[1]; a2 += (double)v[2]; a3 += (double)v[3];
      }
      fs0[cc] = a0 * (double)fold.gamma[cc];
      fs1[cc] = a1 * (double)fold.gamma[cc];
    }
    __syncthreads();
    if (cc < fold.groups) {
      double t0 = 0.0, t1 = 0.0;
      for (int k = 0; k < cpg; ++k) { t0 += fs0[cc * cpg + k]; t1 += fs1[cc * cpg + k]; }
      const double cnt = (double)vox * cpg;
      fm1[cc] = (float)(t0 / cnt);
      fm2[cc] = (float)(t1 / cnt);
    }
    __syncthreads();
    if (cc < channels) {
      const int g = cc / cpg;
      const float mean = fold.stat[((size_t)b * fold.groups + g) * 2], rstd = fold.stat[((size_t)b * fold.groups + g) * 2 + 1];
      f32x4 o;
      o[0] = rstd * fold.gamma[cc];
      o[1] = -rstd * rstd * fm2[g];
      o[2] = rstd * (-fm1[g] + mean * rstd * fm2[g]);
      o[3] = 0.f;
      *(f32x4*)sGc[cc] = o;
      if (blk == 0) {
        const float sdh = (float)((double)o[0] * a0 - (double)rstd * ((double)fm1[g] * (double)vox + (double)rstd * (double)fm2[g] * a3));
        *(f32x4*)(fold.sums_bc + ((size_t)b * channels + cc) * 4) = f32x4{(float)a0, (float)a1, sdh, (float)a2};
        if (fold.dadd) fold.dadd[(size_t)b * fold.dadd_ld + cc] = (float)a2;
      }
    }
    __syncthreads();
  }
  const int cols = channels >> 2, rows = 256 / cols;
  const int64_t vper = (vox + blocks_per_sample - 1) / blocks_per_sample;
  const int64_t v0 = blk * vper, v1 = (v0 + vper < vox) ? v0 + vper : vox;
  const int colid = tid % cols, row = tid / cols;
  const int c = colid * 4;
  float am = 0.f;
  if (row < rows) {
  f32x4 cf[4], gc[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    cf[e] = *(const f32x4*)(coef + ((size_t)b * channels + c + e) * 4);
    gc[e] = fold.part ? *(const f32x4*)sGc[c + e] : *(const f32x4*)(gcoef + ((size_t)b * channels + c + e) * 4);
  }
  const size_t sb = (size_t)b * vox * channels + c;
  int64_t v = v0 + row;
  for (; v + 3 * rows < v1; v += 4 * rows) {  // four voxels per trip: eight loads in flight
    f32x4 g4[4], h4[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      g4[k] = *(const f32x4*)(dy + sb + (size_t)(v + k * rows) * channels);
      h4[k] = *(const f32x4*)(h + sb + (size_t)(v + k * rows) * channels);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float z = cf[e][0] * h4[k][e] + cf[e][1];
        const float dz = silu ? g4[k][e] * silu_grad(z) : g4[k][e];
        o[e] = gc[e][0] * dz + gc[e][1] * h4[k][e] + gc[e][2];
      }
      *(f32x4*)(dh + sb + (size_t)(v + k * rows) * channels) = o;
      am = fmaxf(am, fmaxf(fmaxf(fabsf(o[0]), fabsf(o[1])), fmaxf(fabsf(o[2]), fabsf(o[3]))));
    }
  }
  for (; v < v1; v += rows) {
    const f32x4 g = *(const f32x4*)(dy + sb + (size_t)v * channels);
    const f32x4 hv = *(const f32x4*)(h + sb + (size_t)v * channels);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float z = cf[e][0] * hv[e] + cf[e][1];
      const float dz = silu ? g[e] * silu_grad(z) : g[e];
      o[e] = gc[e][0] * dz + gc[e][1] * hv[e] + gc[e][2];
    }
    *(f32x4*)(dh + sb + (size_t)v * channels) = o;
    am = fmaxf(am, fmaxf(fmaxf(fabsf(o[0]), fabsf(o[1])), fmaxf(fabsf(o[2]), fabsf(o[3]))));
  }
  }
  if (amax_out) {  // max |dh| for the power-of-two rescaling of the conv gradients that consume dh (saves their own pass over it)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) am = fmaxf(am, __shfl_xor(am, o, 64));
    if ((tid & 63) == 0) sAmax[tid >> 6] = am;
    __syncthreads();
    if (tid == 0) atomicMax(amax_out, __float_as_uint(fmaxf(fmaxf(sAmax[0], sAmax[1]), fmaxf(sAmax[2], sAmax[3]))));
  }
}

// The whole GroupNorm backward of ONE sample in one workgroup, for the grids where the three launches above are three prologues
// around microseconds of streaming (the deepest levels of the U-Net: <= 100 KB per sample and tensor; 24 of the 44 GroupNorm layers
// of a Dataset-2 training step): statistics -> the finalize arithmetic in LDS -> apply, the second pass over dy / h served by L2.
// Same summation structure as the split form with nsplit = 1 (per-thread float partials, fp64 column sums, fp64 group means).
__global__ void __launch_bounds__(512) gn_bwd_small_kernel(const float* __restrict__ dy, const float* __restrict__ h,
                                                           const float* __restrict__ coef, const float* __restrict__ stat,
                                                           const float* __restrict__ gamma, float* __restrict__ dh,
                                                           float* __restrict__ sums_bc, float* __restrict__ dadd, int dadd_ld,
                                                           int channels, int64_t vox, int groups, int silu,
                                                           unsigned* __restrict__ amax_out) {
  // The launch is a chain of dependent latencies around microseconds of streaming (14-20 us for 24-100 KB per tensor); round 4's
  // second session removed four of them: gamma / mean / rstd are fetched into LDS beside the first pass's loads (they were read
  // from global in the middle of the fold, twice), the column sums of all four channels of a quad are formed at once -- rows of a
  // wave by shuffles, waves through ONE LDS hop (eight barrier-separated serial sums before) -- and a sample of at most four row
  // trips per thread (the deepest level) keeps dy / h in registers for the second pass.
  __shared__ double sW[8][32][4][4];   // [wave][column][e][sum]: per-wave column sums (channels <= 128: launcher)
  __shared__ double sCol[256][4];
  __shared__ float m1[64], m2[64];
  __shared__ __attribute__((aligned(16))) float sG[256][4];
  __shared__ float sGam[256], sMean[64], sRstd[64];
  __shared__ float sAmax[8];
  const int tid = threadIdx.x, b = blockIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cols = channels >> 2, rows = 512 / cols;   // cols in {8, 16, 32} (launcher)
  const int colid = tid % cols, row = tid / cols;
  const int c = colid * 4, cpg = channels / groups;
  const size_t sb = (size_t)b * vox * channels + c;
  if (tid < channels) sGam[tid] = gamma[tid];
  if (tid < groups) {
    sMean[tid] = stat[((size_t)b * groups + tid) * 2];
    sRstd[tid] = stat[((size_t)b * groups + tid) * 2 + 1];
  }
  f32x4 cf[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) cf[e] = *(const f32x4*)(coef + ((size_t)b * channels + c + e) * 4);
  const float mean = stat[((size_t)b * groups + c / cpg) * 2], rstd = stat[((size_t)b * groups + c / cpg) * 2 + 1];
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0, s2 = s0, s3 = s0;
  auto acc1 = [&](const f32x4 g, const f32x4 hv) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float z = cf[e][0] * hv[e] + cf[e][1];
      const float dz = silu ? g[e] * silu_grad(z) : g[e];
      s0[e] += dz;
      s1[e] += dz * (hv[e] - mean) * rstd;
      s2[e] += g[e];
      s3[e] += hv[e] - mean;
    }
  };
  const bool keep = vox <= (int64_t)4 * rows;  // block-uniform: the whole sample is one trip of four rows per thread
  f32x4 kg[4], kh[4];
  if (keep) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t v = row + (int64_t)u * rows;
      const int64_t vc = v < vox ? v : vox - 1;
      kg[u] = *(const f32x4*)(dy + sb + (size_t)vc * channels);
      kh[u] = *(const f32x4*)(h + sb + (size_t)vc * channels);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (row + (int64_t)u * rows < vox) acc1(kg[u], kh[u]);
  } else {
    // four voxel rows per trip: eight 16-byte loads in flight per thread
    int64_t v = row;
    for (; v + 3 * rows < vox; v += 4 * rows) {
      f32x4 g[4], hv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        g[u] = *(const f32x4*)(dy + sb + (size_t)(v + u * rows) * channels);
        hv[u] = *(const f32x4*)(h + sb + (size_t)(v + u * rows) * channels);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) acc1(g[u], hv[u]);
    }
    for (; v < vox; v += rows) acc1(*(const f32x4*)(dy + sb + (size_t)v * channels), *(const f32x4*)(h + sb + (size_t)v * channels));
  }
  // column sums in fp64: the rows a wave holds of one column sit cols lanes apart (cols < 64) -> xor shuffles; then the eight waves
  // through LDS, summed in wave order by one thread per (column, e)
  {
    double p[4][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      p[e][0] = (double)s0[e]; p[e][1] = (double)s1[e]; p[e][2] = (double)s2[e]; p[e][3] = (double)s3[e];
    }
    for (int o = 32; o >= cols; o >>= 1) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int q = 0; q < 4; ++q) p[e][q] += __shfl_xor(p[e][q], o, 64);
    }
    if (lane < cols) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int q = 0; q < 4; ++q) sW[wave][lane][e][q] = p[e][q];
    }
  }
  __syncthreads();
  if (tid < channels) {
    // thread = channel cc = 4 column + e (every wave holds rows of every column: cols <= 32)
    const int col = tid >> 2, e = tid & 3;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int w = 0; w < 8; ++w) {
      a0 += sW[w][col][e][0]; a1 += sW[w][col][e][1]; a2 += sW[w][col][e][2]; a3 += sW[w][col][e][3];
    }
    // (rounded to float like the split form's partials)
    sCol[tid][0] = (double)(float)a0; sCol[tid][1] = (double)(float)a1;
    sCol[tid][2] = (double)(float)a2; sCol[tid][3] = (double)(float)a3;
  }
  __syncthreads();
  if (tid < groups) {
    double t0 = 0.0, t1 = 0.0;
    for (int k = 0; k < cpg; ++k) {
      t0 += sCol[tid * cpg + k][0] * (double)sGam[tid * cpg + k];
      t1 += sCol[tid * cpg + k][1] * (double)sGam[tid * cpg + k];
    }
    const double cnt = (double)vox * cpg;
    m1[tid] = (float)(t0 / cnt);
    m2[tid] = (float)(t1 / cnt);
  }
  __syncthreads();
  if (tid < channels) {
    const int cc = tid, g = cc / cpg;
    const float mn = sMean[g], rs = sRstd[g];
    const float A = rs * sGam[cc];
    sG[cc][0] = A;
    sG[cc][1] = -rs * rs * m2[g];
    sG[cc][2] = rs * (-m1[g] + mn * rs * m2[g]);
    sG[cc][3] = 0.f;
    float* o = sums_bc + ((size_t)b * channels + cc) * 4;
    o[0] = (float)sCol[cc][0];
    o[1] = (float)sCol[cc][1];
    o[2] = (float)((double)A * sCol[cc][0] - (double)rs * ((double)m1[g] * (double)vox + (double)rs * (double)m2[g] * sCol[cc][3]));
    o[3] = (float)sCol[cc][2];
    if (dadd) dadd[(size_t)b * dadd_ld + cc] = (float)sCol[cc][2];
  }
  __syncthreads();
  float am = 0.f;
  {
    f32x4 gc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) gc[e] = *(const f32x4*)sG[c + e];
    auto one = [&](const f32x4 g, const f32x4 hv, int64_t v) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float z = cf[e][0] * hv[e] + cf[e][1];
        const float dz = silu ? g[e] * silu_grad(z) : g[e];
        o[e] = gc[e][0] * dz + gc[e][1] * hv[e] + gc[e][2];
      }
      *(f32x4*)(dh + sb + (size_t)v * channels) = o;
      am = fmaxf(am, fmaxf(fmaxf(fabsf(o[0]), fabsf(o[1])), fmaxf(fabsf(o[2]), fabsf(o[3]))));
    };
    if (keep) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (row + (int64_t)u * rows < vox) one(kg[u], kh[u], row + (int64_t)u * rows);
    } else {
      int64_t v = row;
      for (; v + 3 * rows < vox; v += 4 * rows) {
        f32x4 g[4], hv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          g[u] = *(const f32x4*)(dy + sb + (size_t)(v + u * rows) * channels);
          hv[u] = *(const f32x4*)(h + sb + (size_t)(v + u * rows) * channels);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) one(g[u], hv[u], v + u * rows);
      }
      for (; v < vox; v += rows) one(*(const f32x4*)(dy + sb + (size_t)v * channels), *(const f32x4*)(h + sb + (size_t)v * channels), v);
    }
  }
  if (amax_out) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) am = fmaxf(am, __shfl_xor(am, o, 64));
    if ((tid & 63) == 0) sAmax[tid >> 6] = am;
    __syncthreads();
    if (tid == 0) {
      float m = sAmax[0];
      for (int w = 1; w < 8; ++w) m = fmaxf(m, sAmax[w]);
      atomicMax(amax_out, __float_as_uint(m));
    }
  }
}

// dgamma / dbeta (/ the conv-bias gradients that fall out of the same sums) of MANY GroupNorm layers in one launch: the training
// step queues one job per layer while it walks the network backwards and flushes the queue at the end (44 launches -> 1).
__global__ void __launch_bounds__(64) param_grad_multi_kernel(GnParamJobs jobs) {
  const GnParamJob j = jobs.job[blockIdx.y];
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= j.channels) return;
  double g = 0.0, bt = 0.0, bs = 0.0, sy = 0.0;
  for (int n = 0; n < j.batch; ++n) {
    const f32x4 v = *(const f32x4*)(j.sums_bc + ((size_t)n * j.channels + c) * 4);
    bt += (double)v[0]; g += (double)v[1]; bs += (double)v[2]; sy += (double)v[3];
  }
  j.dgamma[c] = (float)g;
  j.dbeta[c] = (float)bt;
  if (j.dbias) j.dbias[c] = (float)bs;
  if (j.dsumdy) j.dsumdy[c] = (float)sy;
}
void launch_gn_param_jobs(const GnParamJobs& jobs, hipStream_t s) {
  if (jobs.n <= 0) return;
  int cmax = 0;
  for (int i = 0; i < jobs.n; ++i) cmax = jobs.job[i].channels > cmax ? jobs.job[i].channels : cmax;
  hipLaunchKernelGGL(param_grad_multi_kernel, dim3((unsigned)((cmax + 63) / 64), (unsigned)jobs.n), dim3(64), 0, s, jobs);
  CD_HIP(hipGetLastError());
}

void launch_gn_backward(const float* dy, const float* h, const float* coef, const float* stat, const float* gamma, float* dh,
                        float* dgamma, float* dbeta, float* dadd, int dadd_ld, int batch, int channels, int64_t vox, int groups,
                        int silu, float* scratch, bool accumulate_params, hipStream_t s, float* dbias, float* dsumdy,
                        GnParamQueue* queue, unsigned* dh_absmax) {
  CD_REQUIRE(channels % 4 == 0 && channels <= 256 && groups <= 64, "group norm backward: <= 256 channels, <= 64 groups");
  const int ns = gn_nsplit_for(vox, batch);
  float* part = scratch;                                         // [B][ns][C][4]
  float* gcoef = part + (size_t)batch * ns * channels * 4;        // [B][C][4]
  float* sums_bc = gcoef + (size_t)batch * channels * 4;          // [B][C][4]
  if (queue) {  // the per-sample sums go to the caller's persistent slot and the batch reduction joins the queue
    CD_REQUIRE(!accumulate_params, "gn backward: queued parameter gradients do not accumulate");
    if (queue->jobs.n == GnParamJobs::kMax) {  // (deeper networks than the shipped ones: flush and go on)
      if (!queue->discard) launch_gn_param_jobs(queue->jobs, s);
      queue->jobs.n = 0;
      queue->next_sums = queue->sums;
    }
    CD_REQUIRE(queue->next_sums + (size_t)batch * channels * 4 <= queue->sums_end, "gn backward: queued sums overflow their region");
    sums_bc = queue->next_sums;
    queue->next_sums += (size_t)batch * channels * 4;
    GnParamJob& j = queue->jobs.job[queue->jobs.n++];
    j.sums_bc = sums_bc; j.batch = batch; j.channels = channels; j.dgamma = dgamma; j.dbeta = dbeta; j.dbias = dbias; j.dsumdy = dsumdy;
  }
  prof::Scope scope("gn_backward", s, 0, 4.0 * batch * (double)vox * channels * 5);
  static const bool no_small = getenv("CD_NO_GN_BWD_SMALL") != nullptr;
  // (one workgroup streams its sample twice: 24 KB at the deepest level in ~6 us against four launches' ~20; at 188 KB -- level 1
  // with 64 channels -- it took 35 us against the split form's 27, so the bound sits between the two)
  static const size_t small_max = getenv("CD_GN_BWD_SMALL_KB") ? (size_t)atoi(getenv("CD_GN_BWD_SMALL_KB")) * 1024 : 100 * 1024;
  if (!no_small && (size_t)vox * channels * 4 <= small_max && channels <= 128 && 512 % (channels >> 2) == 0) {
    hipLaunchKernelGGL(gn_bwd_small_kernel, dim3((unsigned)batch), dim3(512), 0, s, dy, h, coef, stat, gamma, dh, sums_bc, dadd, dadd_ld,
                       channels, vox, groups, silu, dh_absmax);
    if (!queue)
      hipLaunchKernelGGL(param_grad_from_samples_kernel, dim3((channels + 63) / 64), dim3(64), 0, s, sums_bc, batch, channels, dgamma,
                         dbeta, accumulate_params ? 1 : 0, dbias, dsumdy);
    CD_HIP(hipGetLastError());
    return;
  }
  hipLaunchKernelGGL(gn_bwd_stats_kernel, dim3(ns, batch), dim3(256), 0, s, dy, h, coef, stat, part, channels, vox, groups, silu, ns);
  // the finalize arithmetic runs in the apply kernel's prologue when the parameter-gradient reduction is queued behind it
  // (stand-alone calls reduce over the batch right here, between the two, and keep the three-launch form)
  static const bool no_fold = getenv("CD_NO_GN_BWD_FOLD") != nullptr;
  GnBwdFold fold;
  if (queue && !no_fold) {
    fold.part = part; fold.gamma = gamma; fold.stat = stat; fold.sums_bc = sums_bc; fold.dadd = dadd; fold.nsplit = ns;
    fold.dadd_ld = dadd_ld; fold.groups = groups;
  } else {
    hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3(batch), dim3(256), 0, s, part, ns, gamma, stat, gcoef, sums_bc, dadd, dadd_ld,
                       channels, groups, vox);
  }
  if (!queue)
    hipLaunchKernelGGL(param_grad_from_samples_kernel, dim3((channels + 63) / 64), dim3(64), 0, s, sums_bc, batch, channels, dgamma,
                       dbeta, accumulate_params ? 1 : 0, dbias, dsumdy);
  // one round of workgroups: each repeats the finalize arithmetic in its prologue, so fewer and longer-lived ones win (same-box A/B at
  // batch 32: 7.31 -> 7.22 ms per training step from ~1024 to 256 workgroups; the forward gn_apply is neutral to the same change)
  static const int bwd_wgs = getenv("CD_GN_BWD_APPLY_WGS") ? atoi(getenv("CD_GN_BWD_APPLY_WGS")) : 256;
  int bps = gn_apply_blocks_per_sample(batch, channels, vox);
  const int bps_cap = (bwd_wgs + batch - 1) / batch;
  if (fold.part && bps > bps_cap) bps = bps_cap < 1 ? 1 : bps_cap;
  hipLaunchKernelGGL(gn_bwd_apply_kernel, dim3((unsigned)(batch * bps)), dim3(256), 0, s, dy, h, coef, gcoef, dh, channels, vox, silu, bps,
                     dh_absmax, fold);
  CD_HIP(hipGetLastError());
}

size_t gn_backward_scratch_floats(int batch, int channels, int64_t vox) {
  const int ns = gn_nsplit_for(vox, batch);
  return (size_t)batch * ns * channels * 4 + (size_t)batch * channels * 8 + 64;
}

}  // namespace cd
