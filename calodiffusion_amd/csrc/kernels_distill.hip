// Consistency distillation (Song et al. 2023, Algorithm 2; calodiffusion_amd/distill.py), the two streaming passes around the
// denoise calls and the training step: the one-step ODE solve from sigma_hi to sigma_lo with a noise level per sample
// (cd_ode_step) and the EMA update of the target network over all its tensors (cd_ema_step).  Stateless: no plan, no workspace.
#include "guarded.h"

#include <cstdint>

namespace cd {

// ------------------------------------------------------------------------------------------------------------
// One ODE step of the probability-flow ODE dx/dsigma = (x - D(x, sigma)) / sigma from sigma_hi down to sigma_lo:
//   Euler:  d = (x_hi - D_hi) / sigma_hi;                      x_lo = x_hi + (sigma_lo - sigma_hi) d
//   Heun:   d2 = (x_e - D_e) / sigma_lo  (x_e the Euler x_lo);  x_lo = x_hi + (sigma_lo - sigma_hi) (0.5 (d + d2))
// Every product, difference and quotient rounded on its own, as a chain of torch elementwise kernels rounds them.
// ------------------------------------------------------------------------------------------------------------
template <bool HEUN>
__device__ __forceinline__ float ode_one(float xh, float dh, float xe, float de, float sh, float sl, float dt) {
#pragma clang fp contract(off)
  const float num = xh - dh;
  const float d = num / sh;
  if (!HEUN) {
    const float st = dt * d;
    return xh + st;
  }
  const float num2 = xe - de;
  const float d2 = num2 / sl;
  const float sum = d + d2;
  const float avg = 0.5f * sum;
  const float st = dt * avg;
  return xh + st;
}

// One pass: grid (blocks per row, batch), a row = one sample's `per` floats.  16 bytes per lane over the part of the row that starts
// at the first 16-byte boundary of x_hi's row, when the other rows share that boundary (contiguous tensors of one shape do, whatever
// `per`); the floats before it and the up to 3 after the last whole vector go one per lane, and so does the whole row when the
// rows' alignments differ.  A lane reads its elements of x_e before it writes them to x_lo: in place when the two are one buffer
// (no __restrict__ on either).
template <bool HEUN>
__global__ void __launch_bounds__(256) ode_step_kernel(const float* __restrict__ x_hi, const float* __restrict__ d_hi, const float* x_e,
                                                       const float* __restrict__ d_e, const float* __restrict__ sigma_hi,
                                                       const float* __restrict__ sigma_lo, float* x_lo, int64_t per) {
  const int b = blockIdx.y;
  const float sh = sigma_hi[b], sl = sigma_lo[b];
  const float dt = sl - sh;
  const size_t base = (size_t)b * per;
  const float* xh = x_hi + base;
  const float* dh = d_hi + base;
  const float* xe = HEUN ? x_e + base : nullptr;
  const float* de = HEUN ? d_e + base : nullptr;
  float* xl = x_lo + base;
  int64_t head = (int64_t)(((16 - ((uintptr_t)xh & 15)) & 15) >> 2);
  if (head > per) head = per;
  uintptr_t mis = (uintptr_t)(xh + head) | (uintptr_t)(dh + head) | (uintptr_t)(xl + head);
  if (HEUN) mis |= (uintptr_t)(xe + head) | (uintptr_t)(de + head);
  if (mis & 15) head = per;
  const int64_t nvec = (per - head) >> 2, tail = head + nvec * 4;
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  for (int64_t v = t0; v < nvec; v += stride) {
    const int64_t i = head + v * 4;  // (< tail <= per)
    const f32x4 a = *(const f32x4*)(xh + i), c = *(const f32x4*)(dh + i);
    f32x4 e = {0.f, 0.f, 0.f, 0.f}, g = {0.f, 0.f, 0.f, 0.f};
    if (HEUN) {
      e = *(const f32x4*)(xe + i);
      g = *(const f32x4*)(de + i);
    }
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = ode_one<HEUN>(a[k], c[k], e[k], g[k], sh, sl, dt);
    *(f32x4*)(xl + i) = o;
  }
  // the scalar ends: [0, head) and [tail, per)
  const int64_t nscalar = head + (per - tail);
  for (int64_t j = t0; j < nscalar; j += stride) {
    const int64_t i = j < head ? j : tail + (j - head);
    xl[i] = ode_one<HEUN>(xh[i], dh[i], HEUN ? xe[i] : 0.f, HEUN ? de[i] : 0.f, sh, sl, dt);
  }
}

static void launch_ode_step(const float* x_hi, const float* d_hi, const float* x_e, const float* d_e, const float* sigma_hi,
                            const float* sigma_lo, float* x_lo, int batch, int64_t per, hipStream_t s) {
  // a memory-bound pass: about 2048 workgroups at the most, each lane 16 bytes of every operand per trip
  int64_t bx = (per + 1023) / 1024, cap = 2048 / batch;
  if (cap < 1) cap = 1;
  if (bx > cap) bx = cap;
  if (bx < 1) bx = 1;
  const dim3 grid((unsigned)bx, (unsigned)batch);
  if (x_e) hipLaunchKernelGGL(ode_step_kernel<true>, grid, dim3(256), 0, s, x_hi, d_hi, x_e, d_e, sigma_hi, sigma_lo, x_lo, per);
  else hipLaunchKernelGGL(ode_step_kernel<false>, grid, dim3(256), 0, s, x_hi, d_hi, x_e, d_e, sigma_hi, sigma_lo, x_lo, per);
  CD_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------------------
// EMA of the target network: dst <- mu dst + (1 - mu) src over many tensors, one launch per 48 (the kernel-argument table of
// cd_adam_step: a U-Net's ~230 tensors hold about 9 MB together, one launch each would cost more than the arithmetic).
// ------------------------------------------------------------------------------------------------------------
struct EmaChunk {
  float* dst[48];
  const float* src[48];
  int64_t n[48];
};
__global__ void __launch_bounds__(256) ema_kernel(EmaChunk c, float mu, float w) {
#pragma clang fp contract(off)
  const int t = blockIdx.y;
  float* __restrict__ dst = c.dst[t];
  const float* __restrict__ src = c.src[t];
  const int64_t n = c.n[t];
  // 16 bytes per lane when both tensors start on a 16-byte boundary (every tensor of its own allocation does), the up to 3 floats
  // after the last whole vector one per lane; else everything one per lane
  const int64_t nvec = (((uintptr_t)dst | (uintptr_t)src) & 15) ? 0 : n >> 2;
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  for (int64_t v = t0; v < nvec; v += stride) {
    const f32x4 a = *(const f32x4*)(dst + v * 4), b = *(const f32x4*)(src + v * 4);
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float keep = mu * a[k];
      const float take = w * b[k];
      o[k] = keep + take;
    }
    *(f32x4*)(dst + v * 4) = o;
  }
  for (int64_t i = nvec * 4 + t0; i < n; i += stride) {
    const float keep = mu * dst[i];
    const float take = w * src[i];
    dst[i] = keep + take;
  }
}

}  // namespace cd

extern "C" {

int cd_ode_step(const float* x_hi, const float* d_hi, const float* x_e, const float* d_e, const float* sigma_hi, const float* sigma_lo,
                float* x_lo, int batch, int64_t per, void* stream) {
  return guarded([&] {
    CD_REQUIRE(x_hi && d_hi && sigma_hi && sigma_lo && x_lo && batch > 0 && batch <= 65535 && per > 0, "bad argument");
    CD_REQUIRE((x_e == nullptr) == (d_e == nullptr), "cd_ode_step: x_e and d_e come together (Heun) or not at all (Euler)");
    launch_ode_step(x_hi, d_hi, x_e, d_e, sigma_hi, sigma_lo, x_lo, batch, per, (hipStream_t)stream);
  });
}

int cd_ema_step(int n, float* const* dst, const float* const* src, const int64_t* numel, double mu, void* stream) {
  return guarded([&] {
    CD_REQUIRE(n >= 0 && (n == 0 || (dst && src && numel)), "bad argument");
    CD_REQUIRE(mu >= 0.0 && mu < 1.0, "cd_ema_step: mu must lie in [0, 1)");
    // 1 - mu in double (a python float), then rounded once to fp32, as torch rounds the alpha of add(src, alpha=1 - mu)
    const float muf = (float)mu, w = (float)(1.0 - mu);
    for (int i0 = 0; i0 < n; i0 += 48) {
      EmaChunk c{};
      const int k = n - i0 < 48 ? n - i0 : 48;
      int64_t mx = 0;
      for (int j = 0; j < k; ++j) {
        c.dst[j] = dst[i0 + j]; c.src[j] = src[i0 + j]; c.n[j] = numel[i0 + j];
        CD_REQUIRE(c.dst[j] && c.src[j] && c.n[j] >= 0, "ema: null tensor pointer");
        if (c.n[j] > mx) mx = c.n[j];
      }
      int64_t bx = (mx + 1023) / 1024;
      if (bx < 1) bx = 1;
      if (bx > 1024) bx = 1024;
      hipLaunchKernelGGL(ema_kernel, dim3((unsigned)bx, (unsigned)k), dim3(256), 0, (hipStream_t)stream, c, muf, w);
      CD_HIP(hipGetLastError());
    }
  });
}

}  // extern "C"
