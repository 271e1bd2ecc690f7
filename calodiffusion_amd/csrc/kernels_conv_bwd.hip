// What the convolutions' backward needs besides the forward conv kernels (input gradients: re-packed weights) and the weight
// gradients (kernels_wgrad.hip): the bias gradient from channel partials, the fan-in of gradient slices of a channel concat, the
// input gradient of the strided conv on an odd phi ring, and the phi fold of the transposed conv's odd output ring.  Reference:
// torch autograd through CylindricalConv / CylindricalConvTrans (models.py:25-96); host side: conv_backward.hip.
#include "kernels_bwd.h"

namespace cd {

// ------------------------------------------------------------------------------------------------------------
// Per-channel sums over (batch, voxels): bias gradients.  part: channel partials [B][units][C][2] (only the sums are used)
// ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) bias_grad_kernel(const float* __restrict__ part, int units, int batch, int channels,
                                                        float* __restrict__ db, int accumulate) {
  // block = 8 channels x 32 slices of the (batch x units) partial rows; fixed-order tree => deterministic
  __shared__ double sh[32][8];
  const int cl = threadIdx.x & 7, sl = threadIdx.x >> 3;
  const int c = blockIdx.x * 8 + cl;
  const int rows = batch * units;
  double s = 0.0;
  if (c < channels)
    for (int r = sl; r < rows; r += 32) s += (double)part[((size_t)r * channels + c) * 2];
  sh[sl][cl] = s;
  __syncthreads();
  if (sl == 0 && c < channels) {
    double t = 0.0;
    for (int k = 0; k < 32; ++k) t += sh[k][cl];
    db[c] = accumulate ? db[c] + (float)t : (float)t;
  }
}
void launch_bias_grad(const float* part, int units, int batch, int channels, float* db, bool accumulate, hipStream_t s) {
  hipLaunchKernelGGL(bias_grad_kernel, dim3((channels + 7) / 8), dim3(256), 0, s, part, units, batch, channels, db, accumulate ? 1 : 0);
  CD_HIP(hipGetLastError());
}

// out[v][c] = a[v][aoff + c] + (b ? b[v][boff + c] : 0)   (row strides lda / ldb / C): gradient fan-in, channel slices of
// the gradient of a concatenated tensor
__global__ void add_slices_kernel(const float* __restrict__ a, int lda, int aoff, const float* __restrict__ b, int ldb, int boff,
                                  float* __restrict__ out, int channels, int64_t rows) {
  const int cols = channels >> 2;
  if (256 % cols == 0) {
    // a thread keeps its channel quad and walks rows (the general form below divides a 64-bit index twice per element: ~200 vector
    // instructions around three 16-byte memory operations); four rows per trip, their loads issued together
    const int c = (threadIdx.x % cols) * 4, rpb = 256 / cols;
    const int64_t stride = (int64_t)gridDim.x * rpb;
    int64_t r = (int64_t)blockIdx.x * rpb + threadIdx.x / cols;
    for (; r + 3 * stride < rows; r += 4 * stride) {
      f32x4 v[4], w[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[k] = *(const f32x4*)(a + (size_t)(r + k * stride) * lda + aoff + c);
        if (b) w[k] = *(const f32x4*)(b + (size_t)(r + k * stride) * ldb + boff + c);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) *(f32x4*)(out + (size_t)(r + k * stride) * channels + c) = b ? v[k] + w[k] : v[k];
    }
    for (; r < rows; r += stride) {
      f32x4 v = *(const f32x4*)(a + (size_t)r * lda + aoff + c);
      if (b) v += *(const f32x4*)(b + (size_t)r * ldb + boff + c);
      *(f32x4*)(out + (size_t)r * channels + c) = v;
    }
    return;
  }
  const int64_t total = rows * cols;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / cols;
    const int c = (int)(i % cols) * 4;
    f32x4 v = *(const f32x4*)(a + (size_t)r * lda + aoff + c);
    if (b) v += *(const f32x4*)(b + (size_t)r * ldb + boff + c);
    *(f32x4*)(out + (size_t)r * channels + c) = v;
  }
}
void launch_add_slices(const float* a, int lda, int aoff, const float* b, int ldb, int boff, float* out, int channels,
                       int64_t rows, hipStream_t s) {
  int64_t blocks = (rows * (channels / 4) + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(add_slices_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a, lda, aoff, b, ldb, boff, out, channels, rows);
  CD_HIP(hipGetLastError());
}

// Input gradient of the strided (KD,4,4) down conv for ODD phi extents.  With an even phi ring the adjoint coincides with the
// up-conv gather kernel (conv_transpose_kernel); with an odd ring the circular halo rows break its parity classes, so this
// (rare: Dataset-1 grid) case takes a plain gather:  dx[i][ci] = sum_{o,k : in(o,k) = i} sum_co dy[o][co] * w[co][ci][k].
// One thread per (input voxel, ci).
__global__ void strided_dgrad_naive_kernel(const float* __restrict__ dy, const float* __restrict__ w, float* __restrict__ dx,
                                           int cin, int cout, int D, int H, int W, int Do, int Ho, int Wo, int KD, int SZ) {
  const int64_t vox = (int64_t)D * H * W;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (idx >= vox * cin) return;
  const int ci = (int)(idx % cin);
  const int v = (int)(idx / cin);
  const int iw = v % W, ih = (v / W) % H, iz = v / (W * H);
  float acc = 0.f;
  for (int kz = 0; kz < KD; ++kz) {
    const int tz = iz + 1 - kz;
    if (tz < 0 || tz % SZ) continue;
    const int oz = tz / SZ;
    if (oz >= Do) continue;
    for (int kw = 0; kw < 4; ++kw) {
      const int tw = iw + 1 - kw;
      if (tw < 0 || (tw & 1)) continue;
      const int ow = tw >> 1;
      if (ow >= Wo) continue;
      for (int kh = 0; kh < 4; ++kh) {
        // padded row r = 2*oh + kh covers input row (r - 1) mod H for r in [0, H+2)
        for (int rr = 0; rr < 3; ++rr) {
          const int r = ih + 1 + (rr - 1) * H;
          if (r < 0 || r > H + 1) continue;
          const int th = r - kh;
          if (th < 0 || (th & 1)) continue;
          const int oh = th >> 1;
          if (oh >= Ho) continue;
          const float* g = dy + (((size_t)b * Do + oz) * Ho + oh) * (size_t)Wo * cout + (size_t)ow * cout;
          const float* wr = w + (size_t)ci * KD * 16 + (kz * 4 + kh) * 4 + kw;
          for (int co = 0; co < cout; ++co) acc = fmaf(g[co], wr[(size_t)co * cin * KD * 16], acc);
        }
      }
    }
  }
  dx[((size_t)b * vox + v) * cin + ci] = acc;
}
void launch_strided_dgrad_naive(const float* dy, const float* w, float* dx, int batch, int cin, int cout, Dims3 din, Dims3 dout,
                                int kd, int sz, hipStream_t s) {
  const int64_t total = din.vox() * cin;
  hipLaunchKernelGGL(strided_dgrad_naive_kernel, dim3((unsigned)((total + 255) / 256), batch), dim3(256), 0, s, dy, w, dx, cin, cout,
                     din.d, din.h, din.w, dout.d, dout.h, dout.w, kd, sz);
  CD_HIP(hipGetLastError());
}

// Up-sampling to an ODD phi extent (output_padding 1 along phi): the forward's last phi row duplicates row 0 (both read
// the same wrapped inputs), so its adjoint first folds the gradient of row H-1 into row 0 and then proceeds on the even
// ring of H-1 rows.  dst: (B, D, H-1, W, C) <- src: (B, D, H, W, C)
__global__ void fold_phi_kernel(const float* __restrict__ src, float* __restrict__ dst, int D, int H, int W, int C, int batch) {
  const int c4 = C >> 2;
  const int64_t total = (int64_t)batch * D * (H - 1) * W * c4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int q = (int)(i % c4);
    int64_t r = i / c4;
    const int w = (int)(r % W);
    r /= W;
    const int h = (int)(r % (H - 1));
    const int64_t bz = r / (H - 1);
    const float* s0 = src + (((size_t)bz * H + h) * W + w) * C + q * 4;
    f32x4 v = *(const f32x4*)s0;
    if (h == 0) v += *(const f32x4*)(src + (((size_t)bz * H + (H - 1)) * W + w) * C + q * 4);
    *(f32x4*)(dst + (size_t)i * 4) = v;
  }
}
void launch_fold_phi(const float* src, float* dst, int batch, Dims3 d, int C, hipStream_t s) {
  int64_t blocks = ((int64_t)batch * d.d * (d.h - 1) * d.w * (C / 4) + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(fold_phi_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, dst, d.d, d.h, d.w, C, batch);
  CD_HIP(hipGetLastError());
}

}  // namespace cd
