// The U-Net's first convolution for gfx950: scalar and matrix-core forms.
#include "conv_internal.h"

namespace cd {

// ------------------------------------------------------------------------------------------------------------
// init conv: 3x3x3 cylindrical conv from a few planar channels (x, and the constant R / Z / phi coordinate images,
// synthesised from their 1-D profiles instead of being materialised: calodiffusion.py:121-142) to 32*k channels-last.
// One thread per output voxel; weights are wave-uniform => scalar loads.
// ------------------------------------------------------------------------------------------------------------
template <int CIN>
__global__ void __launch_bounds__(256) init_conv_kernel(InitConvArgs a) {
  const int64_t vox = a.dims.vox();
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  const int ct = blockIdx.z;
  const bool valid = n < vox;
  const int D = a.dims.d, H = a.dims.h, W = a.dims.w;
  const int nn = valid ? (int)n : 0;
  const int w = nn % W, h = (nn / W) % H, z = nn / (W * H);
  float sc = (a.x && a.scale_b) ? a.scale_b[(size_t)b * a.scale_stride] : 1.f;
  if (a.x && a.sigma_b) {  // same expression as embed_kernel's c_in
    const float tv = a.sigma_b[b], sd = a.sigma_data;
    sc = 1.f / sqrtf(tv * tv + sd * sd);
  }

  float acc[32];
  const float* __restrict__ bias = a.bias;
#pragma unroll
  for (int j = 0; j < 32; ++j) acc[j] = bias ? bias[ct * 32 + j] : 0.f;

  // this channel tile's weights in LDS (27 CIN rows of 32): read from global as wave-uniform scalar loads they were 81 dependent
  // round trips per thread -- 52 us for the batch-1 coordinate table the training step refreshes every step (26 workgroups)
  __shared__ __attribute__((aligned(16))) float wsm[27 * CIN * 32];
  for (int i = threadIdx.x; i < 27 * CIN * 32; i += 256) wsm[i] = a.wpk[(size_t)(i >> 5) * a.cout + ct * 32 + (i & 31)];
  __syncthreads();
  for (int kd = 0; kd < 3; ++kd) {
    const int zz = z + kd - 1;
    for (int kh = 0; kh < 3; ++kh) {
      int hh = h + kh - 1;
      hh = hh < 0 ? hh + H : (hh >= H ? hh - H : hh);
      hh = hh % H;  // H == 1 or 2
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int ww = w + kw - 1;
        const bool inb = valid && zz >= 0 && zz < D && ww >= 0 && ww < W;
        const int tap = (kd * 3 + kh) * 3 + kw;
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) {
          float v = 0.f;
          if (inb) {
            if (ci < a.cx) {
              if (a.x) {  // null: only the synthesised channels contribute (coordinate table of the matrix-core path)
                v = a.x[(((size_t)b * a.cx + ci) * D + zz) * H * W + (size_t)hh * W + ww];
                if (ci == 0) v *= sc;
              }
            } else {
              const int k = ci - a.cx;
              if (a.use_rz) v = (k == 0) ? a.r_w[ww] : (k == 1 ? a.z_d[zz] : a.phi_h[hh]);
              else v = a.phi_h[hh];
            }
          }
          const float* wr = wsm + (tap * CIN + ci) * 32;
#pragma unroll
          for (int j = 0; j < 32; ++j) acc[j] = fmaf(v, wr[j], acc[j]);
        }
      }
    }
  }
  if (valid) {
    f32x4* o = (f32x4*)(a.out + ((size_t)b * vox + n) * a.cout + ct * 32);
#pragma unroll
    for (int q = 0; q < 8; ++q) o[q] = f32x4{acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
  }
}

// The same conv on the matrix cores when x is the only data channel (the denoiser's case).  The conv is linear in its input
// channels: the coordinate channels' contribution (+ bias) is the same for every sample and step -- `table` (vox, cout), filled
// by one batch-1 launch of the kernel above with x = null -- and what remains is a 27-tap, one-channel conv of c_in * x:
// K = 27 padded to 32 = two fp16 k-steps (f16x2: three MFMAs each) per 32 voxels instead of 27 * cin * 32 scalar FMAs per
// voxel.  A workgroup owns TZ z-planes of one sample: c_in * x of those planes (+ halo: zero planes / columns outside the
// grid, phi rows wrapped) sits in LDS as fp32, so every tap of every voxel is "base + constant".
__global__ void __launch_bounds__(256) init_conv_f16x2_kernel(InitConvArgs a, const float* __restrict__ table, int TZ) {
  extern __shared__ __attribute__((aligned(16))) float img[];
  __shared__ __attribute__((aligned(16))) float trn[4 * 32 * 36];  // per-wave output tile on its way to row-major quads
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
  const int b = blockIdx.y;
  const int D = a.dims.d, H = a.dims.h, W = a.dims.w, PV = H * W;
  const int z0 = blockIdx.x * TZ, nz = min(TZ, D - z0);
  const int HP = H + 2, WP = W + 2;
  float sc = a.scale_b ? a.scale_b[(size_t)b * a.scale_stride] : 1.f;
  if (a.sigma_b) {  // same expression as embed_kernel's c_in
    const float tv = a.sigma_b[b], sd = a.sigma_data;
    sc = 1.f / sqrtf(tv * tv + sd * sd);
  }
  {
    const float* xb = a.x + (size_t)b * D * PV;
    float amax = 0.f;
    const float inv_wp = 1.f / (float)WP, inv_hp = 1.f / (float)HP;
    for (int i = tid; i < (nz + 2) * HP * WP; i += 256) {
      const int r = (int)(((float)i + 0.5f) * inv_wp), lw = i - r * WP, lz = (int)(((float)r + 0.5f) * inv_hp), lh = r - lz * HP;
      const int gz = z0 - 1 + lz, gw = lw - 1;
      int gh = lh - 1;
      gh = gh < 0 ? gh + H : (gh >= H ? gh - H : gh);
      gh = gh % H;  // H == 1 or 2
      float v = 0.f;
      if (gz >= 0 && gz < D && gw >= 0 && gw < W) v = xb[((size_t)gz * H + gh) * W + gw] * sc;
      amax = fmaxf(amax, fabsf(v));
      img[i] = v;
    }
    if (a.status && amax > 65504.f) atomicOr(a.status, 1);
  }
  // this lane's 16 im2col columns: k = ks*16 + half*8 + e = tap index (k >= 27: zero weight, any readable cell)
  int toff[2][8];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = ks * 16 + half * 8 + e;
      const int kz = k / 9, kh = (k / 3) % 3, kw = k % 3;
      toff[ks][e] = k < 27 ? (kz * HP + kh) * WP + kw : 0;
    }
  __syncthreads();
  const int nvox = nz * PV, ntiles = (nvox + 31) / 32;
  const int64_t vox = a.dims.vox();
  const float inv_pv = 1.f / (float)PV, inv_w = 1.f / (float)W;
  for (int ct = 0; ct < a.cout / 32; ++ct) {
    u32x4 w1[2], w2[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      f32x4 wv[2];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = ks * 16 + half * 8 + e;
        wv[e >> 2][e & 3] = k < 27 ? a.wpk[((size_t)k * a.cin) * a.cout + ct * 32 + col] : 0.f;
      }
      u32x2 a1, a2, b1, b2;
      split2(wv[0], a1, a2);
      split2(wv[1], b1, b2);
      w1[ks] = u32x4{a1[0], a1[1], b1[0], b1[1]};
      w2[ks] = u32x4{a2[0], a2[1], b2[0], b2[1]};
    }
    // the table rows of a tile as whole 16-byte quads, row 8 k + (lane >> 3), channels 4 (lane & 7) .. + 3 -- the layout the tile is
    // stored in after a transpose through LDS (16 scalar row stores per lane in accumulator layout ran at a third of the HBM rate) --
    // requested ONE TILE AHEAD (round 4): with two waves per SIMD a tile's gather and six MFMAs are ~150 ns, an L2 round trip several
    // times that, and the tile ended up waiting for its own table rows
    auto load_table = [&](int tile, f32x4 (&t4)[4]) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int vr = min(tile * 32 + 8 * k + (lane >> 3), nvox - 1);
        t4[k] = *(const f32x4*)(table + ((size_t)z0 * PV + vr) * a.cout + ct * 32 + (lane & 7) * 4);
      }
    };
    f32x4 tb[4], tbn[4];
    load_table(min(wave, ntiles - 1), tb);
    for (int tile = wave; tile < ntiles; tile += 4) {
      const int v = min(tile * 32 + col, nvox - 1);
      // (exact small-integer division by reciprocal: (v + 0.5) / d is never within float error of an integer for v < 2^20; two run-time
      // integer divisions were ~80 of a tile's ~300 instructions)
      const int lz = (int)(((float)v + 0.5f) * inv_pv), p = v - lz * PV, h = (int)(((float)p + 0.5f) * inv_w), w = p - h * W;
      const float* base = img + (lz * HP + h) * WP + w;
      load_table(min(tile + 4, ntiles - 1), tbn);
      f32x16 accA, accB;
#pragma unroll
      for (int r = 0; r < 16; ++r) accA[r] = accB[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        f32x4 xv[2];
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[e >> 2][e & 3] = base[toff[ks][e]];
        u32x2 a1, a2, b1, b2;
        split2(xv[0], a1, a2);
        split2(xv[1], b1, b2);
        const u32x4 x1 = {a1[0], a1[1], b1[0], b1[1]}, x2 = {a2[0], a2[1], b2[0], b2[1]};
        accA = MFMA_F16(x1, w1[ks], accA);
        accB = MFMA_F16(x1, w2[ks], accB);
        accB = MFMA_F16(x2, w1[ks], accB);
      }
      float* tr = trn + wave * (32 * 36);  // this wave's 32 x 32 tile, rows padded to 36 floats
#pragma unroll
      for (int r = 0; r < 16; ++r) tr[((r & 3) + 8 * (r >> 2) + 4 * half) * 36 + col] = accA[r] + accB[r] * (1.f / 2048.f);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (one wave: its own LDS writes are visible to its reads in order)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int row = 8 * k + (lane >> 3);
        const int vr = tile * 32 + row;
        const f32x4 o = *(const f32x4*)(tr + row * 36 + (lane & 7) * 4) + tb[k];
        if (vr < nvox) *(f32x4*)(a.out + ((size_t)b * vox + (size_t)z0 * PV + vr) * a.cout + ct * 32 + (lane & 7) * 4) = o;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) tb[k] = tbn[k];
    }
  }
}

void launch_init_coord_table(const InitConvArgs& a, hipStream_t s) {
  CD_REQUIRE(a.coord_table && a.cout % 32 == 0 && a.cin >= 1 && a.cin <= 4, "init conv table: bad arguments");
  // the scalar kernel at batch 1 without x
  InitConvArgs t = a;
  t.x = nullptr; t.cx = 1; t.batch = 1; t.out = a.coord_table; t.scale_b = nullptr; t.sigma_b = nullptr;
  dim3 tgrid((unsigned)((a.dims.vox() + 255) / 256), 1u, (unsigned)(a.cout / 32));
  switch (a.cin) {
    case 1: hipLaunchKernelGGL(init_conv_kernel<1>, tgrid, dim3(256), 0, s, t); break;
    case 2: hipLaunchKernelGGL(init_conv_kernel<2>, tgrid, dim3(256), 0, s, t); break;
    case 3: hipLaunchKernelGGL(init_conv_kernel<3>, tgrid, dim3(256), 0, s, t); break;
    case 4: hipLaunchKernelGGL(init_conv_kernel<4>, tgrid, dim3(256), 0, s, t); break;
  }
  CD_HIP(hipGetLastError());
}

void launch_init_conv(const InitConvArgs& a, hipStream_t s) {
  CD_REQUIRE(a.cout % 32 == 0, "init conv: output channels must be a multiple of 32");
  CD_REQUIRE(a.cin >= 1 && a.cin <= 4 && a.cx <= a.cin, "init conv: 1..4 input channels supported");
  const bool full_range = conv_precision() != PREC_F16X2;
  static const bool no_mfma = getenv("CD_NO_INIT_MFMA") != nullptr;
  if (a.coord_table && a.cx == 1 && a.x && !full_range && !no_mfma) {
    prof::Scope scope("init_conv", s, 2.0 * 27 * a.cin * a.cout * (double)a.dims.vox() * a.batch,
                      4.0 * a.batch * (double)a.dims.vox() * (a.cx + a.cout));
    if (!a.table_ready) launch_init_coord_table(a, s);  // (~25 us of scalar-kernel latency: callers that can, keep the table)
    // 2. the x part on the matrix cores: TZ planes per workgroup, about two rounds of workgroups
    const int D = a.dims.d;
    static const int init_wgs = getenv("CD_INIT_WGS") ? atoi(getenv("CD_INIT_WGS")) : 512;
    int slabs = (init_wgs + a.batch - 1) / a.batch;
    slabs = slabs < 1 ? 1 : (slabs > D ? D : slabs);
    int TZ = (D + slabs - 1) / slabs;
    while (TZ > 1 && (size_t)(TZ + 2) * (a.dims.h + 2) * (a.dims.w + 2) * 4 > 60 * 1024) --TZ;
    const size_t lds = (size_t)(TZ + 2) * (a.dims.h + 2) * (a.dims.w + 2) * 4;
    CD_REQUIRE(lds <= 64 * 1024, "init conv: plane too large for the LDS image");
    dim3 grid((unsigned)((D + TZ - 1) / TZ), (unsigned)a.batch);
    hipLaunchKernelGGL(init_conv_f16x2_kernel, grid, dim3(256), lds, s, a, (const float*)a.coord_table, TZ);
    CD_HIP(hipGetLastError());
    return;
  }
  dim3 grid((unsigned)((a.dims.vox() + 255) / 256), (unsigned)a.batch, (unsigned)(a.cout / 32));
  prof::Scope scope("init_conv", s, 2.0 * 27 * a.cin * a.cout * (double)a.dims.vox() * a.batch,
                    4.0 * a.batch * (double)a.dims.vox() * (a.cx + a.cout));
  switch (a.cin) {
    case 1: hipLaunchKernelGGL(init_conv_kernel<1>, grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL(init_conv_kernel<2>, grid, dim3(256), 0, s, a); break;
    case 3: hipLaunchKernelGGL(init_conv_kernel<3>, grid, dim3(256), 0, s, a); break;
    case 4: hipLaunchKernelGGL(init_conv_kernel<4>, grid, dim3(256), 0, s, a); break;
  }
  CD_HIP(hipGetLastError());
}

}  // namespace cd
