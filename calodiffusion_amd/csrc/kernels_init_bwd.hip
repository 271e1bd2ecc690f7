// Backward of the init conv (cin <= 4 logical channels: c_in * x and the synthesised coordinate channels; forward:
// kernels_init_conv.hip): the input gradient of the data channel with the EDM preconditioning in its epilogue (cd_denoise_vjp),
// and the weight gradient -- a scalar kernel, or the general 3x3x3 weight-gradient ladder on a padded 32-channel input.
#include "kernels_bwd.h"
#include "kernels_wgrad.h"

namespace cd {

// ------------------------------------------------------------------------------------------------------------
// Init conv input gradient of the data channel with the EDM preconditioning in its epilogue (cd_denoise_vjp):
//   dx[b][v] = a_b gy[b][v] + c_in_b sum_{c,tap} W[c][0][tap] G[b][v - tap][c]
//   a_b = c_skip (hybrid), 1 (noise_pred), 0 (mean_pred);  phi wraps, z and r are zero-padded (the forward's cyl_conv).
// Channels first, stencil second: per staged voxel the 27 tap sums P[tap] = sum_c W[c][tap] G[v][c] (27 C0 FMAs on one 4 C0-byte
// row of G), parked in LDS for one z-plane of a phi band; each output voxel then gathers its in-plane 3x3 neighbours' P for the
// three z-taps and keeps three running plane sums in registers while the block walks its z-chunk, VZ planes per trip (each weight
// read from LDS then serves VZ FMAs: with one plane per trip the broadcast weight reads bound the kernel).  G is read once per chunk
// (+ one halo plane on either side, + one halo phi row on either side when a plane is split into bands); the next trip's rows are
// loaded while the current ones are reduced.  Deterministic: every sum has a fixed order.
// ------------------------------------------------------------------------------------------------------------
template <int C0, int VZ>
__global__ void __launch_bounds__(256) init_dgrad_kernel(const float* __restrict__ g, const float* __restrict__ w_raw, int cin,
                                                         const float* __restrict__ gy, const float* __restrict__ scal, int objective,
                                                         float* __restrict__ dx, Dims3 dims, int band, int halo, int zc) {
  constexpr int NQ = C0 / 4;
  __shared__ __attribute__((aligned(16))) float sW[C0][28];  // W[c][0][tap], padded to 7 float4
  __shared__ float sP[VZ][27][256];
  const int tid = threadIdx.x;
  const int chunk = blockIdx.x, bi = blockIdx.y, b = blockIdx.z;
  const int D = dims.d, H = dims.h, W = dims.w;
  const int64_t HW = (int64_t)H * W;
  for (int i = tid; i < C0 * 28; i += blockDim.x) {
    const int c = i / 28, tap = i % 28;
    sW[c][tap] = tap < 27 ? w_raw[(size_t)c * cin * 27 + tap] : 0.f;
  }
  const int rows = band + 2 * halo;
  const int lr = tid / W, w = tid % W;
  const bool stage = lr < rows;  // this thread stages voxel (row lr of the band incl. halo, column w)
  const int h0 = bi * band;
  int hs = h0 - halo + lr;
  hs = ((hs % H) + H) % H;
  const int orow = lr - halo, ho = h0 + orow;
  const bool out = stage && orow >= 0 && orow < band && ho < H;
  const int z0 = chunk * zc, z1 = min(z0 + zc, D);
  const float* gb = g + ((size_t)b * D * HW + (size_t)hs * W + w) * C0;
  // planes z0 - 1 .. z1 are read (the halo planes included); others count as zero
  auto live = [&](int z) { return z >= 0 && z < D && z <= z1; };
  auto load = [&](int z, f32x4* v) {
    const bool ok = stage && live(z);
#pragma unroll
    for (int q = 0; q < NQ; ++q) v[q] = ok ? *(const f32x4*)(gb + (size_t)z * HW * C0 + q * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
  };
  f32x4 cur[VZ][NQ];
#pragma unroll
  for (int k = 0; k < VZ; ++k) load(z0 - 1 + k, cur[k]);
  __syncthreads();
  float am = 0.f, a0 = 0.f, ap = 0.f;  // running sums of output planes zi - 1, zi, zi + 1
  // VZ input planes per trip: each weight read from LDS feeds VZ FMAs
  for (int zb = z0 - 1; zb <= z1; zb += VZ) {
    float sm[VZ][3];
#pragma unroll
    for (int k = 0; k < VZ; ++k) sm[k][0] = sm[k][1] = sm[k][2] = 0.f;
    bool any = false;
#pragma unroll
    for (int k = 0; k < VZ; ++k) any = any || live(zb + k);
    if (any) {  // (block-uniform)
      f32x4 nxt[VZ][NQ];
#pragma unroll
      for (int k = 0; k < VZ; ++k) load(zb + VZ + k, nxt[k]);
      if (stage) {
        float acc[VZ][27];
#pragma unroll
        for (int k = 0; k < VZ; ++k)
#pragma unroll
          for (int t = 0; t < 27; ++t) acc[k][t] = 0.f;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int c = q * 4 + e;
#pragma unroll
            for (int t4 = 0; t4 < 7; ++t4) {
              const f32x4 wv = *(const f32x4*)&sW[c][t4 * 4];
#pragma unroll
              for (int j = 0; j < 4; ++j)
                if (t4 * 4 + j < 27)
#pragma unroll
                  for (int k = 0; k < VZ; ++k) acc[k][t4 * 4 + j] = fmaf(wv[j], cur[k][q][e], acc[k][t4 * 4 + j]);
            }
          }
        }
#pragma unroll
        for (int k = 0; k < VZ; ++k)
#pragma unroll
          for (int t = 0; t < 27; ++t) sP[k][t][tid] = acc[k][t];
      }
      __syncthreads();
      if (out) {
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
          int nr = lr - kh + 1;  // staged row of the neighbour h - kh + 1 (a band's halo rows hold it; a whole plane wraps)
          if (!halo) nr = nr < 0 ? nr + H : (nr >= H ? nr - H : nr);
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) {
            const int ww = w - kw + 1;
            if (ww < 0 || ww >= W) continue;
            const int j = nr * W + ww, t = kh * 3 + kw;
#pragma unroll
            for (int k = 0; k < VZ; ++k) {
              sm[k][0] += sP[k][t][j];
              sm[k][1] += sP[k][9 + t][j];
              sm[k][2] += sP[k][18 + t][j];
            }
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < VZ; ++k)
#pragma unroll
        for (int q = 0; q < NQ; ++q) cur[k][q] = nxt[k][q];
    }
#pragma unroll
    for (int k = 0; k < VZ; ++k) {
      const int zi = zb + k;
      if (zi > z1) break;
      am += sm[k][0];
      a0 += sm[k][1];
      ap += sm[k][2];
      const int u = zi - 1;  // complete: it has the contributions of planes u - 1, u, u + 1
      if (out && u >= z0 && u < z1) {
        const size_t o = (size_t)b * D * HW + (size_t)u * HW + (size_t)ho * W + w;
        const float cin_b = scal[b * 4 + 0];
        dx[o] = objective == 2 ? cin_b * am : fmaf(objective == 0 ? scal[b * 4 + 1] : 1.f, gy[o], cin_b * am);
      }
      am = a0;
      a0 = ap;
      ap = 0.f;
    }
  }
}
void launch_init_dgrad(const float* g, const float* w_raw, int cin, int c0, const float* gy, const float* scal, int objective, float* dx,
                       int batch, Dims3 dims, hipStream_t s) {
  CD_REQUIRE(c0 == 16 || c0 == 32 || c0 == 64, "init conv input gradient: 16, 32 or 64 output channels");
  CD_REQUIRE(dims.w >= 1 && dims.w <= 64, "init conv input gradient: r extent up to 64");
  // a whole phi ring per block where it fits the 256 threads, else bands of rows with one halo row on either side
  int band = dims.h, halo = 0;
  if ((int64_t)dims.h * dims.w > 256) {
    band = 256 / dims.w - 2;
    halo = 1;
  }
  const int nbands = (dims.h + band - 1) / band;
  const int threads = ((band + 2 * halo) * dims.w + 63) / 64 * 64;
  // enough workgroups for two per CU; a chunk keeps >= 3 planes so the two halo planes stay a minority of its reads
  int nchunks = (512 + batch * nbands - 1) / (batch * nbands);
  const int maxchunks = (dims.d + 2) / 3;
  nchunks = nchunks < 1 ? 1 : (nchunks > maxchunks ? maxchunks : nchunks);
  const int zc = (dims.d + nchunks - 1) / nchunks;
  nchunks = (dims.d + zc - 1) / zc;
  prof::Scope scope("init_dgrad", s, 2.0 * 27 * c0 * batch * (double)dims.vox(), 4.0 * batch * (double)dims.vox() * (c0 + 2));
  const dim3 grid((unsigned)nchunks, (unsigned)nbands, (unsigned)batch);
  switch (c0) {
    case 16: hipLaunchKernelGGL((init_dgrad_kernel<16, 2>), grid, dim3(threads), 0, s, g, w_raw, cin, gy, scal, objective, dx, dims, band, halo, zc); break;
    case 32: hipLaunchKernelGGL((init_dgrad_kernel<32, 2>), grid, dim3(threads), 0, s, g, w_raw, cin, gy, scal, objective, dx, dims, band, halo, zc); break;
    default: hipLaunchKernelGGL((init_dgrad_kernel<64, 1>), grid, dim3(threads), 0, s, g, w_raw, cin, gy, scal, objective, dx, dims, band, halo, zc); break;
  }
  CD_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------------------
// init conv weight gradient (few input channels, coordinate channels synthesised as in init_conv_kernel):
//   dW[co][ci][tap] = sum_{b,v} g[b][v][co] * xin[b][in(v,tap)][ci]
// lane = output channel; a wave walks a voxel range with 27*CIN accumulators per lane; partials [b][chunk][tap*CIN+ci][32]
// ------------------------------------------------------------------------------------------------------------
template <int CIN>
__global__ void __launch_bounds__(256) init_wgrad_kernel(InitConvArgs a, const float* __restrict__ g, float* __restrict__ part,
                                                         int chunk_vox, int nchunks) {
  __shared__ float red[4][27 * CIN][32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int co = lane & 31, half = lane >> 5;
  const int chunk = blockIdx.x, b = blockIdx.y, ct = blockIdx.z;
  const int D = a.dims.d, H = a.dims.h, W = a.dims.w;
  const int64_t vox = a.dims.vox();
  const float sc = a.scale_b ? a.scale_b[(size_t)b * a.scale_stride] : 1.f;
  float acc[27 * CIN];
#pragma unroll
  for (int i = 0; i < 27 * CIN; ++i) acc[i] = 0.f;
  const int v0 = chunk * chunk_vox, v1 = min((int64_t)(v0 + chunk_vox), vox);
  for (int v = v0 + wave * 2 + half; v < v1; v += 8) {
    const float gv = g[((size_t)b * vox + v) * a.cout + ct * 32 + co];
    const int w = v % W, h = (v / W) % H, z = v / (W * H);
#pragma unroll
    for (int kd = 0; kd < 3; ++kd) {
      const int zz = z + kd - 1;
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        int hh = h + kh - 1;
        hh = hh < 0 ? hh + H : (hh >= H ? hh - H : hh);
        hh = hh % H;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int ww = w + kw - 1;
          const bool inb = zz >= 0 && zz < D && ww >= 0 && ww < W;
#pragma unroll
          for (int ci = 0; ci < CIN; ++ci) {
            float xv = 0.f;
            if (inb) {
              if (ci < a.cx) {
                xv = a.x[(((size_t)b * a.cx + ci) * D + zz) * H * W + (size_t)hh * W + ww];
                if (ci == 0) xv *= sc;
              } else {
                const int k = ci - a.cx;
                if (a.use_rz) xv = (k == 0) ? a.r_w[ww] : (k == 1 ? a.z_d[zz] : a.phi_h[hh]);
                else xv = a.phi_h[hh];
              }
            }
            acc[((kd * 3 + kh) * 3 + kw) * CIN + ci] = fmaf(gv, xv, acc[((kd * 3 + kh) * 3 + kw) * CIN + ci]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 27 * CIN; ++i) {
    const float t = acc[i] + __shfl_xor(acc[i], 32, 64);
    if (half == 0) red[wave][i][co] = t;
  }
  __syncthreads();
  float* dst = part + ((((size_t)b * nchunks + chunk) * gridDim.z + ct) * 27 * CIN) * 32;
  for (int i = tid; i < 27 * CIN * 32; i += 256) {
    const int r = i >> 5, c = i & 31;
    dst[i] = (red[0][r][c] + red[1][r][c]) + (red[2][r][c] + red[3][r][c]);
  }
}
__global__ void init_wgrad_reduce_kernel(const float* __restrict__ part, int nslots, int ctiles, int cin, int cout, float* __restrict__ dw) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;  // over cout*cin*27
  if (idx >= cout * cin * 27) return;
  const int tap = idx % 27, ci = (idx / 27) % cin, co = idx / (27 * cin);
  const int ct = co / 32, c = co % 32;
  double s = 0.0;
  for (int k = 0; k < nslots; ++k) s += (double)part[((((size_t)k * ctiles + ct) * 27 * cin) + tap * cin + ci) * 32 + c];
  dw[idx] = (float)s;
}
// The init conv's weight gradient through the general 3x3x3 weight-gradient kernels: its logical input (c_in * x and the
// synthesised coordinate channels) is written once as a 32-channel channels-last tensor (zero beyond cin), the 32 x 32 x 27
// gradient is computed like any other level-0 conv's (fp16 matrix pipe) and the first cin input columns are kept.  The scalar
// kernel above needs 81 broadcast loads per voxel pair: 0.98 ms per step against ~0.15 ms this way.
__global__ void __launch_bounds__(256) init_pad_input_kernel(InitConvArgs a, float* __restrict__ out) {
  const int64_t vox = a.dims.vox();
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (n >= vox) return;
  const int H = a.dims.h, W = a.dims.w;
  const int w = (int)(n % W), h = (int)((n / W) % H), z = (int)(n / ((int64_t)W * H));
  float sc = a.scale_b ? a.scale_b[(size_t)b * a.scale_stride] : 1.f;
  if (a.sigma_b) {
    const float tv = a.sigma_b[b], sd = a.sigma_data;
    sc = 1.f / sqrtf(tv * tv + sd * sd);
  }
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  for (int ci = 0; ci < a.cin; ++ci) {
    if (ci < a.cx) {
      v[ci] = a.x[((size_t)b * a.cx + ci) * vox + n];
      if (ci == 0) v[ci] *= sc;
    } else {
      const int k = ci - a.cx;
      v[ci] = a.use_rz ? (k == 0 ? a.r_w[w] : (k == 1 ? a.z_d[z] : a.phi_h[h])) : a.phi_h[h];
    }
  }
  f32x4* o = (f32x4*)(out + ((size_t)b * vox + n) * 32);
  o[0] = f32x4{v[0], v[1], v[2], v[3]};
#pragma unroll
  for (int q = 1; q < 8; ++q) o[q] = f32x4{0.f, 0.f, 0.f, 0.f};
}
__global__ void init_extract_dw_kernel(const float* __restrict__ dw32, float* __restrict__ dw, int cout, int cin) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;  // over cout * cin * 27
  if (idx >= cout * cin * 27) return;
  const int tap = idx % 27, ci = (idx / 27) % cin, co = idx / (27 * cin);
  dw[idx] = dw32[((size_t)co * 32 + ci) * 27 + tap];
}
size_t init_wgrad_mfma_floats(int batch, int64_t vox, int cout) {  // padded input + 32-wide gradient + slot partials
  return (size_t)batch * vox * 32 + (size_t)cout * 32 * 27 + 64 + wgrad_partial_floats(vox, batch, false, cout, 32, 27) + 128;
}
void launch_init_wgrad_mfma(const InitConvArgs& a, const float* g, float* scratch, float* dw, hipStream_t s, AbsmaxWords* words) {
  CD_REQUIRE(a.cin <= 4 && a.cout % 32 == 0, "init conv wgrad: 1..4 input channels, 32 k output channels");
  const int64_t vox = a.dims.vox();
  float* xin = scratch;
  float* dw32 = xin + (((size_t)a.batch * vox * 32 + 63) & ~(size_t)63);
  float* part = dw32 + (((size_t)a.cout * 32 * 27 + 63) & ~(size_t)63);
  hipLaunchKernelGGL(init_pad_input_kernel, dim3((unsigned)((vox + 255) / 256), (unsigned)a.batch), dim3(256), 0, s, a, xin);
  CD_HIP(hipGetLastError());
  WgradAux aux;  // (no queue: dw32 is read right below)
  aux.words = words;
  WgradOp op;
  op.g = g; op.A = a.cout; op.x = xin; op.Bc = 32; op.xld = 32; op.geom = ConvGeom{a.dims, a.dims, 3, 3, 3, 1, 1, 1}; op.batch = a.batch;
  op.partial = part; op.dw = dw32; op.aux = aux;
  launch_wgrad(op, s);
  const int total = a.cout * a.cin * 27;
  hipLaunchKernelGGL(init_extract_dw_kernel, dim3((total + 255) / 256), dim3(256), 0, s, dw32, dw, a.cout, a.cin);
  CD_HIP(hipGetLastError());
}

size_t init_wgrad_partial_floats(int batch, int64_t vox, int cin, int cout) {
  const int nchunks = (int)((vox + 1023) / 1024);
  return (size_t)batch * nchunks * (cout / 32) * 27 * cin * 32;
}
void launch_init_wgrad(const InitConvArgs& a, const float* g, float* part, float* dw, hipStream_t s) {
  const int64_t vox = a.dims.vox();
  const int nchunks = (int)((vox + 1023) / 1024);
  dim3 grid(nchunks, a.batch, a.cout / 32);
  switch (a.cin) {
    case 1: hipLaunchKernelGGL(init_wgrad_kernel<1>, grid, dim3(256), 0, s, a, g, part, 1024, nchunks); break;
    case 2: hipLaunchKernelGGL(init_wgrad_kernel<2>, grid, dim3(256), 0, s, a, g, part, 1024, nchunks); break;
    case 3: hipLaunchKernelGGL(init_wgrad_kernel<3>, grid, dim3(256), 0, s, a, g, part, 1024, nchunks); break;
    case 4: hipLaunchKernelGGL(init_wgrad_kernel<4>, grid, dim3(256), 0, s, a, g, part, 1024, nchunks); break;
    default: CD_REQUIRE(false, "init conv wgrad: 1..4 input channels");
  }
  const int total = a.cout * a.cin * 27;
  hipLaunchKernelGGL(init_wgrad_reduce_kernel, dim3((total + 255) / 256), dim3(256), 0, s, part, a.batch * nchunks, a.cout / 32, a.cin,
                     a.cout, dw);
  CD_HIP(hipGetLastError());
}

}  // namespace cd
