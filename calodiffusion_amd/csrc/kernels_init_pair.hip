// The init conv and the first block's first 3x3x3 conv as one launch: a one-channel 5x5x5 conv of c_in x on the matrix cores
// (InitPairArgs, kernels_conv.h), and the kernels that compose its weights and table.
#include "conv_internal.h"

namespace cd {

// offset index k = (dz * 5 + dh) * 5 + dw of the composed kernel; conv1's tap t = (tz, th, tw) reads the init conv's output at
// p + t - 1, whose tap s reads x at p + t + s - 2: d = t + s.  A class leaves out the taps t that land in conv1's zero padding.
__device__ __forceinline__ bool init_pair_tap_valid(int cls3, int t) { return !((cls3 == 0 && t == 0) || (cls3 == 2 && t == 2)); }

// one workgroup per (class, k-step, k-half), one thread per composed weight (e, co): fp64 in a fixed order; the 32 threads of e = 0
// then split their lane's eight values as the packers do.  (The plan rebuilds this with every parameter upload, a training step's
// included: one thread per lane of the image, 18 workgroups of long serial sums, took 260 us.)
__global__ void __launch_bounds__(256) init_pair_weights_kernel(const float* __restrict__ w0, int cin, const float* __restrict__ w1,
                                                                u32x4* __restrict__ wc) {
  __shared__ float sv[8][33];
  const int half = blockIdx.x & 1, ks = (blockIdx.x >> 1) & 7, cls = blockIdx.x >> 4;
  const int zc = cls / 3, rc = cls % 3, e = threadIdx.x >> 5, co = threadIdx.x & 31;
  const int k = ks * 16 + half * 8 + e;
  double acc = 0.0;
  if (k < 125) {
    const int dz = k / 25, dh = (k / 5) % 5, dw = k % 5;
    for (int tz = 0; tz < 3; ++tz) {
      const int sz = dz - tz;
      if (sz < 0 || sz > 2 || !init_pair_tap_valid(zc, tz)) continue;
      for (int th = 0; th < 3; ++th) {
        const int sh = dh - th;
        if (sh < 0 || sh > 2) continue;
        for (int tw = 0; tw < 3; ++tw) {
          const int sw = dw - tw;
          if (sw < 0 || sw > 2 || !init_pair_tap_valid(rc, tw)) continue;
          const int t = (tz * 3 + th) * 3 + tw, s = (sz * 3 + sh) * 3 + sw;
          for (int ci = 0; ci < 32; ++ci) acc += (double)w1[((size_t)co * 32 + ci) * 27 + t] * (double)w0[((size_t)ci * cin) * 27 + s];
        }
      }
    }
  }
  sv[e][co] = (float)acc;
  __syncthreads();
  if (e != 0) return;
  f32x4 v[2];
#pragma unroll
  for (int q = 0; q < 8; ++q) v[q >> 2][q & 3] = sv[q][co];
  u32x2 a1, a2, b1, b2;
  split2(v[0], a1, a2);
  split2(v[1], b1, b2);
  u32x4* dst = wc + ((size_t)(cls * kInitPairKSteps + ks) * 2) * 64 + half * 32 + co;
  dst[0] = u32x4{a1[0], a1[1], b1[0], b1[1]};
  dst[64] = u32x4{a2[0], a2[1], b2[0], b2[1]};
}

// T1 = conv1(T) + b1 with conv1's own padding (z, r zero; phi circular): 8 voxels x 32 output channels per workgroup, one tap's
// 32 x 32 weights in LDS at a time (the next tap's on their way in registers meanwhile), fp64 in tap-major order
__global__ void __launch_bounds__(256) init_pair_table_kernel(const float* __restrict__ T, const float* __restrict__ w1,
                                                              const float* __restrict__ b1, float* __restrict__ t1, Dims3 dims) {
  __shared__ float sw[2][32 * 33];
  const int tid = threadIdx.x, co = tid & 31;
  const int64_t vox = dims.vox(), v = (int64_t)blockIdx.x * 8 + (tid >> 5);
  const bool valid = v < vox;
  const int D = dims.d, H = dims.h, W = dims.w;
  const int vv = valid ? (int)v : 0;
  const int w = vv % W, h = (vv / W) % H, z = vv / (W * H);
  double acc = b1 ? (double)b1[co] : 0.0;
  float nxt[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) nxt[q] = w1[(size_t)(tid + 256 * q) * 27];  // element i = co' * 32 + ci of tap 0
  for (int t = 0; t < 27; ++t) {
    float* s = sw[t & 1];  // (two buffers: one barrier per tap)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = tid + 256 * q;
      s[(i & 31) * 33 + (i >> 5)] = nxt[q];
    }
    if (t + 1 < 27)
#pragma unroll
      for (int q = 0; q < 4; ++q) nxt[q] = w1[(size_t)(tid + 256 * q) * 27 + t + 1];
    __syncthreads();
    const int zz = z + t / 9 - 1, ww = w + t % 3 - 1;
    const int hh = ((h + (t / 3) % 3 - 1) % H + H) % H;
    if (valid && zz >= 0 && zz < D && ww >= 0 && ww < W) {
      const float* row = T + (((size_t)zz * H + hh) * W + ww) * 32;
      for (int ci = 0; ci < 32; ++ci) acc += (double)s[ci * 33 + co] * (double)row[ci];
    }
  }
  if (valid) t1[(size_t)v * 32 + co] = (float)acc;
}

void launch_init_pair_build(const float* w0, int cin, const float* w1, const float* b1, const float* init_table, void* wc, float* table,
                            Dims3 dims, hipStream_t s) {
  CD_REQUIRE(w0 && w1 && init_table && wc && table && cin >= 1 && cin <= 4, "init pair: bad arguments");
  hipLaunchKernelGGL(init_pair_weights_kernel, dim3(kInitPairClasses * kInitPairKSteps * 2), dim3(256), 0, s, w0, cin, w1, (u32x4*)wc);
  CD_HIP(hipGetLastError());
  hipLaunchKernelGGL(init_pair_table_kernel, dim3((unsigned)((dims.vox() + 7) / 8)), dim3(256), 0, s, init_table, w1, b1, table, dims);
  CD_HIP(hipGetLastError());
}

// exact i / d for 0 <= i < 2^20 by reciprocal: (i + 0.5) / d is never within float error of an integer
__device__ __forceinline__ int small_div(int i, float inv) { return (int)(((float)i + 0.5f) * inv); }

// A workgroup owns TZ planes of one sample.  c_in x of those planes with a halo of 2 (zero planes / columns outside the grid, phi
// rows wrapped) sits in LDS ALREADY SPLIT -- each cell the two fp16 terms of the f16x2 product in one word -- because every cell
// is gathered by up to 125 offsets: the im2col gather is one LDS read and one half-word merge per element.  The slab's voxels are
// dealt to 32-row tiles class by class (the weights of a class stay in registers over its tiles); each wave takes a contiguous
// quarter of the tile list.  Epilogue as the init conv's: tile transposed through LDS to 16-byte quads, table rows added, and on
// top the channel sums of what was stored -- one unit of partials per workgroup, every order fixed.
__global__ void __launch_bounds__(256, 2) init_pair_f16x2_kernel(InitPairArgs a, int TZ) {
  extern __shared__ __attribute__((aligned(16))) unsigned pimg[];
  __shared__ __attribute__((aligned(16))) float trn[4 * 32 * 36];  // per-wave output tile on its way to row-major quads
  __shared__ int vrow[4 * 32];                                     // per-wave: voxel (within the slab) of each tile row, -1 = none
  __shared__ float red[4 * 32 * 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
  const int b = blockIdx.y;
  const int D = a.dims.d, H = a.dims.h, W = a.dims.w, PV = H * W;
  const int z0 = blockIdx.x * TZ, nz = min(TZ, D - z0);
  const int HP = H + 4, WP = W + 4;
  float sc = a.scale_b ? a.scale_b[(size_t)b * a.scale_stride] : 1.f;
  if (a.sigma_b) {  // same expression as embed_kernel's c_in
    const float tv = a.sigma_b[b], sd = a.sigma_data;
    sc = 1.f / sqrtf(tv * tv + sd * sd);
  }
  {
    const float* xb = a.x + (size_t)b * D * PV;
    float amax = 0.f;
    const float inv_wp = 1.f / (float)WP, inv_hp = 1.f / (float)HP;
    const int ncell = (nz + 4) * HP * WP;
    // eight cells per thread and trip, their loads issued together: one memory latency per trip, not per cell (a slab is ~10 cells
    // per thread, and every workgroup of the launch starts with this loop)
    for (int i0 = tid; i0 < ncell; i0 += 256 * 8) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = min(i0 + 256 * j, ncell - 1);
        const int r = small_div(i, inv_wp), lw = i - r * WP, lz = small_div(r, inv_hp), lh = r - lz * HP;
        const int gz = z0 - 2 + lz, gw = lw - 2;
        int gh = lh - 2;  // in [-2, H + 2): at most two wraps either way, whatever H
        gh = gh < 0 ? gh + H : gh;
        gh = gh < 0 ? gh + H : gh;
        gh = gh >= H ? gh - H : gh;
        gh = gh >= H ? gh - H : gh;
        const bool in = gz >= 0 && gz < D && gw >= 0 && gw < W;
        const float xv = xb[in ? ((size_t)gz * H + gh) * W + gw : (size_t)0];
        v[j] = in ? xv : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float vs = v[j] * sc;
        amax = fmaxf(amax, fabsf(vs));
        const _Float16 hi = (_Float16)vs, lo = (_Float16)((vs - (float)hi) * 2048.f);
        if (i0 + 256 * j < ncell) pimg[i0 + 256 * j] = pack_h2(hi, lo);
      }
    }
    if (a.status && amax > 65504.f) atomicOr(a.status, 1);
  }
  // this lane's 64 im2col columns: k = ks*16 + half*8 + e = offset index (k >= 125: zero weight, any readable cell)
  int toff[kInitPairKSteps][8];
#pragma unroll
  for (int ks = 0; ks < kInitPairKSteps; ++ks)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = ks * 16 + half * 8 + e;
      const int dz = k / 25, dh = (k / 5) % 5, dw = k % 5;
      toff[ks][e] = k < 125 ? (dz * HP + dh) * WP + dw : 0;
    }
  __syncthreads();

  // planes of each z class within the slab, and the tile list: class by class, ceil(voxels / 32) tiles each
  const int first = z0 == 0 ? 1 : 0, last = z0 + nz == D ? 1 : 0;
  int total = 0;
#pragma unroll
  for (int g = 0; g < kInitPairClasses; ++g) {
    const int zc = g / 3, rc = g % 3;
    const int np = zc == 0 ? first : (zc == 2 ? last : nz - first - last);
    const int nw = rc == 1 ? W - 2 : 1;
    total += (np * H * nw + 31) >> 5;
  }
  const int t_lo = wave * total / 4, t_hi = (wave + 1) * total / 4;
  const int64_t vox = a.dims.vox();
  const u32x4* wc = (const u32x4*)a.wc;
  const float* tab = a.table + (size_t)z0 * PV * 32 + (lane & 7) * 4;
  float* outp = a.out + ((size_t)b * vox + (size_t)z0 * PV) * 32 + (lane & 7) * 4;
  float* tr = trn + wave * (32 * 36);  // this wave's 32 x 32 tile, rows padded to 36 floats
  int* vr = vrow + wave * 32;
  f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
  int t0 = 0;
#pragma unroll 1
  for (int g = 0; g < kInitPairClasses; ++g) {
    const int zc = g / 3, rc = g % 3;
    const int pa = zc == 0 ? 0 : (zc == 2 ? nz - 1 : first);
    const int np = zc == 0 ? first : (zc == 2 ? last : nz - first - last);
    const int nw = rc == 1 ? W - 2 : 1, w0 = rc == 0 ? 0 : (rc == 1 ? 1 : W - 1);
    const int nv = np * H * nw, nt = (nv + 31) >> 5;
    const int ta = max(t_lo, t0), tb_end = min(t_hi, t0 + nt);
    const int tbase = t0;
    t0 += nt;
    if (ta >= tb_end) continue;
    u32x4 w1r[kInitPairKSteps], w2r[kInitPairKSteps];
#pragma unroll
    for (int ks = 0; ks < kInitPairKSteps; ++ks) {
      w1r[ks] = wc[((size_t)(g * kInitPairKSteps + ks) * 2) * 64 + lane];
      w2r[ks] = wc[((size_t)(g * kInitPairKSteps + ks) * 2 + 1) * 64 + lane];
    }
    const int hnw = H * nw;
    const float inv_hnw = 1.f / (float)hnw, inv_nw = 1.f / (float)nw;
#pragma unroll 1
    for (int tile = ta; tile < tb_end; ++tile) {
      const int iraw = (tile - tbase) * 32 + col, i = min(iraw, nv - 1);
      const int pl = small_div(i, inv_hnw), rem = i - pl * hnw, h = small_div(rem, inv_nw), w = w0 + rem - h * nw;
      const int lz = pa + pl;
      if (half == 0) vr[col] = iraw < nv ? (lz * H + h) * W + w : -1;
      const unsigned* base = pimg + (lz * HP + h) * WP + w;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (one wave: its own LDS writes are visible to its reads in order)
      int rowv[4];
      f32x4 tb[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        rowv[k] = vr[8 * k + (lane >> 3)];
        tb[k] = *(const f32x4*)(tab + (size_t)max(rowv[k], 0) * 32);
      }
      f32x16 accA, accB;
#pragma unroll
      for (int r = 0; r < 16; ++r) accA[r] = accB[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < kInitPairKSteps; ++ks) {
        unsigned p[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) p[e] = base[toff[ks][e]];
        u32x4 x1, x2;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          x1[q] = (p[2 * q] & 0xffffu) | (p[2 * q + 1] << 16);
          x2[q] = (p[2 * q] >> 16) | (p[2 * q + 1] & 0xffff0000u);
        }
        accA = MFMA_F16(x1, w1r[ks], accA);
        accB = MFMA_F16(x1, w2r[ks], accB);
        accB = MFMA_F16(x2, w1r[ks], accB);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) tr[((r & 3) + 8 * (r >> 2) + 4 * half) * 36 + col] = accA[r] + accB[r] * (1.f / 2048.f);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int row = 8 * k + (lane >> 3);
        const f32x4 o = *(const f32x4*)(tr + row * 36 + (lane & 7) * 4) + tb[k];
        if (rowv[k] >= 0) {
          *(f32x4*)(outp + (size_t)rowv[k] * 32) = o;
          s1 += o;
          s2 += o * o;
        }
      }
    }
  }
  // channel partials: lanes with equal (lane & 7) hold the same four channels
#pragma unroll
  for (int m = 8; m < 64; m <<= 1)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s1[j] += __shfl_xor(s1[j], m, 64);
      s2[j] += __shfl_xor(s2[j], m, 64);
    }
  if (lane < 8)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      red[(wave * 32 + lane * 4 + j) * 2] = s1[j];
      red[(wave * 32 + lane * 4 + j) * 2 + 1] = s2[j];
    }
  __syncthreads();
  if (tid < 64 && a.ch_part) {
    const int c = tid >> 1, q = tid & 1;
    const float sum = ((red[(0 * 32 + c) * 2 + q] + red[(1 * 32 + c) * 2 + q]) + red[(2 * 32 + c) * 2 + q]) + red[(3 * 32 + c) * 2 + q];
    a.ch_part[(((size_t)b * gridDim.x + blockIdx.x) * 32 + c) * 2 + q] = sum;
  }
}

static constexpr size_t kInitPairMaxImage = 44 * 1024;  // dynamic LDS; with the static 20 KiB a workgroup stays within 64 KiB
static size_t init_pair_image_bytes(Dims3 d, int TZ) { return (size_t)(TZ + 4) * (d.h + 4) * (d.w + 4) * 4; }

bool init_pair_eligible(Dims3 d) {
  return d.d >= 2 && d.w >= 2 && d.h >= 1 && d.vox() < (1 << 20) && init_pair_image_bytes(d, 1) <= kInitPairMaxImage;
}

// planes per workgroup: about two rounds of workgroups on the chip, as the init conv deals them
static int init_pair_tz(Dims3 d, int batch, int slabs) {
  if (slabs <= 0) slabs = (512 + batch - 1) / batch;
  slabs = slabs < 1 ? 1 : (slabs > d.d ? d.d : slabs);
  int TZ = (d.d + slabs - 1) / slabs;
  while (TZ > 1 && init_pair_image_bytes(d, TZ) > kInitPairMaxImage) --TZ;
  return TZ;
}
int init_pair_units(Dims3 d, int batch, int slabs) {
  const int TZ = init_pair_tz(d, batch, slabs);
  return (d.d + TZ - 1) / TZ;
}

void launch_init_pair_conv(const InitPairArgs& a, int* units, hipStream_t s) {
  CD_REQUIRE(a.x && a.wc && a.table && a.out && a.batch > 0, "init pair conv: bad arguments");
  CD_REQUIRE(init_pair_eligible(a.dims), "init pair conv: this grid is not eligible (one voxel along z or r, or a plane too large for LDS)");
  const int D = a.dims.d;
  const int TZ = init_pair_tz(a.dims, a.batch, a.slabs);
  const size_t lds = init_pair_image_bytes(a.dims, TZ);
  const int nslab = (D + TZ - 1) / TZ;
  CD_REQUIRE(TZ >= 1 && lds <= kInitPairMaxImage, "init pair conv: plane too large for the LDS image");
  CD_REQUIRE(nslab >= 1 && nslab <= D && (size_t)nslab * TZ >= (size_t)D && a.batch <= 65535, "init pair conv: bad grid");
  char cat[96];
  std::snprintf(cat, sizeof cat, "init_pair_conv5x5x5 C1->32 @%dx%dx%d", D, a.dims.h, a.dims.w);
  // (the work of the conv it stands for: the 32 -> 32 3x3x3 conv over the init conv's output)
  prof::Scope scope(cat, s, 2.0 * 27 * 32 * 32 * (double)a.dims.vox() * a.batch, 4.0 * a.batch * (double)a.dims.vox() * (32 + 32));
  hipLaunchKernelGGL(init_pair_f16x2_kernel, dim3((unsigned)nslab, (unsigned)a.batch), dim3(256), lds, s, a, TZ);
  CD_HIP(hipGetLastError());
  if (units) *units = nslab;
}

}  // namespace cd
