// Pointwise (1x1x1) convolution for gfx950; operand layout as in kernels_conv.hip.
#include "conv_internal.h"
#include "gn_defer.h"

namespace cd {

// ------------------------------------------------------------------------------------------------------------
// pointwise (1x1x1) conv = per-voxel channel GEMM, A operand straight from global memory (HBM-bound).
// Optional A prologues: GroupNorm(1) affine (PreNorm -> to_qkv) or a 32-way channel softmax (q of linear attention).
// Optional per-sample weights (the folded  W_out * context^T  of linear attention) and residual add.
// ------------------------------------------------------------------------------------------------------------
template <int CT, int PRO>
__global__ void __launch_bounds__(256) pointwise_kernel(PointwiseArgs a, int CTtot) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, col = lane & 31;
  const int b = blockIdx.y;
  const int ct0 = blockIdx.z * CT;
  const int64_t n0 = (int64_t)blockIdx.x * 128 + wave * 32;
  const int64_t n = n0 + col;
  const bool valid = n < a.vox;

  // fused block close (PointwiseArgs::gn_res): the normalisation's coefficients folded here, and this lane's 16 x CT values of the
  // normalised tensor requested before the matrix loop
  __shared__ __attribute__((aligned(16))) float sGn[128 * 4];
  __shared__ __attribute__((aligned(16))) char sGnScratch[128 * 16 + 64 * 8];
  float hv[CT][16];
  // `full`: the wave's 32 voxels and the workgroup's channel tiles all exist (every tile but a sample's last): the epilogue then
  // addresses its 16 rows as 32-bit offsets from one wave-uniform pointer, without a predicate per element (the general form costs
  // ~25 vector instructions per element in 64-bit index arithmetic and exec masking)
  const bool full = n0 + 32 <= a.vox && (ct0 + CT) * 32 <= a.cout;
  const int rl = 4 * half;  // accumulator register r of a tile = row (r & 3) + 8 (r >> 2) + rl, column col
  if (a.gn_res) {
    gn_defer_to_lds(a.gn_defer, b, sGn, sGnScratch);
    if (full) {
      const float* hp = a.gn_res + ((size_t)b * a.vox + n0) * a.cout + ct0 * 32 + col;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) hv[ct][r] = hp[((r & 3) + 8 * (r >> 2) + rl) * a.cout + ct * 32];
    } else {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const int co = min((ct0 + ct) * 32 + col, a.cout - 1);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t nr = min(n0 + (r & 3) + 8 * (r >> 2) + 4 * half, a.vox - 1);
          hv[ct][r] = a.gn_res[((size_t)b * a.vox + nr) * a.cout + co];
        }
      }
    }
  }

  f32x16 acc[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;

  const int nchunk = (a.c0 + a.c1) >> 5;
  const float* wb = a.wpk + (size_t)b * a.w_batch_stride;
  if (PRO == A_NONE && a.wpk16) {
    // fp16 pipe.  The lane keeps the f32 path's loads -- its voxel's channels 16 half .. 16 half + 15 of the chunk, 64 contiguous
    // bytes -- and runs them as two k-steps of 8: k-slot (half, j) of k-step s' is channel 16 half + 8 s' + j, which in the packed
    // image (k-step s: slot (h, j) = channel 16 s + 8 h + j) is what lane (h = s', col) of k-step s = half holds -- the same image,
    // another lane's entry.
    f32x16 accB[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) accB[ct][r] = 0.f;
    float amax = 0.f;
    for (int chunk = 0; chunk < nchunk; ++chunk) {
      const float* src;
      if (chunk * 32 < a.c0) src = a.in0 + ((size_t)b * a.vox + (valid ? n : 0)) * a.ld0 + a.off0 + chunk * 32 + half * 16;
      else src = a.in1 + ((size_t)b * a.vox + (valid ? n : 0)) * a.ld1 + (chunk * 32 - a.c0) + half * 16;
      f32x4 av[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        av[q] = *(const f32x4*)(src + q * 4);
        if (!valid) av[q] = f32x4{0.f, 0.f, 0.f, 0.f};
        amax = fmaxf(fmaxf(fmaxf(amax, fabsf(av[q][0])), fabsf(av[q][1])), fmaxf(fabsf(av[q][2]), fabsf(av[q][3])));
      }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        u32x2 h0, l0, h1, l1;
        split2(av[2 * ks], h0, l0);
        split2(av[2 * ks + 1], h1, l1);
        const u32x4 a1 = {h0[0], h0[1], h1[0], h1[1]}, a2 = {l0[0], l0[1], l1[0], l1[1]};
        const u32x4* wp = (const u32x4*)a.wpk16 + ((size_t)(chunk * 2 + half) * CTtot + ct0) * 128 + ks * 32 + col;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const u32x4 w1 = wp[ct * 128], w2 = wp[ct * 128 + 64];
          acc[ct] = MFMA_F16(a1, w1, acc[ct]);
          accB[ct] = MFMA_F16(a1, w2, accB[ct]);
          accB[ct] = MFMA_F16(a2, w1, accB[ct]);
        }
      }
    }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ct][r] += accB[ct][r] * (1.f / 2048.f);
    if (a.status && amax > 65504.f) atomicOr(a.status, 1);
  } else
  for (int chunk = 0; chunk < nchunk; ++chunk) {
    const float* src;
    if (chunk * 32 < a.c0) src = a.in0 + ((size_t)b * a.vox + (valid ? n : 0)) * a.ld0 + a.off0 + chunk * 32 + half * 16;
    else src = a.in1 + ((size_t)b * a.vox + (valid ? n : 0)) * a.ld1 + (chunk * 32 - a.c0) + half * 16;
    f32x4 av[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      av[q] = *(const f32x4*)(src + q * 4);
      if (!valid) av[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (PRO == A_AFFINE) {
      const float* cfp = a.coef + ((size_t)b * (a.c0 + a.c1) + chunk * 32 + half * 16) * 4;
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const f32x4 cf = *(const f32x4*)(cfp + (q * 4 + e) * 4);
          av[q][e] = cf[0] * av[q][e] + cf[1];
        }
    } else if (PRO == A_EXPNORM) {
      const float* cfp = a.coef + ((size_t)b * (a.c0 + a.c1) + chunk * 32 + half * 16) * 2;
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) av[q][e] = valid ? expf(av[q][e] - cfp[(q * 4 + e) * 2]) * cfp[(q * 4 + e) * 2 + 1] : 0.f;
    } else if (PRO == A_SOFTMAX32) {
      float m = av[0][0];
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) m = fmaxf(m, av[q][e]);
      m = fmaxf(m, __shfl_xor(m, 32, 64));
      float ssum = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          av[q][e] = expf(av[q][e] - m);
          ssum += av[q][e];
        }
      ssum += __shfl_xor(ssum, 32, 64);
      const float inv = 1.f / ssum;
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) av[q][e] *= inv;
    }
    const f32x4* wq = (const f32x4*)wb + ((size_t)chunk * CTtot + ct0) * 256 + lane;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      f32x4 bw[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) bw[q] = wq[ct * 256 + q * 64];
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[ct] = MFMA32(av[q][e], bw[q][e], acc[ct]);
    }
  }

  // final values in place (bias, residual, fused block close), then the stores and the channel statistics read them
  if (full) {
    const int ld = a.out_ld ? a.out_ld : a.cout;
    // the output tile leaves as 16-byte quads (row 8 k + (lane >> 3), channels 4 (lane & 7) .. + 3) after a transpose through LDS:
    // 16 scalar row stores per lane in accumulator layout ran at a fraction of the HBM rate (see init_conv_f16x2_kernel)
    __shared__ __attribute__((aligned(16))) float sTr[4][32 * 36];
    float* tr = sTr[wave];
    float* op = a.out + ((size_t)b * a.vox + n0) * ld + a.out_off + ct0 * 32 + (lane & 7) * 4;
    const float* rp = a.residual ? a.residual + ((size_t)b * a.vox + n0) * a.cout + ct0 * 32 + col : nullptr;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const float bv = a.bias ? a.bias[(ct0 + ct) * 32 + col] : 0.f;
      f32x4 cf = {0.f, 0.f, 0.f, 0.f};
      if (a.gn_res) cf = *(const f32x4*)(sGn + ((ct0 + ct) * 32 + col) * 4);
      float rv[16];
      if (rp) {
#pragma unroll
        for (int r = 0; r < 16; ++r) rv[r] = rp[((r & 3) + 8 * (r >> 2) + rl) * a.cout + ct * 32];
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = acc[ct][r] + bv;
        if (rp) v += rv[r];
        if (a.gn_res) {
          const float u = cf[0] * hv[ct][r] + cf[1];
          v += u * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(u * -1.4426950408889634f)) + cf[2];
        }
        acc[ct][r] = v;
        tr[((r & 3) + 8 * (r >> 2) + rl) * 36 + col] = v;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (one wave: its own LDS writes are visible to its reads in order)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int row = 8 * k + (lane >> 3);
        *(f32x4*)(op + (size_t)row * ld + ct * 32) = *(const f32x4*)(tr + row * 36 + (lane & 7) * 4);
      }
      if (ct + 1 < CT) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the tile buffer is reused by the next channel tile)
    }
  } else {
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int co = (ct0 + ct) * 32 + col;
    const bool cok = co < a.cout;
    const float bv = (a.bias && cok) ? a.bias[co] : 0.f;
    f32x4 cf = {0.f, 0.f, 0.f, 0.f};
    if (a.gn_res && cok) cf = *(const f32x4*)(sGn + co * 4);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t nr = n0 + (r & 3) + 8 * (r >> 2) + 4 * half;
      float v = acc[ct][r] + bv;
      if (a.residual && cok && nr < a.vox) v += a.residual[((size_t)b * a.vox + nr) * a.cout + co];
      if (a.gn_res) {  // + silu(scale h + shift) + add, SiLU on the transcendental unit as in gn_apply_kernel
        const float u = cf[0] * hv[ct][r] + cf[1];
        v += u * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(u * -1.4426950408889634f)) + cf[2];
      }
      acc[ct][r] = v;
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
    const int64_t nr = n0 + row;
    if (nr < a.vox) {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const int co = (ct0 + ct) * 32 + col;
        if (co < a.cout) a.out[((size_t)b * a.vox + nr) * (a.out_ld ? a.out_ld : a.cout) + a.out_off + co] = acc[ct][r];
      }
    }
  }
  }
  if (a.ch_part) {  // per-channel {sum, sum of squares} of this workgroup's 128 output voxels
    __shared__ float red[4][CT * 32][2];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
        if (full || n0 + row < a.vox) {
          const float v = acc[ct][r];
          s1 += v;
          s2 += v * v;
        }
      }
      s1 += __shfl_xor(s1, 32, 64);
      s2 += __shfl_xor(s2, 32, 64);
      if (half == 0) {
        red[wave][ct * 32 + col][0] = s1;
        red[wave][ct * 32 + col][1] = s2;
      }
    }
    __syncthreads();
    if (tid < CT * 32 && ct0 * 32 + tid < a.cout) {
      const float t1 = (red[0][tid][0] + red[1][tid][0]) + (red[2][tid][0] + red[3][tid][0]);
      const float t2 = (red[0][tid][1] + red[1][tid][1]) + (red[2][tid][1] + red[3][tid][1]);
      float* dst = a.ch_part + (((size_t)b * gridDim.x + blockIdx.x) * a.cout + ct0 * 32 + tid) * 2;
      dst[0] = t1;
      dst[1] = t2;
    }
  }
}

void launch_pointwise(const PointwiseArgs& a, hipStream_t s) {
  CD_REQUIRE(a.c0 % 32 == 0 && a.c1 % 32 == 0 && a.c0 > 0, "pointwise conv: channels must be multiples of 32");
  CD_REQUIRE(a.prologue != A_SOFTMAX32 || (a.c0 == 32 && a.c1 == 0), "softmax prologue needs exactly 32 channels");
  CD_REQUIRE(!a.gn_res || (a.gn_defer.part && a.gn_defer.C == a.cout && a.cout <= 128 && !a.out_ld),
             "pointwise conv: the fused block close normalises a packed tensor of the output's width (<= 128 channels)");
  CD_REQUIRE(a.out_off % 4 == 0 && a.out_ld % 4 == 0 && (a.cout % 4 == 0 || a.out_ld), "pointwise conv: output rows must be 16-byte aligned");
  CD_REQUIRE(!a.wpk16 || (a.prologue == A_NONE && !a.w_batch_stride && a.cout % 32 == 0),
             "pointwise conv: the fp16-pipe form takes shared weights, whole 32-channel tiles and no input prologue");
  const int CTtot = (a.cout + 31) / 32;
  const int CT = CTtot <= 3 ? CTtot : (CTtot % 2 == 0 ? 2 : 1);
  dim3 grid((unsigned)((a.vox + 127) / 128), (unsigned)a.batch, (unsigned)(CTtot / CT));
  char cat[128];
  std::snprintf(cat, sizeof cat, "pointwise_p%d C%d->%d n%ld", a.prologue, a.c0 + a.c1, a.cout, (long)a.vox);
  prof::Scope scope(cat, s, 2.0 * (a.c0 + a.c1) * a.cout * (double)a.vox * a.batch,
                    4.0 * a.batch * (double)a.vox * (a.c0 + a.c1 + a.cout + (a.residual ? a.cout : 0)));
#define CD_PW_CASE(C, P)                                                                   \
  if (CT == C && a.prologue == P) {                                                        \
    hipLaunchKernelGGL((pointwise_kernel<C, P>), grid, dim3(256), 0, s, a, CTtot);         \
    CD_HIP(hipGetLastError());                                                             \
    return;                                                                                \
  }
  CD_PW_CASE(1, A_NONE) CD_PW_CASE(2, A_NONE) CD_PW_CASE(3, A_NONE)
  CD_PW_CASE(1, A_AFFINE) CD_PW_CASE(2, A_AFFINE) CD_PW_CASE(3, A_AFFINE)
  CD_PW_CASE(1, A_SOFTMAX32) CD_PW_CASE(2, A_SOFTMAX32) CD_PW_CASE(3, A_SOFTMAX32)
  CD_PW_CASE(1, A_EXPNORM) CD_PW_CASE(2, A_EXPNORM) CD_PW_CASE(3, A_EXPNORM)
#undef CD_PW_CASE
  CD_REQUIRE(false, "pointwise conv: no kernel instance");
}

}  // namespace cd
