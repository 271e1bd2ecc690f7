// Convolution kernels for gfx950 (MI355X): phi-periodic 3D convolutions as implicit GEMMs on the fp32 matrix cores.
//
// All dense contractions use v_mfma_f32_32x32x2_f32 (exact fp32 FMA chains, 64 FLOP/clk/SIMD = the chip's fp32 peak):
//   M = 32 output voxels (A operand, one channels-last voxel per lane, staged through LDS with its halo),
//   N = 32 output channels (B operand = pre-packed weights, 1-KiB coalesced wave loads, L2-resident),
//   K = 2 input channels per instruction: lane half h = lane>>5 owns channels [16h, 16h+16) of a 32-channel chunk,
//       so MFMA m of a tap contracts channels (m, 16+m).
// Reference semantics: CylindricalConv / CylindricalConvTrans / Downsample / Upsample,
// calodiffusion/models/models.py:25-96, 335-369: circular padding along phi (H), zero padding along z (D) and r (W).
//
// This unit: the process-wide precision, weight packing, and launch_conv_mfma, which picks the kernel family of a forward conv.
// The kernels themselves are in kernels_conv_{zs,small,flat,tiled,transpose}.hip, kernels_pointwise.hip and kernels_init_conv.hip
// (conv_internal.h).
#include "conv_internal.h"
#include <cstring>
#include <algorithm>
#include <vector>

namespace cd {

// process-wide arithmetic of the convolutions (cd_common.h); the plan flips it to bf16x3 for the re-run of a trajectory
// whose f16x2 pass left the fp16 range
static int g_conv_precision = -1;
static thread_local int tl_conv_precision_override = -1;
void set_conv_precision_override(int p) { tl_conv_precision_override = p; }
int conv_precision() {
  if (tl_conv_precision_override >= 0) return tl_conv_precision_override;
  if (g_conv_precision < 0) {
    const char* e = getenv("CD_CONV_PRECISION");
    g_conv_precision = !e ? PREC_F16X2 : (!strcmp(e, "f32") ? PREC_F32 : (!strcmp(e, "bf16x3") ? PREC_BF16X3 : PREC_F16X2));
  }
  return g_conv_precision;
}
void set_conv_precision(int p) { g_conv_precision = p; }

// ------------------------------------------------------------------------------------------------------------
// weight packing (see kernels_conv.h for the layout)
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void pack_weights_elem(size_t idx, const float* __restrict__ w, float* __restrict__ wpk, int cout, int cin,
                                                  int taps, int transposed, int flip) {
  const int e = idx & 3, lane = (idx >> 2) & 63, q = (idx >> 8) & 3;
  size_t rest = idx >> 10;
  const int CT = (cout + 31) / 32;
  const int ct = rest % CT;
  rest /= CT;
  const int tap = rest % taps;
  const int chunk = rest / taps;
  const int h = lane >> 5, j = lane & 31, m = q * 4 + e;
  const int ci = chunk * 32 + h * 16 + m, co = ct * 32 + j;
  float v = 0.f;
  const int st = flip ? taps - 1 - tap : tap;  // source tap (flipped for the input gradient of a stride-1 conv)
  if (co < cout && ci < cin)
    v = transposed ? w[((size_t)ci * cout + co) * taps + st] : w[((size_t)co * cin + ci) * taps + st];
  wpk[idx] = v;
}
__global__ void pack_weights_kernel(const float* __restrict__ w, float* __restrict__ wpk, int cout, int cin, int taps,
                                    int transposed, size_t total, int flip) {
  size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (idx >= total) return;
  pack_weights_elem(idx, w, wpk, cout, cin, taps, transposed, flip);
}

void launch_pack_weights(const float* w_torch, float* wpk, int cout, int cin, int taps, bool transposed, hipStream_t s, bool flip) {
  CD_REQUIRE(cin % 32 == 0, "MFMA convolutions need input channels in multiples of 32");
  size_t total = packed_weight_floats(cin, cout, taps);
  hipLaunchKernelGGL(pack_weights_kernel, dim3((total + 255) / 256), dim3(256), 0, s, w_torch, wpk, cout, cin, taps,
                     transposed ? 1 : 0, total, flip ? 1 : 0);
  CD_HIP(hipGetLastError());
}

// init conv weights: [tap][ci][cout] so that the 32 output-channel weights of one (tap, ci) are contiguous (scalar loads)
__device__ __forceinline__ void pack_init_weights_elem(int idx, const float* __restrict__ w, float* __restrict__ wpk, int cout, int cin) {
  const int co = idx % cout;
  const int ci = (idx / cout) % cin;
  const int tap = idx / (cout * cin);
  wpk[idx] = w[((size_t)co * cin + ci) * 27 + tap];
}
__global__ void pack_init_weights_kernel(const float* __restrict__ w, float* __restrict__ wpk, int cout, int cin) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= cout * cin * 27) return;
  pack_init_weights_elem(idx, w, wpk, cout, cin);
}
void launch_pack_init_weights(const float* w_torch, float* wpk, int cout, int cin, hipStream_t s) {
  int total = cout * cin * 27;
  hipLaunchKernelGGL(pack_init_weights_kernel, dim3((total + 255) / 256), dim3(256), 0, s, w_torch, wpk, cout, cin);
  CD_HIP(hipGetLastError());
}

// packed bf16x3 weights: [sub-chunk = ci/16][tap][ct][term][lane = h*32+j][8 bf16] = W_term[co = ct*32+j][ci = sc*16+8h+0..7]
__device__ __forceinline__ void pack_weights_bf16x3_elem(size_t idx, const float* __restrict__ w, u32x4* __restrict__ wpk, int cout,
                                                         int cin, int taps, int transposed, int flip) {
  const int lane = idx & 63;
  size_t rest = idx >> 6;
  const int CT = (cout + 31) / 32;
  const int ct = rest % CT;
  rest /= CT;
  const int tap = rest % taps;
  const int sc = rest / taps;
  const int h = lane >> 5, j = lane & 31;
  const int co = ct * 32 + j;
  f32x4 v[2];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int ci = sc * 16 + h * 8 + e;
    const int st = flip ? taps - 1 - tap : tap;
    const size_t src = transposed ? ((size_t)ci * cout + co) * taps + st : ((size_t)co * cin + ci) * taps + st;
    v[e >> 2][e & 3] = (co < cout && ci < cin) ? w[src] : 0.f;
  }
  u32x2 a1, a2, a3, b1, b2, b3;
  split3(v[0], a1, a2, a3);
  split3(v[1], b1, b2, b3);
  u32x4* dst = wpk + (((size_t)(sc * taps + tap) * CT + ct) * 3) * 64 + lane;
  dst[0] = u32x4{a1[0], a1[1], b1[0], b1[1]};
  dst[64] = u32x4{a2[0], a2[1], b2[0], b2[1]};
  dst[128] = u32x4{a3[0], a3[1], b3[0], b3[1]};
}
__global__ void pack_weights_bf16x3_kernel(const float* __restrict__ w, u32x4* __restrict__ wpk, int cout, int cin, int taps,
                                           size_t total, int transposed, int flip) {
  const size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x;  // one thread per (sc, tap, ct, lane)
  if (idx >= total) return;
  pack_weights_bf16x3_elem(idx, w, wpk, cout, cin, taps, transposed, flip);
}

// every tensor of a plan in one launch: blockIdx.y = job; raw copy, then the f32 (or init) image, then the bf16x3 image, each read
// from the caller's tensor
__global__ void __launch_bounds__(256) pack_jobs_kernel(const PackJob* __restrict__ jobs) {
  const PackJob j = jobs[blockIdx.y];
  const size_t t0 = blockIdx.x * (size_t)256 + threadIdx.x, stride = gridDim.x * (size_t)256;
  for (size_t i = t0; i < j.numel; i += stride) j.raw[i] = j.src[i];
  if (j.pk) {
    if (j.kind == 3) {
      for (size_t i = t0; i < j.n_pk; i += stride) pack_init_weights_elem((int)i, j.src, j.pk, j.cout, j.cin);
    } else {
      for (size_t i = t0; i < j.n_pk; i += stride) pack_weights_elem(i, j.src, j.pk, j.cout, j.cin, j.taps, j.kind == 2 || j.tr, j.flip);
    }
  }
  if (j.bf3)
    for (size_t i = t0; i < j.n_bf3; i += stride)
      pack_weights_bf16x3_elem(i, j.src, (u32x4*)j.bf3, j.cout, j.cin, j.taps, j.kind == 2 || j.tr, j.flip);
}
void launch_pack_jobs(const PackJob* d_jobs, int njobs, hipStream_t s) {
  if (njobs <= 0) return;
  hipLaunchKernelGGL(pack_jobs_kernel, dim3(48, (unsigned)njobs), dim3(256), 0, s, d_jobs);
  CD_HIP(hipGetLastError());
}

void launch_pack_weights_bf16x3(const float* w_torch, void* wpk, int cout, int cin, int taps, hipStream_t s, bool transposed,
                                bool flip) {
  CD_REQUIRE(cin % 16 == 0, "bf16x3 convolution needs input channels in multiples of 16");
  const size_t total = (size_t)(cin / 16) * taps * ((cout + 31) / 32) * 64;
  hipLaunchKernelGGL(pack_weights_bf16x3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, w_torch, (u32x4*)wpk, cout,
                     cin, taps, total, transposed ? 1 : 0, flip ? 1 : 0);
  CD_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------------------
// forward conv (3x3x3 stride 1, and the strided (3,4,4) down-sampling conv): which kernel runs it
// ------------------------------------------------------------------------------------------------------------
std::map<std::string, int>& tune_cache() {
  static std::map<std::string, int> c;
  return c;
}

namespace {
struct ConvTile {
  int TZ, TH, NW, VT;
  size_t lds;
};

// Candidate output tiles / wave layouts, ranked by an estimate of whole-chip MFMA time (tile quantisation in 32-voxel
// MFMA rows, SIMD balance, tail rounds over 256 CUs) subject to the 160 KiB LDS per CU; the best few are timed on the
// device once per geometry (autotune above), the top-ranked one is the fallback when timing is not possible.
std::vector<ConvTile> conv_tile_candidates(const ConvGeom& g, int batch, int CT, int keep, int vox_bytes = 144) {
  std::vector<std::pair<double, ConvTile>> all;
  const int max_vt = 8 / CT;
  for (int TZ = 1; TZ <= g.out.d && TZ <= 12; ++TZ) {
    for (int nth = 1; nth <= g.out.h; ++nth) {
      const int TH = (g.out.h + nth - 1) / nth;
      if (nth > 1 && (g.out.h + nth - 2) / (nth - 1) == TH) continue;  // same TH as previous nth
      const int IZ = (TZ - 1) * g.sz + g.kd, IH = (TH - 1) * g.sh + g.kh;
      const size_t lds = ((size_t)IZ * IH * g.in.w + 1) * vox_bytes;
      if (lds > 150 * 1024) continue;
      const int tiles = (TZ * TH * g.out.w + 31) / 32;
      for (int NW = 1; NW <= 8; ++NW) {
        const int VT = (tiles + NW - 1) / NW;
        if (VT > max_vt || VT < 1) continue;
        if (NW > 1 && (tiles + NW - 2) / (NW - 1) == VT) continue;  // a smaller NW already covers it with the same VT
        const int nTZ = (g.out.d + TZ - 1) / TZ;
        const long nblocks = (long)batch * nTZ * nth;
        int bpc = (int)(160 * 1024 / lds);
        bpc = bpc < 1 ? 1 : bpc;
        while (bpc > 1 && bpc * NW > 16) --bpc;
        const long per_cu = (nblocks + 255) / 256;
        const long rounds = (per_cu + bpc - 1) / bpc;
        const int resident = (int)(per_cu < bpc ? per_cu : bpc);
        double per_round = (double)((resident * NW + 3) / 4) * VT;
        const double cost = rounds * per_round + 0.02 * (double)IZ * IH * g.in.w / 32.0 * rounds;
        all.push_back({cost, ConvTile{TZ, TH, NW, VT, lds}});
      }
    }
  }
  CD_REQUIRE(!all.empty(), "no convolution tiling fits in LDS (grid too wide in r?)");
  std::stable_sort(all.begin(), all.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
  std::vector<ConvTile> out;
  for (auto& c : all) {
    out.push_back(c.second);
    if ((int)out.size() >= keep) break;
  }
  return out;
}

// the halo-tiled kernels' argument block for output tile `t` of conv `g`
ConvKArgs conv_k_args(const ConvGeom& g, const ConvTile& t, const ConvFusion& fu, const float* in0, int c0, const float* in1, int c1,
                      const float* wpk, const float* bias, float* out, int cout) {
  ConvKArgs a;
  a.in0 = in0; a.in1 = in1; a.c0 = c0; a.c1 = c1; a.wpk = wpk; a.bias = bias; a.out = out;
  a.Din = g.in.d; a.Hin = g.in.h; a.Win = g.in.w; a.Do = g.out.d; a.Ho = g.out.h; a.Wo = g.out.w;
  a.KD = g.kd; a.KH = g.kh; a.KW = g.kw; a.SZ = g.sz; a.SH = g.sh; a.SW = g.sw;
  a.TZ = t.TZ; a.TH = t.TH; a.nTZ = (g.out.d + t.TZ - 1) / t.TZ; a.nTH = (g.out.h + t.TH - 1) / t.TH;
  a.IZ = (t.TZ - 1) * g.sz + g.kd; a.IH = (t.TH - 1) * g.sh + g.kh;
  a.cout = cout; a.CTtot = cout / 32; a.coef = fu.coef; a.act = fu.act;
  return a;
}
}  // namespace

void launch_conv_mfma(const float* in0, int c0, const float* in1, int c1, const float* wpk, const float* bias, float* out,
                      int batch, int cout, const ConvGeom& g, hipStream_t s, const ConvFusion& fu_in) {
  CD_REQUIRE((!fu_in.coef && !fu_in.defer.part) || c1 == 0, "conv: a fused input normalisation needs a single (non-concatenated) source");
  if (fu_in.units) *fu_in.units = 0;  // set by kernels that produce the output statistics themselves
  CD_REQUIRE(c0 % 32 == 0 && c1 % 32 == 0 && c0 > 0, "conv: channel counts must be multiples of 32");
  CD_REQUIRE(cout % 32 == 0, "conv: output channels must be a multiple of 32");
  CD_REQUIRE(g.kw <= 4, "conv: r kernel extent > 4 unsupported");
  const int CTtot = cout / 32;
  const int CT = CTtot <= 3 ? CTtot : 2;
  CD_REQUIRE(CTtot % CT == 0, "conv: unsupported output channel count");
  char cat[128];
  std::snprintf(cat, sizeof cat, "conv%dx%dx%d_s%d C%d->%d @%dx%dx%d", g.kd, g.kh, g.kw, g.sh, c0 + c1, cout, g.in.d, g.in.h, g.in.w);
  const double taps = (double)g.kd * g.kh * g.kw;
  prof::Scope scope(cat, s, 2.0 * taps * (c0 + c1) * cout * (double)g.out.vox() * batch,
                    4.0 * batch * ((double)g.in.vox() * (c0 + c1) + (double)g.out.vox() * cout));
  // deferred input normalisation: the split-16 kernels fold it in their prologue; for every other kernel the coefficient
  // table is materialised first by a gn_finalize launch
  ConvFusion fu = fu_in;
  auto materialise = [&]() {
    if (!fu.defer.part) return;
    if (fu.defer.coef_out) fu.coef_buf = fu.defer.coef_out;  // (training tape: the table is wanted in memory anyway)
    CD_REQUIRE(fu.coef_buf, "conv: deferred normalisation needs a coefficient buffer for kernels without the prologue");
    launch_gn_finalize(fu.defer.part, fu.defer.units, fu.defer.gamma, fu.defer.beta, fu.defer.add, fu.defer.add_ld, fu.coef_buf, batch,
                       fu.defer.C, fu.defer.groups, fu.defer.vox, s, fu.defer.stat_out);
    fu.coef = fu.coef_buf;
    fu.defer = GnDefer();
  };
  // One rung of the halo-tiled kernels: nterm = 2 (f16x2) / 3 (bf16x3) on that 16-bit image `w`, 0 = f32 MFMA on the f32 image.
  // false: no candidate tiling has a kernel instance in that arithmetic (f16x2 holds two accumulators per tile)
  auto tiled = [&](int nterm, const void* w) -> bool {
    std::vector<ConvTile> cand;
    for (const ConvTile& t : conv_tile_candidates(g, batch, CT, 14, nterm == 2 ? 80 : (nterm == 3 ? 96 : 144)))
      if (nterm == 0 || (nterm == 2 ? t.VT * CT <= 2 : (t.VT <= 4 && !(CT == 3 && t.VT > 2)))) cand.push_back(t);
    if (cand.empty()) return false;
    auto launch = [&](const ConvTile& t) {
      ConvTiled3Args a3;
      a3.k = conv_k_args(g, t, fu, in0, c0, in1, c1, (const float*)w, bias, out, cout);
      const int units = a3.k.nTZ * a3.k.nTH;
      dim3 grid((unsigned)(batch * units), (unsigned)(CTtot / CT));
      if (nterm == 0) {  // (no statistics epilogue: *fu.units stays 0)
        launch_conv_tiled_f32(t.VT, CT, a3.k, grid, t.NW * 64, t.lds, s);
        return;
      }
      a3.status = fu.status;
      const int64_t cap = (g.out.vox() + 31) / 32;  // capacity of the caller's partial buffer (units per sample)
      a3.ch_part = (fu.ch_part && units <= cap) ? fu.ch_part : nullptr;
      if (fu.units) *fu.units = a3.ch_part ? units : 0;
      const size_t red = (size_t)t.NW * CT * 32 * 2 * 4;  // cross-wave reduction scratch of the stats epilogue
      launch_conv_tiled_split16(t.VT, CT, nterm, a3, grid, t.NW * 64, std::max(t.lds, red), s);
    };
    char key[192];
    if (nterm) std::snprintf(key, sizeof key, "tiled_%s %s b%d", nterm == 2 ? "f16x2" : "bf16x3", cat, batch);
    else std::snprintf(key, sizeof key, "tiled %s b%d", cat, batch);
    const int pick = autotune(key, (int)cand.size(), [&](int i) { launch(cand[i]); }, s);
    launch(cand[pick < 0 ? 0 : pick]);
    return true;
  };

  // The ladder.  f16x2 first wherever a kernel has that arm and the process runs in that arithmetic, then the exact split, then f32.
  const int prec = conv_precision();
  const void* w_bf16x3 = prec != PREC_F32 ? fu.wpk_bf16x3 : nullptr;
  const void* w_f16x2 = w_bf16x3 && prec == PREC_F16X2 ? (const char*)w_bf16x3 + packed_bf16x3_bytes(c0 + c1, cout, g.kd * g.kh * g.kw) : nullptr;
  if (w_f16x2 && try_launch_conv_zslide(in0, c0, in1, c1, w_f16x2, bias, out, batch, cout, g, s, fu)) return;
  if (w_f16x2 && try_launch_conv_small(in0, c0, in1, c1, w_f16x2, bias, out, batch, cout, g, s, fu)) return;
  if (w_f16x2 && try_launch_conv3_flat(in0, c0, in1, c1, w_f16x2, bias, out, batch, cout, g, s, fu, 2)) return;
  materialise();  // (the rungs below read the coefficient table)
  if (w_bf16x3 && try_launch_conv3_flat(in0, c0, in1, c1, w_bf16x3, bias, out, batch, cout, g, s, fu, 3)) return;
  if (try_launch_conv3_flat(in0, c0, in1, c1, wpk, bias, out, batch, cout, g, s, fu, 0)) return;
  if (w_f16x2 && !fu.in_absmax && tiled(2, w_f16x2)) return;
  if (w_bf16x3 && tiled(3, w_bf16x3)) return;
  tiled(0, wpk);
}

}  // namespace cd
