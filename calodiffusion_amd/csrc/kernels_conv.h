// Forward convolutions (kernels_conv*.hip, kernels_pointwise.hip, kernels_init_conv.hip): geometry, fusion options, weight
// packing and the launchers.  What the conv units share among themselves is in conv_internal.h.
#pragma once
#include "cd_common.h"
#include "kernels_gn.h"

namespace cd {

// Packed weight layout shared by every MFMA kernel (32x32x2 f32):
//   wpk[chunk][tap][ct][q][lane][e]   chunk = ci/32, ct = co/32, lane = h*32 + j, m = 4q+e
//   holds W[co = ct*32 + j][ci = chunk*32 + h*16 + m][tap]
// so that one wave-wide 16-B load (fixed q) is 1 KiB contiguous and lane (j,h) receives the B-operand
// values of MFMAs m = 4q..4q+3 for its output column j and k-half h.
inline size_t packed_weight_floats(int cin, int cout, int taps) {
  return (size_t)(cin / 32) * taps * ((cout + 31) / 32) * 2048;
}

// ---- kernel launchers (defined in the .hip files) ---------------------------------------------------------
struct ConvGeom {
  Dims3 in, out;
  int kd, kh, kw;   // kernel extents
  int sz, sh, sw;   // strides
};

// SiLU on the transcendental unit: t * rcp(1 + exp2(-t log2 e)), ~3 ulp (libm's expf + a division is ~30 VALU instructions
// per element in kernels whose staging is VALU-bound)
__device__ __forceinline__ float cd_fast_silu(float t) {
  return t * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(t * -1.4426950408889634f));
}

// GroupNorm fusion around a conv (all optional):
//   coef     [B][Cin][4] = {scale, shift, add, -}: y = act(scale*x + shift) + add applied to the input as it is staged
//            (GroupNorm affine folded per sample and channel by launch_gn_finalize; `add` = the time/cond embedding);
//   ch_part  [B][units][Cout][2] = per-workgroup {sum, sum of squares} of the conv output, units <= ceil(vox/32);
//            *units is set to the number of workgroups per sample that wrote partials, or 0 if the chosen kernel
//            cannot (the caller then runs launch_ch_stats on the output).
struct ConvFusion {
  const float* coef = nullptr;
  int act = 0;
  float* ch_part = nullptr;
  int* units = nullptr;
  // 16-bit split images of the weights (launch_pack_weights_split16): the bf16x3 image, followed at
  // packed_bf16x3_bytes() by the f16x2 image
  const void* wpk_bf16x3 = nullptr;
  int* status = nullptr;  // device word; bit 0 is set when a value staged for an f16x2 conv exceeds the fp16 range
  // alternative to `coef`: fold the input normalisation from `defer` in the kernel's prologue.  Kernels without that
  // prologue get the table materialised into `coef_buf` ([B][Cin][4]) by a gn_finalize launch first.
  GnDefer defer;
  float* coef_buf = nullptr;
  // max |input| as a float bit pattern in a device word (launch_absmax_bits), or null.  Given, the f16x2 kernels multiply the
  // staged input by 2^s (bringing that maximum to ~2^10) and their output by 2^-s: the input gradients of a conv are
  // O(1e-6), deep in the fp16 subnormals, and the conv is linear.  Needs bias == null and no input normalisation.
  const unsigned* in_absmax = nullptr;
  // out = conv + add_src (a tensor shaped like `out`, bias == null): the identity shortcut's share of a ResnetBlock's input gradient
  // joins the input-gradient conv's epilogue instead of a separate elementwise pass.  The f16x2 kernels (z-slide, flat, small-grid)
  // honour it and set *add_done = 1 on the host; any other kernel ignores it and the caller adds the tensor itself.
  const float* add_src = nullptr;
  int* add_done = nullptr;
  // z-slide kernel only: deal every strip in this many chunks instead of the launcher's own count (0).  Chunking along voxels changes
  // no output's summation order, only the grouping of the statistics partials (cd_op_zslide_conv: the test of exactly that).
  int zs_chunks = 0;
  // Output side of a ResnetBlock's second conv on a grid small enough for one workgroup to see a whole (sample, 32-channel tile)
  // (kernels_conv_small.hip): the kernel applies the block's closing GroupNorm + SiLU and adds the shortcut itself,
  //   out = silu(gn(conv + bias)) + (res0 | res1),
  // and sets *gn_out.done = 1 on the host; every other kernel ignores the request and the caller runs gn_apply as before.
  struct GnOut {
    const float* gamma = nullptr;  // (cout); null = no request
    const float* beta = nullptr;
    int groups = 0;
    const float* res0 = nullptr;   // shortcut: (B, vox, res_c0) [and res1: (B, vox, cout - res_c0), an un-materialised concat]
    const float* res1 = nullptr;
    int res_c0 = 0;
    float* part_out = nullptr;     // [B][1][cout][2] channel partials of `out` (for a following PreNorm), or null
    int* done = nullptr;
  } gn_out;
};
// Zeroed device words for max |x| bit patterns (launch_absmax_bits, launch_gn_backward), handed out in order from a region the
// caller owns and has zeroed on the stream: a training step's sits beside its demb in the workspace, a cd_op_* primitive's in its
// own scratch
struct AbsmaxWords {
  unsigned* next = nullptr;
  unsigned* end = nullptr;
  unsigned* take() {
    CD_REQUIRE(next && next < end, "internal: out of max-|x| words");
    return next++;
  }
};
// max |x| (bit pattern) into a word taken from `words`; valid in stream order
const unsigned* launch_absmax_bits(const float* x, size_t n, AbsmaxWords* words, hipStream_t s);
// 2^s and 2^-s for a tensor whose max |x| has bit pattern mb: s = 10 - floor(log2 max)
__host__ __device__ inline void pow2_scale_for(unsigned mb, float* scale, float* inv) {
  const int e = (int)((mb >> 23) & 0xff) - 127;
  int sexp = mb == 0u ? 0 : 10 - e;
  sexp = sexp < -100 ? -100 : (sexp > 100 ? 100 : sexp);
  union { unsigned u; float f; } a, b;
  a.u = (unsigned)(127 + sexp) << 23;
  b.u = (unsigned)(127 - sexp) << 23;
  *scale = a.f;
  *inv = b.f;
}
inline size_t packed_bf16x3_bytes(int cin, int cout, int taps) {
  return (size_t)(cin / 16) * taps * ((cout + 31) / 32) * 3 * 64 * 16;
}
inline size_t packed_f16x2_bytes(int cin, int cout, int taps) {
  return (size_t)(cin / 16) * taps * ((cout + 31) / 32) * 2 * 64 * 16;
}
inline size_t packed_split16_bytes(int cin, int cout, int taps) {
  return packed_bf16x3_bytes(cin, cout, taps) + packed_f16x2_bytes(cin, cout, taps);
}
void launch_pack_weights_bf16x3(const float* w_torch, void* wpk, int cout, int cin, int taps, hipStream_t s,
                                bool transposed = false, bool flip = false);
void launch_pack_weights_f16x2(const float* w_torch, void* wpk, int cout, int cin, int taps, hipStream_t s,
                               bool transposed = false, bool flip = false);
inline void launch_pack_weights_split16(const float* w_torch, void* wpk, int cout, int cin, int taps, hipStream_t s,
                                        bool transposed = false, bool flip = false) {
  launch_pack_weights_bf16x3(w_torch, wpk, cout, cin, taps, s, transposed, flip);
  launch_pack_weights_f16x2(w_torch, (char*)wpk + packed_bf16x3_bytes(cin, cout, taps), cout, cin, taps, s, transposed, flip);
}

// packed image Wp[co'][ci'][tap'] (see above) of torch weights: transposed = stored [ci'][co'][tap] (ConvTranspose3d, or the
// input gradient of a Conv3d, whose roles of in/out channels swap); flip = tap' <- taps-1-tap' (input gradient, stride 1)
void launch_pack_weights(const float* w_torch, float* wpk, int cout, int cin, int taps, bool transposed, hipStream_t s,
                         bool flip = false);
void launch_pack_init_weights(const float* w_torch, float* wpk, int cout, int cin, hipStream_t s);
// All weights of a plan in two launches (cd_plan_set_weights: the re-pack after every optimizer step was ~400 launches and 3 ms
// of host time per training step).  One job per tensor; null images are skipped.
struct PackJob {
  const float* src;  // the caller's tensor (device)
  float* raw;        // copy in the plan arena
  float* pk;         // f32 MFMA image (kind 1, 2) or the init conv's [tap][ci][cout] image (kind 3), or null
  void* bf3;         // bf16x3 image or null
  void* f16;         // f16x2 image or null
  int cout, cin, taps;
  int kind;          // 0 = raw only, 1 = conv, 2 = transposed conv (images in transposed channel order), 3 = init conv
  int tr, flip;      // (the input-gradient images of the training step: train.hip dgrad_images) stored [ci][co][tap] / taps reversed;
                     // raw may then be null (numel 0) and src is the plan's own copy of the tensor
  unsigned long long numel, n_pk, n_bf3, n_f16;  // work items of the four phases
};
void launch_pack_jobs(const PackJob* d_jobs, int njobs, hipStream_t s);        // raw copy, f32 / init and bf16x3 images (kernels_conv.hip)
void launch_pack_jobs_f16x2(const PackJob* d_jobs, int njobs, hipStream_t s);  // f16x2 images (kernels_conv_zs.hip)

// forward conv on whichever kernel family fits it (kernels_conv.hip; the families and what they share: conv_internal.h)
void launch_conv_mfma(const float* in0, int c0, const float* in1, int c1, const float* wpk, const float* bias, float* out,
                      int batch, int cout, const ConvGeom& g, hipStream_t s, const ConvFusion& fu = ConvFusion());
// z-slide f16x2 kernel for the full-resolution 3x3x3 convs (kernels_conv_zs.hip); false = geometry not eligible
bool try_launch_conv_zslide(const float* in0, int c0, const float* in1, int c1, const void* wpk_f16x2, const float* bias, float* out,
                            int batch, int cout, const ConvGeom& g, hipStream_t s, const ConvFusion& fu);
// whole-sample-in-LDS f16x2 kernel for the deepest levels (kernels_conv_small.hip); false = geometry not eligible
bool try_launch_conv_small(const float* in0, int c0, const float* in1, int c1, const void* wpk_f16x2, const float* bias, float* out,
                           int batch, int cout, const ConvGeom& g, hipStream_t s, const ConvFusion& fu);
// whole ResnetBlock in one launch where a sample is <= 128 voxels and the block is 32 channels wide (kernels_conv_small.hip)
bool try_launch_res_block_small(const float* x0, int c0, const float* x1, int c1, const void* w1_f16x2, const float* b1,
                                const float* gn1_gamma, const float* gn1_beta, const float* emb, int emb_ld, const void* w2_f16x2,
                                const float* b2, const float* gn2_gamma, const float* gn2_beta, int groups, const float* res0,
                                const float* res1, int res_c0, float* h1, float* out, float* part_out, int batch, int cout,
                                Dims3 dims, int* status, hipStream_t s);
// kernels_conv_transpose.hip
void launch_conv_transpose_mfma(const float* in, int cin, const float* wpk, const float* bias, float* out, int batch,
                                int cout, Dims3 din, Dims3 dout, int kz, int sz, hipStream_t s,
                                const void* wpk_f16x2 = nullptr, int* status = nullptr, const unsigned* in_absmax = nullptr);

enum A_Prologue { A_NONE = 0, A_AFFINE = 1, A_SOFTMAX32 = 2, A_EXPNORM = 3 };
struct PointwiseArgs {
  const float* in0 = nullptr;  // (B, vox, ld0) read at channel offset off0, c0 channels
  int ld0 = 0, off0 = 0, c0 = 0;
  const float* in1 = nullptr;  // optional concat source
  int ld1 = 0, c1 = 0;
  const float* wpk = nullptr;
  int64_t w_batch_stride = 0;  // floats between per-sample weight sets (0 = shared)
  const float* bias = nullptr;
  const float* residual = nullptr;  // (B, vox, cout) added in the epilogue
  float* out = nullptr;
  int batch = 0, cout = 0;
  int64_t vox = 0;
  int prologue = A_NONE;
  const float* coef = nullptr;  // A_AFFINE: [B][Cin][4] {scale, shift, -, -} (a folded GroupNorm, see launch_gn_finalize);
                                // A_EXPNORM: [B][Cin][2] {max, 1/sum}: a <- exp(a - max)/sum (the voxel softmax of k)
  int out_ld = 0, out_off = 0;  // output row stride / channel offset (0 = cout, packed)
  float* ch_part = nullptr;     // optional channel partials of the output: [B][ceil(vox/128)][cout][2]
  // Block close of a ResnetBlock whose shortcut is this 1x1 conv (models.py:200): the epilogue adds  silu(gn(gn_res)) + add  --
  // gn_res the block's second conv output (B, vox, cout), normalisation folded from gn_defer's channel partials -- so the
  // shortcut tensor is never written and the block's own elementwise pass (gn_apply) never runs.  `out` may be gn_res itself.
  const float* gn_res = nullptr;
  GnDefer gn_defer;
  // f16x2 image of the weights ([k-step][cout tile][w1 | w2'] as the conv kernels hold them; shared weights only): with prologue
  // A_NONE the products run on the fp16 pipe -- two-term splits, 3 x 32-cycle MFMAs per 16 channels instead of 8 x 64-cycle fp32
  // ones -- in fp16 RANGE: an input beyond it sets bit 0 of *status (the caller's range fallback re-runs at full range, wpk16 = null)
  const void* wpk16 = nullptr;
  int* status = nullptr;
};
inline int pointwise_units(int64_t vox) { return (int)((vox + 127) / 128); }
void launch_pointwise(const PointwiseArgs& a, hipStream_t s);  // kernels_pointwise.hip

struct InitConvArgs {
  const float* x = nullptr;       // (B, cx, D, H, W) planar
  int cx = 0;                     // planar channels present in x
  int cin = 0;                    // logical input channels of the conv (cx + synthesised coordinate channels)
  const float* scale_b = nullptr; // per-sample multiplier of channel 0 (c_in) or null: scale_b[b * scale_stride]
  int scale_stride = 1;
  const float* sigma_b = nullptr; // alternative to scale_b: channel 0 is scaled by c_in = 1/sqrt(sigma_b[b]^2 + sigma_data^2)
  float sigma_data = 1.f;         // (get_scaling, loss.py:29-41) so that the conv does not wait for the embedding kernel
  const float* r_w = nullptr;     // coordinate profiles, used when cin > cx
  const float* z_d = nullptr;
  const float* phi_h = nullptr;
  int use_rz = 0, use_phi = 0;
  const float* wpk = nullptr;     // [tap][ci][cout]
  const float* bias = nullptr;
  float* out = nullptr;           // channels-last
  int batch = 0, cout = 0;
  Dims3 dims{};
  float* coord_table = nullptr;   // optional (vox, cout) buffer: enables the matrix-core path (cx == 1), which splits the conv
                                  // into the sample-independent coordinate-channel part (+ bias) and the x part
  bool table_ready = false;       // coord_table already holds that part (launch_init_coord_table); else it is filled first
  int* status = nullptr;          // bit 0: a staged value exceeded the fp16 range (matrix-core path)
};
void launch_init_conv(const InitConvArgs& a, hipStream_t s);  // kernels_init_conv.hip
// coordinate channels + bias of the init conv into a.coord_table (vox, cout): changes only with the weights / profiles
void launch_init_coord_table(const InitConvArgs& a, hipStream_t s);

// ---- init conv + the first block's first conv as ONE one-channel 5x5x5 conv of c_in x (kernels_init_pair.hip) ----
// Nothing non-linear lies between the init conv and the 32 -> 32 3x3x3 conv that reads it, and x has one data channel:
//   conv1(init_conv(x)) + b1 = T1 + sum_d Wc[class][d] c_in x(p + d - 2),
// T1 = conv1(coordinate table) + b1 (vox, 32) and Wc the two kernels composed over the 5x5x5 offsets d.  conv1 zero-pads the init
// conv's OUTPUT in z and r, so the composed weights depend on the output voxel's boundary class: class = 3 zc + rc,
// zc / rc = 0 first plane / column, 1 interior, 2 last (the taps that would read the padding are left out of the sum).
constexpr int kInitPairClasses = 9;
constexpr int kInitPairKSteps = 8;  // K = 125 offsets padded to 128
// f16x2 image of the composed weights: [class][k-step][term][lane = half * 32 + co][8 fp16], k = 16 ks + 8 half + e = offset index
constexpr size_t kInitPairWeightBytes = (size_t)kInitPairClasses * kInitPairKSteps * 2 * 64 * 16;
struct InitPairArgs {
  const float* x = nullptr;        // (B, D, H, W): the data channel
  const float* scale_b = nullptr;  // per-sample multiplier c_in (scale_b[b * scale_stride]), or null
  int scale_stride = 1;
  const float* sigma_b = nullptr;  // alternative: c_in = 1 / sqrt(sigma_b[b]^2 + sigma_data^2), as the init conv forms it
  float sigma_data = 1.f;
  const void* wc = nullptr;        // composed weights (kInitPairWeightBytes)
  const float* table = nullptr;    // T1 (vox, 32)
  float* out = nullptr;            // (B, vox, 32) channels-last
  float* ch_part = nullptr;        // [B][units][32][2] channel partials {sum, sum of squares} of `out`, one unit per workgroup
  int batch = 0;
  Dims3 dims{};
  int* status = nullptr;           // bit 0: |c_in x| exceeded the fp16 range
  int slabs = 0;                   // workgroups per sample (0: the launcher's own count)
};
// geometry only: both boundary classes of an axis must be distinct voxels, and one plane with its halo must fit the LDS image
bool init_pair_eligible(Dims3 dims);
// workgroups per sample = units of the channel partials (depends on the batch as the chunk counts of the other convs do)
int init_pair_units(Dims3 dims, int batch, int slabs = 0);
// composed weights and table from the two convs' torch-layout weights (w0: (32, cin, 27), data channel 0; w1: (32, 32, 27)) and the
// init conv's coordinate table (vox, 32): fp64 sums in a fixed order
void launch_init_pair_build(const float* w0, int cin, const float* w1, const float* b1, const float* init_table, void* wc, float* table,
                            Dims3 dims, hipStream_t s);
void launch_init_pair_conv(const InitPairArgs& a, int* units, hipStream_t s);

}  // namespace cd
