// Linear attention, forward: the unfused kernels on the f32 MFMA (kernels_attn_unfused.hip) and the fused forms of the sampling
// path (kernels_attn.hip).  heads = 1, dim_head = 32.
#pragma once
#include "cd_common.h"
#include "kernels_gn.h"

namespace cd {

constexpr float kAttnScale = 0.17677669529663689f;  // 32^-1/2: LinearAttention's dim_head^-1/2

int attn_nsplit_for(int64_t vox, int batch);
size_t attn_partial_floats(int batch, int nsplit);
void launch_attn_context(const float* qkv, float* partials, int batch, int64_t vox, int nsplit, hipStream_t s);
void launch_attn_combine(const float* partials, int nsplit, const float* w_out /*torch (C,32)*/, int cout, float* wpk_b,
                         int batch, float scale, hipStream_t s, float* ctx_out = nullptr /* [B][32][32] unscaled context */,
                         float* kstat_out = nullptr /* [B][32][2] = {max, 1/sum} of the k softmax */,
                         bool layout_T = false /* wpk_b in the K order of launch_attn_out instead of the pointwise one */);
// The unfused attention from the normalised input to y = to_out's conv, in buffers the caller has allocated: qkv = to_qkv(coef x)
// (B, vox, 96), launch_attn_context into partials ([B][nsplit][1088]), launch_attn_combine into the per-sample folded weights wpk_b
// ([B][ceil(C/32)][1024]), then y = wpk_b softmax32(q) + bias with its channel partials ch_part ([B][pointwise_units][C][2]).
// ctx_out / kstat_out: as launch_attn_combine's, for the training tape.
void launch_attn_unfused(const float* x, int C, const float* coef, const float* wqkv, const float* w_out, const float* bias,
                         float* qkv, float* partials, int nsplit, float* wpk_b, float* y, float* ch_part, int batch, int64_t vox,
                         hipStream_t s, float* ctx_out = nullptr, float* kstat_out = nullptr);

// fused linear attention of the sampling path (kernels_attn.hip): qkv is never materialised
int attn_fused_nsplit_for(int64_t vox, int batch);
// whole attention block in one launch for small grids (kernels_attn.hip: attn_small_kernel)
bool attn_small_eligible(int64_t vox);
void launch_attn_small(const float* x, int C, const float* coef, const void* wqkv_f16x2, float* partials, const float* w_out,
                       float scale, const float* bias, const float* out_gamma, const float* out_beta, float* y, float* ch_part,
                       int batch, int64_t vox, hipStream_t s, const GnDefer* defer, int* status = nullptr,
                       // capacity of partials ([B][max_parts][1088]) and ch_part ([B][max_parts][C][2]) in parts per sample: with
                       // CD_ATTN_COOP the sample's voxels are dealt to up to that many co-operating workgroups, which meet at
                       // barriers on coop_sync ([kAttnCoopSamples][2] words the caller owns; null: no co-operative form)
                       int max_parts = 1, unsigned* coop_sync = nullptr);
constexpr int kAttnCoopSamples = 8192;
// moments ([B][nsplit][1056], attn_moment_floats): pass 1 also accumulates the first and second moments of softmax(q), from which
// pass 2 (given the same buffer and the closing GroupNorm's parameters) writes the BLOCK's output gn(y) + x directly -- no y
// tensor, no channel sums, no gn_apply pass
bool attn_moments_eligible(int C);
size_t attn_moment_floats(int batch, int nsplit);
void launch_attn_kv_context(const float* x, int C, const float* coef, const void* wqkv_f16x2, float* partials, int batch,
                            int64_t vox, int nsplit, hipStream_t s, const GnDefer* defer = nullptr, int* status = nullptr,
                            float* moments = nullptr);
void launch_attn_out(const float* x, int C, const float* coef, const void* wqkv_f16x2, const float* wT_b, const float* bias,
                     float* y, float* ch_part /* [B][nsplit][C][2] */, int batch, int64_t vox, int nsplit, hipStream_t s,
                     const GnDefer* defer = nullptr,
                     // wT_b == null: every workgroup merges the pass-1 partials and folds W_out itself (no combine launch)
                     const float* partials = nullptr, const float* w_out = nullptr, float scale = 0.f, int* status = nullptr,
                     const float* moments = nullptr, const float* out_gamma = nullptr, const float* out_beta = nullptr);

}  // namespace cd
