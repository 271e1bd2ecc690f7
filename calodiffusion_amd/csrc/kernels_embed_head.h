// The two ends of the U-Net: time / condition embedding (kernels_embed.hip) and the 1x1x1 head with the EDM combination
// (kernels_head.hip).
#pragma once
#include "cd_common.h"
#include "kernels_gn.h"

namespace cd {

struct EmbedLayer {
  const float* w;  // (cout, 128) torch layout
  const float* b;
  int cout;
  int offset;  // column offset in the per-sample embedding row
};
struct EmbedArgs {
  const float* cond = nullptr;  // (B, cond_size)
  const float* time_or_sigma = nullptr;  // (B,)
  int time_kind = 0;
  float sigma_data = 1.f;
  int cond_size = 0, cond_hidden = 0, half = 0;
  const float *tw1, *tb1, *tw2, *tb2, *tw3, *tb3;
  const float *cw1, *cb1, *cw2, *cb2, *cw3, *cb3;
  const EmbedLayer* layers = nullptr;  // device array
  int n_layers = 0;
  float* emb = nullptr;  // (B, emb_ld)
  int emb_ld = 0;
  float* scal = nullptr;  // (B, 4): c_in, c_skip, c_out, sigma
  int batch = 0;
  // SinusoidalPositionEmbeddings(half/2) (models.py:132-144) in place of the first Linear+GELU of the time / cond branch
  // (CondUnet(time_embed=True / cond_embed=True), models.py:578-601): tw1/tb1 resp. cw1/cb1 are unused then, and cond is (B,)
  int time_sin = 0, cond_sin = 0;
  // Several steps of one trajectory in one launch (the sampler loop's embeddings, a chunk of steps ahead): workgroup b embeds
  // sample b % cond_rows at the time value time_or_sigma[(b / cond_rows) * time_stride].  cond_rows = 0: one step, as before.
  int cond_rows = 0, time_stride = 0;
  // The ResnetBlock projections are linear in SiLU(cat(t, c)) (models.py:176-180, 707): W SiLU(cat(t, c)) + b = [W_t SiLU(t) + b] +
  // [W_c SiLU(c)].  part = 1: row b is a TIME row (time value time_or_sigma[b * time_stride], no condition): the first bracket and
  // the scalings; part = 2: row b is a CONDITION row: the second bracket, no bias, no scalings.  0: the whole expression.
  int part = 0;
};
void launch_embed(const EmbedArgs& a, hipStream_t s);
void launch_silu_linear(const float* cond, const float* w, const float* bias, float* out, int batch, int nin, int nout,
                        hipStream_t s);

struct HeadArgs {
  const float* h = nullptr;   // (B, vox, 32) channels-last
  const float* w = nullptr;   // (32,) torch layout of the 1x1x1 head
  const float* bias = nullptr;
  const float* x = nullptr;   // (B, vox) network input before c_in scaling (null for raw unet_forward)
  const float* scal = nullptr;  // (B,4) or null
  int objective = 0;
  float* out = nullptr;       // (B, vox): F (raw) or x0
  int batch = 0;
  int64_t vox = 0;
  // The closing GroupNorm + SiLU + identity shortcut of the final ResnetBlock applied on the fly (defer.part != null): h is then
  // that block's second conv output and `res` its input; saves the block's own elementwise pass over the level-0 tensor.
  GnDefer defer;
  const float* res = nullptr;
  // DDim.__call__'s update of the running sample (models/sample.py:88-107) in the same pass (needs x and scal): with
  // stepvals = {sigma, sigma_prev*[t>0], ddim_sigma, denom}:  x_next = x0 + sigma_prev (x - x0) / sigma + ddim_sigma noise / denom
  // -- in place of a launch and a pass over x / x0 of its own.  upd_x_next may alias x.
  const float* upd_stepvals = nullptr;  // null: no update
  const float* upd_noise = nullptr;
  float* upd_x_next = nullptr;
  float* upd_xs = nullptr;
  float* upd_x0s = nullptr;
};
void launch_head(const HeadArgs& a, hipStream_t s);

}  // namespace cd
