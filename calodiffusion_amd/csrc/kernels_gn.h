// GroupNorm forward (kernels_gn.hip) and the descriptor of a deferred normalisation (device side: gn_defer.h).
#pragma once
#include "cd_common.h"

namespace cd {

// Deferred GroupNorm coefficients (gn_defer.h): instead of a coefficient table the consumer gets the producer's channel
// partials and the affine parameters and folds them in its prologue.  part == nullptr: not deferred.
struct GnDefer {
  const float* part = nullptr;  // [B][units][C][2]
  int units = 0;
  const float* gamma = nullptr;
  const float* beta = nullptr;
  const float* add = nullptr;   // [B][add_ld] added after the activation, or null
  int add_ld = 0;
  int C = 0, groups = 0;
  int64_t vox = 0;
  // training tape: the folded table ([B][C][4]) and {mean, rstd} per (sample, group) ([B][G][2]) are also written to memory, by
  // every workgroup that folds them (the fold is deterministic, so they all store the same values): the backward pass reads what
  // the forward used, and no gn_finalize launch is needed for it
  float* coef_out = nullptr;
  float* stat_out = nullptr;
};

int gn_nsplit_for(int64_t vox, int batch);
// channel partials [B][nsplit][C][2] of a tensor whose producer has no stats epilogue
void launch_ch_stats(const float* x, float* part, int batch, int channels, int64_t vox, int nsplit, hipStream_t s);
// coef[B][C][4] = {rstd*gamma, beta - mean*rstd*gamma, add_bc[b][c] or 0, 0} from `units` channel partials per sample
void launch_gn_finalize(const float* part, int units, const float* gamma, const float* beta, const float* add_bc, int add_ld,
                        float* coef, int batch, int channels, int groups, int64_t vox, hipStream_t s,
                        float* stat_out = nullptr /* [B][G][2] = {mean, rstd}, kept for the backward pass */);
int gn_apply_blocks_per_sample(int batch, int channels, int64_t vox);
// y = act(scale*x + shift) + add (+ residual; residual1/res_c0: shortcut read from a two-source channel concat);
// part_out (optional): channel partials of y, [B][gn_apply_blocks_per_sample][C][2]
// defer (optional): fold the coefficients in the kernel's prologue instead of reading `coef`
void launch_gn_apply(const float* x, float* y, const float* coef, int batch, int channels, int64_t vox, int silu,
                     const float* residual, const float* residual1, int res_c0, float* part_out, hipStream_t s,
                     const GnDefer* defer = nullptr);

}  // namespace cd
