// Backward: weight gradients of the convolutions (kernels_wgrad.hip, kernels_wgrad16.hip; their rungs: wgrad_internal.h).
#pragma once
#include "cd_common.h"
#include "kernels_conv.h"

namespace cd {

size_t wgrad_partial_floats(int64_t out_vox, int batch, bool per_sample, int A, int Bc, int T);
// Deferred slot reductions of the weight gradients (training step).  Every launch_wgrad ends in a reduction of its per-workgroup
// partials: ~28 MB read for a few hundred KB of dw whatever the level, 65 launches of 4-7 us per step.  Given a queue
// (WgradAux::queue), launch_wgrad records the reduction as a job instead -- the caller keeps `partial` until the flush -- and
// wgrad_queue_flush runs all of them in ONE launch (same two-level fixed-order sum per output: deterministic).  A full job table
// is flushed on the spot.
struct WgradReduceJob {
  const float* partial;
  float* dw;
  int A, Bc, T, nslots, b_total, b_off;
  unsigned first_block;
};
struct WgradReduceQueue {
  static constexpr int kMax = 80;   // (the job table travels as a kernel argument: 48 B x 80 < 4 KB)
  WgradReduceJob job[kMax];
  int n = 0;
  unsigned blocks = 0;
};
void wgrad_queue_flush(WgradReduceQueue* q, hipStream_t s);
// What a weight gradient takes from its caller besides the tensors (all optional): the queue its slot reduction joins, the words
// its max-|x| passes fill (the fp16-pipe kernels rescale g and x by powers of two), and max |g| / max |x| where the caller has
// measured them already (the input-gradient conv of the same backward)
struct WgradAux {
  WgradReduceQueue* queue = nullptr;
  AbsmaxWords* words = nullptr;
  const unsigned* gmax = nullptr;
  const unsigned* xmax = nullptr;
};
// dW[a][b][tap] = sum_{n,o} g[n][o][a] * x[n][in(o,tap)][xoff + b] in the torch layout (A, b_total, taps); see kernels_wgrad.hip.
// For a transposed conv g is the layer's input and x the output gradient: geom is then that of the strided conv from x's grid to g's.
struct WgradOp {
  const float* g = nullptr;     // (B, geom.out.vox, A): the conv's output gradient
  int A = 0;
  const float* x = nullptr;     // (B, geom.in.vox, xld): the conv's input, Bc channels at offset xoff
  int Bc = 0, xld = 0, xoff = 0;
  ConvGeom geom{};              // in = x's grid, out = g's grid, taps and strides (sh serves both phi and r)
  int batch = 0;
  bool per_sample = false;      // no sum over the batch: dw is (B, A, Bc, taps) (the attention's context gradient)
  float* partial = nullptr;     // wgrad_partial_floats floats
  float* dw = nullptr;
  int b_total = 0, b_off = 0;   // dw's b columns are a slice of a wider weight (a source of a channel concat); 0 = Bc, packed
  // x is read through silu(coef[0] x + coef[1]) + coef[2] per (sample, channel) ([B][xld][4]): only where
  // wgrad_x_norm_supported() says so (the fp16-pipe 3x3x3 kernel)
  const float* xcoef = nullptr;
  WgradAux aux;
};
void launch_wgrad(const WgradOp& op, hipStream_t s);
bool wgrad_x_norm_supported(const ConvGeom& g);

}  // namespace cd
