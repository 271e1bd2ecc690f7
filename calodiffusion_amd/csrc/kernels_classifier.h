// Launchers of the classifier two-sample test's kernels (kernels_classifier.hip), called by classifier.hip (internal; the public
// ABI is include/calodiff.h, "classifier two-sample test").
#pragma once
#include "cd_common.h"

namespace cd {

// The dropout decision of element (row-in-batch, column) of layer `layer` at step `step`: threshold = 0 keeps everything.
struct ClsDropout {
  uint64_t seed = 0, step = 0;
  int layer = 0;
  uint32_t threshold = 0;  // an element is dropped when its Philox word is below it: floor(p 2^32)
  float scale = 1.f;       // 1 / (1 - p) of the kept ones
};
ClsDropout cls_dropout(float p, uint64_t seed, uint64_t step, int layer);

// y (rows, n_out) = act(x (rows, n_in) . w (n_out, n_in)^T + bias), act = LeakyReLU(slope) then dropout, where `act` != 0
void launch_cls_linear(const float* x, const float* w, const float* bias, float* y, int rows, int n_in, int n_out, int act, float slope,
                       const ClsDropout& drop, hipStream_t s);
// g = dy * act'(y) * mask (rows, n_out) into `g`, db [n_out] = its column sums.  dy == nullptr: dy[r][c] = dz[r] * w_next[c] (the layer
// before the output layer), and dw_next [n_out] = sum_r dz[r] y[r][c].  mask: bytes (rows, n_out) or nullptr (then `drop` decides).
void launch_cls_gate(const float* dy, const float* dz, const float* w_next, float* dw_next, const float* y, const uint8_t* mask, int act,
                     float slope, const ClsDropout& drop, float* g, float* db, int rows, int n_out, hipStream_t s);
// dx (rows, n_in) = g . w
void launch_cls_dgrad(const float* g, const float* w, float* dx, int rows, int n_in, int n_out, hipStream_t s);
// dw (n_out, n_in) = g^T . x
void launch_cls_wgrad(const float* g, const float* x, float* dw, int rows, int n_in, int n_out, hipStream_t s);
// z [rows] = h (rows, n) . w [n] + b[0]
void launch_cls_rowdot(const float* h, const float* w, const float* b, float* z, int rows, int n, hipStream_t s);
// xb (count, d) = x[idx], yb [count] = labels[idx] (labels nullable); an index outside [0, rows_total) gives a row of NaN
void launch_cls_gather(const float* x, const float* labels, int64_t rows_total, const int32_t* idx, int count, int d, float* xb, float* yb,
                       hipStream_t s);
// BCE with logits over rows <= 256: *loss (fp64) = mean, dz[r] = (sigmoid(z) - y) / rows, *db_out = sum_r dz[r]
void launch_cls_loss(const float* z, const float* y, int rows, double* loss, float* dz, float* db_out, hipStream_t s);
// mask (rows, n) bytes: 1 = kept
void launch_cls_mask(const ClsDropout& drop, int rows, int n, uint8_t* mask, hipStream_t s);

}  // namespace cd
