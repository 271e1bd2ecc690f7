// The rungs of the weight-gradient ladder (internal; launch_wgrad in kernels_wgrad.hip is their only caller).  A rung launches its
// kernel for `op` and reports in *nslots how many partial slots it left in op.partial, or returns false without a launch when the
// shape is not its own.  The ladder then runs the slot reduction.
//   kernels_wgrad16.hip   fp16 matrix pipe: stride-1 3x3x3 (ring / unit kernels) and the strided (KD,4,4) conv
//   kernels_wgrad.hip     fp32: flat 3x3x3, streaming 1x1x1 (and, not a rung that can decline, the generic wgrad_kernel)
#pragma once
#include "kernels_wgrad.h"

namespace cd {

// chunks per sample of the generic kernel = the slots per sample a caller's `partial` holds (wgrad_partial_floats)
int wgrad_chunks(int64_t out_vox, int batch, bool per_sample, int A, int Bc, int T);

bool wgrad_f16x2_eligible(Dims3 d);  // the stride-1 3x3x3 fp16 kernels take this grid
bool try_launch_wgrad_f16x2(const WgradOp& op, int* nslots, hipStream_t s);
bool try_launch_wgrad_flat(const WgradOp& op, int* nslots, hipStream_t s);
bool try_launch_wgrad_strided_f16x2(const WgradOp& op, int* nslots, hipStream_t s);
bool try_launch_wgrad1x1(const WgradOp& op, int* nslots, hipStream_t s);

}  // namespace cd
