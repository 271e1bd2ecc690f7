// Narrow U-Net widths (kernels_widen.hip): a config width C that the MFMA kernels cannot run is widened at the plan boundary to
// Cw = C k (k = 2 or 4) by duplicating channels inside each GroupNorm group, which leaves every group's mean and variance as they
// were.  With cpg = C / groups, wide channel j lies in group g = j / (k cpg) at w = j % (k cpg): it holds real channel
// g cpg + w % cpg and is copy number w / cpg (copy 0: the primary).  The map depends on C and the group count only.
//   expand (weight sync): along an output axis every copy carries the real channel's values; along an input axis the primary
//                         carries the real column and the other copies are zero
//   fold (gradients):     the exact transpose -- the sum over the copies of an output axis, the primary column of an input axis
#pragma once
#include "cd_common.h"

namespace cd {

// One tensor [out][in][taps] (in_first: [in][out][taps], the transposed conv) in its config shape (narrow) and its wide shape.
// The input axis is up to two segments, each with its own map (the concatenated inputs of the up path).  An axis that is not a
// widened U-Net width has k = 1 and cpg = its extent: the identity.
struct WidenJob {
  float* narrow;       // expand: the caller's tensor (read); fold: the caller's gradient slot (written)
  float* wide;         // expand: the plan's raw copy (written); fold: the wide gradient (read)
  int out_w, out_cpg, out_k;        // wide extent of the output axis, real channels per group, copies
  int in_w[2], in_cpg[2], in_k[2];  // the same per input segment; in_w[1] = 0: one segment
  int taps, in_first;
  unsigned long long n_wide, n_narrow;
};

void launch_widen_expand(const WidenJob* d_jobs, int njobs, hipStream_t s);  // every job's wide tensor from its narrow one
void launch_widen_expand_one(const WidenJob& job, hipStream_t s);             // one job, passed by value
void launch_widen_fold(const WidenJob* d_jobs, int njobs, hipStream_t s);    // every job's narrow gradient from its wide one

}  // namespace cd
