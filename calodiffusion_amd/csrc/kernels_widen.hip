// Narrow U-Net widths: the widening of a plan's tensors at weight sync and the fold of their gradients (kernels_widen.h).
// Both run once per weight sync / training step over a few hundred thousand floats; neither is on the denoise path.
#include "kernels_widen.h"

namespace cd {

namespace {

// wide channel -> (real channel, copy number) on an axis of `cpg` real channels per group in `k` copies
__device__ __forceinline__ int widen_real(int j, int cpg, int k, int* copy) {
  const int span = k * cpg, g = j / span, w = j % span;
  *copy = w / cpg;
  return g * cpg + w % cpg;
}
// real channel -> its wide channel of copy number `copy`
__device__ __forceinline__ int widen_wide(int c, int cpg, int k, int copy) {
  return (c / cpg) * k * cpg + copy * cpg + c % cpg;
}

__device__ __forceinline__ void widen_expand_job(const WidenJob& j, size_t t0, size_t stride) {
  const int in_w = j.in_w[0] + j.in_w[1];
  const int in_n0 = j.in_w[0] / j.in_k[0], in_n = in_n0 + j.in_w[1] / j.in_k[1];
  const int out_n = j.out_w / j.out_k;
  for (size_t i = t0; i < j.n_wide; i += stride) {
    const int tap = (int)(i % j.taps);
    const size_t r = i / j.taps;
    const int ow = j.in_first ? (int)(r % j.out_w) : (int)(r / in_w);
    const int iw = j.in_first ? (int)(r / j.out_w) : (int)(r % in_w);
    int oc, ic;
    const int ro = widen_real(ow, j.out_cpg, j.out_k, &oc);
    const int seg = iw >= j.in_w[0] ? 1 : 0;
    const int ri = (seg ? in_n0 : 0) + widen_real(iw - (seg ? j.in_w[0] : 0), j.in_cpg[seg], j.in_k[seg], &ic);
    const size_t src = j.in_first ? ((size_t)ri * out_n + ro) * j.taps + tap : ((size_t)ro * in_n + ri) * j.taps + tap;
    j.wide[i] = ic == 0 ? j.narrow[src] : 0.f;
  }
}

__global__ void __launch_bounds__(256) widen_expand_kernel(const WidenJob* __restrict__ jobs) {
  const WidenJob j = jobs[blockIdx.y];
  widen_expand_job(j, blockIdx.x * (size_t)256 + threadIdx.x, gridDim.x * (size_t)256);
}
__global__ void __launch_bounds__(256) widen_expand_one_kernel(const WidenJob j) {
  widen_expand_job(j, blockIdx.x * (size_t)256 + threadIdx.x, gridDim.x * (size_t)256);
}

// The transpose of the expansion.  The copies are summed in ascending order by one thread: the same bits on every call.
__global__ void __launch_bounds__(256) widen_fold_kernel(const WidenJob* __restrict__ jobs) {
  const WidenJob j = jobs[blockIdx.y];
  const int in_w = j.in_w[0] + j.in_w[1];
  const int in_n0 = j.in_w[0] / j.in_k[0], in_n = in_n0 + j.in_w[1] / j.in_k[1];
  const int out_n = j.out_w / j.out_k;
  const size_t stride = gridDim.x * (size_t)256;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < j.n_narrow; i += stride) {
    const int tap = (int)(i % j.taps);
    const size_t r = i / j.taps;
    const int ro = j.in_first ? (int)(r % out_n) : (int)(r / in_n);
    const int ri = j.in_first ? (int)(r / out_n) : (int)(r % in_n);
    const int seg = ri >= in_n0 ? 1 : 0;
    const int iw = (seg ? j.in_w[0] : 0) + widen_wide(ri - (seg ? in_n0 : 0), j.in_cpg[seg], j.in_k[seg], 0);
    float acc = 0.f;
    for (int c = 0; c < j.out_k; ++c) {
      const int ow = widen_wide(ro, j.out_cpg, j.out_k, c);
      acc += j.wide[j.in_first ? ((size_t)iw * j.out_w + ow) * j.taps + tap : ((size_t)ow * in_w + iw) * j.taps + tap];
    }
    j.narrow[i] = acc;
  }
}

}  // namespace

void launch_widen_expand(const WidenJob* d_jobs, int njobs, hipStream_t s) {
  if (njobs <= 0) return;
  hipLaunchKernelGGL(widen_expand_kernel, dim3(48, (unsigned)njobs), dim3(256), 0, s, d_jobs);
  CD_HIP(hipGetLastError());
}
void launch_widen_expand_one(const WidenJob& job, hipStream_t s) {
  const unsigned blocks = (unsigned)((job.n_wide + 255) / 256);
  hipLaunchKernelGGL(widen_expand_one_kernel, dim3(blocks < 256 ? (blocks ? blocks : 1) : 256), dim3(256), 0, s, job);
  CD_HIP(hipGetLastError());
}
void launch_widen_fold(const WidenJob* d_jobs, int njobs, hipStream_t s) {
  if (njobs <= 0) return;
  hipLaunchKernelGGL(widen_fold_kernel, dim3(32, (unsigned)njobs), dim3(256), 0, s, d_jobs);
  CD_HIP(hipGetLastError());
}

}  // namespace cd
