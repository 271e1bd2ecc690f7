// What every translation unit of the gfx950 CaloDiffusion hot-path library shares (internal; the public ABI is include/calodiff.h):
// the error plumbing, the profiler hooks, the convolution precision and the tensor extents.  Each kernel family declares its
// argument structs and launchers in a header of its own, next to its kernels (kernels_<family>.h; DESIGN.md lists them).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <string>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace cd {

// ---- error plumbing ---------------------------------------------------------------------------------
void set_error(const std::string& msg);
struct Fail {
  int code;
  std::string msg;
};
#define CD_HIP(expr)                                                                                  \
  do {                                                                                                \
    hipError_t _e = (expr);                                                                           \
    if (_e != hipSuccess)                                                                             \
      throw cd::Fail{-2, std::string(#expr) + ": " + hipGetErrorString(_e)};                          \
  } while (0)
#define CD_REQUIRE(cond, msg)                                                                         \
  do {                                                                                                \
    if (!(cond)) throw cd::Fail{-1, std::string(msg)};                                                \
  } while (0)

// ---- optional per-launch profiling with HIP events (eager mode only; bench.py's roofline leg) -----------------
namespace prof {
bool enabled();
void begin();
// writes a JSON object {"<category>": {"launches": n, "ms": total, "flops": per_launch, "bytes": per_launch}, ...}
int end(char* buf, int cap);
struct Scope {
  Scope(const char* category, hipStream_t s, double flops, double bytes);
  ~Scope();
  int idx;
  hipStream_t stream;
};
}  // namespace prof

// ---- arithmetic of the 3x3x3 / strided / transposed convolutions (process-wide; CD_CONV_PRECISION sets the initial value) ---
//   0 = f16x2 (default: two-term fp16 split, fp16 range), 1 = bf16x3 (exact three-term bf16 split, fp32 range), 2 = f32 MFMA
enum ConvPrecision { PREC_F16X2 = 0, PREC_BF16X3 = 1, PREC_F32 = 2 };
int conv_precision();
void set_conv_precision(int p);
// this thread's override of the process-wide setting (-1 = none): the bf16x3 re-run of a range fallback must not switch the
// kernels of other plans / threads / ranks of the process in mid-call
void set_conv_precision_override(int p);

// ---- channels-last tensor view ------------------------------------------------------------------------
// Internal activation layout: (B, D, H, W, C) fp32, C a multiple of 32 => every voxel is a whole number of 128-B lines.
struct Dims3 {
  int d, h, w;
  __host__ __device__ int64_t vox() const { return (int64_t)d * h * w; }
};

}  // namespace cd
