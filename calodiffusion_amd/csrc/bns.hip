// BespokeNonStationary theta training (cd_bns_theta_grad): the sampler chain from the data batch, the reference's PSNR loss and
// the gradient of that loss with respect to theta, in one call.  Reference: BespokeNonStationary.optimize_sampler /
// sampler (calodiffusion/models/sample.py:1047-1085) under torch autograd, for theta only.
//
// Launches of one call (N steps):
//   forward   N x {denoise (forward_impl), bns_step}                          every x_i and U_i kept in the workspace
//   loss      bns_loss_partial, bns_loss_final, bns_seed                       g_N
//   reverse   N x {bns_dtheta_partial, bns_dtheta_final} and, for i > 0,
//             (N-1) x {input-only denoise VJP (denoise_vjp_impl), bns_accum}   g_i = a_i g_{i+1} + VJP(b_i g_{i+1})
#include "plan_internal.h"

namespace cd {

// ------------------------------------------------------------------------------------------------------------
// The kernels.  theta (2, n_steps) device.  Every reduction runs over a grid whose size depends on the element count only, in
// fp64, partials (2 * kBnsMaxBlocks doubles) summed by one block in index order: repeated calls are bitwise equal.
// ------------------------------------------------------------------------------------------------------------
namespace {
constexpr int kBnsMaxBlocks = 1024;
constexpr int kBnsThreads = 256;
int bns_blocks(int64_t n) {
  int64_t b = (n + 4 * kBnsThreads - 1) / (4 * kBnsThreads);
  return (int)(b < 1 ? 1 : b > kBnsMaxBlocks ? kBnsMaxBlocks : b);
}
// sum of v over the block (every thread gets it); sh: kBnsThreads doubles
__device__ double bns_block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = kBnsThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}
}  // namespace

// x_next = x * a_i + u * b_i as the reference writes it (two products and a sum, each rounded on its own)
__global__ void __launch_bounds__(256) bns_step_kernel(float* __restrict__ x_next, const float* __restrict__ x,
                                                       const float* __restrict__ u, const float* __restrict__ theta, int n_steps,
                                                       int i, int64_t n) {
#pragma clang fp contract(off)
  const float a = theta[i], b = theta[n_steps + i];
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) {
    const float xa = x[k] * a;
    const float ub = u[k] * b;
    x_next[k] = xa + ub;
  }
}
static void launch_bns_step(float* x_next, const float* x, const float* u, const float* theta, int n_steps, int i, int64_t n,
                            hipStream_t s) {
  int64_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(bns_step_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x_next, x, u, theta, n_steps, i, n);
  CD_HIP(hipGetLastError());
}

// per-row maxima of data over its last axis (width w) and per-block partial sums of (data - x)^2
__global__ void __launch_bounds__(kBnsThreads) bns_loss_partial_kernel(const float* __restrict__ data, const float* __restrict__ x,
                                                                       int64_t n, int w, float* __restrict__ rowmax,
                                                                       double* __restrict__ partial) {
  __shared__ double sh[kBnsThreads];
  double acc = 0.0;
  for (int64_t k = (int64_t)blockIdx.x * kBnsThreads + threadIdx.x; k < n; k += (int64_t)gridDim.x * kBnsThreads) {
    const double d = (double)data[k] - (double)x[k];
    acc += d * d;
  }
  const int64_t rows = n / w;
  for (int64_t r = (int64_t)blockIdx.x * kBnsThreads + threadIdx.x; r < rows; r += (int64_t)gridDim.x * kBnsThreads) {
    const float* row = data + r * w;
    float m = row[0];
    for (int j = 1; j < w; ++j) m = fmaxf(m, row[j]);  // (torch.max propagates NaN; data is finite)
    rowmax[r] = m;
  }
  const double t = bns_block_sum(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}
// one block: mse, the loss (the reference's PSNR loss) and the seed coefficient scal[0] of g_N = scal[0] * (x_N - data)
__global__ void __launch_bounds__(kBnsThreads) bns_loss_final_kernel(const double* __restrict__ partial, int nparts,
                                                                     const float* __restrict__ rowmax, int64_t rows, int64_t n,
                                                                     double* __restrict__ loss_out, float* __restrict__ scal) {
  __shared__ double sh[kBnsThreads];
  __shared__ double mse_s;
  double acc = 0.0;
  for (int k = threadIdx.x; k < nparts; k += kBnsThreads) acc += partial[k];
  const double sse = bns_block_sum(acc, sh);
  if (threadIdx.x == 0) mse_s = sse / (double)n;
  __syncthreads();
  const double mse = mse_s;
  if (mse == 0.0) {  // the reference returns the int 100 (on which its torch.mean raises): loss 100, zero gradient
    if (threadIdx.x == 0) {
      *loss_out = 100.0;
      scal[0] = 0.f;
    }
    return;
  }
  const double root = sqrt(mse);
  double lsum = 0.0;
  int zero = 0;
  for (int64_t r = threadIdx.x; r < rows; r += kBnsThreads) {
    const double m = (double)rowmax[r];
    lsum += 20.0 * log10(m / root);  // NaN for m < 0, -inf for m == 0
    zero |= m == 0.0;
  }
  const double tot = bns_block_sum(lsum, sh);
  const double any_zero = bns_block_sum((double)zero, sh);
  if (threadIdx.x == 0) {
    *loss_out = tot / (double)rows;
    // d loss / d x_N = -20 / (ln 10 mse numel) (x_N - data); a zero maximum makes log10's backward 1/0 times a zero factor:
    // torch's gradient is NaN everywhere
    scal[0] = any_zero != 0.0 ? __builtin_nanf("") : (float)(-20.0 / (2.302585092994045684 * mse * (double)n));
  }
}
static void launch_bns_loss(const float* data, const float* x_n, int64_t n, int w, float* rowmax, double* partial, double* loss_out,
                            float* scal, hipStream_t s) {
  const int nb = bns_blocks(n);
  hipLaunchKernelGGL(bns_loss_partial_kernel, dim3(nb), dim3(kBnsThreads), 0, s, data, x_n, n, w, rowmax, partial);
  CD_HIP(hipGetLastError());
  hipLaunchKernelGGL(bns_loss_final_kernel, dim3(1), dim3(kBnsThreads), 0, s, partial, nb, rowmax, n / w, n, loss_out, scal);
  CD_HIP(hipGetLastError());
}

// g = scal[0] * (x_N - data)
__global__ void __launch_bounds__(256) bns_seed_kernel(float* __restrict__ g, const float* __restrict__ x_n,
                                                       const float* __restrict__ data, const float* __restrict__ scal, int64_t n) {
  const float c = scal[0];
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) g[k] = c * (x_n[k] - data[k]);
}
static void launch_bns_seed(float* g, const float* x_n, const float* data, const float* scal, int64_t n, hipStream_t s) {
  int64_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(bns_seed_kernel, dim3((unsigned)blocks), dim3(256), 0, s, g, x_n, data, scal, n);
  CD_HIP(hipGetLastError());
}

// step i of the reverse chain, g = g_{i+1} on entry: partials of <g, x_i> and <g, U_i>; with `chain`, gy = b_i g (the denoiser's
// upstream gradient) and g = a_i g (g_i once the VJP's dx is added)
__global__ void __launch_bounds__(kBnsThreads) bns_dtheta_partial_kernel(float* __restrict__ g, const float* __restrict__ x,
                                                                         const float* __restrict__ u, const float* __restrict__ theta,
                                                                         int n_steps, int i, float* __restrict__ gy, int chain,
                                                                         int64_t n, double* __restrict__ partial) {
  __shared__ double sh[kBnsThreads];
  const float a = theta[i], b = theta[n_steps + i];
  double ax = 0.0, au = 0.0;
  for (int64_t k = (int64_t)blockIdx.x * kBnsThreads + threadIdx.x; k < n; k += (int64_t)gridDim.x * kBnsThreads) {
    const float gv = g[k];
    ax += (double)gv * (double)x[k];
    au += (double)gv * (double)u[k];
    if (chain) {
      gy[k] = b * gv;
      g[k] = a * gv;
    }
  }
  const double tx = bns_block_sum(ax, sh);
  const double tu = bns_block_sum(au, sh);
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = tx;
    partial[2 * blockIdx.x + 1] = tu;
  }
}
__global__ void __launch_bounds__(kBnsThreads) bns_dtheta_final_kernel(const double* __restrict__ partial, int nparts, int n_steps,
                                                                       int i, float* __restrict__ dtheta) {
  __shared__ double sh[kBnsThreads];
  double ax = 0.0, au = 0.0;
  for (int k = threadIdx.x; k < nparts; k += kBnsThreads) {
    ax += partial[2 * k];
    au += partial[2 * k + 1];
  }
  const double tx = bns_block_sum(ax, sh);
  const double tu = bns_block_sum(au, sh);
  if (threadIdx.x == 0) {
    dtheta[i] = (float)tx;
    dtheta[n_steps + i] = (float)tu;
  }
}
static void launch_bns_dtheta(float* g, const float* x, const float* u, const float* theta, int n_steps, int i, float* gy, bool chain,
                              int64_t n, double* partial, float* dtheta, hipStream_t s) {
  const int nb = bns_blocks(n);
  hipLaunchKernelGGL(bns_dtheta_partial_kernel, dim3(nb), dim3(kBnsThreads), 0, s, g, x, u, theta, n_steps, i, gy, chain ? 1 : 0, n,
                     partial);
  CD_HIP(hipGetLastError());
  hipLaunchKernelGGL(bns_dtheta_final_kernel, dim3(1), dim3(kBnsThreads), 0, s, partial, nb, n_steps, i, dtheta);
  CD_HIP(hipGetLastError());
}

// g += dx
__global__ void __launch_bounds__(256) bns_accum_kernel(float* __restrict__ g, const float* __restrict__ dx, int64_t n) {
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) g[k] = g[k] + dx[k];
}
static void launch_bns_accum(float* g, const float* dx, int64_t n, hipStream_t s) {
  int64_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(bns_accum_kernel, dim3((unsigned)blocks), dim3(256), 0, s, g, dx, n);
  CD_HIP(hipGetLastError());
}

// The call's own blocks at the front of the workspace; the network (forward or VJP) gets the rest, reset for every use
struct BnsFront {
  float* xs = nullptr;  // x_1 .. x_N
  float* us = nullptr;  // U_0 .. U_{N-1}
  float *g = nullptr, *gy = nullptr, *dx = nullptr, *rowmax = nullptr, *scal = nullptr;
  double* partial = nullptr;
};
static size_t bns_front(CdPlan* p, int B, int N, BnsFront& f) {
  const Dims3 dims = p->shapes[0];
  const size_t n = (size_t)B * dims.vox();
  Arena& ws = p->ws;
  f.xs = ws.get<float>((size_t)N * n);
  f.us = ws.get<float>((size_t)N * n);
  f.g = ws.get<float>(n);
  f.gy = ws.get<float>(n);
  f.dx = ws.get<float>(n);
  f.rowmax = ws.get<float>(n / dims.w);
  f.scal = ws.get<float>(64);
  f.partial = ws.get<double>(2 * (size_t)kBnsMaxBlocks);
  return ws.high();
}

static void bns_check(CdPlan* plan, int batch, int n_steps) {
  CD_REQUIRE(plan && batch > 0 && n_steps >= 1 && n_steps <= 4096, "bad argument (n_steps 1..4096)");
  CD_REQUIRE(!plan->desc.time_sin && !plan->desc.cond_sin, "the theta gradient needs the Linear time/cond embeddings");
  CD_REQUIRE(!plan->flat(), "the theta gradient runs on the grid: not for a plan with a flat-state embedding (cd_plan_set_radial / cd_plan_set_geom)");
}

}  // namespace cd

extern "C" {

int cd_plan_bns_workspace_bytes(CdPlan* plan, int batch, int n_steps, size_t* bytes) {
  return guarded([&] {
    bns_check(plan, batch, n_steps);
    CD_REQUIRE(bytes, "bad argument");
    dgrad_images(plan);
    BnsFront f;
    plan->ws.reset(nullptr, 0, true);
    const size_t front = bns_front(plan, batch, n_steps, f);
    const size_t fwd = dry_forward_bytes(plan, batch, [] {});
    plan->ws.reset(nullptr, 0, true);
    denoise_vjp_impl(plan, batch, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, false, nullptr);
    const size_t vjp = plan->ws.high();
    *bytes = front + (fwd > vjp ? fwd : vjp) + 8192;
  });
}

int cd_bns_theta_grad(CdPlan* plan, int batch, int n_steps, const float* data, const float* cond, const float* theta,
                      const float* sigma, double* loss_out, float* dtheta, void* workspace, size_t workspace_bytes, void* stream) {
  return guarded([&] {
    bns_check(plan, batch, n_steps);
    CD_REQUIRE(data && cond && theta && sigma && loss_out && dtheta && workspace, "bad argument");
    check_ready(plan, true);
    dgrad_images(plan);
    hipStream_t s = (hipStream_t)stream;
    const int N = n_steps, B = batch;
    const int64_t n = (int64_t)B * plan->shapes[0].vox();
    plan->ws.reset((char*)workspace, workspace_bytes, false);
    BnsFront f;
    const size_t used = bns_front(plan, B, N, f);
    CD_REQUIRE(used <= workspace_bytes, "workspace too small: call cd_plan_bns_workspace_bytes");
    char* sub = (char*)workspace + used;
    const size_t sub_bytes = workspace_bytes - used;
    auto x_at = [&](int i) -> const float* { return i == 0 ? data : f.xs + (size_t)(i - 1) * n; };
    auto u_at = [&](int i) { return f.us + (size_t)i * n; };

    // forward: x_0 = data, U_i = denoise(x_i, sigma_i), x_{i+1} = x_i a_i + U_i b_i
    for (int i = 0; i < N; ++i) {
      plan->ws.reset(sub, sub_bytes, false);
      forward_impl(plan, B, x_at(i), cond, sigma + (size_t)i * B, u_at(i), false, s);
      launch_bns_step(f.xs + (size_t)i * n, x_at(i), u_at(i), theta, N, i, n, s);
    }
    // loss and the seed g_N
    const float* x_n = f.xs + (size_t)(N - 1) * n;
    launch_bns_loss(data, x_n, n, plan->shapes[0].w, f.rowmax, f.partial, loss_out, f.scal, s);
    launch_bns_seed(f.g, x_n, data, f.scal, n, s);
    // reverse chain
    for (int i = N - 1; i >= 0; --i) {
      const bool chain = i > 0;  // (x_0 = data needs no gradient)
      launch_bns_dtheta(f.g, x_at(i), u_at(i), theta, N, i, f.gy, chain, n, f.partial, dtheta, s);
      if (!chain) break;
      plan->ws.reset(sub, sub_bytes, false);
      denoise_vjp_impl(plan, B, x_at(i), sigma + (size_t)i * B, cond, f.gy, f.dx, nullptr, false, s);
      launch_bns_accum(f.g, f.dx, n, s);
    }
  });
}

}  // extern "C"
