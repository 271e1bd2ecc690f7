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
  CD_REQUIRE(!plan->rad.map, "the theta gradient runs on the grid: not for a plan with a flat-state embedding (cd_plan_set_radial)");
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
