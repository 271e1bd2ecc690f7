// Internal interface of the host units that walk the network (plan.hip, forward.hip, conv_backward.hip, sampler.hip, train.hip,
// ops.hip, bns.hip): the plan and its weight records, the launch-sequence pieces more than one unit calls, and the dry-run and
// range-fallback wrappers around them.  The workspace allocator is arena.h, the entry points' wrapper guarded.h; the units that
// never see a plan include those alone.  The public ABI is include/calodiff.h.
#pragma once
#include "arena.h"
#include "guarded.h"
#include "kernels_bwd.h"
#include "kernels_conv.h"
#include "kernels_embed_head.h"
#include "kernels_geom.h"
#include "kernels_gn.h"
#include "kernels_sampler.h"
#include "kernels_wgrad.h"
#include "kernels_widen.h"

#include <map>
#include <string>
#include <vector>

namespace cd {

// ------------------------------------------------------------------------------------------------------------
// weight registry
// ------------------------------------------------------------------------------------------------------------
enum PackKind { PK_NONE = 0, PK_CONV = 1, PK_CONVT = 2, PK_INIT = 3 };
struct WeightEntry {
  std::string name;
  int64_t numel = 0;    // as the kernels see it (wide, in a plan with narrow levels)
  int64_t src_numel = 0;  // as the caller gives it and receives its gradient (the config's own shape)
  size_t raw_off = 0;   // floats into the arena
  PackKind pack = PK_NONE;
  int cin = 0, cout = 0, taps = 0;
  size_t pk_off = 0;
  size_t pk3_off = 0;  // split-bf16 image of 3x3x3 convs (floats into the arena; 0 = none)
  size_t grad_off = 0; // floats into the flat gradient buffer of cd_train_step
  // narrow widths (kernels_widen.h): the tensor's map (pointers unset) and its slot in the step's wide gradient block
  bool widened = false;
  WidenJob widen{};
  size_t wide_grad_off = 0;
  bool set = false;
  // input-gradient images of the training step (dgrad_images below), floats into the step's image block; dg_mode 0 = none
  int dg_mode = 0;
  size_t dg_pk_off = 0, dg_pk3_off = 0;
  bool dg_1x1 = false;  // a 1x1 conv kept raw for the forward (attention to_out: folded per sample) whose backward wants the image
};
// packed images a convolution's input gradient reads (conv_backward / conv_transpose_backward); null members: pack on the fly
struct DgImg {
  const float* pk = nullptr;
  const void* pk3 = nullptr;
};

struct ResW {
  int cin = 0, cout = 0;
  bool has_mlp = false, has_res = false;
  int c1w = -1, c1b = -1, n1g = -1, n1b = -1, c2w = -1, c2b = -1, n2g = -1, n2b = -1, mw = -1, mb = -1, rw = -1, rb = -1;
  int emb_off = 0;
};
struct AttnW {
  int c = 0;
  int ng = -1, nb = -1, qkv = -1, ow = -1, ob = -1, gg = -1, gb = -1;
};
struct LevelW {
  ResW r1, r2;
  AttnW attn;
  int sw = -1, sb = -1;  // down / up sampling conv
};

// A sampler entry point's cached step graph (cd_ddim_sample, cd_sampler_run: one each), valid while the call's key matches the
// one it was captured under
struct StepGraph {
  struct Key {
    int batch = 0, n_coef = 0, n_bufs = 0, noisy = 0; const void* ws = nullptr; const void* cond = nullptr; const void* x = nullptr;
    const void* xs = nullptr; const void* x0s = nullptr; uint64_t ops_hash = 0;
    int precision = 0;  // the captured kernels are those of the convolution precision in force at capture time
    bool operator==(const Key& o) const {
      return precision == o.precision && batch == o.batch && n_coef == o.n_coef && n_bufs == o.n_bufs && noisy == o.noisy && ws == o.ws &&
             cond == o.cond && x == o.x && xs == o.xs && x0s == o.x0s && ops_hash == o.ops_hash;
    }
  } key;
  hipGraphExec_t exec = nullptr;
  hipGraphExec_t chunk = nullptr;  // several consecutive steps as ONE graph (same key): no gap between their launches
  bool valid_for(const Key& k) const { return exec && key == k; }
  void destroy() {
    if (exec) {
      hipGraphExecDestroy(exec);
      exec = nullptr;
    }
    if (chunk) {
      hipGraphExecDestroy(chunk);
      chunk = nullptr;
    }
  }
};

}  // namespace cd

using namespace cd;

struct CdPlan {
  CdUnetDesc desc{};  // layer_sizes: the widths the kernels run (cfg_sizes widened by the width rule)
  int cfg_sizes[CD_MAX_SIZES] = {};  // LAYER_SIZE_UNET as the config states it
  int nres = 0;
  std::vector<Dims3> shapes;           // per level
  std::vector<int> up_kz;              // per up step (i = 0 .. nres-2)
  std::vector<Dims3> up_out;           // expected output dims of each up step
  std::vector<WeightEntry> weights;
  std::map<std::string, int> index;
  float* arena = nullptr;
  size_t arena_floats = 0;

  int init_w = -1, init_b = -1, head_w = -1, head_b = -1;
  int tw[3] = {-1, -1, -1}, tb[3] = {-1, -1, -1}, cw[3] = {-1, -1, -1}, cb[3] = {-1, -1, -1};
  std::vector<LevelW> downs, ups;
  ResW mid1, mid2, fin;
  AttnW mid_attn;
  int emb_ld = 0;
  EmbedLayer* d_embed_layers = nullptr;
  int n_embed_layers = 0;
  std::vector<std::pair<int, int>> embed_list;  // (weight idx of mlp w, emb offset) in ResW order

  float* d_coords = nullptr;  // r[W], z[D], phi[H]
  float* d_init_table = nullptr;  // (vox, C0): coordinate-channel part + bias of the init conv (refresh_init_table)
  bool coords_set = false;
  // init conv + downs[0].r1's first conv as one launch (kernels_init_pair.hip): the composed weights and the table conv1(d_init_table)
  // + b1, rebuilt with d_init_table and whenever that conv's weight or bias is set (refresh_init_pair).  Null where the geometry or
  // the widths rule the form out; init_pair_ready once all four tensors have been set.
  void* d_pair_w = nullptr;
  float* d_pair_table = nullptr;
  bool init_pair_ready = false;

  // sampler state (device): step table, counter, stepvals
  static constexpr int kMaxSteps = 4096;
  static constexpr int kEmbedChunk = 16;  // sampler steps whose embeddings one launch computes ahead (cd_ddim_sample)
  float* d_table = nullptr;
  int* d_counter = nullptr;
  float* d_stepvals = nullptr;
  // device word the f16x2 kernels of the current call OR their range flag into: d_counter + 2 (the sticky word cd_plan_status
  // reports) or, inside an entry point with its own bf16x3 fallback, d_counter + 3 (that call's private word)
  int* status_word = nullptr;

  // the samplers' step graphs are captured on a private stream (the caller's may be the legacy null stream, which cannot capture)
  hipStream_t cap_stream = nullptr;
  // job list of cd_plan_set_weights: host copy (with the callers' pointers of the last call) and device copy
  std::vector<PackJob> pack_jobs;
  PackJob* d_pack_jobs = nullptr;
  // training: the re-packed (channel-transposed, tap-flipped) weight images of every convolution's input gradient, made by ONE
  // job list per step (two launches) instead of two or three pack launches inside each conv_backward (118 launches per step).
  // The images live in a block of the step's workspace (dg_floats, at dg_images during a step); the device job list points into
  // the block at dg_jobs_at and is re-pointed when a step's block lies elsewhere (dg_jobs: host copy)
  size_t dg_floats = 0;
  std::vector<PackJob> dg_jobs;
  PackJob* d_dg_jobs = nullptr;
  const float* dg_jobs_at = nullptr;
  const float* dg_images = nullptr;
  DgImg dg(int i) const {
    DgImg g;
    const WeightEntry& w = weights[i];
    if (dg_images && w.dg_mode) {
      g.pk = dg_images + w.dg_pk_off;
      if (w.dg_mode != 1) g.pk3 = dg_images + w.dg_pk3_off;
    }
    return g;
  }
  // barrier words of the co-operative attention (launch_attn_small, CD_ATTN_COOP): [kAttnCoopSamples][2]
  unsigned* d_attn_sync = nullptr;
  // the samplers' cached step graphs: cd_ddim_sample's (with a chunk graph of kEmbedChunk steps) and that of a uniform sampler
  // program (cd_sampler_run; one-step graph only)
  StepGraph ddim_graph, prog_graph;

  // training: flat gradient layout and the device job list of the small Linear weight gradients
  size_t grad_floats = 0;
  std::vector<LinearWgradJob> lin_jobs_host;
  LinearWgradJob* d_lin_jobs = nullptr;

  // flat-state embedding: enc before and dec after the U-Net, in one of two kinds -- Dataset 1's radial matrices
  // (cd_plan_set_radial: the caller's map and its live matrices) or HGCal's packed maps (cd_plan_set_geom); neither = none.  With
  // one, the state of every denoise-based entry point is the flat shower and the gradients of the two maps follow the U-Net's
  // in the flat gradient buffer.  forward.hip and train.hip reach it through launch_embed_* below only.
  struct FlatEmbed {
    const CdRadialMap* map = nullptr;
    const float* enc_w = nullptr;
    const float* dec_w = nullptr;
    const CdGeomMap* genc = nullptr;
    const CdGeomMap* gdec = nullptr;
    bool want_grads = true;
    int64_t state() const { return map ? (int64_t)map->V : (int64_t)genc->layers * genc->cols; }
    // floats of one gradient slot (enc's and dec's are equal); a frozen pair of HGCal maps has none
    size_t grad_floats() const {
      const size_t n = map ? (size_t)map->wtotal : (want_grads ? (size_t)genc->layers * genc->rows * genc->cols : 0);
      return (n + 63) & ~(size_t)63;
    }
  } fe;
  const FlatEmbed* flat() const { return (fe.map || fe.genc) ? &fe : nullptr; }
  int64_t state_per() const { return flat() ? fe.state() : shapes[0].vox(); }
  size_t embed_grad_floats() const { return flat() ? fe.grad_floats() : 0; }
  size_t enc_grad_off() const { return grad_floats; }
  size_t dec_grad_off() const { return grad_floats + embed_grad_floats(); }

  // narrow widths: any level runs widened; the job lists of the widening stage (cd_plan_set_weights; host copy with the callers'
  // pointers of the last call) and of the gradient fold (pointed at the step's wide block and the caller's buffer), and the
  // floats of that wide block
  bool widened = false;
  std::vector<WidenJob> expand_jobs, fold_jobs;
  WidenJob *d_expand_jobs = nullptr, *d_fold_jobs = nullptr;
  size_t wide_grad_floats = 0;

  Arena ws;

  const float* raw(int i) const { return arena + weights[i].raw_off; }
  const float* packed(int i) const { return arena + weights[i].pk_off; }
  const void* packed3(int i) const { return weights[i].pk3_off ? (const void*)(arena + weights[i].pk3_off) : nullptr; }
};

namespace cd {

// ------------------------------------------------------------------------------------------------------------
// launch sequences
// ------------------------------------------------------------------------------------------------------------
struct Run {
  Arena* ws;
  hipStream_t s;
  int B;
  int groups;
  int* status = nullptr;  // device word for sticky range flags (cd_plan_status), or null
  GnParamQueue* gq = nullptr;  // training step: the GroupNorm layers' parameter-gradient reductions, flushed once at the end
  // training step: the weight gradients' slot reductions, flushed once at the end (null: each runs where it arises), and the
  // workspace blocks of their partials, held until that flush
  WgradReduceQueue* wq = nullptr;
  std::vector<float*> wq_held;
  AbsmaxWords amax;  // zeroed words for max |x| (launch_absmax_bits, launch_gn_backward); none in a dry run
  // backward passes: false = input gradients only (cd_denoise_vjp without grads): no weight / bias / GroupNorm-parameter work
  bool param_grads = true;
  bool dry() const { return ws->dry(); }
  unsigned* amax_word() { return dry() ? nullptr : amax.take(); }
  // partial buffer of one launch_wgrad; with a queue it stays taken until the flush, so one buffer per queued reduction
  float* wgrad_part(size_t floats) {
    float* part = ws->get<float>(floats);
    if (wq) wq_held.push_back(part);
    return part;
  }
  void release_wgrad_part(float* part) {
    if (!wq) ws->release(part);
  }
  WgradAux wgrad_aux(const unsigned* gmax = nullptr, const unsigned* xmax = nullptr) {
    WgradAux a;
    a.queue = wq; a.words = &amax; a.gmax = gmax; a.xmax = xmax;
    return a;
  }
};

// weights of one block resolved to device pointers (conv weights in packed MFMA layout)
struct ResP {
  int cin = 0, cout = 0;
  bool has_res = false;
  const float *c1w = nullptr, *c1b = nullptr, *n1g = nullptr, *n1b = nullptr;
  const void *c1w3 = nullptr, *c2w3 = nullptr;  // split-bf16 images of the two 3x3x3 convs
  const float *c2w = nullptr, *c2b = nullptr, *n2g = nullptr, *n2b = nullptr;
  const float *rw = nullptr, *rb = nullptr;
  const void* rw16 = nullptr;  // f16x2 image of the 1x1 shortcut conv
  const float* emb = nullptr;  // (B, emb_ld) slice for this block, or null
  int emb_ld = 0;
};
struct AttnP {
  int c = 0;
  const float *ng = nullptr, *nb = nullptr, *qkv = nullptr, *ow = nullptr, *ob = nullptr, *gg = nullptr, *gb = nullptr;
  const void* qkv16 = nullptr;  // f16x2 image of to_qkv (fused attention kernels)
  unsigned* coop_sync = nullptr;  // the plan's barrier words of the co-operative form (launch_attn_small), or null
};

ResP resolve(const CdPlan* p, const ResW& w, const float* emb);
AttnP resolve(const CdPlan* p, const AttnW& w);

// Options of the sampler loop (cd_ddim_sample): embeddings / scalings already in place (computed a chunk of steps ahead), and the
// sampler's update of the running sample fused into the head kernel.
struct FwdOpts {
  float* emb_pre = nullptr;   // (B, emb_ld) ready-made: no embedding launch
  float* scal_pre = nullptr;  // (B, 4)
  const HeadArgs* upd = nullptr;  // only the upd_* fields are read
};

// forward.hip
struct LazyClose;
float* stats_pass(Run& r, const float* x, int C, int64_t vox, int* units);
float* conv3_with_stats(Run& r, const float* x0, int c0, const float* x1, int c1, const float* wpk, const void* wpk3,
                        const float* bias, float* out, int cout, Dims3 dims, const float* coef_in, int* units,
                        const GnDefer* defer_in = nullptr, float* coef_buf = nullptr, const ConvFusion::GnOut* gn_out = nullptr);
// the first conv of a block already computed whole by another launch (the composed init pair): its output and channel partials,
// both workspace blocks res_block takes over
struct ConvDone {
  float* h1 = nullptr;
  float* part = nullptr;
  int units = 0;
};
float* res_block(Run& r, const ResP& w, const float* x0, int c0, const float* x1, int c1, Dims3 dims,
                 float** part_out = nullptr, int* units_out = nullptr, LazyClose* lazy = nullptr, float* h1_side = nullptr,
                 const ConvDone* h1_done = nullptr);
float* attn_block(Run& r, const AttnP& w, const float* x, Dims3 dims, float* xpart = nullptr, int xunits = 0);
// conv_backward.hip
void bias_grad(Run& r, const float* dy, int C, int64_t vox, float* db);
void conv_backward(Run& r, const float* x0, int c0, const float* x1, int c1, const float* w_raw, const float* dy, float* dx,
                   float* dw, float* db, int cout, const ConvGeom& g, const DgImg* img = nullptr, const float* xcoef = nullptr,
                   const float* dx_add = nullptr, int* dx_added = nullptr, const unsigned* dy_max = nullptr);
void conv_transpose_backward(Run& r, const float* x, const float* w_raw, const float* dy, float* dx, float* dw, float* db, int c,
                             Dims3 din, Dims3 dout, int kz, int sz, const DgImg* img = nullptr);
// forward.hip
EmbedArgs embed_args(CdPlan* p, int B, const float* cond, const float* t, int kind, float* emb, float* scal);
void forward_impl(CdPlan* p, int B, const float* x, const float* cond, const float* t, float* out, bool raw, hipStream_t s,
                  const FwdOpts* opt = nullptr);
// The one interface to a plan's flat-state embedding that forward.hip and train.hip call (the launches per kind: kernels_geom.h).
// g (B, grid) = enc(c_in x)
inline void launch_embed_in(const CdPlan::FlatEmbed& e, const float* x, const float* scal, float* g, int batch, hipStream_t s) {
  if (e.map) radial_embed_in(e.map, e.enc_w, x, scal, g, batch, s);
  else geom_embed_in(e.genc, x, scal, g, batch, s);
}
// out (B, V) = the objective's combination of x and dec(F), as launch_head forms it on the grid; upd: its fused sampler update
inline void launch_embed_out(const CdPlan::FlatEmbed& e, const float* F, const float* x, const float* scal, int objective, float* out,
                             const HeadArgs* upd, int batch, hipStream_t s) {
  if (e.map) radial_embed_out(e.map, e.dec_w, F, x, scal, objective, out, upd, batch, s);
  else geom_embed_out(e.gdec, F, x, scal, objective, out, upd, batch, s);
}
// dF = dec's VJP of gf, and dd (nullable) = the gradient of dec's map
inline void launch_embed_dec_vjp(const CdPlan::FlatEmbed& e, const float* F, const float* gf, float* dF, float* dd, int batch,
                                 hipStream_t s) {
  if (e.map) radial_embed_dec_vjp(e.map, e.dec_w, F, gf, dF, dd, batch, s);
  else geom_embed_dec_vjp(e.gdec, F, gf, dF, dd, batch, s);
}
// dx = enc's VJP of dg (which carries c_in) plus, with gy, the preconditioning's direct x term; dw (nullable) = the gradient of
// enc's map
inline void launch_embed_enc_vjp(const CdPlan::FlatEmbed& e, const float* x, const float* dg, const float* gy, const float* scal,
                                 int objective, float* dx, float* dw, int batch, hipStream_t s) {
  if (e.map) radial_embed_enc_vjp(e.map, e.enc_w, x, dg, gy, scal, objective, dx, dw, batch, s);
  else geom_embed_enc_vjp(e.genc, x, dg, gy, scal, objective, dx, dw, batch, s);
}
// plan.hip
void check_ready(CdPlan* p, bool need_coords);
// train.hip
void dgrad_images(CdPlan* p);  // lays out the input-gradient weight images once per plan (before any backward pass)
void denoise_vjp_impl(CdPlan* p, int B, const float* x, const float* sigma, const float* cond, const float* gy, float* dx, float* grads,
                      bool param_grads, hipStream_t s);

// High-water mark of a dry run of the forward's allocation sequence (after `front`, the caller's own blocks).  The sequence
// depends on the convolution precision (whole-block launches, fused / unfused attention), and a range fallback re-runs a call
// in bf16x3 on the SAME workspace: the answer is the larger of the precision in force and the fallback's.
template <typename F>
size_t dry_forward_bytes(CdPlan* plan, int batch, F&& front) {
  struct Restore {
    ~Restore() { set_conv_precision_override(-1); }
  } restore;
  size_t need = 0;
  // (all three arithmetic modes, not only the one in force and the fallback's: cd_set_conv_precision may switch after the caller
  // sized -- and cached -- its workspace)
  for (int mode : {(int)PREC_F16X2, (int)PREC_BF16X3, (int)PREC_F32}) {
    set_conv_precision_override(mode);
    plan->ws.reset(nullptr, 0, true);
    front();
    forward_impl(plan, batch, nullptr, nullptr, nullptr, nullptr, false, nullptr);
    need = plan->ws.high() > need ? plan->ws.high() : need;
  }
  return need;
}

// Range fallback of the entry points that promise finite results (the samplers, cd_denoise_safe): `run(eager)` enqueues the
// whole call.  The f16x2 kernels of THIS call raise bit 0 of a private word (d_counter + 3, cleared first), so a flag left in
// the sticky word by an earlier, un-queried cd_denoise / cd_unet_forward / cd_train_step is neither mistaken for this call's
// overflow nor lost.  If the call left the fp16 range it is run again with the exact bf16x3 convolutions (full fp32 range;
// eagerly, a cached step graph holds the f16x2 kernels) -- the precision is overridden for THIS THREAD only, other plans /
// threads of the process keep their kernels -- and bit 1 is OR-ed into the sticky word.  Returns whether the fallback ran.
template <typename F>
bool run_with_range_fallback(CdPlan* plan, hipStream_t s, F&& run, bool report_sticky = true) {
  struct Restore {
    CdPlan* p;
    ~Restore() {
      p->status_word = p->d_counter + 2;
      set_conv_precision_override(-1);
    }
  } restore{plan};
  plan->status_word = plan->d_counter + 3;
  CD_HIP(hipMemsetAsync(plan->d_counter + 3, 0, sizeof(int), s));
  run(false);
  if (conv_precision() != PREC_F16X2) return false;
  int flags = 0;
  CD_HIP(hipMemcpyAsync(&flags, plan->d_counter + 3, sizeof(int), hipMemcpyDeviceToHost, s));
  CD_HIP(hipStreamSynchronize(s));
  if (!(flags & 1)) return false;
  set_conv_precision_override(PREC_BF16X3);
  run(true);
  if (report_sticky) launch_or_word(plan->d_counter + 2, 2, s);
  return true;
}

}  // namespace cd
