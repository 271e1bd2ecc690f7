// Training step and the denoise VJP (cd_train_step, cd_train_step_target, cd_denoise_vjp): forward with a tape of saved activations, then the
// backward pass.  Reference: TrainDiffusion.training_loop body (train/train_diffusion.py:52-63) =
// Diffusion.compute_loss -> hybrid_weight.loss_function (loss.py:163-179) -> denoise -> CondUnet.forward, then
// loss.backward().  torch autograd is replaced by the explicit chain below; gradients land in a flat buffer in the plan's
// weight order (cd_plan_grad_layout) and are exposed to torch.optim through calodiffusion_amd.engine.
//
// Nothing is released between forward and backward (the tape owns the activations); temporaries of the backward are
// released as soon as they are consumed, the weight gradients' partials once their queued reductions have been launched.
#include "plan_internal.h"
#include "kernels_attn.h"
#include "kernels_loss.h"

#include <cstdlib>

namespace cd {

struct ResTape {
  const ResW* w = nullptr;
  const float* x0 = nullptr;
  const float* x1 = nullptr;
  int c0 = 0, c1 = 0;
  Dims3 dims{};
  float *h1 = nullptr, *coef1 = nullptr, *stat1 = nullptr, *h2 = nullptr, *coef2 = nullptr, *stat2 = nullptr, *y = nullptr;
};
struct AttnTape {
  const AttnW* w = nullptr;
  const float* x = nullptr;
  Dims3 dims{};
  float *coefn = nullptr, *statn = nullptr, *qkv = nullptr, *ctx = nullptr, *kstat = nullptr, *y0 = nullptr, *coefg = nullptr,
        *statg = nullptr, *y = nullptr;
};
struct TrainTape {
  std::vector<ResTape> down_r1, down_r2, up_r1, up_r2;
  std::vector<AttnTape> down_at, up_at;
  ResTape mid1, mid2, fin;
  AttnTape mid_at;
  std::vector<const float*> down_in;   // input of each down-sampling conv (= skip tensor)
  std::vector<const float*> up_in;     // input of each up-sampling conv
  float *h0 = nullptr, *emb = nullptr, *scal = nullptr, *x0 = nullptr;
};

// Where a step's gradients land: the caller's flat buffer (base), or for a widened tensor its slot in the step's wide block,
// which fold_wide_grads maps back into the caller's buffer at the end of the step
struct Grads {
  CdPlan* p;
  float* base;
  float* wide = nullptr;
  float* at(int widx) const {
    const WeightEntry& w = p->weights[widx];
    return w.widened ? wide + w.wide_grad_off : base + w.grad_off;
  }
};

// narrow widths: the step's wide gradient block (widened plans with parameter gradients only; first in the workspace) ...
static void take_wide_grads(CdPlan* p, Run& r, Grads& G) {
  if (p->widened && r.param_grads) G.wide = r.ws->get<float>(p->wide_grad_floats);
}
// ... and the fold of every widened tensor's gradient into the caller's buffer, one launch after the last gradient is written
static void fold_wide_grads(CdPlan* p, Run& r, const Grads& G) {
  if (!G.wide || r.dry()) return;
  std::vector<WidenJob>& jobs = p->fold_jobs;
  if (jobs.empty()) {
    for (const auto& w : p->weights)
      if (w.widened) jobs.push_back(w.widen);
    CD_HIP(hipMalloc((void**)&p->d_fold_jobs, sizeof(WidenJob) * jobs.size()));
  }
  size_t k = 0;
  bool moved = false;
  for (const auto& w : p->weights) {
    if (!w.widened) continue;
    WidenJob& j = jobs[k++];
    moved = moved || j.narrow != G.base + w.grad_off || j.wide != G.wide + w.wide_grad_off;
    j.narrow = G.base + w.grad_off; j.wide = G.wide + w.wide_grad_off;
  }
  // (the caller's buffer is a fresh tensor each step: the list is re-sent; in stream order, so the previous fold has read its own)
  if (moved) CD_HIP(hipMemcpyAsync(p->d_fold_jobs, jobs.data(), sizeof(WidenJob) * jobs.size(), hipMemcpyHostToDevice, r.s));
  launch_widen_fold(p->d_fold_jobs, (int)jobs.size(), r.s);
}

// ---- forward pieces (training flavour: keep everything, separate output buffers) ------------------------------------
float* res_block_train(Run& r, CdPlan* p, const ResW& W, const float* emb, const float* x0, int c0, const float* x1, int c1,
                       Dims3 dims, ResTape& t, float** part_out = nullptr, int* units_out = nullptr) {
  Arena* ws = r.ws;
  const ResP w = resolve(p, W, emb);
  const int64_t vox = dims.vox();
  const int G = r.groups;
  t.w = &W; t.x0 = x0; t.x1 = x1; t.c0 = c0; t.c1 = c1; t.dims = dims;
  int u1 = 0, u2 = 0;
  t.h1 = ws->get<float>((size_t)r.B * vox * w.cout);
  float* p1 = conv3_with_stats(r, x0, c0, x1, c1, w.c1w, w.c1w3, w.c1b, t.h1, w.cout, dims, nullptr, &u1);
  t.coef1 = ws->get<float>((size_t)r.B * w.cout * 4);
  t.stat1 = ws->get<float>((size_t)r.B * G * 2);
  // The consumers fold the GroupNorm coefficients from the partials in their prologue (gn_defer.h) and leave them on the tape
  // (GnDefer::coef_out / stat_out): no gn_finalize launch per normalisation (round 4: 28 + 6 of a step's 44 went this way)
  static const bool tape_defer = getenv("CD_NO_TRAIN_GNDEFER") == nullptr;
  GnDefer d1;
  d1.part = p1; d1.units = u1; d1.gamma = w.n1g; d1.beta = w.n1b; d1.add = w.emb; d1.add_ld = w.emb_ld; d1.C = w.cout; d1.groups = G;
  d1.vox = vox; d1.coef_out = t.coef1; d1.stat_out = t.stat1;
  if (!r.dry() && !tape_defer) launch_gn_finalize(p1, u1, w.n1g, w.n1b, w.emb, w.emb_ld, t.coef1, r.B, w.cout, G, vox, r.s, t.stat1);
  t.h2 = ws->get<float>((size_t)r.B * vox * w.cout);
  float* p2 = conv3_with_stats(r, t.h1, w.cout, nullptr, 0, w.c2w, w.c2w3, w.c2b, t.h2, w.cout, dims, t.coef1, &u2,
                               tape_defer ? &d1 : nullptr, t.coef1);
  ws->release(p1);
  t.coef2 = ws->get<float>((size_t)r.B * w.cout * 4);
  t.stat2 = ws->get<float>((size_t)r.B * G * 2);
  GnDefer d2;
  d2.part = p2; d2.units = u2; d2.gamma = w.n2g; d2.beta = w.n2b; d2.C = w.cout; d2.groups = G; d2.vox = vox;
  d2.coef_out = t.coef2; d2.stat_out = t.stat2;
  const GnDefer* dp2 = tape_defer ? &d2 : nullptr;
  if (!r.dry() && !tape_defer) launch_gn_finalize(p2, u2, w.n2g, w.n2b, nullptr, 0, t.coef2, r.B, w.cout, G, vox, r.s, t.stat2);
  t.y = ws->get<float>((size_t)r.B * vox * w.cout);
  float* po = nullptr;
  if (part_out) {
    const int bps = gn_apply_blocks_per_sample(r.B, w.cout, vox);
    po = ws->get<float>((size_t)r.B * bps * w.cout * 2);
    *part_out = po;
    *units_out = bps;
  }
  if (w.has_res) {
    float* res = ws->get<float>((size_t)r.B * vox * w.cout);
    if (!r.dry()) {
      PointwiseArgs a;
      a.in0 = x0; a.ld0 = c0; a.off0 = 0; a.c0 = c0; a.in1 = x1; a.ld1 = c1; a.c1 = c1;
      a.wpk = w.rw; a.bias = w.rb; a.out = res; a.batch = r.B; a.cout = w.cout; a.vox = vox;
      launch_pointwise(a, r.s);
      launch_gn_apply(t.h2, t.y, t.coef2, r.B, w.cout, vox, 1, res, nullptr, 0, po, r.s, dp2);
    }
    ws->release(res);
  } else {
    if (!r.dry()) launch_gn_apply(t.h2, t.y, t.coef2, r.B, w.cout, vox, 1, x0, c1 ? x1 : nullptr, c0, po, r.s, dp2);
  }
  ws->release(p2);
  return t.y;
}

float* attn_block_train(Run& r, CdPlan* p, const AttnW& W, const float* x, Dims3 dims, AttnTape& t, float* xpart, int xunits) {
  Arena* ws = r.ws;
  const AttnP w = resolve(p, W);
  const int64_t vox = dims.vox();
  const int C = w.c;
  t.w = &W; t.x = x; t.dims = dims;
  float* own = nullptr;
  if (!xpart) {
    own = stats_pass(r, x, C, vox, &xunits);
    xpart = own;
  }
  t.coefn = ws->get<float>((size_t)r.B * C * 4);
  t.statn = ws->get<float>((size_t)r.B * 2);
  if (!r.dry()) launch_gn_finalize(xpart, xunits, w.ng, w.nb, nullptr, 0, t.coefn, r.B, C, 1, vox, r.s, t.statn);
  if (own) ws->release(own);
  t.qkv = ws->get<float>((size_t)r.B * vox * 96);
  const int nsp = attn_nsplit_for(vox, r.B);
  float* part = ws->get<float>(attn_partial_floats(r.B, nsp));
  const int CT = (C + 31) / 32;
  float* wpb = ws->get<float>((size_t)r.B * CT * 1024);
  t.ctx = ws->get<float>((size_t)r.B * 1024);
  t.kstat = ws->get<float>((size_t)r.B * 64);
  t.y0 = ws->get<float>((size_t)r.B * vox * C);
  const int yu = pointwise_units(vox);
  float* ypart = ws->get<float>((size_t)r.B * yu * C * 2);
  if (!r.dry())
    launch_attn_unfused(x, C, t.coefn, w.qkv, w.ow, w.ob, t.qkv, part, nsp, wpb, t.y0, ypart, r.B, vox, r.s, t.ctx, t.kstat);
  ws->release(part);
  ws->release(wpb);
  t.coefg = ws->get<float>((size_t)r.B * C * 4);
  t.statg = ws->get<float>((size_t)r.B * 2);
  t.y = ws->get<float>((size_t)r.B * vox * C);
  if (!r.dry()) {
    static const bool tape_defer = getenv("CD_NO_TRAIN_GNDEFER") == nullptr;
    GnDefer dg;
    dg.part = ypart; dg.units = yu; dg.gamma = w.gg; dg.beta = w.gb; dg.C = C; dg.groups = 1; dg.vox = vox;
    dg.coef_out = t.coefg; dg.stat_out = t.statg;
    if (!tape_defer) launch_gn_finalize(ypart, yu, w.gg, w.gb, nullptr, 0, t.coefg, r.B, C, 1, vox, r.s, t.statg);
    launch_gn_apply(t.y0, t.y, t.coefg, r.B, C, vox, 0, x, nullptr, 0, nullptr, r.s, tape_defer ? &dg : nullptr);
  }
  ws->release(ypart);
  return t.y;
}

float* unet_body_train(CdPlan* p, Run& r, const float* emb, float* h, TrainTape& T) {
  const CdUnetDesc& d = p->desc;
  const int nres = p->nres;
  const int zs = d.compress_z ? 2 : 1;
  T.down_r1.resize(nres); T.down_r2.resize(nres); T.up_r1.resize(nres); T.up_r2.resize(nres);
  T.down_at.resize(nres); T.up_at.resize(nres);
  T.down_in.assign(nres, nullptr); T.up_in.assign(nres, nullptr);
  std::vector<float*> skips(nres, nullptr);
  float* x = h;
  int cx = d.layer_sizes[0];
  for (int i = 0; i < nres; ++i) {
    const Dims3 dims = p->shapes[i];
    x = res_block_train(r, p, p->downs[i].r1, emb, x, cx, nullptr, 0, dims, T.down_r1[i]);
    cx = p->downs[i].r1.cout;
    float* xp = nullptr;
    int xu = 0;
    x = res_block_train(r, p, p->downs[i].r2, emb, x, cx, nullptr, 0, dims, T.down_r2[i], d.block_attn ? &xp : nullptr, &xu);
    if (d.block_attn) {
      x = attn_block_train(r, p, p->downs[i].attn, x, dims, T.down_at[i], xp, xu);
      r.ws->release(xp);
    }
    skips[i] = x;
    if (i + 1 < nres) {
      const Dims3 nd = p->shapes[i + 1];
      float* y = r.ws->get<float>((size_t)r.B * nd.vox() * cx);
      if (!r.dry()) {
        ConvGeom g{dims, nd, 3, 4, 4, zs, 2, 2};
        ConvFusion fu;
        fu.wpk_bf16x3 = p->packed3(p->downs[i].sw);
        launch_conv_mfma(x, cx, nullptr, 0, p->packed(p->downs[i].sw), p->raw(p->downs[i].sb), y, r.B, cx, g, r.s, fu);
      }
      T.down_in[i] = x;
      x = y;
    }
  }
  const Dims3 md = p->shapes[nres - 1];
  float* mp = nullptr;
  int mu = 0;
  x = res_block_train(r, p, p->mid1, emb, x, cx, nullptr, 0, md, T.mid1, d.mid_attn ? &mp : nullptr, &mu);
  if (d.mid_attn) {
    x = attn_block_train(r, p, p->mid_attn, x, md, T.mid_at, mp, mu);
    r.ws->release(mp);
  }
  x = res_block_train(r, p, p->mid2, emb, x, cx, nullptr, 0, md, T.mid2);
  for (int i = 0; i < nres; ++i) {
    const int lv = nres - 1 - i;
    const Dims3 dims = p->shapes[lv];
    const int cs = d.layer_sizes[lv + 1];
    x = res_block_train(r, p, p->ups[i].r1, emb, x, cx, skips[lv], cs, dims, T.up_r1[i]);
    cx = p->ups[i].r1.cout;
    float* up = nullptr;
    int uu = 0;
    x = res_block_train(r, p, p->ups[i].r2, emb, x, cx, nullptr, 0, dims, T.up_r2[i], d.block_attn ? &up : nullptr, &uu);
    if (d.block_attn) {
      x = attn_block_train(r, p, p->ups[i].attn, x, dims, T.up_at[i], up, uu);
      r.ws->release(up);
    }
    if (i + 1 < nres) {
      const Dims3 od = p->up_out[i];
      float* y = r.ws->get<float>((size_t)r.B * od.vox() * cx);
      if (!r.dry())
        launch_conv_transpose_mfma(x, cx, p->packed(p->ups[i].sw), p->raw(p->ups[i].sb), y, r.B, cx, dims, od, p->up_kz[i], zs, r.s,
                                   p->packed3(p->ups[i].sw), r.status);
      T.up_in[i] = x;
      x = y;
    }
  }
  return res_block_train(r, p, p->fin, nullptr, x, cx, nullptr, 0, p->shapes[0], T.fin);
}

// ---- backward pieces ---------------------------------------------------------------------------------------------
static ConvGeom conv1x1_geom(Dims3 d) { return ConvGeom{d, d, 1, 1, 1, 1, 1, 1}; }
// returns the gradient of the (concatenated) block input: (B, vox, c0+c1); consumes nothing of the tape
float* res_block_bwd(Run& r, CdPlan* p, const ResTape& t, const float* dy, const Grads& G, float* demb) {
  Arena* ws = r.ws;
  const ResW& W = *t.w;
  const int C = W.cout, cin = W.cin, Gn = r.groups;
  const int64_t vox = t.dims.vox();
  ConvGeom g{t.dims, t.dims, 3, 3, 3, 1, 1, 1};
  float* scratch = ws->get<float>(gn_backward_scratch_floats(r.B, C, vox));
  // block2: y = silu(gn2(h2)) + shortcut
  float* dh2 = ws->get<float>((size_t)r.B * vox * C);
  unsigned* dh2_max = r.amax_word();  // max |dh2|: left by the GroupNorm backward for the conv backward that consumes dh2
  if (!r.dry())
    launch_gn_backward(dy, t.h2, t.coef2, t.stat2, p->raw(W.n2g), dh2, G.at(W.n2g), G.at(W.n2b), nullptr, 0, r.B, C, vox, Gn, 1,
                       scratch, false, r.s, G.at(W.c2b), W.has_res ? G.at(W.rb) : nullptr, r.gq, dh2_max);  // (+ the biases of conv2 and the shortcut)
  // a1 = silu(gn1(h1)) + emb was only ever formed inside conv2's LDS staging: the weight gradient re-forms it the same way while
  // it stages h1 (round 4; a gn_apply pass and a tensor per block before), or it is recomputed here for the kernels that cannot
  static const bool no_xnorm = getenv("CD_NO_WGRAD_XNORM") != nullptr;
  const bool xnorm = !no_xnorm && wgrad_x_norm_supported(g);
  float* a1 = (xnorm || !r.param_grads) ? nullptr : ws->get<float>((size_t)r.B * vox * C);
  if (!r.dry() && a1) launch_gn_apply(t.h1, a1, t.coef1, r.B, C, vox, 1, nullptr, nullptr, 0, nullptr, r.s);
  float* da1 = ws->get<float>((size_t)r.B * vox * C);
  const DgImg i2 = p->dg(W.c2w), i1 = p->dg(W.c1w);
  conv_backward(r, a1 ? a1 : t.h1, C, nullptr, 0, p->raw(W.c2w), dh2, da1, G.at(W.c2w), nullptr, C, g, &i2, xnorm ? t.coef1 : nullptr,
                nullptr, nullptr, dh2_max);
  if (a1) ws->release(a1);
  ws->release(dh2);
  float* dh1 = ws->get<float>((size_t)r.B * vox * C);
  unsigned* dh1_max = r.amax_word();
  if (!r.dry())
    launch_gn_backward(da1, t.h1, t.coef1, t.stat1, p->raw(W.n1g), dh1, G.at(W.n1g), G.at(W.n1b),
                       W.has_mlp ? demb + W.emb_off : nullptr, p->emb_ld, r.B, C, vox, Gn, 1, scratch, false, r.s, G.at(W.c1b), nullptr, r.gq,
                       dh1_max);
  ws->release(da1);
  float* dx = ws->get<float>((size_t)r.B * vox * cin);
  // identity shortcut: its share of the input gradient (dy itself) is added by the input-gradient conv where that kernel can
  static const bool no_dxadd = getenv("CD_NO_DGRAD_ADD") != nullptr;
  int added = 0;
  conv_backward(r, t.x0, t.c0, t.x1, t.c1, p->raw(W.c1w), dh1, dx, G.at(W.c1w), nullptr, C, g, &i1, nullptr,
                (!W.has_res && !no_dxadd) ? dy : nullptr, &added, dh1_max);
  ws->release(dh1);
  ws->release(scratch);
  // shortcut
  if (W.has_res) {
    const DgImg ir = p->dg(W.rw);
    float* wp = ir.pk ? nullptr : ws->get<float>(packed_weight_floats(C, cin, 1));
    if (!r.dry()) {
      if (!ir.pk) launch_pack_weights(p->raw(W.rw), wp, cin, C, 1, true, r.s);
      PointwiseArgs a;
      a.in0 = dy; a.ld0 = C; a.c0 = C; a.wpk = ir.pk ? ir.pk : wp; a.out = dx; a.residual = dx; a.batch = r.B; a.cout = cin; a.vox = vox;
      launch_pointwise(a, r.s);
    }
    const float* xs[2] = {t.x0, t.x1};
    const int cs[2] = {t.c0, t.c1};
    for (int k = 0; k < 2 && cs[k] && r.param_grads; ++k) {
      float* part = r.wgrad_part(wgrad_partial_floats(vox, r.B, false, C, cs[k], 1));
      if (!r.dry()) {
        WgradOp op;
        op.g = dy; op.A = C; op.x = xs[k]; op.Bc = cs[k]; op.xld = cs[k]; op.geom = conv1x1_geom(t.dims); op.batch = r.B;
        op.partial = part; op.dw = G.at(W.rw); op.b_total = cin; op.b_off = k ? t.c0 : 0; op.aux = r.wgrad_aux();
        launch_wgrad(op, r.s);
      }
      r.release_wgrad_part(part);
    }
    if (wp) ws->release(wp);
  } else {
    if (!r.dry() && !added) launch_add_slices(dx, cin, 0, dy, C, 0, dx, cin, (int64_t)r.B * vox, r.s);
  }
  return dx;
}

float* attn_block_bwd(Run& r, CdPlan* p, const AttnTape& t, const float* dy, const Grads& G) {
  Arena* ws = r.ws;
  const AttnW& W = *t.w;
  const int C = W.c;
  const int64_t vox = t.dims.vox();
  const int64_t rows = (int64_t)r.B * vox;
  const Dims3 d1 = t.dims;
  const float scale = kAttnScale;
  float* scratch = ws->get<float>(gn_backward_scratch_floats(r.B, C > 96 ? C : 96, vox));
  // out = gn_g(y0) + x
  float* dy0 = ws->get<float>((size_t)rows * C);
  if (!r.dry())
    launch_gn_backward(dy, t.y0, t.coefg, t.statg, p->raw(W.gg), dy0, G.at(W.gg), G.at(W.gb), nullptr, 0, r.B, C, vox, 1, 0, scratch,
                       false, r.s, G.at(W.ob), nullptr, r.gq);  // (+ the bias of to_out's conv, which produced y0)
  // y0 = Wout o + b,  o[n][e] = sum_d (scale*ctx[d][e]) qs[n][d]
  const bool pg = r.param_grads;
  float* qs = ws->get<float>((size_t)rows * 32);
  float* o = pg ? ws->get<float>((size_t)rows * 32) : nullptr;  // (o only feeds the weight gradient of to_out)
  float* pk = ws->get<float>((size_t)r.B * 1024);
  float* pkT = ws->get<float>((size_t)r.B * 1024);
  float* part = pg ? r.wgrad_part(wgrad_partial_floats(vox, r.B, false, C, 32, 1)) : nullptr;
  if (!r.dry()) {
    launch_softmax32(t.qkv, qs, rows, r.s);
    launch_pack_sample32_pair(t.ctx, pk, pkT, r.B, scale, r.s);  // pk: W[co=e][ci=d] = scale*ctx[d][e]; pkT: W[co=d][ci=e] (used below)
    if (pg) {
      PointwiseArgs a;
      a.in0 = qs; a.ld0 = 32; a.c0 = 32; a.wpk = pk; a.w_batch_stride = 1024; a.out = o; a.batch = r.B; a.cout = 32; a.vox = vox;
      launch_pointwise(a, r.s);
      WgradOp op;
      op.g = dy0; op.A = C; op.x = o; op.Bc = 32; op.xld = 32; op.geom = conv1x1_geom(d1); op.batch = r.B; op.partial = part;
      op.dw = G.at(W.ow); op.aux = r.wgrad_aux();
      launch_wgrad(op, r.s);
    }
  }
  if (pg) {
    r.release_wgrad_part(part);
    ws->release(o);
  }
  // do = Wout^T dy0
  float* dO = ws->get<float>((size_t)rows * 32);
  const DgImg io = p->dg(W.ow);
  float* wp = io.pk ? nullptr : ws->get<float>(packed_weight_floats(C, 32, 1));
  if (!r.dry()) {
    if (!io.pk) launch_pack_weights(p->raw(W.ow), wp, 32, C, 1, true, r.s);
    PointwiseArgs a;
    a.in0 = dy0; a.ld0 = C; a.c0 = C; a.wpk = io.pk ? io.pk : wp; a.out = dO; a.batch = r.B; a.cout = 32; a.vox = vox;
    launch_pointwise(a, r.s);
  }
  if (wp) ws->release(wp);
  ws->release(dy0);
  // dctxs[d][e] = sum_n qs[n][d] do[n][e]  (per sample);  dctx = scale * dctxs
  float* dctx = ws->get<float>((size_t)r.B * 1024);
  float* ppart = ws->get<float>(wgrad_partial_floats(vox, r.B, true, 32, 32, 1));
  float* dqkv = ws->get<float>((size_t)rows * 96);
  float* tmp = ws->get<float>((size_t)rows * 32);
  if (!r.dry()) {
    WgradOp op;  // (per sample: not queued, no aux)
    op.g = qs; op.A = 32; op.x = dO; op.Bc = 32; op.xld = 32; op.geom = conv1x1_geom(d1); op.batch = r.B; op.per_sample = true;
    op.partial = ppart; op.dw = dctx;
    launch_wgrad(op, r.s);
    // dqs[n][d] = sum_e scale*ctx[d][e] do[n][e]  -> W[co=d][ci=e] = scale*ctx[d][e]: the transposed image packed above
    PointwiseArgs a;
    a.in0 = dO; a.ld0 = 32; a.c0 = 32; a.wpk = pkT; a.w_batch_stride = 1024; a.out = tmp; a.batch = r.B; a.cout = 32; a.vox = vox;
    launch_pointwise(a, r.s);
    launch_softmax32_bwd(qs, tmp, dqkv, rows, r.s);  // -> dqkv[:, 0:32]
    // dv[n][e] = sum_d ks[n][d] (scale*dctxs[d][e])  -> W[co=e][ci=d] = scale*dctxs[d][e], A = voxel-softmax of k
    launch_pack_sample32_pair(dctx, pk, pkT, r.B, scale, r.s);  // (both images of dctx: pk here, pkT for dks below)
    PointwiseArgs b;
    b.in0 = t.qkv; b.ld0 = 96; b.off0 = 32; b.c0 = 32; b.wpk = pk; b.w_batch_stride = 1024; b.out = dqkv; b.out_ld = 96; b.out_off = 64;
    b.batch = r.B; b.cout = 32; b.vox = vox; b.prologue = A_EXPNORM; b.coef = t.kstat;
    launch_pointwise(b, r.s);
    // dks[n][d] = sum_e (scale*dctxs[d][e]) v[n][e]  -> W[co=d][ci=e] = scale*dctxs[d][e]
    PointwiseArgs c;
    c.in0 = t.qkv; c.ld0 = 96; c.off0 = 64; c.c0 = 32; c.wpk = pkT; c.w_batch_stride = 1024; c.out = tmp; c.batch = r.B; c.cout = 32;
    c.vox = vox;
    launch_pointwise(c, r.s);
    // dk = ks*(dks - r),  r[d] = sum_e (scale*dctxs[d][e]) * ctx[d][e]
    launch_ksoftmax_bwd(t.qkv, tmp, t.kstat, t.ctx, dctx, scale, dqkv, r.B, vox, r.s);
  }
  ws->release(tmp);
  ws->release(ppart);
  ws->release(dctx);
  ws->release(dO);
  ws->release(pk);
  ws->release(pkT);
  ws->release(qs);
  // qkv = Wqkv xn
  float* xn = pg ? ws->get<float>((size_t)rows * C) : nullptr;
  float* dxn = ws->get<float>((size_t)rows * C);
  const DgImg iq = p->dg(W.qkv);
  float* wq = iq.pk ? nullptr : ws->get<float>(packed_weight_floats(96, C, 1));
  part = pg ? r.wgrad_part(wgrad_partial_floats(vox, r.B, false, 96, C, 1)) : nullptr;
  if (!r.dry()) {
    if (pg) {
      launch_gn_apply(t.x, xn, t.coefn, r.B, C, vox, 0, nullptr, nullptr, 0, nullptr, r.s);
      WgradOp op;
      op.g = dqkv; op.A = 96; op.x = xn; op.Bc = C; op.xld = C; op.geom = conv1x1_geom(d1); op.batch = r.B; op.partial = part;
      op.dw = G.at(W.qkv); op.aux = r.wgrad_aux();
      launch_wgrad(op, r.s);
    }
    if (!iq.pk) launch_pack_weights(p->raw(W.qkv), wq, C, 96, 1, true, r.s);
    PointwiseArgs a;
    a.in0 = dqkv; a.ld0 = 96; a.c0 = 96; a.wpk = iq.pk ? iq.pk : wq; a.out = dxn; a.batch = r.B; a.cout = C; a.vox = vox;
    launch_pointwise(a, r.s);
  }
  if (wq) ws->release(wq);
  if (pg) ws->release(xn);
  ws->release(dqkv);
  if (pg) r.release_wgrad_part(part);
  float* dx = ws->get<float>((size_t)rows * C);
  if (!r.dry()) {
    launch_gn_backward(dxn, t.x, t.coefn, t.statn, p->raw(W.ng), dx, G.at(W.ng), G.at(W.nb), nullptr, 0, r.B, C, vox, 1, 0, scratch,
                       false, r.s, nullptr, nullptr, r.gq);
    launch_add_slices(dx, C, 0, dy, C, 0, dx, C, rows, r.s);  // residual branch
  }
  ws->release(dxn);
  ws->release(scratch);
  return dx;
}

// the device job list of dgrad_images (below) pointed at this step's images block `img`: a copy only when the block has moved
// (the engine keeps one training workspace per batch size)
void point_dgrad_jobs(CdPlan* p, float* img, hipStream_t s) {
  if (p->dg_jobs_at == img) return;
  size_t k = 0;
  for (const auto& w : p->weights) {
    if (!w.dg_mode) continue;
    PackJob& j = p->dg_jobs[k++];
    j.pk = img + w.dg_pk_off;
    if (w.dg_mode == 2 || w.dg_mode == 4) {
      j.bf3 = img + w.dg_pk3_off;
      j.f16 = (char*)(img + w.dg_pk3_off) + packed_bf16x3_bytes(j.cin, j.cout, w.taps);
    } else if (w.dg_mode == 3) {
      j.f16 = img + w.dg_pk3_off;
    }
  }
  CD_HIP(hipMemcpyAsync(p->d_dg_jobs, p->dg_jobs.data(), sizeof(PackJob) * p->dg_jobs.size(), hipMemcpyHostToDevice, s));
  p->dg_jobs_at = img;
}

// What the taped forward leaves for the backward pass: the tape, the network input and the arguments of its first launches.
struct TapedForward {
  TrainTape T;
  InitConvArgs ia;
  EmbedArgs ea;
  const float* xn = nullptr;  // network input before c_in (data + sigma noise, or the caller's x)
  double* lpart = nullptr;    // training: the loss partials
  float* hf = nullptr;        // the head's input (the last ResnetBlock's output)
  // flat-state embedding: g_in = enc(c_in xn), the head's raw output on the grid and the cotangent of dec's output, (B, V)
  float *g_in = nullptr, *f_grid = nullptr, *gf = nullptr;
};

// Taped forward shared by cd_train_step (training: the input is data + sigma * noise, formed here) and cd_denoise_vjp (the
// caller's x; no head output, no loss buffers).  Also packs this call's input-gradient weight images.
void taped_forward(CdPlan* p, Run& r, bool training, const float* data, const float* noise, const float* x, const float* sigma,
                   const float* cond, TapedForward& f) {
  const CdUnetDesc& d = p->desc;
  const int B = r.B;
  const Dims3 dims = p->shapes[0];
  const CdPlan::FlatEmbed* fe = p->flat();
  const int64_t per = p->state_per(), n = (int64_t)B * per;  // the state: the grid, or the flat shower of an embedding
  Arena* ws = r.ws;
  hipStream_t s = r.s;
  TrainTape& T = f.T;
  // this call's input-gradient weight images (dgrad_images below), for the whole call
  float* dg_img = ws->get<float>(p->dg_floats);
  p->dg_images = dg_img;
  float* xn = training ? ws->get<float>((size_t)n) : nullptr;
  f.xn = training ? xn : x;
  if (training) {
    T.x0 = ws->get<float>((size_t)n);
    f.lpart = ws->get<double>((size_t)B + 8);
  }
  T.emb = ws->get<float>((size_t)B * p->emb_ld);
  T.scal = ws->get<float>((size_t)B * 4);
  T.h0 = ws->get<float>((size_t)B * dims.vox() * d.layer_sizes[0]);
  if (fe) {
    f.g_in = ws->get<float>((size_t)B * dims.vox());
    f.f_grid = ws->get<float>((size_t)B * dims.vox());
    f.gf = ws->get<float>((size_t)n);
  }
  InitConvArgs& ia = f.ia;
  ia.x = fe ? f.g_in : f.xn; ia.cin = d.in_channels; ia.cx = 1; ia.scale_b = fe ? nullptr : T.scal;  // (g_in carries c_in)
  ia.scale_stride = 4; ia.use_rz = d.rz_input; ia.use_phi = d.phi_input;
  ia.r_w = p->d_coords; ia.z_d = p->d_coords + d.grid[2]; ia.phi_h = p->d_coords + d.grid[2] + d.grid[0];
  ia.wpk = p->packed(p->init_w); ia.bias = p->raw(p->init_b); ia.out = T.h0; ia.batch = B; ia.cout = d.layer_sizes[0]; ia.dims = dims;
  ia.coord_table = p->d_init_table; ia.table_ready = true; ia.status = r.status;
  f.ea = embed_args(p, B, cond, sigma, d.time_embed_kind, T.emb, T.scal);
  if (!r.dry()) {
    if (!p->dg_jobs.empty()) {  // the images of all convolutions in two launches
      point_dgrad_jobs(p, dg_img, s);
      launch_pack_jobs(p->d_dg_jobs, (int)p->dg_jobs.size(), s);
      launch_pack_jobs_f16x2(p->d_dg_jobs, (int)p->dg_jobs.size(), s);
    }
    if (training) launch_axpy_sigma(data, noise, sigma, xn, B, per, s);
    launch_embed(f.ea, s);
    if (fe) launch_embed_in(*fe, f.xn, T.scal, f.g_in, B, s);
    launch_init_conv(ia, s);
  }
  f.hf = unet_body_train(p, r, T.emb, T.h0, T);
}

struct BackwardState;
// Flat-state embedding, the top of the backward pass: the cotangent gf of dec's output is in place; dec's VJP gives the head its
// cotangent on the grid (and dec_w its gradient), the head's backward runs raw (no preconditioning: mean_pred's chain of 1)
void embed_head_backward(CdPlan* p, Run& r, const TapedForward& f, const Grads& G, BackwardState& bs, float* hpart);
// ... and its bottom: the init conv's input gradient on the grid (times c_in, no direct term), then enc's VJP: dx with the
// preconditioning's direct x term (gy; null in training, whose input is data: dx is scratch there, and with frozen matrices
// nothing is launched) and enc_w's gradient.  Consumes nothing.
void embed_input_backward(CdPlan* p, Run& r, const TapedForward& f, const float* g, const float* gy, float* dx, const Grads& G);

// State of one backward pass: the GroupNorm layers queue their parameter-gradient reductions (per-sample sums in `qsums`), one
// launch flushes them at the end; the weight gradients queue the reductions of their per-workgroup partials (65 launches of 4-7 us
// otherwise), each partial in a workspace block of its own until then (Run::wgrad_part).
struct BackwardState {
  WgradReduceQueue wq;
  GnParamQueue gq;
  float* qsums = nullptr;
  float* demb = nullptr;  // gradient of the (B, emb_ld) block embeddings
  float* g = nullptr;     // (B, vox, 32) gradient at the head input, for the head's backward to fill
};
void begin_backward(CdPlan* p, Run& r, BackwardState& bs) {
  const CdUnetDesc& d = p->desc;
  const int nres = p->nres, B = r.B;
  const int64_t n = (int64_t)B * p->shapes[0].vox();
  Arena* ws = r.ws;
  static const bool no_wq = getenv("CD_NO_WGRAD_QUEUE") != nullptr;
  if (!no_wq && r.param_grads) r.wq = &bs.wq;
  int cmax = 32;
  for (int i = 0; i <= nres; ++i) cmax = d.layer_sizes[i] > cmax ? d.layer_sizes[i] : cmax;
  const size_t nsums = (size_t)GnParamJobs::kMax * 2 * B * cmax * 4;
  bs.qsums = ws->get<float>(nsums);
  bs.gq.sums = bs.gq.next_sums = bs.qsums;
  bs.gq.sums_end = bs.qsums + nsums;
  bs.gq.discard = !r.param_grads;  // (the GroupNorm input gradient still needs its per-sample sums: only their reduction goes)
  r.gq = &bs.gq;
  // demb, and behind it the step's max-|x| words (launch_absmax_bits, launch_gn_backward): one memset zeroes both.  A convolution's
  // backward measures at most two tensors, a GroupNorm backward one: fewer words than weight tensors, twice that is plenty.  (The
  // whole is a multiple of 64 floats: a fill of any other size is two launches.)
  const size_t nemb = (size_t)B * p->emb_ld, nclear = (nemb + 2 * p->weights.size() + 63) & ~(size_t)63;
  bs.demb = ws->get<float>(nclear);
  if (!r.dry()) r.amax = AbsmaxWords{(unsigned*)(bs.demb + nemb), (unsigned*)(bs.demb + nclear)};
  bs.g = ws->get<float>((size_t)n * 32);
  if (!r.dry()) CD_HIP(hipMemsetAsync(bs.demb, 0, sizeof(float) * nclear, r.s));
}

// The body's backward: from the gradient at the head input (consumed) down to the gradient at the init conv's output (returned)
float* body_backward(CdPlan* p, Run& r, const TrainTape& T, float* g, const Grads& G, float* demb) {
  const CdUnetDesc& d = p->desc;
  const int nres = p->nres, B = r.B;
  const int zs = d.compress_z ? 2 : 1;
  Arena* ws = r.ws;
  hipStream_t s = r.s;
  auto step = [&](float* ng, float*& cur) {  // replace the running gradient
    ws->release(cur);
    cur = ng;
  };
  step(res_block_bwd(r, p, T.fin, g, G, demb), g);
  std::vector<float*> gskip(nres, nullptr);
  for (int i = nres - 1; i >= 0; --i) {
    const int lv = nres - 1 - i;
    const Dims3 dl = p->shapes[lv];
    const int cs = d.layer_sizes[lv + 1];
    const int cx = d.layer_sizes[lv + 1];  // width of x entering r1 of this stage (== skip width)
    if (i + 1 < nres) {
      const int c = p->ups[i].r1.cout;
      float* dx = ws->get<float>((size_t)B * dl.vox() * c);
      const DgImg iu = p->dg(p->ups[i].sw);
      conv_transpose_backward(r, T.up_in[i], p->raw(p->ups[i].sw), g, dx, G.at(p->ups[i].sw), G.at(p->ups[i].sb), c, dl, p->up_out[i],
                              p->up_kz[i], zs, &iu);
      step(dx, g);
    }
    if (d.block_attn) step(attn_block_bwd(r, p, T.up_at[i], g, G), g);
    step(res_block_bwd(r, p, T.up_r2[i], g, G, demb), g);
    float* gcat = res_block_bwd(r, p, T.up_r1[i], g, G, demb);  // (B, vox, cx + cs)
    ws->release(g);
    g = ws->get<float>((size_t)B * dl.vox() * cx);
    gskip[lv] = ws->get<float>((size_t)B * dl.vox() * cs);
    if (!r.dry()) {
      launch_add_slices(gcat, cx + cs, 0, nullptr, 0, 0, g, cx, (int64_t)B * dl.vox(), s);
      launch_add_slices(gcat, cx + cs, cx, nullptr, 0, 0, gskip[lv], cs, (int64_t)B * dl.vox(), s);
    }
    ws->release(gcat);
  }
  step(res_block_bwd(r, p, T.mid2, g, G, demb), g);
  if (d.mid_attn) step(attn_block_bwd(r, p, T.mid_at, g, G), g);
  step(res_block_bwd(r, p, T.mid1, g, G, demb), g);
  for (int i = nres - 1; i >= 0; --i) {
    const Dims3 dl = p->shapes[i];
    const int c = d.layer_sizes[i + 1];
    if (i + 1 < nres) {
      float* dx = ws->get<float>((size_t)B * dl.vox() * c);
      ConvGeom gd{dl, p->shapes[i + 1], 3, 4, 4, zs, 2, 2};
      const DgImg id = p->dg(p->downs[i].sw);
      conv_backward(r, T.down_in[i], c, nullptr, 0, p->raw(p->downs[i].sw), g, dx, G.at(p->downs[i].sw), G.at(p->downs[i].sb), c, gd, &id);
      step(dx, g);
    }
    // the level's output also fed the skip connection
    if (!r.dry()) launch_add_slices(g, c, 0, gskip[i], c, 0, g, c, (int64_t)B * dl.vox(), s);
    ws->release(gskip[i]);
    if (d.block_attn) step(attn_block_bwd(r, p, T.down_at[i], g, G), g);
    step(res_block_bwd(r, p, T.down_r2[i], g, G, demb), g);
    step(res_block_bwd(r, p, T.down_r1[i], g, G, demb), g);
  }
  return g;
}

// The init conv's weight and bias gradients from g (its output gradient, released here), then every queued reduction and the
// conditioning MLPs' backward
void finish_param_grads(CdPlan* p, Run& r, const TapedForward& f, float* g, const Grads& G, BackwardState& bs) {
  const CdUnetDesc& d = p->desc;
  const int B = r.B;
  const int64_t per = p->shapes[0].vox();
  Arena* ws = r.ws;
  hipStream_t s = r.s;
  float* demb = bs.demb;
  static const bool init_scalar = getenv("CD_INIT_WGRAD_SCALAR") != nullptr;
  if (init_scalar) {
    float* ipart = ws->get<float>(init_wgrad_partial_floats(B, per, d.in_channels, d.layer_sizes[0]));
    if (!r.dry()) launch_init_wgrad(f.ia, g, ipart, G.at(p->init_w), s);
    ws->release(ipart);
  } else {
    float* iscr = ws->get<float>(init_wgrad_mfma_floats(B, per, d.layer_sizes[0]));
    if (!r.dry()) launch_init_wgrad_mfma(f.ia, g, iscr, G.at(p->init_w), s, &r.amax);
    ws->release(iscr);
  }
  bias_grad(r, g, d.layer_sizes[0], per, G.at(p->init_b));
  ws->release(g);
  if (!r.dry()) launch_gn_param_jobs(bs.gq.jobs, s);  // every GroupNorm layer's dgamma / dbeta / conv-bias gradient: one launch
  r.gq = nullptr;
  if (!r.dry() && r.wq) wgrad_queue_flush(r.wq, s);  // every queued slot reduction: one launch
  for (float* part : r.wq_held) ws->release(part);
  r.wq_held.clear();
  r.wq = nullptr;
  ws->release(bs.qsums);
  // conditioning MLPs
  const int half = d.cond_dim / 2, hidden = d.cond_size > half / 2 ? d.cond_size : half / 2, q = half / 2;
  const EmbedTapeLayout L = embed_tape_layout(d.cond_size, hidden, half);
  float* etape = ws->get<float>((size_t)B * L.total);
  if (!r.dry()) {
    launch_embed_bwd(f.ea, demb, etape, s);
    std::vector<LinearWgradJob>& jobs = p->lin_jobs_host;
    jobs.clear();
    auto add = [&](int off_delta, int off_in, int widx, int bidx, int nout, int nin) {
      jobs.push_back(LinearWgradJob{etape + off_delta, etape + off_in, G.at(widx), G.at(bidx), nout, nin, L.total, L.total});
    };
    add(L.d1t, L.t_in, p->tw[0], p->tb[0], q, 1);
    add(L.d2t, L.a1t, p->tw[1], p->tb[1], half, q);
    add(L.d3t, L.a2t, p->tw[2], p->tb[2], half, half);
    add(L.d1c, L.cond_in, p->cw[0], p->cb[0], hidden, d.cond_size);
    add(L.d2c, L.a1c, p->cw[1], p->cb[1], half, hidden);
    add(L.d3c, L.a2c, p->cw[2], p->cb[2], half, half);
    int max_elems = hidden * (d.cond_size > half ? d.cond_size : half);
    if (max_elems < half * half) max_elems = half * half;
    for (auto& e : p->embed_list) {
      const WeightEntry& w = p->weights[e.first];
      const int cout = (int)(w.numel / d.cond_dim);
      jobs.push_back(LinearWgradJob{demb + e.second, etape + L.sc, G.at(e.first), G.at(e.first + 1), cout, 2 * half, p->emb_ld, L.total});
      if (cout * 2 * half > max_elems) max_elems = cout * 2 * half;
    }
    CD_REQUIRE(jobs.size() <= 64, "too many linear layers");
    CD_HIP(hipMemcpyAsync(p->d_lin_jobs, jobs.data(), sizeof(LinearWgradJob) * jobs.size(), hipMemcpyHostToDevice, s));
    launch_linear_wgrad(p->d_lin_jobs, (int)jobs.size(), max_elems, B, s);
  }
}

// loss + all parameter gradients.  Returns nothing; grads (flat) and loss_out are written on the stream.
// target (cd_train_step_target; null in cd_train_step): the loss compares the denoiser's output with it instead of with what the
// objective compares with -- residual out - target, weight 1 (kResidualOnOutput) -- in the same launches; the network's input
// stays data + sigma * noise.
void train_step_impl(CdPlan* p, int B, const float* data, const float* noise, const float* sigma, const float* cond, double* loss_out,
                     float* grads, hipStream_t s, int loss_type = 0, const float* target = nullptr) {
  const CdUnetDesc& d = p->desc;
  const CdPlan::FlatEmbed* fe = p->flat();
  const int64_t vox = p->shapes[0].vox(), per = p->state_per();
  const float* cmp = target ? target : data;
  const int res_obj = target ? kResidualOnOutput : d.objective;
  Run r{&p->ws, s, B, d.groups};
  r.status = p->status_word;
  Grads G{p, grads};
  take_wide_grads(p, r, G);
  TapedForward f;
  taped_forward(p, r, true, data, noise, nullptr, sigma, cond, f);
  const TrainTape& T = f.T;
  if (!r.dry()) {
    HeadArgs ha;
    ha.h = f.hf; ha.w = p->raw(p->head_w); ha.bias = p->raw(p->head_b); ha.out = fe ? f.f_grid : T.x0; ha.batch = B; ha.vox = vox;
    if (!fe) { ha.x = f.xn; ha.scal = T.scal; ha.objective = d.objective; }
    launch_head(ha, s);
    if (fe) launch_embed_out(*fe, f.f_grid, f.xn, T.scal, d.objective, T.x0, nullptr, B, s);
    launch_loss_partial(T.x0, cmp, noise, sigma, f.lpart, B, per, s, loss_type, res_obj);
    launch_loss_final(f.lpart, sigma, loss_out, B, per, s, loss_type, res_obj);
  }
  BackwardState bs;
  begin_backward(p, r, bs);
  float* hpart = r.ws->get<float>((size_t)head_bwd_blocks(B, vox) * 33);
  if (fe) {
    if (!r.dry()) launch_embed_cotangent(T.x0, data, noise, nullptr, T.scal, f.gf, B, per, loss_type, d.objective, s);
    embed_head_backward(p, r, f, G, bs, hpart);
  } else if (!r.dry()) {
    launch_head_loss_bwd(T.x0, cmp, noise, T.scal, f.hf, p->raw(p->head_w), bs.g, hpart, G.at(p->head_w), G.at(p->head_b), B, per, s,
                         loss_type, d.objective, res_obj);
  }
  float* g = body_backward(p, r, T, bs.g, G, bs.demb);
  // the embedding's encoder: its weight gradient (the input is data: no input gradient is wanted, the row program's goes to gf)
  if (fe) embed_input_backward(p, r, f, g, nullptr, f.gf, G);
  // init conv: weight and bias gradients only (its input is data)
  finish_param_grads(p, r, f, g, G, bs);
  fold_wide_grads(p, r, G);
}

void embed_head_backward(CdPlan* p, Run& r, const TapedForward& f, const Grads& G, BackwardState& bs, float* hpart) {
  const int B = r.B;
  const int64_t vox = p->shapes[0].vox();
  const bool want = r.param_grads && p->fe.want_grads && G.base;
  float* dF = r.ws->get<float>((size_t)B * vox);
  if (!r.dry()) {
    launch_embed_dec_vjp(p->fe, f.f_grid, f.gf, dF, want ? G.base + p->dec_grad_off() : nullptr, B, r.s);
    launch_head_vjp(dF, f.T.scal, f.hf, p->raw(p->head_w), bs.g, r.param_grads ? hpart : nullptr,
                    r.param_grads ? G.at(p->head_w) : nullptr, r.param_grads ? G.at(p->head_b) : nullptr, B, vox, CD_OBJ_MEAN_PRED, r.s);
  }
  r.ws->release(dF);
}

void embed_input_backward(CdPlan* p, Run& r, const TapedForward& f, const float* g, const float* gy, float* dx, const Grads& G) {
  const CdUnetDesc& d = p->desc;
  const int B = r.B;
  const Dims3 dims = p->shapes[0];
  const bool want = r.param_grads && p->fe.want_grads && G.base;
  float* dg = r.ws->get<float>((size_t)B * dims.vox());
  if (!r.dry() && (gy || want)) {
    launch_init_dgrad(g, p->raw(p->init_w), d.in_channels, d.layer_sizes[0], nullptr, f.T.scal, CD_OBJ_MEAN_PRED, dg, B, dims, r.s);
    launch_embed_enc_vjp(p->fe, f.xn, dg, gy, f.T.scal, d.objective, dx, want ? G.base + p->enc_grad_off() : nullptr,
                         B, r.s);
  }
  r.ws->release(dg);
}

// Vector-Jacobian product of cd_denoise: dx = (dD/dx)^T gy and, with grads, every parameter's gradient (the taped forward is
// recomputed from x).  Without grads (param_grads false) no weight, bias, GroupNorm-parameter or embedding work is launched; the
// input-gradient path is the same launches either way, so dx is the same bits.
void denoise_vjp_impl(CdPlan* p, int B, const float* x, const float* sigma, const float* cond, const float* gy, float* dx, float* grads,
                      bool param_grads, hipStream_t s) {
  const CdUnetDesc& d = p->desc;
  const CdPlan::FlatEmbed* fe = p->flat();
  const Dims3 dims = p->shapes[0];
  const int64_t per = dims.vox();
  Run r{&p->ws, s, B, d.groups};
  r.status = p->status_word;
  r.param_grads = param_grads;
  Grads G{p, grads};
  take_wide_grads(p, r, G);
  TapedForward f;
  taped_forward(p, r, false, nullptr, nullptr, x, sigma, cond, f);
  const TrainTape& T = f.T;
  BackwardState bs;
  begin_backward(p, r, bs);
  float* hpart = param_grads ? r.ws->get<float>((size_t)head_bwd_blocks(B, per) * 33) : nullptr;
  if (fe) {
    if (!r.dry()) {
      // the head's raw output on the grid, which dec_w's gradient pairs with the cotangent
      HeadArgs ha;
      ha.h = f.hf; ha.w = p->raw(p->head_w); ha.bias = p->raw(p->head_b); ha.out = f.f_grid; ha.batch = B; ha.vox = per;
      if (param_grads && p->fe.want_grads) launch_head(ha, s);
      launch_embed_cotangent(nullptr, nullptr, nullptr, gy, T.scal, f.gf, B, p->state_per(), 0, d.objective, s);
    }
    embed_head_backward(p, r, f, G, bs, hpart);
  } else if (!r.dry()) {
    launch_head_vjp(gy, T.scal, f.hf, p->raw(p->head_w), bs.g, hpart, param_grads ? G.at(p->head_w) : nullptr,
                    param_grads ? G.at(p->head_b) : nullptr, B, per, d.objective, s);
  }
  float* g = body_backward(p, r, T, bs.g, G, bs.demb);
  // init conv: the data channel's input gradient, the preconditioning folded in (the coordinate channels are constants)
  if (fe) embed_input_backward(p, r, f, g, gy, dx, G);
  else if (!r.dry())
    launch_init_dgrad(g, p->raw(p->init_w), d.in_channels, d.layer_sizes[0], gy, T.scal, d.objective, dx, B, dims, s);
  if (param_grads) {
    finish_param_grads(p, r, f, g, G, bs);
    fold_wide_grads(p, r, G);
  } else {
    r.ws->release(g);
    r.gq = nullptr;
    r.ws->release(bs.qsums);
  }
}

// The weight images every convolution's INPUT gradient reads (the forward kernels run on channel-transposed, tap-flipped weights:
// conv_backward / conv_transpose_backward), laid out once per plan (dg_floats) and described by one job list whose sources are the
// plan's own raw copies of the tensors; the images themselves go to a block of each step's workspace (train_step_impl re-points
// the list when that block moves, and launches it once per step).  The packers write every float of every image, and the
// alignment gaps between the images are never read: the block needs no clearing.  dg_mode: 1 = 1x1 conv (f32 image,
// transposed), 2 = 3x3x3 stride 1 (f32 + split16 images, transposed + flipped), 3 = strided down conv (f32 + f16x2 images,
// transposed: its adjoint is the up-conv gather kernel), 4 = up conv (f32 + split16 images of the tensor read as a plain conv:
// its adjoint is the strided conv).
void dgrad_images(CdPlan* p) {
  if (p->d_dg_jobs) return;
  size_t off = 0;
  auto bump = [&](size_t n) { size_t o = off; off += (n + 63) & ~(size_t)63; return o; };
  std::vector<PackJob> jobs;
  for (auto& w : p->weights) {
    if (w.pack != PK_CONV && w.pack != PK_CONVT && !w.dg_1x1) continue;
    PackJob j{};
    j.kind = 1;
    j.taps = w.taps;
    if (w.pack == PK_CONVT) {
      w.dg_mode = 4;
      j.cout = w.cout; j.cin = w.cin;
    } else {
      w.dg_mode = w.taps == 1 ? 1 : (w.taps == 27 ? 2 : 3);
      j.cout = w.cin; j.cin = w.cout;  // the gradient's convolution maps the conv's output channels back to its input channels
      j.tr = 1;
      j.flip = w.dg_mode == 2 ? 1 : 0;
    }
    if (j.cin % 32 || j.cout % 32) {  // (the init conv's 3 / 4 input channels never need an input gradient)
      w.dg_mode = 0;
      continue;
    }
    w.dg_pk_off = bump(packed_weight_floats(j.cin, j.cout, w.taps));
    const unsigned long long n16 = (unsigned long long)(j.cin / 16) * w.taps * ((j.cout + 31) / 32) * 64;
    if (w.dg_mode == 2 || w.dg_mode == 4) w.dg_pk3_off = bump(packed_split16_bytes(j.cin, j.cout, w.taps) / 4);
    else if (w.dg_mode == 3) w.dg_pk3_off = bump(packed_f16x2_bytes(j.cin, j.cout, w.taps) / 4 + 64);
    j.n_pk = packed_weight_floats(j.cin, j.cout, w.taps);
    if (w.dg_mode == 2 || w.dg_mode == 4) j.n_bf3 = j.n_f16 = n16;
    else if (w.dg_mode == 3) j.n_f16 = n16;
    jobs.push_back(j);
  }
  size_t k = 0;
  for (auto& w : p->weights)
    if (w.dg_mode) jobs[k++].src = p->arena + w.raw_off;
  p->dg_floats = off;
  p->dg_jobs = jobs;
  CD_HIP(hipMalloc((void**)&p->d_dg_jobs, sizeof(PackJob) * (jobs.size() + 1)));
}

}  // namespace cd

extern "C" {

int cd_plan_train_workspace_bytes(CdPlan* plan, int batch, size_t* bytes) {
  return guarded([&] {
    CD_REQUIRE(plan && bytes && batch > 0, "bad argument");
    CD_REQUIRE(!plan->desc.time_sin && !plan->desc.cond_sin, "the training step needs the Linear time/cond embeddings");
    dgrad_images(plan);
    plan->ws.reset(nullptr, 0, true);
    train_step_impl(plan, batch, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    *bytes = plan->ws.high() + 4096;
  });
}

int cd_train_step(CdPlan* plan, int batch, const float* data, const float* noise, const float* sigma, const float* cond,
                  int loss_type, double* loss_out, float* grads, void* workspace, size_t workspace_bytes, void* stream) {
  return guarded([&] {
    CD_REQUIRE(plan && data && noise && sigma && cond && loss_out && grads && workspace && batch > 0, "bad argument");
    CD_REQUIRE(loss_type >= CD_LOSS_L2 && loss_type <= CD_LOSS_HUBER, "loss_type must be one of CD_LOSS_L2 / L1 / MSE / HUBER");
    check_ready(plan, true);
    dgrad_images(plan);
    plan->ws.reset((char*)workspace, workspace_bytes, false);
    train_step_impl(plan, batch, data, noise, sigma, cond, loss_out, grads, (hipStream_t)stream, loss_type);
  });
}

int cd_train_step_target(CdPlan* plan, int batch, const float* data, const float* noise, const float* sigma, const float* cond,
                         const float* target, int loss_type, double* loss_out, float* grads, void* workspace, size_t workspace_bytes,
                         void* stream) {
  return guarded([&] {
    CD_REQUIRE(plan && data && noise && sigma && cond && target && loss_out && grads && workspace && batch > 0, "bad argument");
    CD_REQUIRE(loss_type >= CD_LOSS_L1 && loss_type <= CD_LOSS_HUBER,
               "loss_type must be one of CD_LOSS_L1 / MSE / HUBER: the weight of CD_LOSS_L2 has no meaning against a given target "
               "(use CD_LOSS_MSE)");
    CD_REQUIRE(!plan->flat(), "cd_train_step_target compares on the grid: a plan with a geometry embedding is not provided");
    check_ready(plan, true);
    dgrad_images(plan);
    plan->ws.reset((char*)workspace, workspace_bytes, false);
    train_step_impl(plan, batch, data, noise, sigma, cond, loss_out, grads, (hipStream_t)stream, loss_type, target);
  });
}

int cd_plan_vjp_workspace_bytes(CdPlan* plan, int batch, int with_param_grads, size_t* bytes) {
  return guarded([&] {
    CD_REQUIRE(plan && bytes && batch > 0, "bad argument");
    CD_REQUIRE(!plan->desc.time_sin && !plan->desc.cond_sin, "the training step needs the Linear time/cond embeddings");
    dgrad_images(plan);
    plan->ws.reset(nullptr, 0, true);
    denoise_vjp_impl(plan, batch, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, with_param_grads != 0, nullptr);
    *bytes = plan->ws.high() + 4096;
  });
}

int cd_denoise_vjp(CdPlan* plan, int batch, const float* x, const float* sigma, const float* cond, const float* gy, float* dx,
                   float* grads, void* workspace, size_t workspace_bytes, void* stream) {
  return guarded([&] {
    CD_REQUIRE(plan && x && sigma && cond && gy && dx && workspace && batch > 0, "bad argument");
    CD_REQUIRE(!plan->desc.time_sin && !plan->desc.cond_sin, "the training step needs the Linear time/cond embeddings");
    check_ready(plan, true);
    dgrad_images(plan);
    plan->ws.reset((char*)workspace, workspace_bytes, false);
    denoise_vjp_impl(plan, batch, x, sigma, cond, gy, dx, grads, grads != nullptr, (hipStream_t)stream);
  });
}

}  // extern "C"
