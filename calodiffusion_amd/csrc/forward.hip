// The network's forward launch sequences on one HIP stream: CondUnet.forward / CaloDiffusion.denoise, and the entry points that
// run one forward (cd_unet_forward, cd_denoise*, the hybrid_weight loss).  Nothing here allocates or synchronises inside a compute
// call, so a sampler step is hipGraph-capturable.
#include "plan_internal.h"
#include "kernels_attn.h"
#include "kernels_deep.h"
#include "kernels_loss.h"

#include <cstdio>
#include <cstdlib>

namespace cd {

ResP resolve(const CdPlan* p, const ResW& w, const float* emb) {
  ResP r;
  r.cin = w.cin; r.cout = w.cout; r.has_res = w.has_res;
  r.c1w3 = p->packed3(w.c1w); r.c2w3 = p->packed3(w.c2w);
  r.c1w = p->packed(w.c1w); r.c1b = p->raw(w.c1b); r.n1g = p->raw(w.n1g); r.n1b = p->raw(w.n1b);
  r.c2w = p->packed(w.c2w); r.c2b = p->raw(w.c2b); r.n2g = p->raw(w.n2g); r.n2b = p->raw(w.n2b);
  if (w.has_res) {
    r.rw = p->packed(w.rw); r.rb = p->raw(w.rb);
    if (p->packed3(w.rw)) r.rw16 = (const char*)p->packed3(w.rw) + packed_bf16x3_bytes(w.cin, w.cout, 1);
  }
  if (w.has_mlp && emb) { r.emb = emb + w.emb_off; r.emb_ld = p->emb_ld; }
  return r;
}
AttnP resolve(const CdPlan* p, const AttnW& w) {
  AttnP a;
  a.c = w.c;
  a.ng = p->raw(w.ng); a.nb = p->raw(w.nb); a.qkv = p->packed(w.qkv); a.ow = p->raw(w.ow); a.ob = p->raw(w.ob);
  a.qkv16 = (const char*)p->packed3(w.qkv) + packed_bf16x3_bytes(w.c, 96, 1);
  a.gg = p->raw(w.gg); a.gb = p->raw(w.gb);
  a.coop_sync = p->d_attn_sync;
  return a;
}

// channel partials of a tensor from a standalone pass (producer without a stats epilogue)
float* stats_pass(Run& r, const float* x, int C, int64_t vox, int* units) {
  const int ns = gn_nsplit_for(vox, r.B);
  float* part = r.ws->get<float>((size_t)r.B * ns * C * 2);
  if (!r.dry()) launch_ch_stats(x, part, r.B, C, vox, ns, r.s);
  *units = ns;
  return part;
}

// conv + channel partials of its output (fused epilogue when the kernel supports it); input optionally normalised
// on the fly by `coef_in` (+SiLU).  Returns the partial buffer (caller releases) and sets *units.
// defer_in (optional, instead of coef_in): the input normalisation as partials + affine parameters, folded by the conv
// kernel itself; coef_buf is the [B][Cin][4] table a kernel without that prologue gets materialised.
float* conv3_with_stats(Run& r, const float* x0, int c0, const float* x1, int c1, const float* wpk, const void* wpk3,
                        const float* bias, float* out, int cout, Dims3 dims, const float* coef_in, int* units,
                        const GnDefer* defer_in, float* coef_buf, const ConvFusion::GnOut* gn_out) {
  const int64_t vox = dims.vox();
  const int cap = (int)((vox + 31) / 32);
  float* part = r.ws->get<float>((size_t)r.B * cap * cout * 2);
  int u = 0;
  if (!r.dry()) {
    ConvGeom g{dims, dims, 3, 3, 3, 1, 1, 1};
    ConvFusion fu;
    fu.coef = coef_in; fu.act = 1; fu.ch_part = part; fu.units = &u; fu.wpk_bf16x3 = wpk3; fu.status = r.status;
    if (defer_in) { fu.defer = *defer_in; fu.coef_buf = coef_buf; fu.coef = nullptr; }
    if (gn_out) fu.gn_out = *gn_out;
    launch_conv_mfma(x0, c0, x1, c1, wpk, bias, out, r.B, cout, g, r.s, fu);
    if (gn_out && *gn_out->done) {
      // (the kernel normalised its own output: `out` is the block output, there are no partials of the conv output)
    } else if (u == 0) {  // kernel without a stats epilogue: separate pass, same buffer (nsplit <= cap)
      u = gn_nsplit_for(vox, r.B);
      if (u > cap) u = cap;
      launch_ch_stats(out, part, r.B, cout, vox, u, r.s);
    }
  }
  *units = u;
  return part;
}

// The x half of a concat conv whose x1 half already ran as the side job of the deepest level's launch (kernels_deep_side.hip):
// `out` holds conv(x1, second K-block) + bias; this is the one continuation launch of the z-slide kernel that adds the first
// K-block to it (ConvFusion::add_src) and emits the channel partials.  Same partial buffer and units as conv3_with_stats.
static float* conv3_x_half_with_stats(Run& r, const float* x0, int c0, int c1, const void* wpk3, float* out, int cout, Dims3 dims,
                                      int* units) {
  const int64_t vox = dims.vox();
  const int cap = (int)((vox + 31) / 32);
  float* part = r.ws->get<float>((size_t)r.B * cap * cout * 2);
  int u = 0;
  if (!r.dry()) {
    ConvGeom g{dims, dims, 3, 3, 3, 1, 1, 1};
    ConvFusion fu;
    int added = 0;
    fu.act = 1; fu.ch_part = part; fu.units = &u; fu.status = r.status; fu.add_src = out; fu.add_done = &added;
    char cat[128];
    std::snprintf(cat, sizeof cat, "conv3x3x3_s1 C%d(of %d)->%d @%dx%dx%d", c0, c0 + c1, cout, dims.d, dims.h, dims.w);
    prof::Scope scope(cat, r.s, 2.0 * 27 * c0 * cout * (double)vox * r.B, 4.0 * r.B * (double)vox * (c0 + 2 * cout));
    const bool ran = try_launch_conv_zslide(x0, c0, nullptr, 0, (const char*)wpk3 + packed_bf16x3_bytes(c0 + c1, cout, 27), nullptr, out,
                                            r.B, cout, g, r.s, fu);
    CD_REQUIRE(ran && added && u > 0, "internal: the x half of a side conv must run as a z-slide continuation");
  }
  *units = u;
  return part;
}

// ResnetBlock.forward (models.py:191-200): block1 -> (+ mlp(cond)) -> block2 -> + res_conv(x).
//   conv1 (stats epilogue) -> finalize -> conv2 normalises h1 while staging it (stats epilogue) -> finalize ->
//   one elementwise pass: silu(gn(h2)) + shortcut.  `part_out`/`units_out` (optional): channel partials of the block
//   output for a following PreNorm.
// `lazy` (optional): leave the closing GroupNorm + SiLU + identity shortcut to the consumer (the head kernel).  If the block
// qualifies it returns its second conv's raw output, lazy->gn describes the normalisation, lazy->part (to be released by the
// caller) holds its partials and the shortcut is x0.
// `h1_side` (optional): the first conv's output buffer, a workspace block this call takes over, in which the x1 half of that conv
// (and its bias) has already been computed -- only the x0 half is left to add (conv3_x_half_with_stats).
struct LazyClose {
  GnDefer gn;
  float* part = nullptr;
  bool on = false;
};
// `h1_done` (optional): the first conv's output AND its channel partials, computed whole by an earlier launch (the composed init
// pair, kernels_init_pair.hip): the conv is skipped, both blocks are taken over.
float* res_block(Run& r, const ResP& w, const float* x0, int c0, const float* x1, int c1, Dims3 dims,
                 float** part_out, int* units_out, LazyClose* lazy, float* h1_side, const ConvDone* h1_done) {
  Arena* ws = r.ws;
  CD_REQUIRE(c0 + c1 == w.cin, "internal: resnet block input width mismatch");
  const int64_t vox = dims.vox();
  const int G = r.groups;
  int u1 = 0, u2 = 0;
  static const bool defer_gn = getenv("CD_NO_GNDEFER") == nullptr;  // consumers fold the GroupNorm coefficients (gn_defer.h)
  float* h1 = h1_done ? h1_done->h1 : (h1_side ? h1_side : ws->get<float>((size_t)r.B * vox * w.cout));
  // a 32-channel block on a grid of <= 128 voxels is ONE launch (kernels_conv_small.hip): decided below, once the shortcut exists
  const bool whole = vox <= 128 && w.cout == 32 && defer_gn && conv_precision() == PREC_F16X2 && w.c1w3 && w.c2w3;
  float* p1 = nullptr;
  CD_REQUIRE(!h1_side || (!whole && c1 > 0), "internal: a side conv belongs to a concat conv on a full-resolution grid");
  CD_REQUIRE(!h1_done || (!whole && !h1_side && c1 == 0), "internal: a finished first conv belongs to a single-input block on a full-resolution grid");
  if (h1_done) { p1 = h1_done->part; u1 = h1_done->units; }
  else if (h1_side) p1 = conv3_x_half_with_stats(r, x0, c0, c1, w.c1w3, h1, w.cout, dims, &u1);
  else if (!whole) p1 = conv3_with_stats(r, x0, c0, x1, c1, w.c1w, w.c1w3, w.c1b, h1, w.cout, dims, nullptr, &u1);
  else p1 = ws->get<float>((size_t)r.B * ((vox + 31) / 32) * w.cout * 2);  // (same block as conv3_with_stats would take)
  float* coef1 = ws->get<float>((size_t)r.B * w.cout * 4);
  GnDefer d1;
  d1.part = p1; d1.units = u1; d1.gamma = w.n1g; d1.beta = w.n1b; d1.add = w.emb; d1.add_ld = w.emb_ld; d1.C = w.cout; d1.groups = G;
  d1.vox = vox;
  if (!r.dry() && !defer_gn) launch_gn_finalize(p1, u1, w.n1g, w.n1b, w.emb, w.emb_ld, coef1, r.B, w.cout, G, vox, r.s);
  float* h2 = ws->get<float>((size_t)r.B * vox * w.cout);
  // Grids of at most 128 voxels (one workgroup sees a whole sample, kernels_conv_small.hip): the second conv closes the block
  // itself -- GroupNorm, SiLU, shortcut -- so the shortcut has to exist before it runs.
  const bool small = vox <= 128;
  float* po = nullptr;
  // A block whose shortcut is a 1x1 conv (models.py:200) is closed BY that conv (PointwiseArgs::gn_res): after the second conv it
  // computes shortcut + silu(gn(h2)) in one pass -- the shortcut tensor and the elementwise pass over the grid never exist.
  const bool no_pw_close = getenv("CD_NO_PW_CLOSE") != nullptr;  // (read per call: the parity test switches it in one process)
  const bool pw_close = w.has_res && !small && defer_gn && !no_pw_close && w.cout <= 128;
  // partials per sample of the block's output: those of whichever kernel closes it (1 if the second conv does)
  const int bps = pw_close ? pointwise_units(vox) : gn_apply_blocks_per_sample(r.B, w.cout, vox);
  if (part_out) {
    po = ws->get<float>((size_t)r.B * bps * w.cout * 2);
    *part_out = po;
  }
  float* res = nullptr;
  auto shortcut_conv = [&](const GnDefer* close = nullptr) {
    if (!close) res = ws->get<float>((size_t)r.B * vox * w.cout);
    if (!r.dry()) {
      PointwiseArgs a;
      a.in0 = x0; a.ld0 = c0; a.off0 = 0; a.c0 = c0; a.in1 = x1; a.ld1 = c1; a.c1 = c1;
      a.wpk = w.rw; a.bias = w.rb; a.out = close ? h2 : res; a.batch = r.B; a.cout = w.cout; a.vox = vox;
      if (conv_precision() == PREC_F16X2 && !getenv("CD_PW_F32")) { a.wpk16 = w.rw16; a.status = r.status; }  // (fp16 pipe, under the range fallback)
      if (close) { a.gn_res = h2; a.gn_defer = *close; a.ch_part = po; }
      launch_pointwise(a, r.s);
    }
  };
  if (small && w.has_res) shortcut_conv();
  int fused = 0;
  if (whole && !r.dry()) {
    const float* sc0 = w.has_res ? res : x0;
    const float* sc1 = w.has_res ? nullptr : (c1 ? x1 : nullptr);
    if (try_launch_res_block_small(x0, c0, x1, c1, (const char*)w.c1w3 + packed_bf16x3_bytes(c0 + c1, 32, 27), w.c1b, w.n1g, w.n1b,
                                   w.emb, w.emb_ld, (const char*)w.c2w3 + packed_bf16x3_bytes(32, 32, 27), w.c2b, w.n2g, w.n2b, G, sc0,
                                   sc1, w.has_res ? 0 : c0, h1, h2, po, r.B, w.cout, dims, r.status, r.s))
      fused = 2;
    else
      p1 = (ws->release(p1), conv3_with_stats(r, x0, c0, x1, c1, w.c1w, w.c1w3, w.c1b, h1, w.cout, dims, nullptr, &u1));
  }
  ConvFusion::GnOut go;
  if (small && defer_gn && fused != 2) {
    go.gamma = w.n2g; go.beta = w.n2b; go.groups = G; go.part_out = po; go.done = &fused;
    if (w.has_res) { go.res0 = res; }
    else { go.res0 = x0; go.res1 = c1 ? x1 : nullptr; go.res_c0 = c0; }
  }
  float* p2 = nullptr;
  if (fused == 2) p2 = ws->get<float>((size_t)r.B * ((vox + 31) / 32) * w.cout * 2);  // (conv2 ran inside the block launch)
  else p2 = conv3_with_stats(r, h1, w.cout, nullptr, 0, w.c2w, w.c2w3, w.c2b, h2, w.cout, dims, coef1, &u2, defer_gn ? &d1 : nullptr,
                             coef1, go.gamma ? &go : nullptr);
  ws->release(p1);
  ws->release(h1);
  ws->release(coef1);
  float* coef2 = ws->get<float>((size_t)r.B * w.cout * 4);
  GnDefer d2;
  d2.part = p2; d2.units = u2; d2.gamma = w.n2g; d2.beta = w.n2b; d2.C = w.cout; d2.groups = G; d2.vox = vox;
  if (!r.dry() && !defer_gn) launch_gn_finalize(p2, u2, w.n2g, w.n2b, nullptr, 0, coef2, r.B, w.cout, G, vox, r.s);
  const GnDefer* dp2 = defer_gn ? &d2 : nullptr;
  if (part_out) *units_out = fused ? 1 : bps;
  if (pw_close) {
    shortcut_conv(&d2);
  } else if (w.has_res) {
    if (!res) shortcut_conv();
    if (!r.dry() && !fused) launch_gn_apply(h2, h2, coef2, r.B, w.cout, vox, 1, res, nullptr, 0, po, r.s, dp2);
    ws->release(res);
  } else if (lazy && !small && defer_gn && c1 == 0 && w.cout == 32 && !part_out) {
    lazy->gn = d2;
    lazy->part = p2;
    lazy->on = true;
    ws->release(coef2);
    return h2;
  } else {
    // identity shortcut; for a concatenated input it is read from the two sources (models.py:200,741)
    if (!r.dry() && !fused) launch_gn_apply(h2, h2, coef2, r.B, w.cout, vox, 1, x0, c1 ? x1 : nullptr, c0, po, r.s, dp2);
  }
  ws->release(p2);
  ws->release(coef2);
  return h2;
}

// Residual(PreNorm(LinearAttention)) (models.py:111-117, 281-329).  xpart/xunits: channel partials of x if its producer
// emitted them (else a stats pass runs here).
float* attn_block(Run& r, const AttnP& w, const float* x, Dims3 dims, float* xpart, int xunits) {
  Arena* ws = r.ws;
  const int64_t vox = dims.vox();
  const int C = w.c;
  float* own = nullptr;
  if (!xpart) {
    own = stats_pass(r, x, C, vox, &xunits);
    xpart = own;
  }
  // The fused kernels run every product on the fp16 pipe (f16x2 splits: fp16 RANGE); the full-range precisions (bf16x3 / f32,
  // and with them the re-run of a range fallback) take the unfused form on the f32-input MFMA instead.
  static const bool no_fused_env = getenv("CD_NO_FUSED_ATTN") != nullptr;
  static const bool defer_env = getenv("CD_NO_GNDEFER") == nullptr;
  const bool no_fused = no_fused_env || conv_precision() != PREC_F16X2;
  const bool defer_gn = defer_env && !no_fused;  // consumers fold the coefficients (gn_defer.h)
  float* coefn = ws->get<float>((size_t)r.B * C * 4);
  GnDefer dn;
  dn.part = xpart; dn.units = xunits; dn.gamma = w.ng; dn.beta = w.nb; dn.C = C; dn.groups = 1; dn.vox = vox;
  const GnDefer* dnp = defer_gn ? &dn : nullptr;
  if (!r.dry() && !defer_gn) launch_gn_finalize(xpart, xunits, w.ng, w.nb, nullptr, 0, coefn, r.B, C, 1, vox, r.s);
  const int CT = (C + 31) / 32;
  float* y = nullptr;
  float* ypart = nullptr;
  int yu = 0;
  // grids of a few hundred voxels: the whole block -- both passes, the closing GroupNorm and the residual -- in one launch
  const bool single = !no_fused && defer_gn && attn_small_eligible(vox);
  bool moments = false;
  if (!no_fused) {
    // fused path (kernels_attn.hip): x -> {max, sum, context} partials -> per-sample folded W_out -> y; qkv never exists
    const int nsp = attn_fused_nsplit_for(vox, r.B);
    const int cap = single && nsp < 4 ? 4 : nsp;  // (the single-launch form may deal a sample to up to 4 co-operating workgroups)
    float* part = ws->get<float>(attn_partial_floats(r.B, cap));
    // Moment form (kernels_attn.hip): pass 1 also accumulates the moments of softmax(q), pass 2 then knows the closing GroupNorm's
    // statistics in closed form and writes gn(y) + x itself -- y is never written and the gn_apply pass below does not run
    // (read per call: the parity test switches it in one process)
    static const bool sep_combine = getenv("CD_ATTN_COMBINE_LAUNCH") != nullptr;  // A/B: the separate combine launch
    // It costs pass 1 ~40 % more per tile and both passes a few microseconds of prologue / epilogue, and saves a pass that moves
    // 3 B vox C floats: it pays from ~4 M elements per tensor (same-box A/B: Dataset-2 level 0, 13 M, +1.4 %; Dataset-3, 41 M,
    // +1.8 %; HGCal at batch 16, 3.6 M, -0.3 %)
    const char* mom_env = getenv("CD_ATTN_MOM_MIN");  // (read per call, like the switch: the parity test sets it)
    const int64_t mom_min = mom_env ? atoll(mom_env) : (4ll << 20);
    moments = !single && !sep_combine && defer_gn && attn_moments_eligible(C) && (vox * C) % 4 == 0 && (int64_t)r.B * vox * C >= mom_min &&
              getenv("CD_NO_ATTN_MOMENTS") == nullptr;
    float* momb = moments ? ws->get<float>(attn_moment_floats(r.B, nsp)) : nullptr;
    float* wpb = ws->get<float>((size_t)r.B * CT * 1024);
    y = ws->get<float>((size_t)r.B * vox * C);
    yu = nsp;
    ypart = ws->get<float>((size_t)r.B * cap * C * 2);
    if (!r.dry() && single) {
      launch_attn_small(x, C, coefn, w.qkv16, part, w.ow, kAttnScale, w.ob, w.gg, w.gb, y, ypart, r.B, vox,
                        r.s, dnp, r.status, cap, w.coop_sync);
    } else if (!r.dry()) {
      launch_attn_kv_context(x, C, coefn, w.qkv16, part, r.B, vox, nsp, r.s, dnp, r.status, momb);
      if (sep_combine) {
        launch_attn_combine(part, nsp, w.ow, C, wpb, r.B, kAttnScale, r.s, nullptr, nullptr, true);
        launch_attn_out(x, C, coefn, w.qkv16, wpb, w.ob, y, ypart, r.B, vox, nsp, r.s, dnp, nullptr, nullptr, 0.f, r.status);
      } else {
        launch_attn_out(x, C, coefn, w.qkv16, nullptr, w.ob, y, moments ? nullptr : ypart, r.B, vox, nsp, r.s, dnp, part, w.ow,
                        kAttnScale, r.status, momb, w.gg, w.gb);
      }
    }
    if (momb) ws->release(momb);
    if (own) ws->release(own);
    own = nullptr;
    ws->release(coefn);
    ws->release(part);
    ws->release(wpb);
  } else {
    float* qkv = ws->get<float>((size_t)r.B * vox * 96);
    // (coefn's block is free for the requests below: only the first launch of the sequence reads the table, and the launches that
    // write what may then lie there follow it on the stream)
    ws->release(coefn);
    const int nsp = attn_nsplit_for(vox, r.B);
    float* part = ws->get<float>(attn_partial_floats(r.B, nsp));
    float* wpb = ws->get<float>((size_t)r.B * CT * 1024);
    y = ws->get<float>((size_t)r.B * vox * C);
    yu = pointwise_units(vox);
    ypart = ws->get<float>((size_t)r.B * yu * C * 2);
    if (!r.dry()) launch_attn_unfused(x, C, coefn, w.qkv, w.ow, w.ob, qkv, part, nsp, wpb, y, ypart, r.B, vox, r.s);
    ws->release(part);
    ws->release(wpb);
    ws->release(qkv);
}
  if (own) ws->release(own);
  float* coefg = ws->get<float>((size_t)r.B * C * 4);
  if (!r.dry() && !single && !moments) {
    GnDefer dg;
    dg.part = ypart; dg.units = yu; dg.gamma = w.gg; dg.beta = w.gb; dg.C = C; dg.groups = 1; dg.vox = vox;
    if (!defer_gn) launch_gn_finalize(ypart, yu, w.gg, w.gb, nullptr, 0, coefg, r.B, C, 1, vox, r.s);
    launch_gn_apply(y, y, coefg, r.B, C, vox, 0, x, nullptr, 0, nullptr, r.s, defer_gn ? &dg : nullptr);
  }
  ws->release(ypart);
  ws->release(coefg);
  return y;
}

// Descriptor of the deepest level for the one-launch form (kernels_deep.hip); false if the level does not qualify.
bool deep_level_desc(const CdPlan* p, const float* emb, DeepLevelDesc* out) {
  const CdUnetDesc& d = p->desc;
  const int nres = p->nres;
  if (conv_precision() != PREC_F16X2) return false;  // (the full-range precisions keep the per-op kernels)
  DeepLevelDesc L;
  L.dims = p->shapes[nres - 1];
  L.Ca = d.layer_sizes[nres - 1]; L.Cb = d.layer_sizes[nres]; L.groups = d.groups;
  const ResW* rw[6] = {&p->downs[nres - 1].r1, &p->downs[nres - 1].r2, &p->mid1, &p->mid2, &p->ups[0].r1, &p->ups[0].r2};
  for (int i = 0; i < 6; ++i) {
    const ResW& w = *rw[i];
    DeepLevelDesc::Res& r = L.res[i];
    const bool cat = i == 4;  // ups r1 reads cat(x, skip): two Cb-wide halves
    r.c0 = cat ? L.Cb : w.cin; r.c1 = cat ? w.cin - L.Cb : 0; r.cout = w.cout;
    if (!p->packed3(w.c1w) || !p->packed3(w.c2w)) return false;
    r.w1 = (const char*)p->packed3(w.c1w) + packed_bf16x3_bytes(w.cin, w.cout, 27);
    r.w2 = (const char*)p->packed3(w.c2w) + packed_bf16x3_bytes(w.cout, w.cout, 27);
    r.b1 = p->raw(w.c1b); r.b2 = p->raw(w.c2b); r.g1 = p->raw(w.n1g); r.be1 = p->raw(w.n1b); r.g2 = p->raw(w.n2g); r.be2 = p->raw(w.n2b);
    if (w.has_mlp && emb) { r.emb = emb + w.emb_off; r.emb_ld = p->emb_ld; }
    if (w.has_res) {
      if (!p->packed3(w.rw)) return false;
      r.wres = (const char*)p->packed3(w.rw) + packed_bf16x3_bytes(w.cin, w.cout, 1);
      r.bres = p->raw(w.rb);
    }
  }
  const AttnW* aw[3] = {&p->downs[nres - 1].attn, &p->mid_attn, &p->ups[0].attn};
  const bool on[3] = {d.block_attn != 0, d.mid_attn != 0, d.block_attn != 0};
  for (int i = 0; i < 3; ++i) {
    L.has_attn[i] = on[i] ? 1 : 0;
    if (!on[i]) continue;
    const AttnW& w = *aw[i];
    DeepLevelDesc::Attn& a = L.attn[i];
    a.C = w.c; a.ng = p->raw(w.ng); a.nb = p->raw(w.nb); a.wout = p->raw(w.ow); a.bout = p->raw(w.ob); a.gg = p->raw(w.gg); a.gb = p->raw(w.gb);
    if (!p->packed3(w.qkv)) return false;
    a.wqkv = (const char*)p->packed3(w.qkv) + packed_bf16x3_bytes(w.c, 96, 1);
  }
  if (L.res[0].c0 != L.Ca || L.res[0].cout != L.Cb || L.res[4].cout != L.Ca || L.res[4].c1 != L.Cb || L.res[5].cout != L.Ca) return false;
  if (!deep_level_eligible(L)) return false;
  *out = L;
  return true;
}

// CondUnet.forward after init_conv / embeddings (models.py:713-748). Takes ownership of h (a workspace block).
// `lazy`: see res_block -- when set on return, the result is the final block's raw conv output, *xin its (still allocated) input.
// `first` (optional): downs[0]'s first block's first conv, already computed (res_block's h1_done).
float* unet_body(CdPlan* p, Run& r, const float* emb, float* h, LazyClose* lazy = nullptr, float** xin = nullptr,
                 const ConvDone* first = nullptr) {
  const CdUnetDesc& d = p->desc;
  const int nres = p->nres;
  const int zs = d.compress_z ? 2 : 1;
  std::vector<float*> skips(nres, nullptr);
  float* x = h;
  int cx = d.layer_sizes[0];
  // The deepest level (downs[-1], the mid blocks, ups[0] up to its transposed conv) as ONE launch where a sample is <= 128 voxels
  DeepLevelDesc deep;
  const bool deep_on = deep_level_desc(p, emb, &deep);
  // ... and, in the same launch, on the CUs that level leaves idle: the skip half of the first conv of level 0's first up-block,
  // conv(cat(x, skips[0])) -- skips[0] is final long before, x only after everything below level 0 (kernels_deep_side.hip).  The
  // conv's output is allocated here, the x half is added by res_block when it gets there.  Anything not eligible (and the training
  // tape, the VJP and the full-range precisions, none of which come through here with deep_on) runs the conv whole, as before.
  const ResW& side_w = p->ups[nres - 1].r1;
  const int side_c = nres >= 2 ? d.layer_sizes[1] : 0;
  const bool side_on = deep_on && nres >= 2 && side_w.cin == 2 * side_c && p->packed3(side_w.c1w) &&
                       deep_side_conv_chunks(r.B, side_c, side_w.cout, p->shapes[0]) > 0;
  float* side_h1 = nullptr;
  for (int i = 0; i < nres; ++i) {
    const Dims3 dims = p->shapes[i];
    if (deep_on && i == nres - 1) {
      float* y = r.ws->get<float>((size_t)r.B * dims.vox() * cx);
      if (side_on) {
        side_h1 = r.ws->get<float>((size_t)r.B * p->shapes[0].vox() * side_w.cout);
        if (!r.dry()) {
          DeepSideConv sc;
          sc.in = skips[0]; sc.ldc = side_c; sc.cin = side_c;
          // f16x2 image [k-step][tap][ct][term][lane] x 16 B: the skip channels are k-steps side_c / 16 onwards
          sc.wpk = (const char*)p->packed3(side_w.c1w) + packed_bf16x3_bytes(side_w.cin, side_w.cout, 27) +
                   (size_t)(side_c / 16) * 27 * (side_w.cout / 32) * 128 * 16;
          sc.bias = p->raw(side_w.c1b); sc.out = side_h1; sc.cout = side_w.cout; sc.dims = p->shapes[0];
          launch_deep_level_side(deep, x, y, r.B, r.status, sc, r.s);
        }
      } else if (!r.dry()) {
        launch_deep_level(deep, x, y, r.B, r.status, r.s);
      }
      r.ws->release(x);
      x = y;
      break;
    }
    float* t = res_block(r, resolve(p, p->downs[i].r1, emb), x, cx, nullptr, 0, dims, nullptr, nullptr, nullptr, nullptr,
                         i == 0 ? first : nullptr);
    r.ws->release(x);
    x = t; cx = p->downs[i].r1.cout;
    float* xp = nullptr;
    int xu = 0;
    t = res_block(r, resolve(p, p->downs[i].r2, emb), x, cx, nullptr, 0, dims, d.block_attn ? &xp : nullptr, &xu);
    r.ws->release(x);
    x = t;
    if (d.block_attn) {
      t = attn_block(r, resolve(p, p->downs[i].attn), x, dims, xp, xu);
      r.ws->release(xp);
      r.ws->release(x);
      x = t;
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
      x = y;
    } else {
      // Identity: the last level's skip and the running tensor are the same tensor (models.py:719-720)
      x = skips[i];
    }
  }
  const Dims3 md = p->shapes[nres - 1];
  float* t = nullptr;
  if (!deep_on) {
    float* mp = nullptr;
    int mu = 0;
    t = res_block(r, resolve(p, p->mid1, emb), x, cx, nullptr, 0, md, d.mid_attn ? &mp : nullptr, &mu);
    // x aliases skips[nres-1]: keep it alive for the concat
    x = t;
    if (d.mid_attn) {
      t = attn_block(r, resolve(p, p->mid_attn), x, md, mp, mu);
      r.ws->release(mp);
      r.ws->release(x);
      x = t;
    }
    t = res_block(r, resolve(p, p->mid2, emb), x, cx, nullptr, 0, md);
    r.ws->release(x);
    x = t;
  }

  for (int i = 0; i < nres; ++i) {
    const int lv = nres - 1 - i;
    const Dims3 dims = p->shapes[lv];
    const int cs = d.layer_sizes[lv + 1];  // width of the skip (and of x after the previous stage)
    if (!(deep_on && i == 0)) {  // (the deep-level launch already ran ups[0]'s blocks: x is their output, layer_sizes[lv] wide)
      CD_REQUIRE(cx == cs, "internal: up path width mismatch");
      t = res_block(r, resolve(p, p->ups[i].r1, emb), x, cx, skips[lv], cs, dims, nullptr, nullptr, nullptr,
                    lv == 0 ? side_h1 : nullptr);
      r.ws->release(x);
      r.ws->release(skips[lv]);
      x = t; cx = p->ups[i].r1.cout;
      float* up = nullptr;
      int uu = 0;
      t = res_block(r, resolve(p, p->ups[i].r2, emb), x, cx, nullptr, 0, dims, d.block_attn ? &up : nullptr, &uu);
      r.ws->release(x);
      x = t;
      if (d.block_attn) {
        t = attn_block(r, resolve(p, p->ups[i].attn), x, dims, up, uu);
        r.ws->release(up);
        r.ws->release(x);
        x = t;
      }
    }
    if (i + 1 < nres) {
      const Dims3 od = p->up_out[i];
      float* y = r.ws->get<float>((size_t)r.B * od.vox() * cx);
      if (!r.dry())
        launch_conv_transpose_mfma(x, cx, p->packed(p->ups[i].sw), p->raw(p->ups[i].sb), y, r.B, cx, dims, od, p->up_kz[i], zs, r.s,
                                   p->packed3(p->ups[i].sw), r.status);
      r.ws->release(x);
      x = y;
    }
  }
  t = res_block(r, resolve(p, p->fin, nullptr), x, cx, nullptr, 0, p->shapes[0], nullptr, nullptr, lazy);
  if (lazy && lazy->on) *xin = x;  // (the head reads it as the shortcut; released by the caller)
  else r.ws->release(x);
  return t;
}

EmbedArgs embed_args(CdPlan* p, int B, const float* cond, const float* t, int kind, float* emb, float* scal) {
  const CdUnetDesc& d = p->desc;
  EmbedArgs e;
  e.cond = cond; e.time_or_sigma = t; e.time_kind = kind; e.sigma_data = d.sigma_data;
  e.cond_size = d.cond_size; e.half = d.cond_dim / 2;
  e.cond_hidden = d.cond_size > e.half / 2 ? d.cond_size : e.half / 2;
  e.time_sin = d.time_sin; e.cond_sin = d.cond_sin;
  e.tw1 = d.time_sin ? nullptr : p->raw(p->tw[0]); e.tb1 = d.time_sin ? nullptr : p->raw(p->tb[0]);
  e.tw2 = p->raw(p->tw[1]); e.tb2 = p->raw(p->tb[1]);
  e.tw3 = p->raw(p->tw[2]); e.tb3 = p->raw(p->tb[2]);
  e.cw1 = d.cond_sin ? nullptr : p->raw(p->cw[0]); e.cb1 = d.cond_sin ? nullptr : p->raw(p->cb[0]);
  e.cw2 = p->raw(p->cw[1]); e.cb2 = p->raw(p->cb[1]);
  e.cw3 = p->raw(p->cw[2]); e.cb3 = p->raw(p->cb[2]);
  e.layers = p->d_embed_layers; e.n_layers = p->n_embed_layers; e.emb = emb; e.emb_ld = p->emb_ld; e.scal = scal; e.batch = B;
  return e;
}

// shared by cd_unet_forward (raw = true) and cd_denoise; workspace must have been reset by the caller
void forward_impl(CdPlan* p, int B, const float* x, const float* cond, const float* t, float* out, bool raw, hipStream_t s,
                  const FwdOpts* opt) {
  const CdUnetDesc& d = p->desc;
  const Dims3 dims = p->shapes[0];
  Run r{&p->ws, s, B, d.groups};
  r.status = p->status_word;
  const bool pre = opt && opt->emb_pre;
  float* emb = pre ? opt->emb_pre : p->ws.get<float>((size_t)B * p->emb_ld);
  float* scal = pre ? opt->scal_pre : p->ws.get<float>((size_t)B * 4);
  float* h = p->ws.get<float>((size_t)B * dims.vox() * d.layer_sizes[0]);
  // flat-state embedding (cd_plan_set_radial / cd_plan_set_geom): x and out are (B, V); the network runs on g_in = enc(c_in x) and leaves its raw
  // output on the grid, which embed-out decodes and combines with x
  const CdPlan::FlatEmbed* fe = raw ? nullptr : p->flat();
  float* g_in = fe ? p->ws.get<float>((size_t)B * dims.vox()) : nullptr;
  float* f_grid = fe ? p->ws.get<float>((size_t)B * dims.vox()) : nullptr;
  if (!r.dry()) {
    // (running this launch beside the init conv on a second stream was measured: no gain inside the step graph)
    if (!pre) launch_embed(embed_args(p, B, cond, t, raw ? CD_TIME_RAW : d.time_embed_kind, emb, raw ? nullptr : scal), s);
    if (fe) launch_embed_in(*fe, x, scal, g_in, B, s);
    InitConvArgs a;
    a.x = fe ? g_in : x; a.cin = d.in_channels; a.wpk = p->packed(p->init_w); a.bias = p->raw(p->init_b); a.out = h; a.batch = B;
    a.cout = d.layer_sizes[0]; a.dims = dims;
    if (raw) {
      a.cx = d.in_channels;
    } else {
      a.cx = 1; a.sigma_b = fe ? nullptr : t; a.sigma_data = d.sigma_data; a.use_rz = d.rz_input; a.use_phi = d.phi_input;  // (g_in carries c_in)
      a.r_w = p->d_coords; a.z_d = p->d_coords + d.grid[2]; a.phi_h = p->d_coords + d.grid[2] + d.grid[0];
      a.coord_table = p->d_init_table; a.table_ready = true; a.status = r.status;
    }
    launch_init_conv(a, s);
  }
  // The first block's first conv reads h with nothing non-linear in between: in the denoise form (one data channel, the coordinate
  // table) it runs composed with the init conv as a one-channel 5x5x5 conv of c_in x (kernels_init_pair.hip).  h itself is still
  // needed, as the block's shortcut.  Geometry and widths decide (build_plan: d_pair_w), never the batch; the full-range precisions
  // (and with them a range fallback's re-run), cd_unet_forward, the training tape and the VJP keep the chained convs.  The two
  // blocks are the ones res_block would take next, in its order: the workspace sequence is the same in both forms.
  // (CD_NO_INIT_PAIR read per call: the parity test switches it in one process)
  ConvDone pair;
  const bool pair_on = !raw && p->d_pair_w && p->init_pair_ready && conv_precision() == PREC_F16X2 && getenv("CD_NO_INIT_PAIR") == nullptr;
  if (pair_on) {
    pair.h1 = p->ws.get<float>((size_t)B * dims.vox() * 32);
    pair.part = p->ws.get<float>((size_t)B * ((dims.vox() + 31) / 32) * 32 * 2);  // (units <= D <= ceil(vox / 32): build_plan)
    if (!r.dry()) {
      InitPairArgs ia;
      ia.x = fe ? g_in : x; ia.sigma_b = fe ? nullptr : t; ia.sigma_data = d.sigma_data;  // (g_in carries c_in)
      ia.wc = p->d_pair_w; ia.table = p->d_pair_table; ia.out = pair.h1; ia.ch_part = pair.part; ia.batch = B; ia.dims = dims;
      ia.status = r.status;
      launch_init_pair_conv(ia, &pair.units, s);
    }
  }
  LazyClose lazy;
  float* xin = nullptr;
  static const bool head_fused = getenv("CD_NO_HEAD_GN") == nullptr;
  float* hf = unet_body(p, r, emb, h, head_fused ? &lazy : nullptr, &xin, pair_on ? &pair : nullptr);
  if (!r.dry()) {
    HeadArgs ha;
    ha.h = hf; ha.w = p->raw(p->head_w); ha.bias = p->raw(p->head_b); ha.out = fe ? f_grid : out; ha.batch = B; ha.vox = dims.vox();
    if (!raw && !fe) { ha.x = x; ha.scal = scal; ha.objective = d.objective; }
    if (lazy.on) { ha.defer = lazy.gn; ha.res = xin; }
    if (opt && opt->upd && !fe) {
      ha.upd_stepvals = opt->upd->upd_stepvals; ha.upd_noise = opt->upd->upd_noise; ha.upd_x_next = opt->upd->upd_x_next;
      ha.upd_xs = opt->upd->upd_xs; ha.upd_x0s = opt->upd->upd_x0s;
    }
    launch_head(ha, s);
    // (the sampler's fused update moves with the combination: it acts on the flat state)
    if (fe) launch_embed_out(*fe, f_grid, x, scal, d.objective, out, opt ? opt->upd : nullptr, B, s);
  }
  if (fe) {
    r.ws->release(f_grid);
    r.ws->release(g_in);
  }
  if (lazy.on) {
    r.ws->release(lazy.part);
    r.ws->release(xin);
  }
  r.ws->release(hf);
  if (!pre) {
    r.ws->release(scal);
    r.ws->release(emb);
  }
}

}  // namespace cd

extern "C" {

int cd_plan_workspace_bytes(CdPlan* plan, int batch, size_t* bytes) {
  return guarded([&] {
    CD_REQUIRE(plan && bytes && batch > 0, "bad argument");
    const int64_t n = (int64_t)batch * plan->state_per();
    *bytes = dry_forward_bytes(plan, batch, [&] {
      // superset of what any entry point allocates around forward_impl: x0 / noise / x_noisy, sigma, partials
      plan->ws.get<float>((size_t)n);
      plan->ws.get<float>((size_t)n);
      plan->ws.get<float>((size_t)batch + 64);
      plan->ws.get<double>((size_t)batch + 8);
      // cd_ddim_sample: this step's embeddings / scalings and the chunk computed ahead
      plan->ws.get<float>((size_t)batch * plan->emb_ld);
      plan->ws.get<float>((size_t)batch * 4);
      plan->ws.get<float>((size_t)CdPlan::kEmbedChunk * batch * plan->emb_ld);
      plan->ws.get<float>((size_t)CdPlan::kEmbedChunk * batch * 4);
    }) + 4096;
  });
}

int cd_unet_forward(CdPlan* plan, int batch, const float* x, const float* cond, const float* time, float* out,
                    void* workspace, size_t workspace_bytes, void* stream) {
  return guarded([&] {
    CD_REQUIRE(plan && x && cond && time && out && workspace && batch > 0, "bad argument");
    check_ready(plan, false);
    plan->ws.reset((char*)workspace, workspace_bytes, false);
    forward_impl(plan, batch, x, cond, time, out, true, (hipStream_t)stream);
  });
}

int cd_denoise(CdPlan* plan, int batch, const float* x, const float* sigma, const float* cond, float* out,
               void* workspace, size_t workspace_bytes, void* stream) {
  return guarded([&] {
    CD_REQUIRE(plan && x && sigma && cond && out && workspace && batch > 0, "bad argument");
    check_ready(plan, true);
    plan->ws.reset((char*)workspace, workspace_bytes, false);
    forward_impl(plan, batch, x, cond, sigma, out, false, (hipStream_t)stream);
  });
}

int cd_denoise_safe(CdPlan* plan, int batch, const float* x, const float* sigma, const float* cond, float* out,
                    void* workspace, size_t workspace_bytes, int* fell_back, void* stream) {
  return guarded([&] {
    CD_REQUIRE(plan && x && sigma && cond && out && workspace && batch > 0, "bad argument");
    check_ready(plan, true);
    const bool fb = run_with_range_fallback(plan, (hipStream_t)stream, [&](bool) {
      plan->ws.reset((char*)workspace, workspace_bytes, false);
      forward_impl(plan, batch, x, cond, sigma, out, false, (hipStream_t)stream);
    }, /*report_sticky=*/fell_back == nullptr);
    if (fell_back) *fell_back = fb ? 1 : 0;
  });
}

int cd_loss_hybrid_l2(CdPlan* plan, int batch, const float* data, const float* noise, const float* sigma,
                      const float* cond, double* loss_out, void* workspace, size_t workspace_bytes, void* stream) {
  return cd_loss_hybrid(plan, batch, data, noise, sigma, cond, CD_LOSS_L2, loss_out, workspace, workspace_bytes, stream);
}

int cd_loss_hybrid(CdPlan* plan, int batch, const float* data, const float* noise, const float* sigma, const float* cond,
                   int loss_type, double* loss_out, void* workspace, size_t workspace_bytes, void* stream) {
  return guarded([&] {
    CD_REQUIRE(plan && data && noise && sigma && cond && loss_out && workspace && batch > 0, "bad argument");
    CD_REQUIRE(loss_type >= CD_LOSS_L2 && loss_type <= CD_LOSS_HUBER, "loss_type must be one of CD_LOSS_L2 / L1 / MSE / HUBER");
    check_ready(plan, true);
    hipStream_t s = (hipStream_t)stream;
    const int64_t per = plan->state_per();
    const int64_t n = (int64_t)batch * per;
    plan->ws.reset((char*)workspace, workspace_bytes, false);
    float* xn = plan->ws.get<float>((size_t)n);
    float* x0 = plan->ws.get<float>((size_t)n);
    double* part = plan->ws.get<double>((size_t)batch + 8);
    const size_t used = plan->ws.high();
    launch_axpy_sigma(data, noise, sigma, xn, batch, per, s);
    plan->ws.reset((char*)workspace + used, workspace_bytes > used ? workspace_bytes - used : 0, false);
    forward_impl(plan, batch, xn, cond, sigma, x0, false, s);
    launch_loss_partial(x0, data, noise, sigma, part, batch, per, s, loss_type, plan->desc.objective);
    launch_loss_final(part, sigma, loss_out, batch, per, s, loss_type, plan->desc.objective);
  });
}

}  // extern "C"
