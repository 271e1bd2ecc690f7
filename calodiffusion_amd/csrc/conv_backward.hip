// Backward of the convolutions as launch sequences (the training step, cd_denoise_vjp and the op primitives share them): the
// input gradient on the forward conv kernels with re-packed weights, the weight gradient (launch_wgrad, kernels_wgrad.hip) and the
// bias gradient.  Reference: torch autograd through CylindricalConv / CylindricalConvTrans, models.py:25-96.
#include "plan_internal.h"

namespace cd {

// per-channel sums of a (B, vox, C) tensor over batch and voxels -> db (bias gradients)
void bias_grad(Run& r, const float* dy, int C, int64_t vox, float* db) {
  int units = 0;
  float* part = stats_pass(r, dy, C, vox, &units);
  if (!r.dry()) launch_bias_grad(part, units, r.B, C, db, false, r.s);
  r.ws->release(part);
}

// Backward of a phi-periodic Conv3d y = conv(cat(x0, x1), w) + b  (3x3x3 stride 1, 1x1x1, or the (3,4,4) strided conv).
//   dx (optional): (B, vox_in, c0+c1) gradient of the concatenated input
//   dw: torch layout (cout, c0+c1, taps);  db: (cout) or null.   w_raw: torch-layout weights (device).
// img (optional): the input gradient's weight images already packed for this step (CdPlan::dg); without them they are packed here.
// xcoef (optional, single-source x0 only): the conv's input was silu(coef[0] x0 + coef[1]) + coef[2] (see launch_wgrad)
// dy_max (optional): max |dy| in a device word (the GroupNorm backward that wrote dy filled it); else measured here where needed
void conv_backward(Run& r, const float* x0, int c0, const float* x1, int c1, const float* w_raw, const float* dy, float* dx,
                   float* dw, float* db, int cout, const ConvGeom& g, const DgImg* img, const float* xcoef,
                   // dx = (input gradient) + dx_add, a tensor shaped like dx, where the kernel that runs can add it in its
                   // epilogue (3x3x3 stride 1 on the fp16 pipe): *dx_added says whether it did
                   const float* dx_add, int* dx_added, const unsigned* dy_max) {
  Arena* ws = r.ws;
  const int cin = c0 + c1, T = g.kd * g.kh * g.kw;
  const bool pre = img && img->pk;
  if (dx) {
    if (T == 1) {
      float* wp = pre ? nullptr : ws->get<float>(packed_weight_floats(cout, cin, 1));
      if (!r.dry()) {
        if (!pre) launch_pack_weights(w_raw, wp, cin, cout, 1, true, r.s);
        PointwiseArgs a;
        a.in0 = dy; a.ld0 = cout; a.c0 = cout; a.wpk = pre ? img->pk : wp; a.out = dx; a.batch = r.B; a.cout = cin; a.vox = g.in.vox();
        launch_pointwise(a, r.s);
      }
      if (wp) ws->release(wp);
    } else if (g.sz == 1 && g.sh == 1 && g.sw == 1) {
      // dx = conv(dy, W^T flipped): the forward kernels with re-packed weights
      float* wp = pre ? nullptr : ws->get<float>(packed_weight_floats(cout, cin, T));
      float* wp3 = pre ? nullptr : ws->get<float>(packed_split16_bytes(cout, cin, T) / 4);
      if (!r.dry()) {
        if (!pre) {
          launch_pack_weights(w_raw, wp, cin, cout, T, true, r.s, true);
          launch_pack_weights_split16(w_raw, wp3, cin, cout, T, r.s, true, true);
        }
        ConvGeom gd{g.out, g.in, g.kd, g.kh, g.kw, 1, 1, 1};
        ConvFusion fu;
        fu.wpk_bf16x3 = pre ? img->pk3 : wp3;
        if (!dy_max) dy_max = launch_absmax_bits(dy, (size_t)r.B * g.out.vox() * cout, &r.amax, r.s);  // (serves the weight gradient too)
        fu.in_absmax = dy_max;
        fu.add_src = dx_add; fu.add_done = dx_added;
        launch_conv_mfma(dy, cout, nullptr, 0, pre ? img->pk : wp, nullptr, dx, r.B, cin, gd, r.s, fu);
      }
      if (wp3) ws->release(wp3);
      if (wp) ws->release(wp);
    } else if (g.in.h & 1) {
      // odd phi ring: the circular halo breaks the parity classes of the gather kernel (see kernels_conv_bwd.hip)
      if (!r.dry()) launch_strided_dgrad_naive(dy, w_raw, dx, r.B, cin, cout, g.in, g.out, g.kd, g.sz, r.s);
    } else {
      // strided conv: its adjoint is the transposed-conv gather kernel
      // (on the fp16 pipe like the forward up-conv, the tiny gradients rescaled by a power of two from their max)
      float* wp = pre ? nullptr : ws->get<float>(packed_weight_floats(cout, cin, T));
      float* wp16 = pre ? nullptr : ws->get<float>(packed_f16x2_bytes(cout, cin, T) / 4 + 64);
      if (!r.dry()) {
        if (!pre) {
          launch_pack_weights(w_raw, wp, cin, cout, T, true, r.s);
          launch_pack_weights_f16x2(w_raw, wp16, cin, cout, T, r.s, true, false);
        }
        if (!dy_max) dy_max = launch_absmax_bits(dy, (size_t)r.B * g.out.vox() * cout, &r.amax, r.s);
        launch_conv_transpose_mfma(dy, cout, pre ? img->pk : wp, nullptr, dx, r.B, cin, g.out, g.in, g.kd, g.sz, r.s,
                                   pre ? img->pk3 : wp16, r.status, dy_max);
      }
      if (wp16) ws->release(wp16);
      if (wp) ws->release(wp);
    }
  }
  if (!r.param_grads) return;
  CD_REQUIRE(!xcoef || !c1, "conv backward: a normalised input has one source");
  const float* xs[2] = {x0, x1};
  const int cs[2] = {c0, c1};
  for (int k = 0; k < 2 && cs[k]; ++k) {
    float* part = r.wgrad_part(wgrad_partial_floats(g.out.vox(), r.B, false, cout, cs[k], T));
    if (!r.dry()) {
      WgradOp op;
      op.g = dy; op.A = cout; op.x = xs[k]; op.Bc = cs[k]; op.xld = cs[k]; op.geom = g; op.batch = r.B; op.partial = part;
      op.dw = dw; op.b_total = cin; op.b_off = k ? c0 : 0; op.xcoef = xcoef; op.aux = r.wgrad_aux(dy_max);
      launch_wgrad(op, r.s);
    }
    r.release_wgrad_part(part);
  }
  if (db) bias_grad(r, dy, cout, g.out.vox(), db);
}

// Backward of the phi-periodic ConvTranspose3d (Upsample): y = convT(x, w) + b, w stored (cin, cout, kz, 4, 4)
void conv_transpose_backward(Run& r, const float* x, const float* w_raw, const float* dy, float* dx, float* dw, float* db, int c,
                             Dims3 din, Dims3 dout, int kz, int sz, const DgImg* img) {
  Arena* ws = r.ws;
  const int T = kz * 16;
  const bool pre = img && img->pk;
  const unsigned* dy_max = nullptr;  // (measured by the input gradient's conv; the weight gradient reads dy as its x operand)
  // Odd output phi extent (output_padding 1 along phi: Dataset-3 level 1, Dataset-1 grid): the forward's last phi row
  // duplicates row 0, so fold its gradient into row 0 and continue on the even ring (kernels_conv_bwd.hip: fold_phi_kernel).
  float* folded = nullptr;
  const float* dy_full = dy;
  const Dims3 dout_full = dout;
  if (dout.h & 1) {
    folded = ws->get<float>((size_t)r.B * dout.d * (dout.h - 1) * dout.w * c);
    if (!r.dry()) launch_fold_phi(dy, folded, r.B, dout, c, r.s);
    dy = folded;
    dout.h -= 1;
  }
  if (dx) {
    // dx[i][ci] = sum_k dy[s*i + k - 1][co] w[ci][co][k]: a strided conv of dy with w viewed as (co' = ci, ci' = co)
    float* wp = pre ? nullptr : ws->get<float>(packed_weight_floats(c, c, T));
    float* wp3 = pre ? nullptr : ws->get<float>(packed_split16_bytes(c, c, T) / 4);
    if (!r.dry()) {
      if (!pre) {
        launch_pack_weights(w_raw, wp, c, c, T, false, r.s);
        launch_pack_weights_split16(w_raw, wp3, c, c, T, r.s, false, false);
      }
      ConvGeom gd{dout, din, kz, 4, 4, sz, 2, 2};
      ConvFusion fu;
      fu.wpk_bf16x3 = pre ? img->pk3 : wp3;
      dy_max = launch_absmax_bits(dy, (size_t)r.B * dout.vox() * c, &r.amax, r.s);
      fu.in_absmax = dy_max;
      launch_conv_mfma(dy, c, nullptr, 0, pre ? img->pk : wp, nullptr, dx, r.B, c, gd, r.s, fu);
    }
    if (wp3) ws->release(wp3);
    if (wp) ws->release(wp);
  }
  // dw[ci][co][k] = sum_i x[i][ci] * dy[s*i + k - 1][co]: the strided-conv weight gradient with the two tensors' roles swapped
  if (r.param_grads) {
    float* part = r.wgrad_part(wgrad_partial_floats(din.vox(), r.B, false, c, c, T));
    if (!r.dry()) {
      WgradOp op;
      op.g = x; op.A = c; op.x = dy; op.Bc = c; op.xld = c; op.geom = ConvGeom{dout, din, kz, 4, 4, sz, 2, 2}; op.batch = r.B;
      op.partial = part; op.dw = dw; op.aux = r.wgrad_aux(nullptr, dy_max);
      launch_wgrad(op, r.s);
    }
    r.release_wgrad_part(part);
    if (db) bias_grad(r, dy_full, c, dout_full.vox(), db);
  }
  if (folded) ws->release(folded);
}

}  // namespace cd
