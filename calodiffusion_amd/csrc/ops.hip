// The cd_op_* primitives: single layers of the network (convolutions, GroupNorm, ResnetBlock, attention and their backward
// passes) on caller-owned buffers, for the tests' layer-by-layer comparison with the reference.
#include "plan_internal.h"
#include "kernels_loss.h"

namespace cd {

// ------------------------------------------------------------------------------------------------------------
// layout transposes (tests / generic unet_forward input only; the denoise path never transposes: its I/O has C = 1)
// ------------------------------------------------------------------------------------------------------------
__global__ void to_cl_kernel(const float* __restrict__ src, float* __restrict__ dst, int channels, int64_t vox) {
  const int b = blockIdx.y;
  const int64_t total = vox * channels;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % channels);
    const int64_t v = i / channels;
    dst[(size_t)b * total + i] = src[(size_t)b * total + (size_t)c * vox + v];
  }
}
__global__ void to_planar_kernel(const float* __restrict__ src, float* __restrict__ dst, int channels, int64_t vox) {
  const int b = blockIdx.y;
  const int64_t total = vox * channels;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t v = i % vox;
    const int c = (int)(i / vox);
    dst[(size_t)b * total + i] = src[(size_t)b * total + (size_t)v * channels + c];
  }
}
static void launch_transpose_to_cl(const float* ncdhw, float* ndhwc, int batch, int channels, int64_t vox, hipStream_t s) {
  int64_t bx = (vox * channels + 255) / 256;
  if (bx > 1024) bx = 1024;
  hipLaunchKernelGGL(to_cl_kernel, dim3((unsigned)bx, batch), dim3(256), 0, s, ncdhw, ndhwc, channels, vox);
  CD_HIP(hipGetLastError());
}
static void launch_transpose_to_planar(const float* ndhwc, float* ncdhw, int batch, int channels, int64_t vox, hipStream_t s) {
  int64_t bx = (vox * channels + 255) / 256;
  if (bx > 1024) bx = 1024;
  hipLaunchKernelGGL(to_planar_kernel, dim3((unsigned)bx, batch), dim3(256), 0, s, ndhwc, ncdhw, channels, vox);
  CD_HIP(hipGetLastError());
}

}  // namespace cd

extern "C" {

// the zeroed max-|x| words of a primitive's convolution backward, from its own workspace (at most two measured tensors per source)
static AbsmaxWords op_absmax_words(Arena& ws, hipStream_t s) {
  constexpr size_t kWords = 8;
  unsigned* w = ws.get<unsigned>(kWords);
  CD_HIP(hipMemsetAsync(w, 0, sizeof(unsigned) * kWords, s));
  return AbsmaxWords{w, w + kWords};
}
size_t cd_op_scratch_bytes(int batch, int max_channels, int64_t max_voxels) {
  // packed weights of the largest supported conv (256 x 256 x 64 taps) + norm partials + one activation
  return (size_t)256 * 256 * 64 * 4 * 4 + (size_t)batch * 64 * 64 * 16 + (size_t)batch * max_channels * max_voxels * 4 + (1 << 20);
}

int cd_op_to_channels_last(const float* ncdhw, float* ndhwc, int batch, int channels, int64_t voxels, void* stream) {
  return guarded([&] { launch_transpose_to_cl(ncdhw, ndhwc, batch, channels, voxels, (hipStream_t)stream); });
}
int cd_op_to_ncdhw(const float* ndhwc, float* ncdhw, int batch, int channels, int64_t voxels, void* stream) {
  return guarded([&] { launch_transpose_to_planar(ndhwc, ncdhw, batch, channels, voxels, (hipStream_t)stream); });
}

int cd_op_axpy_sigma(const float* data, const float* noise, const float* sigma, float* out, int batch, int64_t per, void* stream) {
  return guarded([&] {
    CD_REQUIRE(data && noise && sigma && out && batch > 0 && batch <= 65535 && per > 0, "bad argument");
    launch_axpy_sigma(data, noise, sigma, out, batch, per, (hipStream_t)stream);
  });
}

int cd_op_cyl_conv(const float* x0, int c0, const float* x1, int c1, const float* w, const float* bias, float* y,
                   int batch, int cout, const int32_t dims_in[3], const int32_t kernel[3], const int32_t stride[3],
                   void* scratch, void* stream) {
  return guarded([&] {
    CD_REQUIRE(x0 && w && y && scratch, "null argument");
    hipStream_t s = (hipStream_t)stream;
    const int taps = kernel[0] * kernel[1] * kernel[2];
    float* wpk = (float*)scratch;
    launch_pack_weights(w, wpk, cout, c0 + c1, taps, false, s);
    const Dims3 din{dims_in[0], dims_in[1], dims_in[2]};
    if (taps == 1) {
      PointwiseArgs a;
      a.in0 = x0; a.ld0 = c0; a.c0 = c0; a.in1 = x1; a.ld1 = c1; a.c1 = c1; a.wpk = wpk; a.bias = bias; a.out = y;
      a.batch = batch; a.cout = cout; a.vox = din.vox();
      launch_pointwise(a, s);
    } else {
      CD_REQUIRE(cout % 32 == 0, "cout must be a multiple of 32");
      ConvGeom g;
      g.in = din;
      g.kd = kernel[0]; g.kh = kernel[1]; g.kw = kernel[2]; g.sz = stride[0]; g.sh = stride[1]; g.sw = stride[2];
      g.out = Dims3{(din.d + 2 - g.kd) / g.sz + 1, (din.h + 2 - g.kh) / g.sh + 1, (din.w + 2 - g.kw) / g.sw + 1};
      ConvFusion fu;
      if (taps == 27 || taps == 48) {
        float* w3 = wpk + packed_weight_floats(c0 + c1, cout, taps);
        launch_pack_weights_split16(w, w3, cout, c0 + c1, taps, s);
        fu.wpk_bf16x3 = w3;
      }
      launch_conv_mfma(x0, c0, x1, c1, wpk, bias, y, batch, cout, g, s, fu);
    }
  });
}

int cd_op_zslide_conv(const float* x, int cin, const float* w, const float* bias, float* y, float* ch_part, int* units, int batch,
                      int cout, const int32_t dims[3], int chunks, void* scratch, void* stream) {
  return guarded([&] {
    CD_REQUIRE(x && w && y && ch_part && units && scratch && chunks >= 0, "bad argument");
    CD_REQUIRE(cin % 32 == 0 && cout % 32 == 0, "channel counts must be multiples of 32");
    hipStream_t s = (hipStream_t)stream;
    launch_pack_weights_f16x2(w, scratch, cout, cin, 27, s);
    const Dims3 d{dims[0], dims[1], dims[2]};
    ConvGeom g{d, d, 3, 3, 3, 1, 1, 1};
    ConvFusion fu;
    int u = 0;
    fu.act = 1; fu.ch_part = ch_part; fu.units = &u; fu.zs_chunks = chunks;
    CD_REQUIRE(try_launch_conv_zslide(x, cin, nullptr, 0, scratch, bias, y, batch, cout, g, s, fu) && u > 0,
               "this grid is not eligible for the z-slide kernel");
    *units = u;
  });
}

int cd_op_cyl_conv_transpose(const float* x, const float* w, const float* bias, float* y, int batch, int channels,
                             const int32_t dims_in[3], int kernel_z, int stride_z, const int32_t out_pad[3],
                             void* scratch, void* stream) {
  return guarded([&] {
    CD_REQUIRE(x && w && y && scratch, "null argument");
    CD_REQUIRE(out_pad[0] == 0, "z output padding is always 0 (models.py:339)");
    hipStream_t s = (hipStream_t)stream;
    float* wpk = (float*)scratch;
    launch_pack_weights(w, wpk, channels, channels, kernel_z * 16, true, s);
    float* wpk16 = wpk + ((packed_weight_floats(channels, channels, kernel_z * 16) + 63) & ~(size_t)63);
    launch_pack_weights_f16x2(w, wpk16, channels, channels, kernel_z * 16, s, true, false);
    const Dims3 din{dims_in[0], dims_in[1], dims_in[2]};
    const Dims3 dout{(din.d - 1) * stride_z - 2 + kernel_z, 2 * din.h + out_pad[1], 2 * din.w + out_pad[2]};
    launch_conv_transpose_mfma(x, channels, wpk, bias, y, batch, channels, din, dout, kernel_z, stride_z, s, wpk16, nullptr);
  });
}

int cd_op_init_conv(const float* x_ncdhw, const float* w, const float* bias, float* y, int batch, int cin, int cout,
                    const int32_t dims[3], void* scratch, void* stream) {
  return guarded([&] {
    CD_REQUIRE(x_ncdhw && w && y && scratch, "null argument");
    hipStream_t s = (hipStream_t)stream;
    float* wpk = (float*)scratch;
    launch_pack_init_weights(w, wpk, cout, cin, s);
    InitConvArgs a;
    a.x = x_ncdhw; a.cx = cin; a.cin = cin; a.wpk = wpk; a.bias = bias; a.out = y; a.batch = batch; a.cout = cout;
    a.dims = Dims3{dims[0], dims[1], dims[2]};
    launch_init_conv(a, s);
  });
}

int cd_op_init_pair_conv(const float* x, const float* w0, const float* b0, const float* w1, const float* b1, int cin, const float* r_w,
                         const float* z_d, const float* phi_h, int use_rz, int use_phi, const float* scale_b, float* y, float* ch_part,
                         int* units, int batch, const int32_t dims[3], int slabs, void* scratch, void* stream) {
  return guarded([&] {
    CD_REQUIRE(x && w0 && w1 && y && ch_part && units && scratch && batch > 0 && slabs >= 0, "bad argument");
    CD_REQUIRE(cin == 1 + 2 * (use_rz ? 1 : 0) + (use_phi ? 1 : 0), "cin must be 1 + the coordinate channels in use");
    CD_REQUIRE(cin == 1 || (r_w && z_d && phi_h), "coordinate channels need their profiles");
    hipStream_t s = (hipStream_t)stream;
    const Dims3 d{dims[0], dims[1], dims[2]};
    CD_REQUIRE(init_pair_eligible(d), "this grid is not eligible for the composed init pair");
    // scratch: the init conv's [tap][ci][32] image | its coordinate table | the composed weights | the composed table
    auto up = [](size_t n) { return (n + 63) & ~(size_t)63; };
    float* wpk0 = (float*)scratch;
    float* tab0 = wpk0 + up((size_t)27 * cin * 32);
    float* wc = tab0 + up((size_t)d.vox() * 32);
    float* tab1 = wc + up(kInitPairWeightBytes / 4);
    launch_pack_init_weights(w0, wpk0, 32, cin, s);
    InitConvArgs a;
    a.cin = cin; a.cx = 1; a.wpk = wpk0; a.bias = b0; a.cout = 32; a.dims = d; a.use_rz = use_rz; a.use_phi = use_phi;
    a.r_w = r_w; a.z_d = z_d; a.phi_h = phi_h; a.coord_table = tab0;
    launch_init_coord_table(a, s);
    launch_init_pair_build(w0, cin, w1, b1, tab0, wc, tab1, d, s);
    InitPairArgs ia;
    ia.x = x; ia.scale_b = scale_b; ia.wc = wc; ia.table = tab1; ia.out = y; ia.ch_part = ch_part; ia.batch = batch; ia.dims = d;
    ia.slabs = slabs;
    launch_init_pair_conv(ia, units, s);
  });
}

int cd_op_group_norm(const float* x, float* y, const float* gamma, const float* beta, int batch, int channels,
                     int64_t voxels, int groups, int silu, const float* add_bc, const float* residual,
                     void* scratch, void* stream) {
  return guarded([&] {
    CD_REQUIRE(x && y && gamma && beta && scratch, "null argument");
    hipStream_t s = (hipStream_t)stream;
    const int ns = gn_nsplit_for(voxels, batch);
    float* part = (float*)scratch;
    float* coef = part + (size_t)batch * ns * channels * 2;
    launch_ch_stats(x, part, batch, channels, voxels, ns, s);
    launch_gn_finalize(part, ns, gamma, beta, add_bc, channels, coef, batch, channels, groups, voxels, s);
    launch_gn_apply(x, y, coef, batch, channels, voxels, silu, residual, nullptr, 0, nullptr, s);
  });
}

int cd_op_resnet_block(const float* x0, int c0, const float* x1, int c1, const float* const* w, const float* cond, float* y,
                       int batch, int cout, const int32_t dims[3], int groups, void* workspace, size_t workspace_bytes,
                       void* stream) {
  return guarded([&] {
    CD_REQUIRE(x0 && w && y && workspace, "null argument");
    hipStream_t s = (hipStream_t)stream;
    const int cin = c0 + c1;
    Arena ws;
    ws.reset((char*)workspace, workspace_bytes, false);
    float* p1 = ws.get<float>(packed_weight_floats(cin, cout, 27));
    float* p2 = ws.get<float>(packed_weight_floats(cout, cout, 27));
    launch_pack_weights(w[0], p1, cout, cin, 27, false, s);
    launch_pack_weights(w[4], p2, cout, cout, 27, false, s);
    float* q1 = ws.get<float>(packed_split16_bytes(cin, cout, 27) / 4);
    float* q2 = ws.get<float>(packed_split16_bytes(cout, cout, 27) / 4);
    launch_pack_weights_split16(w[0], q1, cout, cin, 27, s);
    launch_pack_weights_split16(w[4], q2, cout, cout, 27, s);
    ResP r;
    r.cin = cin; r.cout = cout; r.has_res = w[10] != nullptr;
    r.c1w3 = q1; r.c2w3 = q2;
    r.c1w = p1; r.c1b = w[1]; r.n1g = w[2]; r.n1b = w[3]; r.c2w = p2; r.c2b = w[5]; r.n2g = w[6]; r.n2b = w[7];
    if (r.has_res) {
      float* p3 = ws.get<float>(packed_weight_floats(cin, cout, 1));
      launch_pack_weights(w[10], p3, cout, cin, 1, false, s);
      r.rw = p3; r.rb = w[11];
    }
    if (w[8] && cond) {
      float* emb = ws.get<float>((size_t)batch * cout);
      launch_silu_linear(cond, w[8], w[9], emb, batch, 128, cout, s);
      r.emb = emb; r.emb_ld = cout;
    }
    Run run{&ws, s, batch, groups};
    const Dims3 d{dims[0], dims[1], dims[2]};
    float* out = res_block(run, r, x0, c0, x1, c1, d);
    CD_HIP(hipMemcpyAsync(y, out, sizeof(float) * (size_t)batch * d.vox() * cout, hipMemcpyDeviceToDevice, s));
  });
}

int cd_op_linear_attention(const float* x, const float* const* w, float* y, int batch, int channels, const int32_t dims[3],
                           void* workspace, size_t workspace_bytes, void* stream) {
  return guarded([&] {
    CD_REQUIRE(x && w && y && workspace, "null argument");
    hipStream_t s = (hipStream_t)stream;
    Arena ws;
    ws.reset((char*)workspace, workspace_bytes, false);
    float* pq = ws.get<float>(packed_weight_floats(channels, 96, 1));
    launch_pack_weights(w[2], pq, 96, channels, 1, false, s);
    float* pq16 = ws.get<float>(packed_f16x2_bytes(channels, 96, 1) / 4);
    launch_pack_weights_f16x2(w[2], pq16, 96, channels, 1, s);
    AttnP a;
    a.c = channels; a.ng = w[0]; a.nb = w[1]; a.qkv = pq; a.ow = w[3]; a.ob = w[4]; a.gg = w[5]; a.gb = w[6];
    a.qkv16 = pq16;
    Run run{&ws, s, batch, 8};
    const Dims3 d{dims[0], dims[1], dims[2]};
    float* out = attn_block(run, a, x, d);
    CD_HIP(hipMemcpyAsync(y, out, sizeof(float) * (size_t)batch * d.vox() * channels, hipMemcpyDeviceToDevice, s));
  });
}

int cd_op_conv_backward(const float* x0, int c0, const float* x1, int c1, const float* w, const float* dy, float* dx, float* dw,
                        float* db, int batch, int cout, const int32_t dims_in[3], const int32_t kernel[3],
                        const int32_t stride[3], void* workspace, size_t workspace_bytes, void* stream) {
  return guarded([&] {
    CD_REQUIRE(x0 && w && dy && dw && workspace, "null argument");
    Arena ws;
    ws.reset((char*)workspace, workspace_bytes, false);
    Run run{&ws, (hipStream_t)stream, batch, 8};
    run.amax = op_absmax_words(ws, run.s);
    ConvGeom g;
    g.in = Dims3{dims_in[0], dims_in[1], dims_in[2]};
    g.kd = kernel[0]; g.kh = kernel[1]; g.kw = kernel[2]; g.sz = stride[0]; g.sh = stride[1]; g.sw = stride[2];
    if (g.kd * g.kh * g.kw == 1) g.out = g.in;
    else g.out = Dims3{(g.in.d + 2 - g.kd) / g.sz + 1, (g.in.h + 2 - g.kh) / g.sh + 1, (g.in.w + 2 - g.kw) / g.sw + 1};
    conv_backward(run, x0, c0, x1, c1, w, dy, dx, dw, db, cout, g);
  });
}

int cd_op_conv_transpose_backward(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int batch,
                                  int channels, const int32_t dims_in[3], int kernel_z, int stride_z, const int32_t out_pad[3],
                                  void* workspace, size_t workspace_bytes, void* stream) {
  return guarded([&] {
    CD_REQUIRE(x && w && dy && dw && workspace, "null argument");
    Arena ws;
    ws.reset((char*)workspace, workspace_bytes, false);
    Run run{&ws, (hipStream_t)stream, batch, 8};
    run.amax = op_absmax_words(ws, run.s);
    const Dims3 din{dims_in[0], dims_in[1], dims_in[2]};
    const Dims3 dout{(din.d - 1) * stride_z - 2 + kernel_z, 2 * din.h + out_pad[1], 2 * din.w + out_pad[2]};
    conv_transpose_backward(run, x, w, dy, dx, dw, db, channels, din, dout, kernel_z, stride_z);
  });
}

int cd_op_group_norm_backward(const float* x, const float* gamma, const float* beta, const float* dy, float* dx, float* dgamma,
                              float* dbeta, float* dadd, int batch, int channels, int64_t voxels, int groups, int silu,
                              void* workspace, size_t workspace_bytes, void* stream) {
  return guarded([&] {
    CD_REQUIRE(x && gamma && beta && dy && dx && dgamma && dbeta && workspace, "null argument");
    hipStream_t s = (hipStream_t)stream;
    Arena ws;
    ws.reset((char*)workspace, workspace_bytes, false);
    Run run{&ws, s, batch, groups};
    int units = 0;
    float* part = stats_pass(run, x, channels, voxels, &units);
    float* coef = ws.get<float>((size_t)batch * channels * 4);
    float* stat = ws.get<float>((size_t)batch * groups * 2);
    launch_gn_finalize(part, units, gamma, beta, nullptr, 0, coef, batch, channels, groups, voxels, s, stat);
    float* scratch = ws.get<float>(gn_backward_scratch_floats(batch, channels, voxels));
    launch_gn_backward(dy, x, coef, stat, gamma, dx, dgamma, dbeta, dadd, channels, batch, channels, voxels, groups, silu, scratch,
                       false, s);
  });
}

}  // extern "C"
