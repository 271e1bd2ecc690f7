// The deepest U-Net level in one launch (kernels_deep.hip), alone or with a side conv on the idle CUs (kernels_deep_side.hip).
#pragma once
#include "cd_common.h"

namespace cd {

// The whole deepest level -- downs[-1], mid blocks, ups[0]: six ResnetBlocks and up to three attention blocks -- in ONE launch,
// one workgroup per sample with the activations resident in LDS (kernels_deep.hip).  Block order: downs r1, downs r2, mid1, mid2,
// ups r1 (input = cat(x, skip)), ups r2; attention after downs r2, mid1 and ups r2.
struct DeepLevelDesc {
  Dims3 dims{};
  int Ca = 0, Cb = 0, groups = 0;  // channels entering / leaving the level (layer_sizes[-2]) and inside it (layer_sizes[-1])
  struct Res {
    int c0 = 0, c1 = 0, cout = 0;
    const void *w1 = nullptr, *w2 = nullptr;  // f16x2 images of the two 3x3x3 convs
    const float *b1 = nullptr, *b2 = nullptr, *g1 = nullptr, *be1 = nullptr, *g2 = nullptr, *be2 = nullptr;
    const float* emb = nullptr;               // (B, emb_ld) slice or null
    int emb_ld = 0;
    const void* wres = nullptr;               // f16x2 image of the 1x1 shortcut conv or null (identity)
    const float* bres = nullptr;
  } res[6];
  struct Attn {
    int C = 0;
    const float *ng = nullptr, *nb = nullptr, *wout = nullptr, *bout = nullptr, *gg = nullptr, *gb = nullptr;
    const void* wqkv = nullptr;               // f16x2 image of to_qkv
  } attn[3];
  int has_attn[3] = {0, 0, 0};
};
bool deep_level_eligible(const DeepLevelDesc& d);
void launch_deep_level(const DeepLevelDesc& d, const float* x_in, float* x_out, int batch, int* status, hipStream_t s);
// The same launch with a side job on the CUs the level leaves idle (kernels_deep_side.hip): one 32-channel K-block of a
// full-resolution 3x3x3 conv whose input does not depend on the level -- out = conv(in, that K-block's weights) + bias, whole tensor.
// The rest of the conv follows as a continuation launch of the z-slide kernel (ConvFusion::add_src = out).
struct DeepSideConv {
  const float* in = nullptr;  // (B, vox, ldc) channels-last, offset to the first of the K-block's `cin` channels
  int ldc = 0, cin = 0;
  const void* wpk = nullptr;  // f16x2 image of the conv, offset to the K-block's first k-step
  const float* bias = nullptr;
  float* out = nullptr;       // (B, vox, cout)
  int cout = 0;
  Dims3 dims{};
};
// chunks per sample the side job would be dealt in, 0 = this conv / batch / environment does not qualify (CD_NO_DEEP_SIDE_CONV=1
// forces that: the conv then runs after the level as before)
int deep_side_conv_chunks(int batch, int cin_side, int cout, Dims3 dims);
void launch_deep_level_side(const DeepLevelDesc& d, const float* x_in, float* x_out, int batch, int* status, const DeepSideConv& side,
                            hipStream_t s);

}  // namespace cd
