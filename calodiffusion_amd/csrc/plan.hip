// Host side of the C ABI (include/calodiff.h): plan construction, the weight arena, coordinates, status and gradient layout.
// The launch sequences are in forward.hip, sampler.hip and train.hip.
#include "plan_internal.h"
#include "kernels_attn.h"

#include <array>
#include <cstdio>
#include <cstring>
#include <memory>

namespace cd {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }

int add_weight(CdPlan* p, const std::string& name, int64_t numel, PackKind pk = PK_NONE, int cin = 0, int cout = 0, int taps = 0) {
  WeightEntry e;
  e.name = name; e.numel = numel; e.src_numel = numel; e.pack = pk; e.cin = cin; e.cout = cout; e.taps = taps;
  p->weights.push_back(e);
  p->index[name] = (int)p->weights.size() - 1;
  return (int)p->weights.size() - 1;
}

// One channel axis of a tensor: n channels as the config counts them, run as n k (kernels_widen.h).  An axis that is no U-Net
// width (q/k/v rows, the attention's hidden inputs, the head's output, in_channels, the conditioning sizes) is plain(n).
struct Ax {
  int n = 0, k = 1, cpg = 1;
  int w() const { return n * k; }
};
static Ax plain(int n) { return Ax{n, 1, n > 0 ? n : 1}; }

// The width rule: the smallest k of {1, 2, 4} with C k a multiple of 32 (<= 256) and C k / groups a multiple of 4; 0 = none
int widen_factor(int c, int groups) {
  if (c <= 0 || c % groups != 0) return 0;
  for (int k : {1, 2, 4})
    if ((c * k) % 32 == 0 && ((c * k) / groups) % 4 == 0 && c * k <= 256) return k;
  return 0;
}

// a tensor [out][in0 | in1][taps] (in_first: [in][out][taps]); records its map if any of its axes is widened
int add_tensor(CdPlan* p, const std::string& name, Ax out, Ax in0, Ax in1, int taps, PackKind pk = PK_NONE, bool in_first = false) {
  const int cin = in0.w() + in1.w();
  const int i = pk == PK_NONE ? add_weight(p, name, (int64_t)out.w() * cin * taps)
                              : add_weight(p, name, (int64_t)out.w() * cin * taps, pk, cin, out.w(), taps);
  WeightEntry& e = p->weights[i];
  e.src_numel = (int64_t)out.n * (in0.n + in1.n) * taps;
  e.widened = out.k > 1 || in0.k > 1 || in1.k > 1;
  WidenJob& j = e.widen;
  j.out_w = out.w(); j.out_cpg = out.cpg; j.out_k = out.k;
  j.in_w[0] = in0.w(); j.in_cpg[0] = in0.cpg; j.in_k[0] = in0.k;
  j.in_w[1] = in1.w(); j.in_cpg[1] = in1.cpg; j.in_k[1] = in1.k;
  j.taps = taps; j.in_first = in_first ? 1 : 0;
  j.n_wide = (unsigned long long)e.numel; j.n_narrow = (unsigned long long)e.src_numel;
  return i;
}
int add_vector(CdPlan* p, const std::string& name, Ax c) { return add_tensor(p, name, c, plain(1), plain(0), 1); }

// A block keeps or drops its 1x1 shortcut by the config's widths, not the wide ones: a 16 -> 32 block keeps it although both
// sides run 32 wide.
ResW add_res(CdPlan* p, const std::string& pre, Ax in0, Ax in1, Ax out, bool mlp) {
  ResW r;
  const int cout = out.w();
  r.cin = in0.w() + in1.w(); r.cout = cout; r.has_mlp = mlp; r.has_res = in0.n + in1.n != out.n;
  // (without a shortcut conv the input is added to the output channel by channel: one map on both sides.  A single input of
  // the output's width has the output's map; a concatenated one has two)
  if (!r.has_res && in1.n > 0 && (in0.k > 1 || in1.k > 1 || out.k > 1))
    throw Fail{CD_EINVAL, pre + ": a concatenated input added to the output without a shortcut conv cannot run widened"};
  if (mlp) {
    r.mw = add_tensor(p, pre + ".mlp.1.weight", out, plain(p->desc.cond_dim), plain(0), 1);
    r.mb = add_vector(p, pre + ".mlp.1.bias", out);
    r.emb_off = p->emb_ld;
    p->emb_ld += cout;
    p->embed_list.push_back({r.mw, r.emb_off});
  }
  r.c1w = add_tensor(p, pre + ".block1.proj.conv.weight", out, in0, in1, 27, PK_CONV);
  r.c1b = add_vector(p, pre + ".block1.proj.conv.bias", out);
  r.n1g = add_vector(p, pre + ".block1.norm.weight", out);
  r.n1b = add_vector(p, pre + ".block1.norm.bias", out);
  r.c2w = add_tensor(p, pre + ".block2.proj.conv.weight", out, out, plain(0), 27, PK_CONV);
  r.c2b = add_vector(p, pre + ".block2.proj.conv.bias", out);
  r.n2g = add_vector(p, pre + ".block2.norm.weight", out);
  r.n2b = add_vector(p, pre + ".block2.norm.bias", out);
  if (r.has_res) {
    r.rw = add_tensor(p, pre + ".res_conv.conv.weight", out, in0, in1, 1, PK_CONV);
    r.rb = add_vector(p, pre + ".res_conv.conv.bias", out);
  }
  return r;
}

AttnW add_attn(CdPlan* p, const std::string& pre, Ax c) {
  AttnW a;
  a.c = c.w();
  a.qkv = add_tensor(p, pre + ".fn.fn.to_qkv.conv.weight", plain(96), c, plain(0), 1, PK_CONV);
  a.ow = add_tensor(p, pre + ".fn.fn.to_out.0.conv.weight", c, plain(32), plain(0), 1);
  p->weights[a.ow].cin = 32; p->weights[a.ow].cout = a.c; p->weights[a.ow].taps = 1; p->weights[a.ow].dg_1x1 = true;
  a.ob = add_vector(p, pre + ".fn.fn.to_out.0.conv.bias", c);
  a.gg = add_vector(p, pre + ".fn.fn.to_out.1.weight", c);
  a.gb = add_vector(p, pre + ".fn.fn.to_out.1.bias", c);
  a.ng = add_vector(p, pre + ".fn.norm.weight", c);
  a.nb = add_vector(p, pre + ".fn.norm.bias", c);
  return a;
}

void check_channels(int c, const char* what) {
  if (c % 32 != 0 || c <= 0 || c > 256)
    throw Fail{CD_EINVAL, std::string(what) + ": channel widths must be multiples of 32 (<= 256) for the MFMA kernels"};
}

void build_plan(CdPlan* p) {
  const CdUnetDesc& d = p->desc;  // (its layer_sizes become the wide widths below)
  CD_REQUIRE(d.n_sizes >= 2 && d.n_sizes <= CD_MAX_SIZES, "LAYER_SIZE_UNET must have 2..8 entries");
  CD_REQUIRE(d.in_channels >= 1 && d.in_channels <= 4, "in_channels must be 1..4");
  CD_REQUIRE(d.cond_dim == 128 || (d.cond_dim % 4 == 0 && d.cond_dim <= 256), "COND_SIZE_UNET must be <= 256");
  CD_REQUIRE(d.cond_size >= 1 && d.cond_size <= 256, "cond_size must be 1..256");
  CD_REQUIRE(d.groups >= 1 && d.groups <= 64, "BLOCK_GROUPS must be 1..64");
  // the width rule: every config width C runs as C k; all further checks are on the wide widths
  std::vector<Ax> ax(d.n_sizes);
  for (int i = 0; i < d.n_sizes; ++i) {
    const int c = d.layer_sizes[i], k = widen_factor(c, d.groups);
    if (!k)
      throw Fail{CD_EINVAL, "LAYER_SIZE_UNET entry " + std::to_string(c) + " with BLOCK_GROUPS " + std::to_string(d.groups) +
                                ": a width C must be a multiple of the group count and have a k in {1, 2, 4} for which C k is a "
                                "multiple of 32, at most 256, and C k / BLOCK_GROUPS a multiple of 4 (a narrow width runs widened "
                                "to C k)"};
    p->cfg_sizes[i] = c;
    ax[i] = Ax{c, k, c / d.groups};
    p->desc.layer_sizes[i] = c * k;
    p->widened = p->widened || k > 1;
  }
  for (int i = 0; i < d.n_sizes; ++i) check_channels(d.layer_sizes[i], "LAYER_SIZE_UNET");
  CD_REQUIRE(d.layer_sizes[0] == 32, "the fused output head needs LAYER_SIZE_UNET[0] to be 32, or 8 or 16 (which run 32 wide)");
  CD_REQUIRE(p->cfg_sizes[0] == p->cfg_sizes[1], "final_conv expects LAYER_SIZE_UNET[1] input channels (models.py:698): sizes 0 and 1 must agree");
  p->nres = d.n_sizes - 1;
  const int nres = p->nres;
  const int zs = d.compress_z ? 2 : 1;

  // level shapes and up-sampling geometry (CondUnet.__init__, models.py:619-635; Upsample, :335-348)
  Dims3 s{d.grid[0], d.grid[1], d.grid[2]};
  CD_REQUIRE(s.d > 0 && s.h > 0 && s.w > 0, "grid extents must be positive");
  p->shapes.push_back(s);
  std::vector<std::array<int, 3>> extras;
  for (int lv = 0; lv + 1 < nres; ++lv) {
    extras.push_back({(s.d + 1) % 2, s.h % 2, s.w % 2});
    const Dims3 n{d.compress_z ? (s.d + 1) / 2 : s.d, s.h / 2, s.w / 2};
    CD_REQUIRE(n.h >= 1 && n.w >= 1, "grid too small for the number of resolution levels");
    // the strided conv must actually produce that shape
    const int od = (s.d + 2 - 3) / zs + 1, oh = (s.h + 2 - 4) / 2 + 1, ow = (s.w + 2 - 4) / 2 + 1;
    CD_REQUIRE(od == n.d && oh == n.h && ow == n.w, "down-sampling output shape mismatch");
    s = n;
    p->shapes.push_back(s);
  }
  for (int i = 0; i + 1 < nres; ++i) {
    const auto e = extras[nres - 2 - i];
    const int kz = e[0] > 0 ? 4 : 3;
    const Dims3 in = p->shapes[nres - 1 - i];
    const Dims3 out{(in.d - 1) * zs - 2 + kz, 2 * in.h + e[1], 2 * in.w + e[2]};
    const Dims3 want = p->shapes[nres - 2 - i];
    CD_REQUIRE(out.d == want.d && out.h == want.h && out.w == want.w,
               "up-sampling output shape does not match the skip connection (the reference would fail in torch.cat)");
    p->up_kz.push_back(kz);
    p->up_out.push_back(out);
  }

  // weights, in CondUnet.state_dict() order
  const int half = d.cond_dim / 2, hidden = d.cond_size > half / 2 ? d.cond_size : half / 2;
  p->init_w = add_tensor(p, "init_conv.conv.weight", ax[0], plain(d.in_channels), plain(0), 27, PK_INIT);
  p->init_b = add_vector(p, "init_conv.conv.bias", ax[0]);
  // Linear branch: time_mlp = [Unflatten, Linear(1, q), GELU, Linear(q, half), GELU, Linear(half, half)] (keys 1, 3, 5);
  // sinusoidal branch: [SinusoidalPositionEmbeddings(q), Linear(q, half), GELU, Linear(half, half)] (keys 1, 3).  The cond
  // MLP likewise (keys 0, 2, 4 resp. 1, 3; its sinusoidal form embeds a scalar condition, so hidden must equal q).
  CD_REQUIRE(!(d.time_sin || d.cond_sin) || (half / 2) % 2 == 0 && half / 2 >= 4, "sinusoidal embeddings need cond_dim / 4 even and >= 4");
  CD_REQUIRE(!d.cond_sin || hidden == half / 2,
             "cond_embed 'sin' embeds one scalar per sample into cond_dim/4 features: cond_size must not exceed cond_dim/4");
  const int tin[3] = {1, half / 2, half}, tout[3] = {half / 2, half, half};
  for (int i = d.time_sin ? 1 : 0; i < 3; ++i) {
    const std::string key = "time_mlp." + std::to_string(d.time_sin ? 2 * i - 1 : 2 * i + 1);
    p->tw[i] = add_weight(p, key + ".weight", (int64_t)tin[i] * tout[i]);
    p->tb[i] = add_weight(p, key + ".bias", tout[i]);
  }
  const int cin3[3] = {d.cond_size, hidden, half}, cout3[3] = {hidden, half, half};
  for (int i = d.cond_sin ? 1 : 0; i < 3; ++i) {
    const std::string key = "cond_mlp." + std::to_string(d.cond_sin ? 2 * i - 1 : 2 * i);
    p->cw[i] = add_weight(p, key + ".weight", (int64_t)cin3[i] * cout3[i]);
    p->cb[i] = add_weight(p, key + ".bias", cout3[i]);
  }
  p->downs.resize(nres);
  p->ups.resize(nres);
  for (int i = 0; i < nres; ++i) {
    const Ax ci = ax[i], co = ax[i + 1];
    const std::string pre = "downs." + std::to_string(i);
    p->downs[i].r1 = add_res(p, pre + ".0", ci, plain(0), co, true);
    p->downs[i].r2 = add_res(p, pre + ".1", co, plain(0), co, true);
    if (i + 1 < nres) {
      p->downs[i].sw = add_tensor(p, pre + ".2.conv.weight", co, co, plain(0), 48, PK_CONV);
      p->downs[i].sb = add_vector(p, pre + ".2.conv.bias", co);
    }
  }
  for (int i = 0; i < nres; ++i) {
    const int lv = nres - 1 - i;
    const Ax ci = ax[lv], co = ax[lv + 1];
    const std::string pre = "ups." + std::to_string(i);
    p->ups[i].r1 = add_res(p, pre + ".0", co, co, ci, true);  // cat(x, skip): two segments, each with its own map
    p->ups[i].r2 = add_res(p, pre + ".1", ci, plain(0), ci, true);
    if (i + 1 < nres) {
      const int kz = p->up_kz[i];
      p->ups[i].sw = add_tensor(p, pre + ".2.convTrans.weight", ci, ci, plain(0), kz * 16, PK_CONVT, true);
      p->ups[i].sb = add_vector(p, pre + ".2.convTrans.bias", ci);
    }
    check_channels(co.w() * 2, "skip concat");
  }
  if (d.block_attn) {
    for (int i = 0; i < nres; ++i) p->downs[i].attn = add_attn(p, "downs_attn." + std::to_string(i), ax[i + 1]);
    for (int i = 0; i < nres; ++i) p->ups[i].attn = add_attn(p, "ups_attn." + std::to_string(i), ax[nres - 1 - i]);
  }
  const Ax mid = ax[nres];
  p->mid1 = add_res(p, "mid_block1", mid, plain(0), mid, true);
  if (d.mid_attn) p->mid_attn = add_attn(p, "mid_attn", mid);
  p->mid2 = add_res(p, "mid_block2", mid, plain(0), mid, true);
  p->fin = add_res(p, "final_conv.0", ax[1], plain(0), ax[0], false);
  p->head_w = add_tensor(p, "final_conv.1.conv.weight", plain(1), ax[0], plain(0), 1);
  p->head_b = add_weight(p, "final_conv.1.conv.bias", 1);

  // arena layout
  size_t off = 0;
  auto bump = [&](size_t n) { size_t o = off; off += (n + 63) & ~(size_t)63; return o; };
  for (auto& w : p->weights) {
    w.raw_off = bump((size_t)w.numel);
    if (w.pack == PK_CONV || w.pack == PK_CONVT) w.pk_off = bump(packed_weight_floats(w.cin, w.cout, w.taps));
    // 16-bit split images: the 3x3x3 / strided convs and the attention's to_qkv (cout = 96)
    // (1x1: the attention's to_qkv and the ResnetBlocks' res_conv, which the deep-level kernel runs on the fp16 pipe)
    if (w.pack == PK_CONV && (w.taps == 27 || w.taps == 48 || w.taps == 1))
      w.pk3_off = bump(packed_split16_bytes(w.cin, w.cout, w.taps) / 4);
    else if (w.pack == PK_CONVT) w.pk3_off = bump(packed_f16x2_bytes(w.cin, w.cout, w.taps) / 4);  // f16x2 image only
    else if (w.pack == PK_INIT) w.pk_off = bump((size_t)w.numel);
  }
  p->arena_floats = off;
  // the caller's flat gradient buffer is laid out by the config's own shapes; widened tensors get a slot in the step's wide block
  size_t goff = 0, wgoff = 0;
  for (auto& w : p->weights) {
    w.grad_off = goff;
    goff += ((size_t)w.src_numel + 63) & ~(size_t)63;
    if (!w.widened) continue;
    w.wide_grad_off = wgoff;
    wgoff += ((size_t)w.numel + 63) & ~(size_t)63;
  }
  p->grad_floats = goff;
  p->wide_grad_floats = wgoff;
  CD_HIP(hipMalloc((void**)&p->d_lin_jobs, sizeof(LinearWgradJob) * 64));
  CD_HIP(hipMalloc((void**)&p->arena, off * sizeof(float)));
  CD_HIP(hipMemset(p->arena, 0, off * sizeof(float)));

  // embedding projection descriptors
  std::vector<EmbedLayer> layers;
  for (auto& e : p->embed_list) {
    const WeightEntry& w = p->weights[e.first];
    EmbedLayer L;
    L.w = p->arena + w.raw_off;
    L.b = p->arena + p->weights[e.first + 1].raw_off;
    L.cout = (int)(w.numel / d.cond_dim);
    L.offset = e.second;
    layers.push_back(L);
  }
  p->n_embed_layers = (int)layers.size();
  CD_HIP(hipMalloc((void**)&p->d_embed_layers, sizeof(EmbedLayer) * (layers.size() + 1)));
  CD_HIP(hipMemcpy(p->d_embed_layers, layers.data(), sizeof(EmbedLayer) * layers.size(), hipMemcpyHostToDevice));
  if (p->emb_ld == 0) p->emb_ld = 4;

  CD_HIP(hipMalloc((void**)&p->d_coords, sizeof(float) * (size_t)(d.grid[0] + d.grid[1] + d.grid[2] + 4)));
  CD_HIP(hipMemset(p->d_coords, 0, sizeof(float) * (size_t)(d.grid[0] + d.grid[1] + d.grid[2] + 4)));
  CD_HIP(hipMalloc((void**)&p->d_init_table, sizeof(float) * (size_t)p->shapes[0].vox() * d.layer_sizes[0]));
  // the composed form of init conv + downs[0].r1's first conv: geometry and widths only (forward_impl adds the precision and the
  // entry point); the deepest level's launch must not be the one that runs that block, a grid of <= 128 voxels runs the block as
  // one launch, and one unit of channel partials per plane must fit the block res_block sets aside (ceil(vox / 32) units)
  if (nres >= 2 && init_pair_eligible(p->shapes[0]) && p->shapes[0].vox() > 128 && p->shapes[0].d <= (p->shapes[0].vox() + 31) / 32 &&
      p->downs[0].r1.cin == 32 && p->downs[0].r1.cout == 32 &&
      !p->downs[0].r1.has_res && d.layer_sizes[0] == 32) {
    CD_HIP(hipMalloc(&p->d_pair_w, kInitPairWeightBytes));
    CD_HIP(hipMalloc((void**)&p->d_pair_table, sizeof(float) * (size_t)p->shapes[0].vox() * 32));
  }
  CD_HIP(hipMalloc((void**)&p->d_table, sizeof(float) * 4 * CdPlan::kMaxSteps));
  CD_HIP(hipMalloc((void**)&p->d_counter, sizeof(int) * 4));  // [0] sampler step counter, [2] range flags
  CD_HIP(hipMemset(p->d_counter, 0, sizeof(int) * 4));
  p->status_word = p->d_counter + 2;
  CD_HIP(hipMalloc((void**)&p->d_stepvals, sizeof(float) * 8));
  CD_HIP(hipMalloc((void**)&p->d_attn_sync, sizeof(unsigned) * 2 * kAttnCoopSamples));
}

void check_ready(CdPlan* p, bool need_coords) {
  // need_coords = a denoise-based entry point: the reference's do_time_embed raises KeyError for TIME_EMBED 'sin'
  // (calodiffusion.py:148-152); only CondUnet.forward reaches the sinusoidal embeddings
  if (need_coords && (p->desc.time_sin || p->desc.cond_sin))
    throw Fail{CD_EINVAL, "sinusoidal time/cond embeddings are reachable through cd_unet_forward only (the reference's denoise "
                          "path raises KeyError for TIME_EMBED 'sin')"};
  for (auto& w : p->weights)
    if (!w.set) throw Fail{CD_EWEIGHTS, "weight '" + w.name + "' was never set (cd_plan_set_weight)"};
  if (need_coords && (p->desc.rz_input || p->desc.phi_input) && !p->coords_set)
    throw Fail{CD_EWEIGHTS, "coordinate profiles were never set (cd_plan_set_coords)"};
}

// The init conv's coordinate channels (R, Z, phi images) and bias contribute the same (vox, C0) tensor to every sample and
// step: kept in the plan, recomputed whenever the init conv's parameters or the coordinate profiles are (re)set.
static void init_conv_coord_args(CdPlan* p, InitConvArgs& a) {
  const CdUnetDesc& d = p->desc;
  a.cin = d.in_channels; a.wpk = p->packed(p->init_w); a.bias = p->raw(p->init_b); a.cout = d.layer_sizes[0]; a.dims = p->shapes[0];
  a.cx = 1; a.use_rz = d.rz_input; a.use_phi = d.phi_input;
  a.r_w = p->d_coords; a.z_d = p->d_coords + d.grid[2]; a.phi_h = p->d_coords + d.grid[2] + d.grid[0];
  a.coord_table = p->d_init_table;
}
// ... and what the composed init pair derives from it and from downs[0].r1's first conv (kernels_init_pair.hip)
static void refresh_init_pair(CdPlan* p, hipStream_t s) {
  const ResW& r1 = p->downs[0].r1;
  if (!p->d_pair_w || !p->weights[p->init_w].set || !p->weights[p->init_b].set || !p->weights[r1.c1w].set || !p->weights[r1.c1b].set) return;
  launch_init_pair_build(p->raw(p->init_w), p->desc.in_channels, p->raw(r1.c1w), p->raw(r1.c1b), p->d_init_table, p->d_pair_w,
                         p->d_pair_table, p->shapes[0], s);
  p->init_pair_ready = true;
}
static void refresh_init_table(CdPlan* p, hipStream_t s) {
  if (!p->weights[p->init_w].set || !p->weights[p->init_b].set) return;
  InitConvArgs a;
  init_conv_coord_args(p, a);
  launch_init_coord_table(a, s);
  refresh_init_pair(p, s);
}

}  // namespace cd

// ------------------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------------------
extern "C" {

const char* cd_last_error(void) { return g_last_error.c_str(); }
int cd_abi_version(void) { return CD_ABI_VERSION; }

int cd_device_check(char* name, int cap) {
  return guarded([&] {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) throw Fail{CD_ENOGPU, "no HIP device visible"};
    int dev = 0;
    CD_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    CD_HIP(hipGetDeviceProperties(&prop, dev));
    if (name && cap > 0) {
      std::snprintf(name, cap, "%s (%s)", prop.name, prop.gcnArchName);
    }
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
      throw Fail{CD_ENOGPU, std::string("this library is built for gfx950 only; found ") + prop.gcnArchName};
  });
}

int cd_set_conv_precision(const char* mode) {
  return guarded([&] {
    CD_REQUIRE(mode, "null argument");
    if (!std::strcmp(mode, "f16x2")) set_conv_precision(PREC_F16X2);
    else if (!std::strcmp(mode, "bf16x3")) set_conv_precision(PREC_BF16X3);
    else if (!std::strcmp(mode, "f32")) set_conv_precision(PREC_F32);
    else throw Fail{CD_EINVAL, std::string("unknown convolution precision '") + mode + "' (f16x2, bf16x3, f32)"};
  });
}
const char* cd_get_conv_precision(void) {
  static const char* names[3] = {"f16x2", "bf16x3", "f32"};
  return names[conv_precision()];
}

int cd_plan_create(const CdUnetDesc* desc, CdPlan** plan) {
  return guarded([&] {
    CD_REQUIRE(desc && plan, "null argument");
    if (desc->struct_size != sizeof(CdUnetDesc))
      throw Fail{CD_EINVAL, "CdUnetDesc.struct_size is " + std::to_string(desc->struct_size) + ", this library expects " +
                                std::to_string(sizeof(CdUnetDesc)) + " (ABI version " + std::to_string(CD_ABI_VERSION) +
                                "): the binding was written against another calodiff.h"};
    std::unique_ptr<CdPlan> p(new CdPlan());
    p->desc = *desc;
    build_plan(p.get());
    *plan = p.release();
  });
}

int cd_plan_destroy(CdPlan* plan) {
  return guarded([&] {
    if (!plan) return;
    plan->ddim_graph.destroy();
    plan->prog_graph.destroy();
    if (plan->cap_stream) hipStreamDestroy(plan->cap_stream);
    if (plan->d_pack_jobs) hipFree(plan->d_pack_jobs);
    if (plan->d_dg_jobs) hipFree(plan->d_dg_jobs);
    if (plan->d_expand_jobs) hipFree(plan->d_expand_jobs);
    if (plan->d_fold_jobs) hipFree(plan->d_fold_jobs);
    if (plan->d_attn_sync) hipFree(plan->d_attn_sync);
    if (plan->arena) hipFree(plan->arena);
    if (plan->d_embed_layers) hipFree(plan->d_embed_layers);
    if (plan->d_coords) hipFree(plan->d_coords);
    if (plan->d_init_table) hipFree(plan->d_init_table);
    if (plan->d_pair_w) hipFree(plan->d_pair_w);
    if (plan->d_pair_table) hipFree(plan->d_pair_table);
    if (plan->d_table) hipFree(plan->d_table);
    if (plan->d_counter) hipFree(plan->d_counter);
    if (plan->d_stepvals) hipFree(plan->d_stepvals);
    if (plan->d_lin_jobs) hipFree(plan->d_lin_jobs);
    delete plan;
  });
}

int cd_plan_num_weights(const CdPlan* plan, int* n) {
  return guarded([&] {
    CD_REQUIRE(plan && n, "null argument");
    *n = (int)plan->weights.size();
  });
}

int cd_plan_weight_name(const CdPlan* plan, int idx, char* name, int cap, int64_t* numel) {
  return guarded([&] {
    CD_REQUIRE(plan && idx >= 0 && idx < (int)plan->weights.size(), "weight index out of range");
    if (name && cap > 0) std::snprintf(name, cap, "%s", plan->weights[idx].name.c_str());
    if (numel) *numel = plan->weights[idx].src_numel;
  });
}

int cd_plan_set_weight(CdPlan* plan, const char* name, const float* dev_ptr, int64_t numel, void* stream) {
  return guarded([&] {
    CD_REQUIRE(plan && name && dev_ptr, "null argument");
    auto it = plan->index.find(name);
    if (it == plan->index.end()) throw Fail{CD_EWEIGHTS, std::string("unknown weight name '") + name + "'"};
    WeightEntry& w = plan->weights[it->second];
    if (w.src_numel != numel)
      throw Fail{CD_EWEIGHTS, std::string("weight '") + name + "' has " + std::to_string(numel) + " elements, expected " + std::to_string(w.src_numel)};
    hipStream_t s = (hipStream_t)stream;
    if (w.widened) {
      WidenJob j = w.widen;
      j.narrow = const_cast<float*>(dev_ptr); j.wide = plan->arena + w.raw_off;
      launch_widen_expand_one(j, s);
    } else {
      CD_HIP(hipMemcpyAsync(plan->arena + w.raw_off, dev_ptr, sizeof(float) * (size_t)numel, hipMemcpyDeviceToDevice, s));
    }
    if (w.pack == PK_CONV) launch_pack_weights(plan->arena + w.raw_off, plan->arena + w.pk_off, w.cout, w.cin, w.taps, false, s);
    if (w.pack == PK_CONVT) {
      launch_pack_weights(plan->arena + w.raw_off, plan->arena + w.pk_off, w.cout, w.cin, w.taps, true, s);
      launch_pack_weights_f16x2(plan->arena + w.raw_off, plan->arena + w.pk3_off, w.cout, w.cin, w.taps, s, true, false);
    } else if (w.pk3_off) {
      launch_pack_weights_split16(plan->arena + w.raw_off, plan->arena + w.pk3_off, w.cout, w.cin, w.taps, s);
    }
    else if (w.pack == PK_INIT) launch_pack_init_weights(plan->arena + w.raw_off, plan->arena + w.pk_off, w.cout, w.cin, s);
    w.set = true;
    if (it->second == plan->init_w || it->second == plan->init_b) refresh_init_table(plan, s);
    else if (it->second == plan->downs[0].r1.c1w || it->second == plan->downs[0].r1.c1b) refresh_init_pair(plan, s);
  });
}

int cd_plan_set_weights(CdPlan* plan, int n, const float* const* dev_ptrs, void* stream) {
  return guarded([&] {
    CD_REQUIRE(plan && dev_ptrs, "null argument");
    if (n != (int)plan->weights.size())
      throw Fail{CD_EWEIGHTS, "cd_plan_set_weights: " + std::to_string(n) + " tensors given, the plan has " +
                                  std::to_string(plan->weights.size())};
    hipStream_t s = (hipStream_t)stream;
    bool changed = plan->pack_jobs.size() != plan->weights.size();
    if (changed) plan->pack_jobs.assign(plan->weights.size(), PackJob{});
    // a widened tensor goes caller -> wide raw copy in the expand launch, and the packers read that copy
    std::vector<WidenJob>& ex = plan->expand_jobs;
    bool ex_changed = false;
    if (plan->widened && ex.empty()) {
      for (const auto& w : plan->weights)
        if (w.widened) ex.push_back(w.widen);
      CD_HIP(hipMalloc((void**)&plan->d_expand_jobs, sizeof(WidenJob) * ex.size()));
      ex_changed = true;
    }
    size_t ke = 0;
    for (int i = 0; i < n; ++i) {
      CD_REQUIRE(dev_ptrs[i], "cd_plan_set_weights: null tensor pointer");
      const WeightEntry& w = plan->weights[i];
      PackJob& j = plan->pack_jobs[i];
      const float* src = dev_ptrs[i];
      if (w.widened) {
        WidenJob& e = ex[ke++];
        if (e.narrow != dev_ptrs[i]) ex_changed = true;
        e.narrow = const_cast<float*>(dev_ptrs[i]); e.wide = plan->arena + w.raw_off;
        src = plan->arena + w.raw_off;
      }
      if (j.src != src) changed = true;
      j.src = src;
      j.raw = plan->arena + w.raw_off;
      j.cout = w.cout; j.cin = w.cin; j.taps = w.taps; j.kind = (int)w.pack;
      j.numel = w.widened ? 0ull : (unsigned long long)w.numel;
      j.pk = nullptr; j.bf3 = nullptr; j.f16 = nullptr; j.n_pk = j.n_bf3 = j.n_f16 = 0;
      const unsigned long long n16 = w.pack == PK_CONV || w.pack == PK_CONVT
                                         ? (unsigned long long)(w.cin / 16) * w.taps * ((w.cout + 31) / 32) * 64 : 0ull;
      if (w.pack == PK_CONV || w.pack == PK_CONVT) {
        j.pk = plan->arena + w.pk_off;
        j.n_pk = packed_weight_floats(w.cin, w.cout, w.taps);
      } else if (w.pack == PK_INIT) {
        j.pk = plan->arena + w.pk_off;
        j.n_pk = (unsigned long long)w.cout * w.cin * 27;
      }
      if (w.pack == PK_CONVT) {  // (f16x2 image only, in transposed channel order)
        j.f16 = plan->arena + w.pk3_off;
        j.n_f16 = n16;
      } else if (w.pack == PK_CONV && w.pk3_off) {
        j.bf3 = plan->arena + w.pk3_off;
        j.f16 = (char*)(plan->arena + w.pk3_off) + packed_bf16x3_bytes(w.cin, w.cout, w.taps);
        j.n_bf3 = j.n_f16 = n16;
      }
    }
    if (!plan->d_pack_jobs) CD_HIP(hipMalloc((void**)&plan->d_pack_jobs, sizeof(PackJob) * plan->weights.size()));
    if (changed || ex_changed) {
      // (rare: torch keeps a parameter's storage across optimizer steps) the kernels of the previous call may still read the lists
      CD_HIP(hipStreamSynchronize(s));
      CD_HIP(hipMemcpy(plan->d_pack_jobs, plan->pack_jobs.data(), sizeof(PackJob) * plan->pack_jobs.size(), hipMemcpyHostToDevice));
      if (!ex.empty()) CD_HIP(hipMemcpy(plan->d_expand_jobs, ex.data(), sizeof(WidenJob) * ex.size(), hipMemcpyHostToDevice));
    }
    launch_widen_expand(plan->d_expand_jobs, (int)ex.size(), s);
    launch_pack_jobs(plan->d_pack_jobs, n, s);
    launch_pack_jobs_f16x2(plan->d_pack_jobs, n, s);
    for (auto& w : plan->weights) w.set = true;
    refresh_init_table(plan, s);
  });
}

int cd_plan_set_coords(CdPlan* plan, const float* r_w, const float* z_d, const float* phi_h, void* stream) {
  return guarded([&] {
    CD_REQUIRE(plan && r_w && z_d && phi_h, "null argument");
    const CdUnetDesc& d = plan->desc;
    hipStream_t s = (hipStream_t)stream;
    CD_HIP(hipMemcpyAsync(plan->d_coords, r_w, sizeof(float) * d.grid[2], hipMemcpyHostToDevice, s));
    CD_HIP(hipMemcpyAsync(plan->d_coords + d.grid[2], z_d, sizeof(float) * d.grid[0], hipMemcpyHostToDevice, s));
    CD_HIP(hipMemcpyAsync(plan->d_coords + d.grid[2] + d.grid[0], phi_h, sizeof(float) * d.grid[1], hipMemcpyHostToDevice, s));
    CD_HIP(hipStreamSynchronize(s));  // the host arrays may be temporaries
    plan->coords_set = true;
    refresh_init_table(plan, s);
  });
}

int cd_plan_status(CdPlan* plan, int* flags, void* stream) {
  return guarded([&] {
    CD_REQUIRE(plan && flags, "null argument");
    hipStream_t s = (hipStream_t)stream;
    CD_HIP(hipMemcpyAsync(flags, plan->d_counter + 2, sizeof(int), hipMemcpyDeviceToHost, s));
    CD_HIP(hipMemsetAsync(plan->d_counter + 2, 0, sizeof(int), s));
    CD_HIP(hipStreamSynchronize(s));
  });
}

int cd_plan_grad_layout(const CdPlan* plan, int idx, int64_t* offset, int64_t* total_floats) {
  return guarded([&] {
    CD_REQUIRE(plan, "null argument");
    const int nw = (int)plan->weights.size();
    if (total_floats) *total_floats = (int64_t)(plan->grad_floats + 2 * plan->embed_grad_floats());
    if (offset) {
      CD_REQUIRE(idx >= 0 && idx < nw + (plan->embed_grad_floats() ? 2 : 0), "weight index out of range");
      *offset = idx < nw ? (int64_t)plan->weights[idx].grad_off
                         : (int64_t)(idx == nw ? plan->enc_grad_off() : plan->dec_grad_off());
    }
  });
}

// Sets one kind of flat-state embedding (clearing the other) or, with neither map, clears whichever is set.
// A cached step graph holds the launches, the state size and the layout of the embedding it was captured with, and the kernels
// of an earlier call may still read the maps.  Equal pointers do not mean an equal embedding (a freed map's or buffer's
// address may be handed out again for another geometry), so every call with a map, and every call that clears one, drops them.
static void set_flat_embedding(CdPlan* plan, const CdRadialMap* map, const float* enc_w, const float* dec_w, const CdGeomMap* genc,
                               const CdGeomMap* gdec, int want_grads, hipStream_t stream) {
  const bool any = map || genc;
  if (any || plan->flat()) {
    CD_HIP(hipStreamSynchronize(stream));
    plan->ddim_graph.destroy();
    plan->prog_graph.destroy();
  }
  CdPlan::FlatEmbed fe;
  fe.map = map; fe.enc_w = map ? enc_w : nullptr; fe.dec_w = map ? dec_w : nullptr;
  fe.genc = genc; fe.gdec = gdec;
  fe.want_grads = any ? want_grads != 0 : true;
  plan->fe = fe;
}

int cd_plan_set_radial(CdPlan* plan, const CdRadialMap* map, const float* enc_w, const float* dec_w, int want_grads, void* stream) {
  return guarded([&] {
    CD_REQUIRE(plan, "null argument");
    if (map) {  // refused before anything touches the device
      CD_REQUIRE(enc_w && dec_w, "cd_plan_set_radial: a map needs enc_w and dec_w");
      const CdUnetDesc& d = plan->desc;
      if (map->layers != d.grid[0] || map->A != d.grid[1] || map->R != d.grid[2])
        throw Fail{CD_EINVAL, "cd_plan_set_radial: the map's grid (L, alpha_out, r_out) = (" + std::to_string(map->layers) + ", " +
                                  std::to_string(map->A) + ", " + std::to_string(map->R) + ") is not the plan's grid (" +
                                  std::to_string(d.grid[0]) + ", " + std::to_string(d.grid[1]) + ", " + std::to_string(d.grid[2]) + ")"};
    }
    set_flat_embedding(plan, map, enc_w, dec_w, nullptr, nullptr, want_grads, (hipStream_t)stream);
  });
}

int cd_plan_set_geom(CdPlan* plan, const CdGeomMap* enc_map, const CdGeomMap* dec_map, int want_grads, void* stream) {
  return guarded([&] {
    CD_REQUIRE(plan, "null argument");
    if (enc_map) {  // refused before anything touches the device
      CD_REQUIRE(dec_map, "cd_plan_set_geom: an encoder map needs a decoder map");
      const CdUnetDesc& d = plan->desc;
      const int L = d.grid[0], E = d.grid[1] * d.grid[2];
      if (enc_map->layers != L || enc_map->rows != E || dec_map->layers != L || dec_map->cols != E)
        throw Fail{CD_EINVAL, "cd_plan_set_geom: enc_map is (" + std::to_string(enc_map->layers) + ", " + std::to_string(enc_map->rows) +
                                  ", cells) and dec_map (" + std::to_string(dec_map->layers) + ", cells, " +
                                  std::to_string(dec_map->cols) + "), the plan's grid gives (" + std::to_string(L) + ", " +
                                  std::to_string(E) + ")"};
      if (enc_map->cols != dec_map->rows)
        throw Fail{CD_EINVAL, "cd_plan_set_geom: enc_map has " + std::to_string(enc_map->cols) + " cells a layer, dec_map " +
                                  std::to_string(dec_map->rows)};
      CD_REQUIRE(enc_map->t_ptr && dec_map->t_ptr, "cd_plan_set_geom: both maps need their transposed view (CD_GEOM_TRANSPOSED)");
    }
    set_flat_embedding(plan, nullptr, nullptr, nullptr, enc_map, enc_map ? dec_map : nullptr, want_grads, (hipStream_t)stream);
  });
}

}  // extern "C"
