// cd_generator_*: "incident energies in, physical showers out" from a generator file (generator_blob.h), without Python.
// The run is the launch sequence of Diffusion.generate / LayerDiffusion.generate, issued through the library's own entry points
// (cd_randn, cd_layer_sample / cd_layer_sampler_run, cd_ddim_sample / cd_sampler_run, cd_reverse_norm) with the Philox offsets the
// Python path hands them; the only kernel of its own is the conditioning row.
#include "arena.h"
#include "energy_map.h"
#include "generator_blob.h"
#include "guarded.h"

#include <memory>
#include <unordered_map>
#include <vector>

static_assert(sizeof(CdStep) == cdgen::kStepBytes && sizeof(CdSamplerOp) == cdgen::kOpBytes, "generator file record sizes");

namespace cd {
namespace {

// an inner entry point has already recorded its message: pass code and message on
void call(int rc) {
  if (rc != CD_OK) throw Fail{rc, std::string(cd_last_error())};
}

struct DeviceBlock {  // freed when create fails half way, or when its staging use is over
  void* p = nullptr;
  ~DeviceBlock() {
    if (p) (void)hipFree(p);
  }
};

constexpr size_t kBlockAlign = 256;
size_t aligned(size_t n) { return (n + kBlockAlign - 1) & ~(kBlockAlign - 1); }

// ------------------------------------------------------------------------------------------------------------
// The conditioning row (CaloDiffusion.cond_tensor's torch.cat([E, layers]) with the incident-energy map in front): thread
// (b, c) writes column c of row b.  Column 0 is e -- the input itself, or energy_to_cond of a physical energy -- and also goes
// to e_norm (the layer stage's (B, 1) condition) and, mapped back by cond_to_energy, to e_phys (cd_reverse_norm's energies);
// columns 1.. are the layer energies.  cond == null: the energies only (before a layer stage has produced the layers).
// ------------------------------------------------------------------------------------------------------------
struct GenCondArgs {
  const float* energy;  // (B) normalised e, or physical energies
  const float* layers;  // (B, cond_size - 1) or null
  float* cond;          // (B, cond_size) or null
  float* e_norm;        // (B)
  float* e_phys;        // (B)
  int batch, cond_size, is_normalised, logE;
  float emin, emax, base, span;
};

__global__ void __launch_bounds__(256) gen_cond_kernel(GenCondArgs a) {
  const int cs = a.cond ? a.cond_size : 1;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.batch * cs) return;
  const int b = idx / cs, c = idx - b * cs;
  if (c == 0) {
    const float e = a.is_normalised ? a.energy[b] : energy_to_cond(a.energy[b], a.emin, a.emax, a.logE);
    a.e_norm[b] = e;
    a.e_phys[b] = cond_to_energy(e, a.emin, a.base, a.span, a.logE);
    if (a.cond) a.cond[(size_t)b * cs] = e;
  } else {
    a.cond[(size_t)b * cs + c] = a.layers[(size_t)b * (cs - 1) + (c - 1)];
  }
}

void launch_gen_cond(const GenCondArgs& a, hipStream_t s) {
  const int n = a.batch * (a.cond ? a.cond_size : 1);
  hipLaunchKernelGGL(gen_cond_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
  CD_HIP(hipGetLastError());
}

// one stage's compiled sampler, host copy
struct Stage {
  cdgen::Sampler h;
  std::vector<CdStep> steps;
  std::vector<CdSamplerOp> ops;
  std::vector<int32_t> op_begin;
  std::vector<float> coefs;
  bool table_draws = false;  // a CdStep table with a non-zero ddim_sigma: per-step noise
  void take(const cdgen::Sampler& s) {
    h = s;
    if (s.kind == 0) {
      steps.resize((size_t)s.n_steps);
      memcpy(steps.data(), s.steps, steps.size() * sizeof(CdStep));
      for (const CdStep& r : steps) table_draws = table_draws || r.ddim_sigma != 0.f;
      return;
    }
    ops.resize((size_t)s.n_ops);
    memcpy(ops.data(), s.ops, ops.size() * sizeof(CdSamplerOp));
    if (s.has_op_begin) {
      op_begin.resize((size_t)s.n_steps + 1);
      memcpy(op_begin.data(), s.op_begin, op_begin.size() * sizeof(int32_t));
    }
    coefs.resize((size_t)s.n_steps * (size_t)s.n_coef);
    memcpy(coefs.data(), s.coefs, coefs.size() * sizeof(float));
  }
};

}  // namespace
}  // namespace cd

struct CdGenerator {
  cdgen::Meta meta;
  cdgen::RevNorm rev;
  uint32_t version = 0;
  int64_t voxels = 0;
  CdPlan* plan = nullptr;
  CdLayerMlpDesc ldesc{};
  Stage unet, layer;
  // the one device block: the layer model's weights, then its step table or program
  char* block = nullptr;
  std::vector<const float*> layer_w;
  const CdStep* d_lsteps = nullptr;
  const CdSamplerOp* d_lops = nullptr;
  const int32_t* d_lop_begin = nullptr;
  const float* d_lcoefs = nullptr;
  ~CdGenerator() {
    if (plan) (void)cd_plan_destroy(plan);
    if (block) (void)hipFree(block);
  }
};

namespace cd {
namespace {

void load_unet(CdGenerator* g, const cdgen::Net& net, hipStream_t s) {
  CdUnetDesc desc;
  CD_REQUIRE(net.desc_bytes == sizeof(CdUnetDesc), "generator file: its CdUnetDesc was written against another calodiff.h");
  memcpy(&desc, net.desc, sizeof(desc));
  CD_REQUIRE(desc.grid[0] == g->rev.dims[0] && desc.grid[1] == g->rev.dims[1] && desc.grid[2] == g->rev.dims[2] &&
                 desc.cond_size == g->meta.cond_size,
             "generator file: the U-Net's grid or conditioning width disagrees with its META / RNRM records");
  call(cd_plan_create(&desc, &g->plan));
  std::vector<float> coord[3];
  for (int i = 0; i < 3; ++i) {
    coord[i].resize(net.n_coord[i]);
    memcpy(coord[i].data(), net.coord[i], coord[i].size() * sizeof(float));
  }
  call(cd_plan_set_coords(g->plan, coord[0].data(), coord[1].data(), coord[2].data(), s));
  // every tensor the plan names, from the file, through a staging block that is freed before create returns
  std::unordered_map<std::string, const cdgen::Weight*> by_name;
  for (const cdgen::Weight& w : net.weights) by_name[w.name] = &w;
  int n = 0;
  call(cd_plan_num_weights(g->plan, &n));
  if ((size_t)n != net.weights.size())
    throw Fail{CD_EWEIGHTS, "generator file: " + std::to_string(net.weights.size()) + " U-Net tensors, the plan takes " + std::to_string(n)};
  std::vector<const cdgen::Weight*> order((size_t)n);
  std::vector<size_t> off((size_t)n);
  size_t total = 0;
  char name[256];
  for (int i = 0; i < n; ++i) {
    int64_t numel = 0;
    call(cd_plan_weight_name(g->plan, i, name, (int)sizeof(name), &numel));
    auto it = by_name.find(name);
    if (it == by_name.end()) throw Fail{CD_EWEIGHTS, std::string("generator file: no U-Net tensor named '") + name + "'"};
    if ((int64_t)it->second->numel != numel)
      throw Fail{CD_EWEIGHTS, std::string("generator file: tensor '") + name + "' has " + std::to_string(it->second->numel) +
                                  " elements, the plan expects " + std::to_string(numel)};
    order[i] = it->second;
    off[i] = total;
    total += aligned((size_t)numel * sizeof(float));
  }
  DeviceBlock staging;
  CD_HIP(hipMalloc(&staging.p, total));
  std::vector<const float*> ptrs((size_t)n);
  for (int i = 0; i < n; ++i) {
    ptrs[i] = (const float*)((char*)staging.p + off[i]);
    CD_HIP(hipMemcpyAsync((char*)staging.p + off[i], order[i]->data, (size_t)order[i]->numel * sizeof(float), hipMemcpyHostToDevice, s));
  }
  call(cd_plan_set_weights(g->plan, n, ptrs.data(), s));
  CD_HIP(hipStreamSynchronize(s));  // the packed images are complete: the staging block goes
}

void load_layer(CdGenerator* g, const cdgen::Net& net, hipStream_t s) {
  CD_REQUIRE(net.desc_bytes == sizeof(CdLayerMlpDesc), "generator file: its CdLayerMlpDesc was written against another calodiff.h");
  memcpy(&g->ldesc, net.desc, sizeof(CdLayerMlpDesc));
  const CdLayerMlpDesc& d = g->ldesc;
  CD_REQUIRE(d.struct_size == sizeof(CdLayerMlpDesc) && d.n_res >= 0 && d.n_res <= 8 && d.dim_in == g->meta.layer_dim && d.cond_size == 1,
             "generator file: the layer model's descriptor disagrees with its META record");
  if (net.weights.size() != (size_t)(2 * (8 + 3 * d.n_res)))
    throw Fail{CD_EWEIGHTS, "generator file: the layer model has " + std::to_string(net.weights.size()) + " tensors, 2*(8 + 3*n_res) expected"};
  const Stage& st = g->layer;
  size_t total = 0;
  std::vector<size_t> off;
  for (const cdgen::Weight& w : net.weights) {
    off.push_back(total);
    total += aligned((size_t)w.numel * sizeof(float));
  }
  const size_t o_steps = total;
  total += aligned(st.steps.size() * sizeof(CdStep));
  const size_t o_ops = total;
  total += aligned(st.ops.size() * sizeof(CdSamplerOp));
  const size_t o_begin = total;
  total += aligned(st.op_begin.size() * sizeof(int32_t));
  const size_t o_coefs = total;
  total += aligned(st.coefs.size() * sizeof(float));
  CD_HIP(hipMalloc((void**)&g->block, total));
  for (size_t i = 0; i < net.weights.size(); ++i) {
    g->layer_w.push_back((const float*)(g->block + off[i]));
    CD_HIP(hipMemcpyAsync(g->block + off[i], net.weights[i].data, (size_t)net.weights[i].numel * sizeof(float), hipMemcpyHostToDevice, s));
  }
  auto put = [&](size_t o, const void* src, size_t bytes) -> const void* {
    if (!bytes) return nullptr;
    CD_HIP(hipMemcpyAsync(g->block + o, src, bytes, hipMemcpyHostToDevice, s));
    return g->block + o;
  };
  g->d_lsteps = (const CdStep*)put(o_steps, st.steps.data(), st.steps.size() * sizeof(CdStep));
  g->d_lops = (const CdSamplerOp*)put(o_ops, st.ops.data(), st.ops.size() * sizeof(CdSamplerOp));
  g->d_lop_begin = (const int32_t*)put(o_begin, st.op_begin.data(), st.op_begin.size() * sizeof(int32_t));
  g->d_lcoefs = (const float*)put(o_coefs, st.coefs.data(), st.coefs.size() * sizeof(float));
  CD_HIP(hipStreamSynchronize(s));  // the host copies may go
}

// the caller's workspace, dealt in one fixed order by the dry run and by every call
struct RunBuffers {
  float *start, *x, *cond, *e_norm, *e_phys, *lstart, *lout, *lnoise;
  void* net;
  size_t net_bytes;
};

RunBuffers deal(CdGenerator* g, int batch, Arena& ar) {
  RunBuffers b{};
  const size_t B = (size_t)batch, vox = (size_t)g->voxels, dim = (size_t)g->meta.layer_dim;
  b.start = ar.get<float>(B * vox);
  b.x = ar.get<float>(B * vox);
  b.cond = ar.get<float>(B * (size_t)g->meta.cond_size);
  b.e_norm = ar.get<float>(B);
  b.e_phys = ar.get<float>(B);
  if (g->meta.has_layer_stage) {
    b.lstart = ar.get<float>(B * dim);
    b.lout = ar.get<float>(B * dim);
    if (g->layer.table_draws) b.lnoise = ar.get<float>((size_t)g->layer.h.n_steps * B * dim);
  }
  if (g->unet.h.kind == 0)
    call(cd_plan_workspace_bytes(g->plan, batch, &b.net_bytes));
  else
    call(cd_plan_sampler_workspace_bytes(g->plan, batch, g->unet.h.n_bufs, g->unet.h.n_steps, g->unet.h.n_coef, &b.net_bytes));
  b.net = ar.alloc(b.net_bytes);
  return b;
}

size_t workspace_need(CdGenerator* g, int batch) {
  Arena ar;
  ar.reset(nullptr, 0, true);
  deal(g, batch, ar);
  return ar.high();
}

}  // namespace
}  // namespace cd

extern "C" {

int cd_generator_create(const void* blob, size_t bytes, CdGenerator** out, void* stream) {
  return guarded([&] {
    CD_REQUIRE(blob && out, "null argument");
    cdgen::Blob view;
    std::string err;
    if (!cdgen::parse(blob, bytes, &view, &err)) throw Fail{CD_EINVAL, err};
    std::unique_ptr<CdGenerator> g(new CdGenerator());
    g->meta = view.meta; g->rev = view.rev; g->version = view.version;
    g->voxels = (int64_t)view.rev.dims[0] * view.rev.dims[1] * view.rev.dims[2];
    g->unet.take(view.unet_sampler);
    hipStream_t s = (hipStream_t)stream;
    load_unet(g.get(), view.unet, s);
    if (view.meta.has_layer_stage) {
      g->layer.take(view.layer_sampler);
      load_layer(g.get(), view.layer, s);
    }
    *out = g.release();
  });
}

int cd_generator_destroy(CdGenerator* gen) {
  return guarded([&] { delete gen; });
}

int cd_generator_checksum(const void* data, size_t bytes, uint64_t* out) {
  return guarded([&] {
    CD_REQUIRE((data || bytes == 0) && out, "null argument");
    *out = cdgen::fnv1a64((const unsigned char*)data, (uint64_t)bytes);
  });
}

int cd_generator_info(const CdGenerator* gen, int32_t* info) {
  return guarded([&] {
    CD_REQUIRE(gen && info, "null argument");
    const cdgen::Meta& m = gen->meta;
    const int32_t v[8] = {(int32_t)gen->voxels, gen->rev.dims[0], m.energy_cols, m.has_layer_stage, m.takes_layers, m.sample_steps,
                          m.has_layer_stage ? m.layer_steps : 0, (int32_t)gen->version};
    memcpy(info, v, sizeof(v));
  });
}

int cd_generator_workspace_bytes(CdGenerator* gen, int batch, size_t* bytes) {
  return guarded([&] {
    CD_REQUIRE(gen && bytes && batch > 0, "bad argument");
    *bytes = workspace_need(gen, batch);
  });
}

int cd_generator_run(CdGenerator* gen, int batch, const float* energy, int energy_is_normalised, const float* layers, uint64_t seed,
                     uint64_t offset, int first_row, int global_batch, float* showers, float* layers_out, uint64_t* next_offset,
                     void* workspace, size_t workspace_bytes, void* stream) {
  return guarded([&] {
    CD_REQUIRE(gen && energy && showers && workspace && batch > 0, "bad argument");
    const cdgen::Meta& m = gen->meta;
    const cdgen::RevNorm& r = gen->rev;
    if (global_batch == 0 && first_row == 0) global_batch = batch;
    CD_REQUIRE(first_row >= 0 && (int64_t)first_row + batch <= (int64_t)global_batch,
               "cd_generator_run: rows [first_row, first_row + batch) exceed global_batch (0, batch = unsharded)");
    const bool given_layers = m.takes_layers && !m.has_layer_stage;
    CD_REQUIRE(!given_layers || layers, "cd_generator_run: this model conditions on layer energies and has no layer stage: `layers` "
                                        "(batch, 1 + layers) is required");
    CD_REQUIRE(given_layers || !layers, m.has_layer_stage ? "cd_generator_run: this model generates its layer energies itself: `layers` must be NULL"
                                                          : "cd_generator_run: this model takes no layer energies: `layers` must be NULL");
    if (workspace_bytes < workspace_need(gen, batch))
      throw Fail{CD_EWORKSPACE, "workspace too small: call cd_generator_workspace_bytes for this batch size"};
    hipStream_t s = (hipStream_t)stream;
    Arena ar;
    ar.reset((char*)workspace, workspace_bytes, false);
    const RunBuffers b = deal(gen, batch, ar);

    const uint64_t B = (uint64_t)batch, gb = (uint64_t)global_batch, lo = (uint64_t)first_row;
    const uint64_t per = (uint64_t)gen->voxels, dim = (uint64_t)m.layer_dim;
    uint64_t off = offset;
    // Diffusion.noise_generation: this shard's rows of the global start tensor, then the stream moves past the whole tensor
    call(cd_randn(b.start, (int64_t)(B * per), seed, off + lo * per, s));
    off += gb * per;

    GenCondArgs c{};
    c.energy = energy; c.e_norm = b.e_norm; c.e_phys = b.e_phys;
    c.batch = batch; c.cond_size = m.cond_size; c.is_normalised = energy_is_normalised ? 1 : 0; c.logE = r.logE;
    c.emin = (float)r.emin; c.emax = (float)r.emax; c.base = (float)(r.emax / r.emin); c.span = (float)(r.emax - r.emin);
    const float* layer_e = layers;
    if (m.has_layer_stage) {
      launch_gen_cond(c, s);  // the energies: the layer model conditions on e alone
      call(cd_randn(b.lstart, (int64_t)(B * dim), seed, off + lo * dim, s));
      off += gb * dim;
      float* lout = layers_out ? layers_out : b.lout;
      const Stage& st = gen->layer;
      const int nw = (int)gen->layer_w.size();
      if (st.h.kind == 0) {
        // LayerMlpEngine.ddim_sample: the noise of a stochastic table is ONE (n_steps, B, dim) block at the stream position
        if (st.table_draws) call(cd_randn(b.lnoise, (int64_t)((uint64_t)st.h.n_steps * B * dim), seed, off + lo * dim, s));
        call(cd_layer_sample(&gen->ldesc, gen->layer_w.data(), nw, batch, b.lstart, b.e_norm, gen->d_lsteps, st.h.n_steps,
                             st.table_draws ? b.lnoise : nullptr, lout, nullptr, nullptr, s));
        off += B * dim * (uint64_t)m.layer_steps;  // LayerDiffusion.sample_layers: start.numel() * layer_steps
      } else {
        call(cd_layer_sampler_run(&gen->ldesc, gen->layer_w.data(), nw, batch, b.lstart, st.h.start_scale, b.e_norm, st.h.n_bufs,
                                  st.h.n_steps, gen->d_lops, st.h.n_ops, gen->d_lop_begin, gen->d_lcoefs, st.h.n_coef, nullptr, seed,
                                  off + lo * dim, gb * dim, lout, nullptr, nullptr, s));
        off += gb * dim * (uint64_t)st.h.noise_tensors_drawn;
      }
      layer_e = lout;
    } else if (layers && layers_out) {
      CD_HIP(hipMemcpyAsync(layers_out, layers, B * dim * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    c.layers = layer_e; c.cond = b.cond;
    launch_gen_cond(c, s);

    const Stage& st = gen->unet;
    if (st.h.kind == 0) {
      call(cd_ddim_sample(gen->plan, batch, b.start, b.cond, st.steps.data(), st.h.n_steps, nullptr, seed, off + lo * per, gb * per, b.x,
                          nullptr, nullptr, st.h.use_graph, b.net, b.net_bytes, s));
    } else {
      call(cd_sampler_run(gen->plan, batch, b.start, st.h.start_scale, b.cond, st.h.n_bufs, st.h.n_steps, st.ops.data(), st.h.n_ops,
                          st.h.has_op_begin ? st.op_begin.data() : nullptr, st.coefs.data(), st.h.n_coef, nullptr, seed, off + lo * per,
                          gb * per, b.x, nullptr, nullptr, st.h.use_graph, b.net, b.net_bytes, s));
    }
    // LayerDiffusion.sample: start.numel() * num_steps; Diffusion.sample: one global tensor per noise tensor drawn
    off += m.has_layer_stage ? B * per * (uint64_t)m.sample_steps : gb * per * (uint64_t)st.h.noise_tensors_drawn;

    call(cd_reverse_norm(b.x, b.e_phys, r.layer_map ? layer_e : nullptr, showers, batch, r.dims, r.consts, r.max_deposit, r.ecut, s));
    if (next_offset) *next_offset = off;
  });
}

}  // extern "C"
