// cd_generator_*: "incident energies in, physical showers out" from a generator file (generator_blob.h), without Python.
// The run is the launch sequence of Diffusion.generate / LayerDiffusion.generate, issued through the library's own entry points
// (cd_randn, cd_layer_sample / cd_layer_sampler_run, cd_ddim_sample / cd_sampler_run, cd_reverse_norm; for an HGCal file
// cd_reverse_norm_staged around cd_geom_apply / cd_geom_decode_sparse, ReverseNormHGCal's tail; for a Dataset-0/1 file
// cd_reverse_norm_ds1 over the file's radial map) with the Philox offsets the Python path hands them; the kernels of its own are the conditioning row and the sampled decode's input scaling.
#include "arena.h"
#include "energy_map.h"
#include "generator_blob.h"
#include "guarded.h"
#include "kernels_geom.h"

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
// (b, c) writes column c of row b.  Columns 0 .. cols - 1 are e -- the input itself, or the map of a physical energy:
// energy_to_cond for the regular grids' one column, energy_to_cond_hgcal per column for HGCal -- and also go to e_norm (the layer
// stage's (B, cols) condition); column 0, mapped back by cond_to_energy / cond_to_energy_hgcal, goes to e_phys (the energies the
// inverse pre-processing scales by); the layer energies follow.  cond == null: the energies only (before a layer stage has
// produced the layers).
// ------------------------------------------------------------------------------------------------------------
struct GenCondArgs {
  const float* energy;  // (B, cols) normalised e, or physical energies
  const float* layers;  // (B, cond_size - cols) or null
  float* cond;          // (B, cond_size) or null
  float* e_norm;        // (B, cols)
  float* e_phys;        // (B)
  int batch, cond_size, cols, is_normalised, logE, hgcal;
  float emin, emax, base, span;
  double emin_col[cdgen::kMaxEnergyCols], emax_col[cdgen::kMaxEnergyCols], span0;  // hgcal
};

__global__ void __launch_bounds__(256) gen_cond_kernel(GenCondArgs a) {
  const int cs = a.cond ? a.cond_size : a.cols;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.batch * cs) return;
  const int b = idx / cs, c = idx - b * cs;
  if (c < a.cols) {
    const float in = a.energy[(size_t)b * a.cols + c];
    const float e = a.is_normalised ? in : a.hgcal ? energy_to_cond_hgcal(in, a.emin_col[c], a.emax_col[c]) : energy_to_cond(in, a.emin, a.emax, a.logE);
    a.e_norm[(size_t)b * a.cols + c] = e;
    if (c == 0) a.e_phys[b] = a.hgcal ? cond_to_energy_hgcal(e, a.emin_col[0], a.span0) : cond_to_energy(e, a.emin, a.base, a.span, a.logE);
    if (a.cond) a.cond[(size_t)b * cs + c] = e;
  } else {
    a.cond[(size_t)b * cs + c] = a.layers[(size_t)b * (cs - a.cols) + (c - a.cols)];
  }
}

void launch_gen_cond(const GenCondArgs& a, hipStream_t s) {
  const int n = a.batch * (a.cond ? a.cond_size : a.cols);
  hipLaunchKernelGGL(gen_cond_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
  CD_HIP(hipGetLastError());
}

// The sampled decode's input, x * embed_std + embed_mean as Decoder._decode forms it with two torch operations: product and sum
// rounded one by one
__global__ void __launch_bounds__(256) gen_affine_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n, float scale, float shift) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) y[i] = __fadd_rn(__fmul_rn(x[i], scale), shift);
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
  int64_t voxels = 0;  // of a shower as the run returns it
  int64_t per = 0;     // of the sampler's state: the grid, the cells of an in-model HGCal file, the flat shower of an in-model Dataset-0/1 file
  // HGCal (format version 2): form -1 none, 0 pre-embedded (dec with its column view), 1 in-model (enc, dec bound to the plan)
  int form = -1, cells = 0;
  float embed_mean = 0.f, embed_std = 1.f;
  CdGeomMap *enc = nullptr, *dec = nullptr;
  // Dataset 0 / 1 (format version 3): rform -1 none, 0 on the converted grid (r_dec = the un-conversion matrices, the run's last
  // step reads them), 1 in-model (r_enc, r_dec bound to the plan); both in the one block r_block
  int rform = -1;
  CdRadialMap* rmap = nullptr;
  char* r_block = nullptr;
  const float *r_enc = nullptr, *r_dec = nullptr;
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
    if (plan) (void)cd_plan_destroy(plan);  // (before the maps it reads)
    if (enc) (void)cd_geom_destroy(enc);
    if (dec) (void)cd_geom_destroy(dec);
    if (rmap) (void)cd_radial_destroy(rmap);
    if (r_block) (void)hipFree(r_block);
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
  CD_REQUIRE(d.struct_size == sizeof(CdLayerMlpDesc) && d.n_res >= 0 && d.n_res <= 8 && d.dim_in == g->meta.layer_dim && d.cond_size == g->meta.energy_cols,
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

// One map of the GEOM section onto the device: the file's arrays may be unaligned, so they are copied out (O(entries) host
// memory, never the dense tensor) and handed to cd_geom_create_csr, which checks them again and builds the views
CdGeomMap* load_geom_map(const cdgen::GeomMap& m, int layers, int flags, hipStream_t s) {
  std::vector<int32_t> row_ptr((size_t)layers * (size_t)m.rows + 1), col_idx((size_t)m.nnz);
  std::vector<float> val((size_t)m.nnz);
  memcpy(row_ptr.data(), m.row_ptr, row_ptr.size() * sizeof(int32_t));
  if (m.nnz) {
    memcpy(col_idx.data(), m.col_idx, col_idx.size() * sizeof(int32_t));
    memcpy(val.data(), m.val, val.size() * sizeof(float));
  }
  CdGeomMap* out = nullptr;
  call(cd_geom_create_csr(row_ptr.data(), col_idx.data(), val.data(), layers, m.rows, m.cols, flags, &out, s));
  return out;
}

// The RADL section onto the device: the layout through cd_radial_create (which checks it again), the matrices into one block.  The
// file's arrays may be unaligned, so they are copied out first.
void load_radial(CdGenerator* g, const cdgen::Radial& r, hipStream_t s) {
  const size_t L = (size_t)r.layers, wt = (size_t)r.wtotal;
  std::vector<int32_t> bound(L + 1), alpha(L), rin(L);
  memcpy(bound.data(), r.bound, bound.size() * sizeof(int32_t));
  memcpy(alpha.data(), r.alpha, alpha.size() * sizeof(int32_t));
  memcpy(rin.data(), r.rin, rin.size() * sizeof(int32_t));
  call(cd_radial_create(r.layers, bound.data(), alpha.data(), rin.data(), r.alpha_out, r.r_out, &g->rmap, s));
  const size_t one = aligned(wt * sizeof(float));
  std::vector<float> host((size_t)r.n_mats * wt);
  if (r.form == 1) memcpy(host.data(), r.enc, wt * sizeof(float));
  memcpy(host.data() + (size_t)(r.n_mats - 1) * wt, r.dec, wt * sizeof(float));
  CD_HIP(hipMalloc((void**)&g->r_block, (size_t)r.n_mats * one));
  for (int k = 0; k < r.n_mats; ++k)
    CD_HIP(hipMemcpyAsync(g->r_block + (size_t)k * one, host.data() + (size_t)k * wt, wt * sizeof(float), hipMemcpyHostToDevice, s));
  CD_HIP(hipStreamSynchronize(s));  // the host copy may go
  g->rform = r.form;
  g->r_dec = (const float*)(g->r_block + (size_t)(r.n_mats - 1) * one);
  g->voxels = r.voxels;
  if (r.form == 1) {
    g->r_enc = (const float*)g->r_block;
    g->per = r.voxels;
    call(cd_plan_set_radial(g->plan, g->rmap, g->r_enc, g->r_dec, 0, s));
  }
}

// the caller's workspace, dealt in one fixed order by the dry run and by every call
struct RunBuffers {
  float *start, *x, *cond, *e_norm, *e_phys, *lstart, *lout, *lnoise;
  void* net;
  size_t net_bytes;
  float* decoded;  // form 0: (B, L, N)
  void* count_ws;  // form 0: the sampled decode's (argmax, count) per (b, l, e)
};

RunBuffers deal(CdGenerator* g, int batch, Arena& ar) {
  RunBuffers b{};
  const size_t B = (size_t)batch, vox = (size_t)g->per, dim = (size_t)g->meta.layer_dim;
  b.start = ar.get<float>(B * vox);
  b.x = ar.get<float>(B * vox);
  b.cond = ar.get<float>(B * (size_t)g->meta.cond_size);
  b.e_norm = ar.get<float>(B * (size_t)g->meta.energy_cols);
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
  if (g->form == 0) {
    size_t count_bytes = 0;
    call(cd_geom_sparse_workspace_bytes(g->dec, batch, &count_bytes));
    b.decoded = ar.get<float>(B * (size_t)g->voxels);
    b.count_ws = ar.alloc(count_bytes);
  }
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
    g->voxels = g->per = (int64_t)view.rev.dims[0] * view.rev.dims[1] * view.rev.dims[2];
    g->unet.take(view.unet_sampler);
    hipStream_t s = (hipStream_t)stream;
    load_unet(g.get(), view.unet, s);
    if (view.geom.form >= 0) {
      const cdgen::Geom& gm = view.geom;
      g->form = gm.form; g->cells = gm.cells; g->embed_mean = gm.embed_mean; g->embed_std = gm.embed_std;
      g->voxels = (int64_t)gm.layers * gm.cells;
      if (gm.form == 0) {
        g->dec = load_geom_map(gm.dec, gm.layers, CD_GEOM_COLUMNS, s);
      } else {
        g->per = g->voxels;
        g->enc = load_geom_map(gm.enc, gm.layers, CD_GEOM_TRANSPOSED, s);
        g->dec = load_geom_map(gm.dec, gm.layers, CD_GEOM_TRANSPOSED, s);
        call(cd_plan_set_geom(g->plan, g->enc, g->dec, 0, s));
      }
    }
    if (view.radial.form >= 0) load_radial(g.get(), view.radial, s);
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

int cd_generator_geometry(const CdGenerator* gen, int32_t* geom) {
  return guarded([&] {
    CD_REQUIRE(gen && geom, "null argument");
    const cdgen::Meta& m = gen->meta;
    const int32_t v[8] = {gen->form >= 0 ? 1 : gen->rform >= 0 ? 2 : 0, gen->form >= 0 ? gen->form : gen->rform, m.data_ndim,
                          m.data_shape[0], m.data_shape[1], m.data_shape[2], m.data_shape[3], 0};
    memcpy(geom, v, sizeof(v));
  });
}

int cd_generator_workspace_bytes(CdGenerator* gen, int batch, size_t* bytes) {
  return guarded([&] {
    CD_REQUIRE(gen && bytes && batch > 0, "bad argument");
    *bytes = workspace_need(gen, batch);
  });
}

int cd_generator_run_ex(CdGenerator* gen, const CdGeneratorRun* args) {
  return guarded([&] {
    CD_REQUIRE(gen && args, "bad argument");
    CD_REQUIRE(args->struct_size == sizeof(CdGeneratorRun),
               "cd_generator_run_ex: struct_size is not sizeof(CdGeneratorRun): the caller was built against another calodiff.h");
    const int batch = args->batch;
    const float *energy = args->energy, *layers = args->layers;
    float *showers = args->showers, *layers_out = args->layers_out;
    int first_row = args->first_row, global_batch = args->global_batch;
    const uint64_t seed = args->seed, offset = args->offset;
    void* workspace = args->workspace;
    const size_t workspace_bytes = args->workspace_bytes;
    CD_REQUIRE(energy && showers && workspace && batch > 0, "bad argument");
    const cdgen::Meta& m = gen->meta;
    const cdgen::RevNorm& r = gen->rev;
    if (global_batch == 0 && first_row == 0) global_batch = batch;
    CD_REQUIRE(first_row >= 0 && (int64_t)first_row + batch <= (int64_t)global_batch,
               "cd_generator_run: rows [first_row, first_row + batch) exceed global_batch (0, batch = unsharded)");
    CD_REQUIRE(args->sparse_mode >= 0 && args->sparse_mode <= 2, "cd_generator_run_ex: sparse_mode is 0 (plain decode), 1 (per shower) or 2 (per batch)");
    CD_REQUIRE(args->sparse_mode == 0 || (gen->form == 0 && gen->dec && gen->dec->col_ptr),
               "cd_generator_run_ex: sparse_mode != 0 needs a file whose decoder has a column view (a pre-embedded HGCal model's): this "
               "file has no sampled decode step");
    const bool given_layers = m.takes_layers && !m.has_layer_stage;
    CD_REQUIRE(!given_layers || layers, "cd_generator_run: this model conditions on layer energies and has no layer stage: `layers` "
                                        "(batch, 1 + layers) is required");
    CD_REQUIRE(given_layers || !layers, m.has_layer_stage ? "cd_generator_run: this model generates its layer energies itself: `layers` must be NULL"
                                                          : "cd_generator_run: this model takes no layer energies: `layers` must be NULL");
    if (workspace_bytes < workspace_need(gen, batch))
      throw Fail{CD_EWORKSPACE, "workspace too small: call cd_generator_workspace_bytes for this batch size"};
    hipStream_t s = (hipStream_t)args->stream;
    Arena ar;
    ar.reset((char*)workspace, workspace_bytes, false);
    const RunBuffers b = deal(gen, batch, ar);

    const uint64_t B = (uint64_t)batch, gb = (uint64_t)global_batch, lo = (uint64_t)first_row;
    const uint64_t per = (uint64_t)gen->per, dim = (uint64_t)m.layer_dim;
    uint64_t off = offset;
    // Diffusion.noise_generation: this shard's rows of the global start tensor, then the stream moves past the whole tensor
    call(cd_randn(b.start, (int64_t)(B * per), seed, off + lo * per, s));
    off += gb * per;

    GenCondArgs c{};
    c.energy = energy; c.e_norm = b.e_norm; c.e_phys = b.e_phys;
    c.batch = batch; c.cond_size = m.cond_size; c.cols = m.energy_cols; c.is_normalised = args->energy_is_normalised ? 1 : 0; c.logE = r.logE;
    c.emin = (float)r.emin; c.emax = (float)r.emax; c.base = (float)(r.emax / r.emin); c.span = (float)(r.emax - r.emin);
    c.hgcal = gen->form >= 0;
    for (int k = 0; k < m.energy_cols; ++k) {
      c.emin_col[k] = r.emin_col[k];
      c.emax_col[k] = r.emax_col[k];
    }
    c.span0 = r.emax_col[0] - r.emin_col[0];
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

    uint64_t decode_next = args->decode_offset;
    if (gen->rform >= 0) {
      // ReverseNormCaloChall for Dataset 0 / 1: the flat form with the layer energies (in-model), the grid form through the
      // un-conversion matrices
      call(cd_reverse_norm_ds1(gen->rmap, gen->rform == 0 ? gen->r_dec : nullptr, b.x, b.e_phys, r.layer_map ? layer_e : nullptr, showers,
                               batch, r.consts64, r.max_deposit, r.ecut, s));
    } else if (gen->form < 0) {
      call(cd_reverse_norm(b.x, b.e_phys, r.layer_map ? layer_e : nullptr, showers, batch, r.dims, r.consts, r.max_deposit, r.ecut, s));
    } else {
      // ReverseNormHGCal: stage 1 on the sampler's output (the start tensor's block is free again), the decode of a pre-embedded
      // model, stage 2 on the cells (the reference's energy cut is disabled: ecut 0)
      const int32_t flat[3] = {(int32_t)per, 1, 1};
      call(cd_reverse_norm_staged(b.x, nullptr, nullptr, b.start, batch, flat, r.consts, r.max_deposit, 0.f, r.alpha, r.layer_eps, 1, s));
      const float* cells = b.start;
      if (gen->form == 0) {
        if (args->sparse_mode == 0) {
          call(cd_geom_apply(gen->dec, b.start, b.decoded, batch, gen->embed_std, gen->embed_mean, 1, s));
        } else {
          const float* x = b.start;
          if (gen->embed_std != 1.f || gen->embed_mean != 0.f) {
            const int64_t n = (int64_t)(B * per);
            hipLaunchKernelGGL(gen_affine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, b.start, b.x, n, gen->embed_std, gen->embed_mean);
            CD_HIP(hipGetLastError());
            x = b.x;
          }
          const int per_batch = args->sparse_mode == 2;
          call(cd_geom_decode_sparse(gen->dec, x, b.decoded, batch, 1, per_batch, nullptr, args->decode_seed, args->decode_offset, b.count_ws, s));
          decode_next += (per_batch ? 1ull : B) * (uint64_t)gen->voxels * (uint64_t)(r.dims[1] * r.dims[2]);
        }
        cells = b.decoded;
      }
      const int32_t by_layer[3] = {r.dims[0], 1, gen->cells}, whole[3] = {1, 1, (int32_t)gen->voxels};
      call(cd_reverse_norm_staged(cells, b.e_phys, r.layer_map ? layer_e : nullptr, showers, batch, r.layer_map ? by_layer : whole, r.consts,
                                  r.max_deposit, 0.f, r.alpha, r.layer_eps, 2, s));
    }
    if (args->next_offset) *args->next_offset = off;
    if (args->next_decode_offset) *args->next_decode_offset = decode_next;
  });
}

int cd_generator_run(CdGenerator* gen, int batch, const float* energy, int energy_is_normalised, const float* layers, uint64_t seed,
                     uint64_t offset, int first_row, int global_batch, float* showers, float* layers_out, uint64_t* next_offset,
                     void* workspace, size_t workspace_bytes, void* stream) {
  CdGeneratorRun a{};
  a.struct_size = sizeof(CdGeneratorRun);
  a.batch = batch; a.energy = energy; a.energy_is_normalised = energy_is_normalised; a.layers = layers; a.seed = seed; a.offset = offset;
  a.first_row = first_row; a.global_batch = global_batch; a.showers = showers; a.layers_out = layers_out; a.next_offset = next_offset;
  a.workspace = workspace; a.workspace_bytes = workspace_bytes; a.stream = stream;
  return cd_generator_run_ex(gen, &a);
}

}  // extern "C"
