// Sampler entry points: the DDIM loop (cd_ddim_sample) and uniform sampler programs (cd_sampler_run), each with a cached step
// graph, and the device Philox noise (cd_randn).
#include "plan_internal.h"

#include <cstdlib>

namespace cd {

// `count` repetitions of `step(stream)` captured on the plan's private stream (the caller's may be the legacy null stream, which
// cannot capture) as one graph, instantiated
template <typename F>
hipGraphExec_t capture_steps(CdPlan* p, int count, F&& step) {
  if (!p->cap_stream) CD_HIP(hipStreamCreateWithFlags(&p->cap_stream, hipStreamNonBlocking));
  hipStream_t cs = p->cap_stream;
  hipGraph_t graph = nullptr;
  CD_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeRelaxed));
  try {
    for (int k = 0; k < count; ++k) step(cs);
  } catch (...) {
    hipStreamEndCapture(cs, &graph);
    if (graph) hipGraphDestroy(graph);
    throw;
  }
  CD_HIP(hipStreamEndCapture(cs, &graph));
  hipGraphExec_t exec = nullptr;
  hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  hipGraphDestroy(graph);
  if (e != hipSuccess) throw Fail{CD_EHIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e)};
  return exec;
}

// the device Philox words {seed, base offset, stride} of launch_randn_step; synchronises: `so` lives on this stack frame
void upload_noise_words(uint64_t* noise_dev, uint64_t seed, uint64_t offset, uint64_t stride, hipStream_t s) {
  const uint64_t so[3] = {seed, offset, stride};
  CD_HIP(hipMemcpyAsync(noise_dev, so, sizeof(so), hipMemcpyHostToDevice, s));
  CD_HIP(hipStreamSynchronize(s));
}

// A sampler step program is checked on the host before anything is enqueued: a bad buffer index would be a wild device pointer
// (cd_sampler_run) or address outside the on-chip buffers (cd_layer_sampler_run).  The callers have checked the sizes.
SamplerProgramCounts validate_sampler_program(const CdSamplerOp* ops, const int32_t* op_begin, int n_steps, int n_ops, int n_bufs,
                                              int n_coef, int batch) {
  if (op_begin) {
    CD_REQUIRE(op_begin[0] == 0 && op_begin[n_steps] == n_ops, "op_begin must run from 0 to n_ops");
    for (int i = 0; i < n_steps; ++i) CD_REQUIRE(op_begin[i] <= op_begin[i + 1], "op_begin must be non-decreasing");
  }
  SamplerProgramCounts c;
  for (int k = 0; k < n_ops; ++k) {
    const CdSamplerOp& o = ops[k];
    CD_REQUIRE(o.kind >= CD_SOP_LINCOMB && o.kind <= CD_SOP_DENOISE_PS, "sampler op: unknown kind");
    const bool lin = o.kind == CD_SOP_LINCOMB || o.kind == CD_SOP_LINDIV;
    const int ns = lin ? o.nsrc : (o.kind == CD_SOP_RANDN ? 0 : 1);
    CD_REQUIRE(ns >= 0 && ns <= 6 && (!lin || ns >= 1), "sampler op: 1..6 sources");
    for (int j = 0; j < ns; ++j) CD_REQUIRE(o.src[j] >= 0 && o.src[j] < n_bufs, "sampler op: source buffer out of range");
    if (o.kind == CD_SOP_RECORD) CD_REQUIRE(o.dst == 0 || o.dst == 1, "record op: dst is 0 (xs) or 1 (x0s)");
    else CD_REQUIRE(o.dst >= 0 && o.dst < n_bufs, "sampler op: destination buffer out of range");
    if (lin) CD_REQUIRE(o.col >= 0 && o.col + ns + (o.kind == CD_SOP_LINDIV ? 1 : 0) <= n_coef, "lincomb op: coefficient columns out of range");
    if (o.kind == CD_SOP_DENOISE || o.kind == CD_SOP_DENOISE_PS) {
      if (o.kind == CD_SOP_DENOISE) CD_REQUIRE(o.col >= 0 && o.col < n_coef, "denoise op: sigma column out of range");
      else CD_REQUIRE(o.col >= 0 && o.col + batch <= n_coef, "per-sample denoise op: sigma columns out of range (col + batch > n_coef)");
      CD_REQUIRE(o.dst != o.src[0], "denoise op: output must not alias its input");
      c.n_denoise += op_begin ? 1 : n_steps;  // once per step of a uniform program, once otherwise
    }
    if (o.kind == CD_SOP_RANDN) ++c.randn_per_step;
  }
  return c;
}

}  // namespace cd

extern "C" {

int cd_randn(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream) {
  return guarded([&] {
    CD_REQUIRE(out && n >= 0, "bad argument");
    launch_randn(out, n, seed, offset, (hipStream_t)stream);
  });
}

int cd_ddim_sample(CdPlan* plan, int batch, const float* start, const float* cond, const CdStep* steps, int n_steps,
                   const float* step_noise, uint64_t seed, uint64_t offset, uint64_t noise_stride, float* x_out, float* xs,
                   float* x0s, int use_graph, void* workspace, size_t workspace_bytes, void* stream) {
  return guarded([&] {
    CD_REQUIRE(plan && start && cond && steps && x_out && workspace && batch > 0, "bad argument");
    CD_REQUIRE(n_steps >= 1 && n_steps <= CdPlan::kMaxSteps, "n_steps out of range (1..4096)");
    check_ready(plan, true);
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)batch * plan->state_per();
    bool noisy = false;
    for (int i = 0; i < n_steps; ++i) noisy |= steps[i].ddim_sigma != 0.f;

    static_assert(sizeof(CdStep) == 16, "CdStep must be 4 floats");
    CD_HIP(hipMemcpyAsync(plan->d_table, steps, sizeof(CdStep) * n_steps, hipMemcpyHostToDevice, s));

    plan->ws.reset((char*)workspace, workspace_bytes, false);
    float* x0 = plan->ws.get<float>((size_t)n);
    float* noise_buf = plan->ws.get<float>((size_t)n);
    float* sigma_b = plan->ws.get<float>((size_t)batch + 64);
    uint64_t* noise_dev = (uint64_t*)plan->ws.get<double>(4);  // {seed, base offset, stride}
    // Embeddings and EDM scalings depend on (sigma_step, cond) only -- not on x: one launch computes them for kEmbedChunk steps
    // ahead (the per-step embedding kernel was 34 us of pure latency in every 2 ms step), load_step hands each step its slice.
    const int K = CdPlan::kEmbedChunk;
    float* emb_cur = plan->ws.get<float>((size_t)batch * plan->emb_ld);
    float* scal_cur = plan->ws.get<float>((size_t)batch * 4);
    float* emb_chunk = plan->ws.get<float>((size_t)K * batch * plan->emb_ld);
    float* scal_chunk = plan->ws.get<float>((size_t)K * batch * 4);
    // Every sample of the batch runs at the step's sigma, and the ResnetBlock projections are linear in SiLU(cat(t, c))
    // (EmbedArgs::part): a chunk needs its K TIME rows only (16 rows instead of 16 x batch: the chunk's launch was 165 us at batch 64,
    // serial with the step graphs), the batch's CONDITION rows are computed once per call; load_step adds the two.  The regions
    // above are sized for the unsplit form (CD_NO_EMBED_SPLIT), the split form uses the front of them.
    static const bool no_split = getenv("CD_NO_EMBED_SPLIT") != nullptr;
    const bool split = !no_split && plan->emb_ld % 4 == 0 && batch >= 2;  // (batch 1: K + 1 rows do not fit the K-row region, nothing to gain)
    float* emb_cond = split ? emb_chunk + (size_t)K * plan->emb_ld : nullptr;  // [batch][emb_ld] behind the K time rows
    StepChunk chunk;
    chunk.emb_src = emb_chunk; chunk.emb_dst = emb_cur; chunk.emb_floats = split ? plan->emb_ld : batch * plan->emb_ld;
    chunk.scal_src = scal_chunk; chunk.scal_dst = scal_cur; chunk.scal_floats = split ? 4 : batch * 4; chunk.chunk_steps = K;
    chunk.emb_cond = emb_cond;
    auto embed_ahead = [&](hipStream_t st, int i0) {  // steps i0 .. i0 + K - 1 (slot = step % K; i0 is a multiple of K)
      const int nst = n_steps - i0 < K ? n_steps - i0 : K;
      if (split) {
        if (i0 == 0) {  // the condition rows, once
          EmbedArgs c = embed_args(plan, batch, cond, plan->d_table, plan->desc.time_embed_kind, emb_cond, nullptr);
          c.part = 2;
          launch_embed(c, st);
        }
        EmbedArgs e = embed_args(plan, nst, cond, plan->d_table + (size_t)i0 * 4, plan->desc.time_embed_kind, emb_chunk, scal_chunk);
        e.part = 1; e.time_stride = 4;
        launch_embed(e, st);
        return;
      }
      EmbedArgs e = embed_args(plan, nst * batch, cond, plan->d_table + (size_t)i0 * 4, plan->desc.time_embed_kind, emb_chunk, scal_chunk);
      e.cond_rows = batch; e.time_stride = 4;
      launch_embed(e, st);
    };
    if (noisy && !step_noise) upload_noise_words(noise_dev, seed, offset, noise_stride ? noise_stride : (uint64_t)n, s);
    // remaining workspace for the network: a nested arena view
    const size_t used = plan->ws.high();
    char* sub = (char*)workspace + used;
    const size_t sub_bytes = workspace_bytes > used ? workspace_bytes - used : 0;

    auto one_step = [&](hipStream_t st, int i, const float* noise_i, float* xs_i, float* x0s_i) {
      launch_load_step(plan->d_table, plan->d_counter, plan->d_stepvals, sigma_b, batch, st, &chunk);
      const float* nz = noise_i;
      if (!nz && noisy) {
        // stream position = offset + i * stride, read from device memory (the step counter is i + 1 after load_step): the same
        // launch serves every step, so stochastic samplers replay one captured graph as well
        launch_randn_step(noise_buf, n, noise_dev, plan->d_counter, st);
        nz = noise_buf;
      }
      // the update of the running sample (x_out, in place) happens in the network's head kernel
      HeadArgs upd;
      upd.upd_stepvals = plan->d_stepvals; upd.upd_noise = nz; upd.upd_x_next = x_out; upd.upd_xs = xs_i; upd.upd_x0s = x0s_i;
      FwdOpts fo;
      fo.emb_pre = emb_cur; fo.scal_pre = scal_cur; fo.upd = &upd;
      plan->ws.reset(sub, sub_bytes, false);
      forward_impl(plan, batch, x_out, cond, sigma_b, x0, false, st, &fo);
    };

    run_with_range_fallback(plan, s, [&](bool eager) {
      CD_HIP(hipMemsetAsync(plan->d_counter, 0, sizeof(int), s));
      // x = start * sigma_start (sample.py:62-66); x_out doubles as the running x
      launch_scale(start, x_out, plan->d_table, n, s);
      // A hipGraph of one step can be replayed only if nothing in it depends on the host-side step index: no trajectories and
      // no caller-supplied per-step noise (the device Philox noise of a stochastic sampler reads its stream position from the
      // step counter, see one_step).
      const bool graphable = use_graph && !eager && !step_noise && !xs && !x0s && !prof::enabled();
      if (graphable) {
        StepGraph& graph = plan->ddim_graph;
        StepGraph::Key key;
        key.batch = batch; key.ws = workspace; key.cond = cond; key.x = x_out; key.noisy = noisy ? 1 : 0;
        key.precision = conv_precision();
        // `count` consecutive steps as one graph: every step reads its index from the device counter, so the same capture serves any
        // position in the schedule
        auto capture = [&](int count) {
          return capture_steps(plan, count, [&](hipStream_t cs) { one_step(cs, 0, nullptr, nullptr, nullptr); });
        };
        if (!graph.valid_for(key)) {
          graph.destroy();
          // one eager pass first: per-geometry kernel tuning (and lazy function attributes) cannot happen during capture.
          // It only writes x0 / scratch, which the replayed steps overwrite.
          launch_load_step(plan->d_table, plan->d_counter, plan->d_stepvals, sigma_b, batch, s);
          plan->ws.reset(sub, sub_bytes, false);
          forward_impl(plan, batch, x_out, cond, sigma_b, x0, false, s);
          CD_HIP(hipMemsetAsync(plan->d_counter, 0, sizeof(int), s));
          CD_HIP(hipStreamSynchronize(s));
          graph.exec = capture(1);
          graph.key = key;
        }
        // Schedules of at least one embedding chunk replay the chunk's kEmbedChunk steps as ONE graph (8.5 us of idle time sat
        // between two graph launches: profiles/r04_graph_gaps.txt); the tail, and short schedules, replay the one-step graph.
        static const bool no_chunk = getenv("CD_NO_CHUNK_GRAPH") != nullptr;
        if (!no_chunk && n_steps >= K && !graph.chunk) graph.chunk = capture(K);
        for (int i = 0; i < n_steps;) {
          if (i % K == 0) embed_ahead(s, i);
          if (!no_chunk && graph.chunk && i % K == 0 && i + K <= n_steps) {
            CD_HIP(hipGraphLaunch(graph.chunk, s));
            i += K;
          } else {
            CD_HIP(hipGraphLaunch(graph.exec, s));
            i += 1;
          }
        }
      } else {
        for (int i = 0; i < n_steps; ++i) {
          if (i % K == 0) embed_ahead(s, i);
          one_step(s, i, step_noise ? step_noise + (size_t)i * n : nullptr, xs ? xs + (size_t)i * n : nullptr,
                   x0s ? x0s + (size_t)i * n : nullptr);
        }
      }
    });
  });
}

// workspace of cd_sampler_run: the buffers, the coefficient table, sigma / Philox words, and the network's own
static size_t sampler_front_bytes(CdPlan* plan, int batch, int n_bufs, size_t table_floats, float** bufs, float** table, float** sigma_b,
                                  uint64_t** noise_dev) {
  const int64_t n = (int64_t)batch * plan->state_per();
  for (int k = 1; k < n_bufs; ++k) {
    float* b = plan->ws.get<float>((size_t)n);
    if (bufs) bufs[k] = b;
  }
  float* t = plan->ws.get<float>(table_floats + 64);
  float* sg = plan->ws.get<float>((size_t)batch + 64);
  uint64_t* nd = (uint64_t*)plan->ws.get<double>(4);
  if (table) *table = t;
  if (sigma_b) *sigma_b = sg;
  if (noise_dev) *noise_dev = nd;
  return plan->ws.high();
}

int cd_plan_sampler_workspace_bytes(CdPlan* plan, int batch, int n_bufs, int n_steps, int n_coef, size_t* bytes) {
  return guarded([&] {
    CD_REQUIRE(plan && bytes && batch > 0 && n_bufs >= 2 && n_bufs <= 16 && n_steps >= 1 && n_coef >= 1, "bad argument");
    plan->ws.reset(nullptr, 0, true);
    const size_t front = sampler_front_bytes(plan, batch, n_bufs, (size_t)n_steps * n_coef, nullptr, nullptr, nullptr, nullptr);
    *bytes = front + dry_forward_bytes(plan, batch, [] {}) + 8192;
  });
}

int cd_sampler_run(CdPlan* plan, int batch, const float* start, float start_scale, const float* cond, int n_bufs, int n_steps,
                   const CdSamplerOp* ops, int n_ops, const int32_t* op_begin, const float* coefs, int n_coef,
                   const float* step_noise, uint64_t seed, uint64_t offset, uint64_t noise_stride, float* x_out, float* xs,
                   float* x0s, int use_graph, void* workspace, size_t workspace_bytes, void* stream) {
  return guarded([&] {
    CD_REQUIRE(plan && start && cond && ops && coefs && x_out && workspace && batch > 0, "bad argument");
    CD_REQUIRE(n_bufs >= 2 && n_bufs <= 16 && n_steps >= 1 && n_steps <= 1 << 20 && n_ops >= 1 && n_coef >= 1, "bad program size");
    check_ready(plan, true);
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)batch * plan->state_per();
    const bool uniform = op_begin == nullptr;
    const int randn_per_step = validate_sampler_program(ops, op_begin, n_steps, n_ops, n_bufs, n_coef, batch).randn_per_step;

    plan->ws.reset((char*)workspace, workspace_bytes, false);
    float* bufs[16] = {nullptr};
    bufs[0] = x_out;
    float *table = nullptr, *sigma_b = nullptr;
    uint64_t* noise_dev = nullptr;
    const size_t used = sampler_front_bytes(plan, batch, n_bufs, (size_t)n_steps * n_coef, bufs, &table, &sigma_b, &noise_dev);
    CD_REQUIRE(used <= workspace_bytes, "workspace too small: call cd_plan_sampler_workspace_bytes");
    char* sub = (char*)workspace + used;
    const size_t sub_bytes = workspace_bytes - used;
    const uint64_t stride = noise_stride ? noise_stride : (uint64_t)n;
    CD_HIP(hipMemcpyAsync(table, coefs, sizeof(float) * (size_t)n_steps * n_coef, hipMemcpyHostToDevice, s));
    upload_noise_words(noise_dev, seed, offset, stride, s);  // (its synchronisation also covers the coefs: they may be a temporary)
    int* counter = plan->d_counter;

    // one op; `draw` = running number of the RANDN op (eager), or -1 when the position comes from the device counter (graph)
    int64_t draws = 0;
    auto run_op = [&](hipStream_t st, const CdSamplerOp& o, int index_in_step, bool from_counter) {
      switch (o.kind) {
        case CD_SOP_LINCOMB:
        case CD_SOP_LINDIV: {
          const float* src[6];
          for (int j = 0; j < o.nsrc; ++j) src[j] = bufs[o.src[j]];
          launch_lincomb(bufs[o.dst], src, o.nsrc, table, n_coef, o.col, counter, n, o.kind == CD_SOP_LINDIV, st);
          break;
        }
        case CD_SOP_DENOISE:
          launch_fill_from_table(sigma_b, batch, table, n_coef, o.col, counter, st);
          plan->ws.reset(sub, sub_bytes, false);
          forward_impl(plan, batch, bufs[o.src[0]], cond, sigma_b, bufs[o.dst], false, st);
          break;
        case CD_SOP_DENOISE_PS:  // the step's `batch` sigma columns, read through the device counter (eager and captured alike)
          launch_fill_row_from_table(sigma_b, batch, table, n_coef, o.col, counter, st);
          plan->ws.reset(sub, sub_bytes, false);
          forward_impl(plan, batch, bufs[o.src[0]], cond, sigma_b, bufs[o.dst], false, st);
          break;
        case CD_SOP_RANDN:
          if (step_noise) CD_HIP(hipMemcpyAsync(bufs[o.dst], step_noise + (size_t)draws * n, sizeof(float) * n, hipMemcpyDeviceToDevice, st));
          else if (from_counter) launch_randn_step(bufs[o.dst], n, noise_dev, counter, st, randn_per_step, index_in_step);
          else launch_randn(bufs[o.dst], n, seed, offset + (uint64_t)draws * stride, st);
          ++draws;
          break;
        case CD_SOP_RECORD: {
          float* traj = o.dst == 0 ? xs : x0s;
          if (traj) launch_record_step(traj, bufs[o.src[0]], counter, n, st);
          break;
        }
      }
    };
    auto run_step = [&](hipStream_t st, int i, bool from_counter) {
      launch_step_advance(counter, st);
      const int b = uniform ? 0 : op_begin[i], e = uniform ? n_ops : op_begin[i + 1];
      int ri = 0;
      for (int k = b; k < e; ++k) {
        run_op(st, ops[k], ri, from_counter);
        if (ops[k].kind == CD_SOP_RANDN) ++ri;
      }
    };

    run_with_range_fallback(plan, s, [&](bool eager) {
      draws = 0;
      CD_HIP(hipMemsetAsync(counter, 0, sizeof(int), s));
      for (int k = 1; k < n_bufs; ++k) CD_HIP(hipMemsetAsync(bufs[k], 0, sizeof(float) * n, s));
      launch_scale_imm(start, x_out, start_scale, n, s);
      const bool graphable = use_graph && !eager && uniform && !step_noise && !prof::enabled();
      if (graphable) {
        StepGraph& graph = plan->prog_graph;
        StepGraph::Key key;
        key.batch = batch; key.n_coef = n_coef; key.n_bufs = n_bufs; key.ws = workspace; key.cond = cond; key.x = x_out;
        key.xs = xs; key.x0s = x0s; key.precision = conv_precision();
        uint64_t h = 1469598103934665603ull;  // FNV-1a over the op list
        for (size_t b = 0; b < sizeof(CdSamplerOp) * (size_t)n_ops; ++b) h = (h ^ ((const unsigned char*)ops)[b]) * 1099511628211ull;
        key.ops_hash = h ^ ((uint64_t)n_steps << 40) ^ (uint64_t)n_ops;
        if (!graph.valid_for(key)) {
          graph.destroy();
          // one eager denoise first (kernel tuning / lazy function attributes cannot happen during capture): x -> buffer 1
          for (int k = 0; k < n_ops; ++k)
            if (ops[k].kind == CD_SOP_DENOISE || ops[k].kind == CD_SOP_DENOISE_PS) {
              launch_step_advance(counter, s);
              if (ops[k].kind == CD_SOP_DENOISE) launch_fill_from_table(sigma_b, batch, table, n_coef, ops[k].col, counter, s);
              else launch_fill_row_from_table(sigma_b, batch, table, n_coef, ops[k].col, counter, s);
              plan->ws.reset(sub, sub_bytes, false);
              forward_impl(plan, batch, x_out, cond, sigma_b, bufs[1], false, s);
              CD_HIP(hipMemsetAsync(counter, 0, sizeof(int), s));
              CD_HIP(hipMemsetAsync(bufs[1], 0, sizeof(float) * n, s));
              break;
            }
          CD_HIP(hipStreamSynchronize(s));
          graph.exec = capture_steps(plan, 1, [&](hipStream_t cs) { run_step(cs, 0, true); });
          graph.key = key;
        }
        for (int i = 0; i < n_steps; ++i) CD_HIP(hipGraphLaunch(graph.exec, s));
      } else {
        for (int i = 0; i < n_steps; ++i) run_step(s, i, false);
      }
    });
  });
}

}  // extern "C"
