// The elementwise ops of the sampler loops and step programs and the Philox noise (kernels_sampler.hip), and the host check of a
// step program (sampler.hip).
#pragma once
#include "cd_common.h"

struct CdSamplerOp;  // include/calodiff.h

namespace cd {

// stepvals <- table[*counter]; sigma_b[0..B) <- stepvals.sigma; (*counter)++.  chunk (optional): the step's slice of the
// embeddings / scalings computed a chunk of steps ahead -- slot (*counter) % chunk_steps of emb_src / scal_src -> emb_dst / scal_dst
struct StepChunk {
  const float* emb_src = nullptr;  // [chunk_steps][emb_floats]
  float* emb_dst = nullptr;
  int emb_floats = 0;
  const float* scal_src = nullptr;  // [chunk_steps][scal_floats]
  float* scal_dst = nullptr;
  int scal_floats = 0;
  int chunk_steps = 0;
  // separable form: emb_src / scal_src hold ONE row per step (EmbedArgs::part = 1), emb_cond one row per sample (part = 2):
  // emb_dst[b] = emb_src[slot] + emb_cond[b], scal_dst[b] = scal_src[slot]; emb_floats / scal_floats are then the ROW lengths
  const float* emb_cond = nullptr;
};
void launch_load_step(const float* table, int* counter, float* stepvals, float* sigma_b, int batch, hipStream_t s,
                      const StepChunk* chunk = nullptr);
void launch_scale(const float* x, float* y, const float* stepvals_sigma, int64_t n, hipStream_t s);
void launch_scale_imm(const float* x, float* y, float scale, int64_t n, hipStream_t s);
void launch_randn(float* out, int64_t n, uint64_t seed, uint64_t offset, hipStream_t s);
// noise tensor number (*step_counter - 1) * per_step + index of a sampler run, from {seed, base offset, stride} in device
// memory: stream position = base + tensor number * stride (graph-replayable; stride = the GLOBAL tensor size, so that batch
// shards on different GPUs draw their slices of the one stream a single-GPU run of the whole batch would use)
void launch_randn_step(float* out, int64_t n, const uint64_t* seed_offset_stride_dev, const int* step_counter, hipStream_t s,
                       int per_step = 1, int index = 0);
// generic sampler programs (cd_sampler_run): per-step scalars are columns of row (*step_counter - 1) of a device table
void launch_step_advance(int* counter, hipStream_t s);  // (*counter)++
void launch_or_word(int* word, int bits, hipStream_t s);  // *word |= bits
void launch_fill_from_table(float* dst, int count, const float* table, int ncol, int col, const int* step_counter, hipStream_t s);
// dst[b] = table[row][col + b], b < count (CD_SOP_DENOISE_PS: a sigma per sample)
void launch_fill_row_from_table(float* dst, int count, const float* table, int ncol, int col, const int* step_counter,
                                hipStream_t s);
// out[i] = sum_k table[row][col + k] * src[k][i]   (nsrc <= 6; out may alias a source); div (CD_SOP_LINDIV): every product and sum
// rounded on its own, then divided by table[row][col + nsrc]
void launch_lincomb(float* out, const float* const* src, int nsrc, const float* table, int ncol, int col, const int* step_counter,
                    int64_t n, bool div, hipStream_t s);
// traj[(*step_counter - 1) * n + i] = src[i]
void launch_record_step(float* traj, const float* src, const int* step_counter, int64_t n, hipStream_t s);

// sampler.hip: the one check of a step program (host arrays; op_begin null = uniform), for cd_sampler_run and cd_layer_sampler_run
struct SamplerProgramCounts {
  int randn_per_step = 0;  // RANDN ops in the op list
  int64_t n_denoise = 0;   // DENOISE ops the program executes
};
SamplerProgramCounts validate_sampler_program(const ::CdSamplerOp* ops, const int32_t* op_begin, int n_steps, int n_ops, int n_bufs,
                                              int n_coef, int batch);

}  // namespace cd
