/*
 * calodiff.h -- C ABI of the MI355X (gfx950) CaloDiffusion denoising hot path.
 *
 * The reference (OzAmram/CaloDiffusion) has no FFI of its own: its seam for this path is a Python
 * class protocol.  Each entry point below states the reference interface it
 * stands behind (file:line into the reference tree).  INTEGRATION.md shows the ctypes binding a
 * maintainer adds on the reference side.
 *
 * Conventions
 *   - every function returns 0 on success or a negative CD_E* code; cd_last_error() gives the message
 *     (thread-local, valid until the next failing call on that thread).  Nothing throws across the ABI.
 *   - all tensor pointers are DEVICE pointers to contiguous fp32 unless marked "host".
 *     User-facing activations are NCDHW (D = layer/z, H = phi, periodic, W = r), as in the reference
 *     (calodiffusion/models/models.py:26,66).  Channels-last (NDHWC) is the library's internal layout
 *     and appears only in the cd_op_* primitive entry points, which say so.
 *   - memory is owned by the caller (PyTorch's caching allocator in the shipped host code).  The
 *     library allocates only plan-private metadata and the packed-weight arena at plan creation /
 *     cd_plan_set_weight time, never inside a compute call (compute calls are hipGraph-capturable).
 *   - `stream` is a hipStream_t passed as void*; all work of a call is enqueued on it and the call
 *     returns without synchronising.
 *   - a plan is not thread-safe; use one plan per device per process.
 */
#ifndef CALODIFF_H
#define CALODIFF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CD_OK 0
#define CD_EINVAL -1       /* bad argument / unsupported configuration */
#define CD_EHIP -2         /* HIP runtime error */
#define CD_ENOGPU -3       /* no gfx950 device visible */
#define CD_EWEIGHTS -4     /* a weight tensor is missing or has the wrong size */
#define CD_EWORKSPACE -5   /* workspace too small */

#define CD_MAX_SIZES 8

/* Bumped whenever a struct layout or an argument list of this header changes.  cd_abi_version() returns the value the
 * library was built with: a binder compares it with the CD_ABI_VERSION it was written against before any other call, and
 * every descriptor struct starts with its own sizeof (struct_size), which the library checks -- a binder written against an
 * older header gets CD_EINVAL from cd_plan_create instead of the library reading past its struct. */
#define CD_ABI_VERSION 3

#define CD_TIME_LOG 0      /* t_emb = 0.5*ln(sigma)         (calodiffusion.py:150) */
#define CD_TIME_SIGMA 1    /* t_emb = sigma/sqrt(1+sigma^2) (calodiffusion.py:149) */
#define CD_TIME_RAW 2      /* t_emb = the value passed (CondUnet.forward's `time` argument) */

#define CD_OBJ_HYBRID 0     /* c_skip*x + c_out*F  (calodiffusion.py:166-167) */
#define CD_OBJ_NOISE_PRED 1 /* x - sigma*F         (calodiffusion.py:161-162) */
#define CD_OBJ_MEAN_PRED 2  /* F                   (calodiffusion.py:164-165) */

typedef struct CdPlan CdPlan;

/* Mirrors the arguments of CondUnet.__init__ (models/models.py:525-543) as CaloDiffusion.init_model
 * derives them from the config (models/calodiffusion.py:39-81). */
typedef struct CdUnetDesc {
  uint32_t struct_size;            /* = sizeof(CdUnetDesc) of the header the caller was built against */
  int32_t grid[3];                 /* D, H, W of SHAPE_FINAL */
  int32_t in_channels;             /* `channels`: 1 (+2 if R_Z_INPUT) (+1 if PHI_INPUT) */
  int32_t n_sizes;                 /* len(LAYER_SIZE_UNET) */
  /* LAYER_SIZE_UNET as the config states it.  A width C runs as C k for the smallest k of {1, 2, 4} with C % groups == 0,
   * C k % 32 == 0, (C k / groups) % 4 == 0 and C k <= 256 (channels duplicated inside each GroupNorm group); a width without
   * such a k is refused with CD_EINVAL.  Tensor sizes (cd_plan_weight_name) and the gradient layout (cd_plan_grad_layout)
   * are always the config's own; a plan with k > 1 somewhere takes one launch more per weight sync and per training step
   * and a larger training / VJP workspace. */
  int32_t layer_sizes[CD_MAX_SIZES];
  int32_t groups;                  /* BLOCK_GROUPS (8) */
  int32_t block_attn, mid_attn, compress_z;
  int32_t cond_size;               /* width of cat(E, layers) */
  int32_t cond_dim;                /* COND_SIZE_UNET */
  int32_t rz_input, phi_input;     /* which coordinate channels cd_denoise synthesises */
  int32_t time_embed_kind;         /* CD_TIME_* used by cd_denoise */
  int32_t objective;               /* CD_OBJ_*  used by cd_denoise */
  float sigma_data;                /* Loss.sigma_data (models/loss.py:18-25) */
  /* CondUnet(time_embed=True / cond_embed=True): SinusoidalPositionEmbeddings (models.py:132-144, 578-601) instead of the
   * first Linear of the time / cond MLP.  Reachable through cd_unet_forward only: the reference's own denoise path raises
   * KeyError for TIME_EMBED 'sin' (calodiffusion.py:148-152), and so do cd_denoise / the samplers / cd_train_step. */
  int32_t time_sin, cond_sin;
} CdUnetDesc;

/* One row per sampler loop iteration; computed on the host exactly as DDim.__call__ does in fp32
 * (models/sample.py:45-101): sigma = sqrt(1-abar_t)/sqrt(abar_t); sigma_prev = sqrt(1-abar_prev-ddim_sigma^2)/denom
 * (already multiplied by the t>0 mask); ddim_sigma = eta*sqrt(...); denom = sqrt(abar_{max(t-1,0)}). */
typedef struct CdStep {
  float sigma;
  float sigma_prev_masked;
  float ddim_sigma;
  float denom;
} CdStep;

const char* cd_last_error(void);
int cd_abi_version(void);  /* CD_ABI_VERSION of the build */
/* 0 if a gfx950 device is usable by this process, CD_ENOGPU otherwise. Fills name (may be NULL). */
int cd_device_check(char* name, int cap);

/* ---- plan ------------------------------------------------------------------------------------------- */
/* Replaces CondUnet.__init__ + CaloDiffusion.init_model (models.py:525-699, calodiffusion.py:39-81). */
int cd_plan_create(const CdUnetDesc* desc, CdPlan** plan);
int cd_plan_destroy(CdPlan* plan);
/* Names follow CondUnet.state_dict() (e.g. "downs.0.0.block1.proj.conv.weight"); iteration helpers so the host
 * can check it feeds every tensor.  *numel is the element count the plan expects. */
int cd_plan_num_weights(const CdPlan* plan, int* n);
int cd_plan_weight_name(const CdPlan* plan, int idx, char* name, int cap, int64_t* numel);
/* Copies/re-packs one state_dict tensor (device pointer, torch layout) into the plan's arena on `stream`.
 * Replaces nn.Module.load_state_dict for this path (calodiffusion.py:31-37). Call again after an optimizer step. */
int cd_plan_set_weight(CdPlan* plan, const char* name, const float* dev_ptr, int64_t numel, void* stream);
/* The same for every tensor at once: dev_ptrs[i] is the tensor cd_plan_weight_name(plan, i, ...) names (n = cd_plan_num_weights),
 * all copied and re-packed by two launches.  This is the call for the training loop -- after optimizer.step() every parameter
 * has changed (train/train.py:144-170); one tensor at a time that was ~400 launches and 3 ms of host time per step. */
int cd_plan_set_weights(CdPlan* plan, int n, const float* const* dev_ptrs, void* stream);
/* Host arrays: the 1-D profiles of the constant R (len W), Z (len D) and phi (len H) input images
 * (utils/utils.py:33-150, calodiffusion.py:17-20). */
int cd_plan_set_coords(CdPlan* plan, const float* r_w, const float* z_d, const float* phi_h, void* stream);
int cd_plan_workspace_bytes(CdPlan* plan, int batch, size_t* bytes);

/* ---- hot path ------------------------------------------------------------------------------------------ */
/* CondUnet.forward(x, cond, time) (models.py:701-748).  x: (B, in_channels, D, H, W); cond: (B, cond_size);
 * time: (B,); out: (B, 1, D, H, W). */
int cd_unet_forward(CdPlan* plan, int batch, const float* x, const float* cond, const float* time, float* out,
                    void* workspace, size_t workspace_bytes, void* stream);
/* CaloDiffusion.denoise / __call__ (calodiffusion.py:154-173) incl. Loss.get_scaling (loss.py:29-41),
 * do_time_embed (calodiffusion.py:144-152), forward + add_RZPhi (calodiffusion.py:86-98,121-142).
 * x: (B,1,D,H,W); sigma: (B,); cond: (B, cond_size) = cat(E, layers); out: (B,1,D,H,W). */
int cd_denoise(CdPlan* plan, int batch, const float* x, const float* sigma, const float* cond, float* out,
               void* workspace, size_t workspace_bytes, void* stream);
/* cd_denoise with the range fallback of the sampler entry points (below): if an operand of the fp16-pipe kernels left the fp16
 * range during the call, the call is run again with the full-range kernels (bf16x3 convolutions, f32-MFMA attention) before it
 * returns and *fell_back is set to 1 (fell_back == NULL: cd_plan_status reports bit 1 instead).  Unlike cd_denoise it SYNCHRONISES `stream`
 * (to read the flag) and is therefore not graph-capturable: it is the entry point for samplers that call the model back from
 * host code (models/sample.py: `model(x, sigma=, E=, layers=)`, e.g. DPMAdaptive :188-309), which must not die mid-trajectory. */
int cd_denoise_safe(CdPlan* plan, int batch, const float* x, const float* sigma, const float* cond, float* out,
                    void* workspace, size_t workspace_bytes, int* fell_back, void* stream);
/* DDim.__call__ / DDPM (models/sample.py:41-121) with Diffusion.sample's start tensor (diffusion.py:77-104).
 * start: (B,1,D,H,W) unit normal; steps: host array of n_steps rows; x_out: (B,1,D,H,W).
 * step_noise: NULL (DDIM, eta = 0: the reference draws and discards it) or device (n_steps, B,1,D,H,W);
 * if NULL and any ddim_sigma != 0 the noise comes from the device Philox stream (seed, offset).
 * xs / x0s: NULL or device (n_steps, B,1,D,H,W) trajectories (`debug`). use_graph: capture one step as a
 * hipGraph and replay it. */
int cd_ddim_sample(CdPlan* plan, int batch, const float* start, const float* cond, const CdStep* steps, int n_steps,
                   const float* step_noise, uint64_t seed, uint64_t offset, uint64_t noise_stride, float* x_out, float* xs,
                   float* x0s, int use_graph, void* workspace, size_t workspace_bytes, void* stream);
/* noise_stride (both sampler entry points): distance in the Philox stream between the noise tensors of consecutive draws;
 * 0 = this call's own tensor size.  A rank holding rows [lo, hi) of a global batch passes offset + lo * voxels and
 * noise_stride = global_batch * voxels: the union of the shards then IS the single-GPU result of the same seed.
 *
 * Range fallback (both sampler entry points, cd_denoise_safe): the default arithmetic (f16x2 convolutions, the fused
 * attention's fp16-pipe products) covers the fp16 range only.  If an operand leaves it during the call (a flag private to the
 * call: a bit 0 left in the sticky word by an earlier cd_denoise is neither consumed nor lost) the call re-runs the whole
 * trajectory with the full-range kernels -- exact bf16x3 convolutions, attention on the f32-input MFMA -- before it returns,
 * synchronising `stream` for the check; cd_plan_status then reports bit 1 (fallback taken).  The switch of arithmetic is local
 * to the calling thread: other plans / threads of the process keep their kernels. */

/* ---- every other sampler of models/sample.py on the same device loop ------------------------------------------------
 * A sampler is a "step program": per step a short list of ops over a few (B,1,D,H,W) buffers, whose scalars are columns of
 * that step's row of a host coefficient table.  Buffer 0 is the running sample x (= x_out); buffers 1 .. n_bufs-1 live in
 * the workspace and start as zeros.  Steps that share one op list (op_begin == NULL) are captured once as a hipGraph and
 * replayed (the device step counter selects the table row, the Philox position and the trajectory slot); otherwise
 * step i runs ops[op_begin[i] .. op_begin[i+1]) eagerly (Restart, DPM-Solver-fast).
 * The host side (calodiffusion_amd/sample.py) builds the programs of EDM Euler(+churn) / Heun / DPM2 (sample.py:577-727,
 * 771-851), LMS (:729-769), Restart (:853-954), DPM / DPM++2S / DPM++2M (:124-186, 311-344, 415-449) and Consistency
 * (:957-1011). */
#define CD_SOP_LINCOMB 0 /* buf[dst] = sum_k coef[col + k] * buf[src[k]], k < nsrc <= 6 (dst may be a source) */
#define CD_SOP_DENOISE 1 /* buf[dst] = denoise(buf[src[0]], sigma = coef[col])  (CaloDiffusion.denoise, as cd_denoise) */
#define CD_SOP_RANDN 2   /* buf[dst] = unit normals: the next tensor of step_noise, or of the Philox stream */
#define CD_SOP_RECORD 3  /* trajectory slot of this step <- buf[src[0]]; dst: 0 = xs, 1 = x0s (skipped if that pointer is NULL) */
#define CD_SOP_LINDIV 4  /* buf[dst] = (((coef[col] * buf[src[0]]) + coef[col+1] * buf[src[1]]) + ...) / coef[col + nsrc]: like \
                            LINCOMB, but in the operation order of a chain of torch elementwise ops -- every product, sum and the \
                            final division rounded to fp32 on its own, no fused multiply-add (DPM-Solver's eps = (x - D) / sigma \
                            and its cancelling updates, utils/sampling.py:402-456) */
#define CD_SOP_DENOISE_PS 5 /* buf[dst] = denoise(buf[src[0]]) with row b at sigma_b = coef[col + b], b < batch: a sigma per \
                               sample (BespokeNonStationary's model_fn, models/sample.py:1107-1109); needs col + batch <= n_coef */
typedef struct CdSamplerOp {
  int32_t kind, dst, nsrc;
  int32_t src[6];
  int32_t col;
} CdSamplerOp;
int cd_plan_sampler_workspace_bytes(CdPlan* plan, int batch, int n_bufs, int n_steps, int n_coef, size_t* bytes);
/* start: (B,1,D,H,W) unit normal, x = start * start_scale first.  coefs: HOST (n_steps, n_coef) fp32.  ops: n_ops entries
 * (op_begin == NULL: the one list of every step; else op_begin has n_steps + 1 entries).  step_noise: NULL or DEVICE
 * (number of RANDN ops executed, B,1,D,H,W), consumed in execution order.  xs / x0s: NULL or (n_steps, B,1,D,H,W).
 * The same programs run on LayerDiffusion's layer model through cd_layer_sampler_run (below, after CdLayerMlpDesc). */
int cd_sampler_run(CdPlan* plan, int batch, const float* start, float start_scale, const float* cond, int n_bufs, int n_steps,
                   const CdSamplerOp* ops, int n_ops, const int32_t* op_begin, const float* coefs, int n_coef,
                   const float* step_noise, uint64_t seed, uint64_t offset, uint64_t noise_stride, float* x_out, float* xs,
                   float* x0s, int use_graph, void* workspace, size_t workspace_bytes, void* stream);
/* Diffusion.noise_generation (diffusion.py:58-61): n unit normals from Philox4x32-10 + Box-Muller;
 * element i depends only on (seed, offset + i), so shards of one global stream can be drawn per rank. */
int cd_randn(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream);
/* Loss.__call__ + hybrid_weight.loss_function + l2_loss forward value (models/loss.py:103-104,118-142,163-179):
 * x_noisy = data + sigma*noise; x0 = denoise(x_noisy); loss = sum(w (x0-data)^2) / (mean(w) numel), w = 1 + sigma^-2.
 * sigma: (B,) device. loss_out: 1 double on device. */
int cd_loss_hybrid_l2(CdPlan* plan, int batch, const float* data, const float* noise, const float* sigma,
                      const float* cond, double* loss_out, void* workspace, size_t workspace_bytes, void* stream);
/* The same for every LOSS_TYPE of Loss._loss (models/loss.py:97-116) under hybrid_weight.loss_function (:163-179), which passes
 * (pred = x0, target = data, weight = 1 + sigma^-2):
 *   CD_LOSS_L2    sum(w (x0-data)^2) / (mean(w) numel)          (the only one that uses the weight; the shipped configs)
 *   CD_LOSS_L1    torch.nn.functional.l1_loss:        mean |x0 - data|
 *   CD_LOSS_MSE   torch.nn.functional.mse_loss:       mean (x0 - data)^2
 *   CD_LOSS_HUBER torch.nn.functional.smooth_l1_loss: mean of d^2/2 where |d| < 1, |d| - 1/2 elsewhere (the reference's CI
 *                 fixture trains with it, tests/test_execution.py:94) */
#define CD_LOSS_L2 0
#define CD_LOSS_L1 1
#define CD_LOSS_MSE 2
#define CD_LOSS_HUBER 3
/* The plan's objective (CdUnetDesc.objective) selects which loss class of models/loss.py this is -- the entry point keeps its
 * name from the shipped configs' hybrid_weight:
 *   CD_OBJ_HYBRID     hybrid_weight (:163-179)  pred = denoise(x_noisy), target = data, weight 1 + sigma^-2
 *   CD_OBJ_NOISE_PRED noise_pred    (:181-196)  pred = (data - (data - sigma denoise(x_noisy))) / sigma, target = noise, weight 1
 *   CD_OBJ_MEAN_PRED  mean_pred     (:198-210)  pred = denoise(x_noisy) = F, target = data, weight sigma^-2
 * (the weight enters CD_LOSS_L2 only).  minsnr (:144-161) cannot be constructed in the reference (its __init__ takes no
 * loss_type, models/diffusion.py:30 passes one) and has no counterpart here. */
int cd_loss_hybrid(CdPlan* plan, int batch, const float* data, const float* noise, const float* sigma, const float* cond,
                   int loss_type, double* loss_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- training step ----------------------------------------------------------------------------------------------- */
/* Body of TrainDiffusion.training_loop (train/train_diffusion.py:52-63) up to loss.backward(): the loss of the plan's objective
 * (as cd_loss_hybrid: hybrid_weight / noise_pred / mean_pred, any CD_LOSS_* type) AND the gradient of that loss with respect to every parameter, written to `grads`, a flat fp32
 * buffer laid out as cd_plan_grad_layout reports (tensor idx of cd_plan_weight_name starts at *offset, torch layout;
 * *total_floats = size of the buffer).  Workspace: cd_plan_train_workspace_bytes (the forward's activations are kept
 * until the backward has consumed them; the input-gradient weight images and the weight gradients' per-workgroup partials, held
 * until their one reduction launch, live there too: the step allocates no device memory of its own). */
int cd_plan_grad_layout(const CdPlan* plan, int idx, int64_t* offset, int64_t* total_floats);
int cd_plan_train_workspace_bytes(CdPlan* plan, int batch, size_t* bytes);

/* Sticky range flags of the compute calls issued on this plan since the last query (synchronises `stream`, then clears):
 *   bit 0: an operand of an fp16-pipe kernel (an activation staged for an f16x2 convolution; the normalised input, v or the
 *          folded output weights of the fused attention) exceeded the fp16 range (|x| > 65504): the outputs of that call
 *          contain inf/NaN.  The reference computes in fp32 throughout; rerun with CD_CONV_PRECISION=bf16x3 (full fp32 range).
 *          (cd_denoise / cd_unet_forward / cd_train_step; cd_denoise_safe and the sampler entry points recover by themselves)
 *   bit 1: a sampler / cd_denoise_safe call took the full-range fallback (its result is valid). */
int cd_plan_status(CdPlan* plan, int* flags, void* stream);
int cd_train_step(CdPlan* plan, int batch, const float* data, const float* noise, const float* sigma, const float* cond,
                  int loss_type /* CD_LOSS_* */, double* loss_out, float* grads, void* workspace, size_t workspace_bytes,
                  void* stream);

/* ---- consistency distillation (Song et al. 2023, Algorithm 2; calodiffusion_amd/distill.py) -------------------------- */
/* cd_train_step against a given target: the network's input is data + sigma * noise as in cd_train_step, the loss compares
 * out = denoise(data + sigma noise, sigma, cond) with `target` (B,1,D,H,W; a constant, never differentiated):
 *   r = out - target;  loss = mean r^2 (CD_LOSS_MSE), mean |r| (CD_LOSS_L1), mean smooth_l1(r) (CD_LOSS_HUBER);  weight 1
 * whatever the plan's objective; d out / d F is the objective's own (c_out, -sigma, 1), as in cd_denoise_vjp.  CD_LOSS_L2 is
 * refused (its weight has no meaning here: use CD_LOSS_MSE), and so is a plan with a geometry embedding.  The taped forward, the
 * backward, `grads` and the workspace (cd_plan_train_workspace_bytes) are cd_train_step's; with target == data on a
 * CD_OBJ_HYBRID plan the launches are cd_train_step's and loss and grads are the same bits. */
int cd_train_step_target(CdPlan* plan, int batch, const float* data, const float* noise, const float* sigma, const float* cond,
                         const float* target, int loss_type /* CD_LOSS_L1 / MSE / HUBER */, double* loss_out, float* grads,
                         void* workspace, size_t workspace_bytes, void* stream);
/* One step of the probability-flow ODE from sigma_hi[b] down to sigma_lo[b], a noise level per sample, over `batch` rows of `per`
 * floats (any `per`: rows need not start on a 16-byte boundary); one pass, no plan and no workspace.  D_hi = denoise(x_hi, sigma_hi):
 *   Euler (x_e == d_e == NULL):  d = (x_hi - D_hi) / sigma_hi;  x_lo = x_hi + (sigma_lo - sigma_hi) d
 *   Heun  (x_e the Euler x_lo, D_e = denoise(x_e, sigma_lo)):  d2 = (x_e - D_e) / sigma_lo;
 *                                                              x_lo = x_hi + (sigma_lo - sigma_hi) (0.5 (d + d2))
 * Every product, difference and quotient is rounded to fp32 on its own.  x_lo may be x_e (in place). */
int cd_ode_step(const float* x_hi, const float* d_hi, const float* x_e /* nullable */, const float* d_e /* nullable */,
                const float* sigma_hi, const float* sigma_lo, float* x_lo, int batch, int64_t per, void* stream);
/* EMA of the target network over n tensors in ceil(n / 48) launches: dst[i] <- mu dst[i] + (1 - mu) src[i], mu in [0, 1)
 * (1 - mu formed in double, as cd_adam_step forms 1 - beta).  dst / src are HOST arrays of n DEVICE pointers, numel their lengths;
 * src is only read.  mu = 0 copies. */
int cd_ema_step(int n, float* const* dst, const float* const* src, const int64_t* numel, double mu, void* stream);

/* ---- differentiable denoise ------------------------------------------------------------------------------------------ */
/* Workspace of cd_denoise_vjp at this batch: with_param_grads 0 sizes the input-gradient-only call (grads == NULL), which needs
 * less; 1 sizes the call that also writes grads.  Same restrictions as cd_plan_train_workspace_bytes. */
int cd_plan_vjp_workspace_bytes(CdPlan* plan, int batch, int with_param_grads, size_t* bytes);
/* Vector-Jacobian product of cd_denoise (the reference's CaloDiffusion.denoise, models/calodiffusion.py:154-169, under
 * torch autograd): given D = denoise(x, sigma, cond) and an upstream gradient gy = dL/dD (B,1,D,H,W), writes dx = dL/dx
 * (B,1,D,H,W) and, when grads is not NULL, dL/dW of every parameter into the flat buffer laid out as cd_plan_grad_layout says
 * (overwritten, not accumulated).  sigma and cond are constants: no gradient is formed for them.  The forward is recomputed
 * (taped) inside the call; arithmetic, range flag and restrictions are those of cd_train_step (Linear time/cond embeddings).
 * With grads == NULL no parameter-gradient work is launched and dx is bitwise the dx of the call with grads.  All scratch is
 * in `workspace` (cd_plan_vjp_workspace_bytes); nothing is allocated and the stream is not synchronised. */
int cd_denoise_vjp(CdPlan* plan, int batch, const float* x, const float* sigma, const float* cond, const float* gy,
                   float* dx, float* grads /* nullable */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- BespokeNonStationary theta training --------------------------------------------------------------------------- */
/* One batch of BespokeNonStationary.optimize_sampler (models/sample.py:1060-1085) up to loss.backward(), for theta only:
 *   x_0 = data;  U_i = denoise(x_i, sigma_i, cond);  x_{i+1} = x_i * a_i + U_i * b_i  (i < n_steps, theta = (a; b), (2, N));
 *   mse = mean((data - x_N)^2);  loss = mean(20 log10(max(data, axis=-1) / sqrt(mse)))   (every row of the last axis)
 * loss_out: one double (the reference's value: NaN if a row maximum is negative, -inf if one is 0; 100 if mse == 0, where the
 * reference's torch.mean raises).  dtheta (2, N): d loss / d theta, as torch autograd forms it: the seed at x_N is
 * -20 / (ln 10 * mse * numel) * (x_N - data), independent of the maxima -- except that a row maximum of exactly 0 makes torch's
 * whole gradient NaN (log10's backward divides by 0), and so it is here; mse == 0 gives a zero gradient.  Then for i = N-1 .. 0:
 * dtheta[0][i] = <g_{i+1}, x_i>, dtheta[1][i] = <g_{i+1}, U_i> (fp64, fixed order: repeated calls are bitwise equal) and
 * g_i = a_i g_{i+1} + VJP of denoise at (x_i, sigma_i) applied to b_i g_{i+1} (cd_denoise_vjp without grads; skipped at i = 0).
 * data / cond / theta / sigma are DEVICE arrays; sigma (n_steps, batch): row i holds the sigma of every sample at step i.
 * Parameter gradients are not formed.  Every x_i and U_i is kept in `workspace` (cd_plan_bns_workspace_bytes: 2 N B voxels
 * floats plus the input-only VJP's scratch); nothing is allocated and the stream is not synchronised.  Restrictions and the
 * range flag are those of cd_train_step. */
int cd_plan_bns_workspace_bytes(CdPlan* plan, int batch, int n_steps, size_t* bytes);
int cd_bns_theta_grad(CdPlan* plan, int batch, int n_steps, const float* data, const float* cond, const float* theta,
                      const float* sigma, double* loss_out, float* dtheta, void* workspace, size_t workspace_bytes, void* stream);

/* torch.optim.Adam step (train/train.py:144: Adam(model.parameters(), lr); no amsgrad) over n tensors in ceil(n / 48)
 * launches: params / grads / exp_avg / exp_avg_sq are HOST arrays of n DEVICE pointers, numel their lengths.  step is the
 * 1-based step count after this update (torch's state['step']).  Same element-wise formulas as torch:
 *   m += (1-beta1)(g - m);  v = beta2 v + (1-beta2) g^2;  p -= lr/(1-beta1^step) * m / (sqrt(v)/sqrt(1-beta2^step) + eps);
 * lr and the betas are doubles (python floats): 1-beta and the bias corrections are formed in double, as torch does. */
int cd_adam_step(int n, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                 const int64_t* numel, double lr, double beta1, double beta2, float eps, float weight_decay, int step, void* stream);

/* Inverse pre-processing of generated showers on the device: utils.ReverseNormCaloChall (calodiffusion/utils/utils.py:446-573)
 * for the regular grids (dataset_num 2 / 3; showerMap 'layer-logit-norm' when layerE != NULL, 'logit-norm' otherwise).
 * voxels (B,1,D,H,W) normalised; energy (B) incident energies already in physical units (emin*(emax/emin)^e on the host);
 * layerE (B, 1+D) normalised {total, layer} energies or NULL; out (B, D*H*W).  consts = {logit_mean, logit_std, totalE_mean,
 * totalE_std, layers_mean, layers_std} (utils/consts.py:82-116). */
int cd_reverse_norm(const float* voxels, const float* energy, const float* layerE, float* out, int batch, const int32_t dims[3],
                    const float consts[6], float max_deposit, float ecut, void* stream);

/* The HGCal variant, utils.ReverseNormHGCal (calodiffusion/utils/HGCal_utils.py:167-292), has a geometry decode in the middle
 * (NN_embed.dec_batches: needs a geometry file that does not ship with the reference).  Its arithmetic either side of the decode:
 *   stage 1  out = reverse_logit(voxels * logit_std + logit_mean, alpha)                     (any shape: dims only give the count)
 *   stage 2  voxels = DECODED showers (B, L, cells) given as dims = {L, 1, cells}: negatives clamped, every layer rescaled to
 *            the layer energy of layerE unless layer or sum < layer_eps, then x max_deposit x energy
 *   stage 0  = cd_reverse_norm with explicit alpha / layer_eps.
 * HGCal: alpha 1e-8, layer_eps 1e-8, energy = emin + (emax - emin) e[:, 0] (host), ecut 0 (the reference's cut is disabled). */
int cd_reverse_norm_staged(const float* voxels, const float* energy, const float* layerE, float* out, int batch,
                           const int32_t dims[3], const float consts[6], float max_deposit, float ecut, float alpha, float layer_eps,
                           int stage, void* stream);

/* Forward pre-processing of raw showers on the device, the inverse of cd_reverse_norm: utils.preprocess_shower
 * (calodiffusion/utils/utils.py:315-436) and the incident-energy map of DataLoaderCaloChall (:290-312, shower_scale included)
 * for the regular grids (dataset_num 2 / 3; showerMap 'layer-logit-norm' when layerE != NULL, 'logit-norm' otherwise).
 * showers (B, D*H*W) raw voxel energies and energy (B) raw incident energies, both multiplied by shower_scale first (0.001
 * for the CaloChallenge files, 1 for arrays that are already scaled); out (B,1,D,H,W) = (logit(showers / (max_deposit e))
 * - logit_mean) / logit_std with logit's alpha 1e-6; layerE (B, 1+D) = {(total - totalE_mean) / totalE_std,
 * (logit(layer / total) - layers_mean) / layers_std} or NULL; e_out (B,1) = log10(e / emin) / log10(emax / emin) if logE,
 * else (e - emin) / (emax - emin).  consts as for cd_reverse_norm.  One workgroup per shower: layer sums are taken in fp64 in
 * a fixed order, so a row does not depend on the batch it is in.  status: ONE device int32, zeroed by the call, then 1 + the
 * highest index of a shower with e <= 0 (or NaN / inf) or without any deposit -- where the reference's masked arrays return
 * fill values; the outputs of such a row are undefined.  Nothing is allocated and the stream is not synchronised: read
 * status after the stream has finished. */
int cd_preprocess(const float* showers, const float* energy, float* out, float* layerE, float* e_out, int32_t* status, int batch,
                  const int32_t dims[3], const float consts[6], float max_deposit, float emin, float emax, int logE,
                  float shower_scale, void* stream);

/* ---- HGCal geometry maps -------------------------------------------------------------------------------------------
 * The linear maps between HGCal's irregular cells and the regular (layer, alpha, r) grid: Embeder / Decoder / HGCalConverter of
 * calodiffusion/utils/HGCal_utils.py:295-407, 636-680.  init_map (:412-486) puts one or two non-zeros in a column of a layer's
 * (alpha*r, cells) matrix and its thresholded pseudo-inverse is as sparse, so a map is kept packed: per-layer CSR of every entry
 * != 0 in ascending column order (dropping exact zeros only, the product equals the dense einsum up to summation order), and
 * optionally the column-major view of the entries > 1e-6, which is the `mask` of generate_sparse_mat (:355-407). */
typedef struct CdGeomMap CdGeomMap;
/* Packs a dense DEVICE tensor (layers, rows, cols) -- Embeder.mat (L, E, N) or Decoder.mat (L, N, E), `mat * mask` for a
 * trainable one (:316, :341).  want_columns != 0 also builds the column view cd_geom_decode_sparse needs.  The handle owns its
 * index and value arrays (device memory allocated here); the call synchronises `stream`.  layers * rows * cols < 2^31. */
int cd_geom_create(const float* dense_dev, int layers, int rows, int cols, int want_columns, CdGeomMap** out, void* stream);
int cd_geom_destroy(CdGeomMap* map);
/* The same with a pattern of its own and further views.  mask_dev (nullable): a dense DEVICE tensor of the map's shape whose
 * non-zeros are the packed entries -- a trainable map's `mask` (:316, :341), so that entries whose value is 0 are kept (they take
 * gradient) and values outside the mask never enter; NULL: the entries != 0 of dense_dev, as cd_geom_create.  flags:
 * CD_GEOM_COLUMNS = want_columns (refused with a mask: that view holds values, which a refresh would leave stale);
 * CD_GEOM_TRANSPOSED builds the transposed view of ALL packed entries cd_geom_apply_vjp and cd_plan_set_geom need: per layer and
 * column the rows in ascending order, each with its place in the CSR arrays (no second copy of the values).  A mask without a
 * non-zero is a valid map and gives zeros. */
#define CD_GEOM_COLUMNS 1
#define CD_GEOM_TRANSPOSED 2
int cd_geom_create_ex(const float* dense_dev, const float* mask_dev /* nullable */, int layers, int rows, int cols, int flags,
                      CdGeomMap** out, void* stream);
/* The same map from its sparse entries, without the dense tensor (HGCal's decoders are 56 MB to 2.4 GB dense for 10^5 - 10^6
 * entries): per-layer CSR in HOST arrays, row_ptr (layers * rows + 1; line l * rows + i holds row i of layer l), col_idx and val
 * (row_ptr[layers * rows] entries each).  The pattern is taken as given: entries whose value is 0 are kept (a trainable map's mask
 * has them).  flags as above; CD_GEOM_COLUMNS builds the column view from the entries > 1e-6.  Every array of the handle equals
 * what cd_geom_create_ex builds from the dense tensor holding these entries (with that pattern as mask_dev if it has zeros), so
 * every consumer is bitwise unchanged.  Checked on the host before anything is uploaded or launched, CD_EINVAL with a message
 * otherwise: row_ptr[0] == 0, row_ptr non-decreasing, columns strictly ascending within a row and < cols, values finite.  The views
 * by column are built on the device from the entries (integer atomics count and place them, then every column is sorted by row:
 * the result does not depend on thread scheduling); peak memory is O(entries + layers * (rows + cols)).  Synchronises `stream`. */
int cd_geom_create_csr(const int32_t* row_ptr, const int32_t* col_idx, const float* val, int layers, int rows, int cols, int flags,
                       CdGeomMap** out, void* stream);
/* Gathers the packed values again from a dense DEVICE tensor of the map's shape (the live `mat` of a trainable map: call it
 * whenever the parameter changed).  One launch; the pattern and every view stay; the column view, if any, keeps its old values. */
int cd_geom_refresh(CdGeomMap* map, const float* dense_dev, void* stream);
/* Embeder.forward (:315-320) and Decoder.forward without sparse decoding (:340-349), with the converter's `norm` (enc :636-640,
 * dec :659-663):  y[r, l, i] = sum_j M[l, i, j] x[r, l, j]  for r < batch_rows (batch x channels);  x (batch_rows, L, cols),
 * y (batch_rows, L, rows).  scale = embed_std, shift = embed_mean: with affine_first the input is x * scale + shift (dec),
 * otherwise the output is (y - shift) / scale (enc), each operation rounded on its own as torch does; scale 1, shift 0 is the
 * plain product.  A row's sum runs over its entries in ascending j with fp32 FMAs: repeated calls are bitwise equal, and a
 * result row does not depend on batch_rows.  Nothing is allocated and the stream is not synchronised. */
int cd_geom_apply(const CdGeomMap* map, const float* x, float* y, int batch_rows, float scale, float shift, int affine_first,
                  void* stream);
/* Decoder.forward(sparse_decoding=True) (:340-349 with generate_sparse_mat, :355-407) without the (B, L, N, E) matrix: every
 * (shower, layer, column e) keeps the entries n with u + m > 1 and the one of largest u + m (the first of equal ones, as
 * torch.argmax), m the entries > 1e-6 of column e and u a uniform in [0, 1) per (b, l, n, e), and the column's input is shared
 * equally among them:  y[b, c, l, n] = sum over selected (n, e), in ascending e, of x[b, c, l, e] / count[b, l, e].
 * x (batch, channels, L, cols), y (batch, channels, L, rows); one selection serves every channel of a shower; per_batch != 0:
 * one selection (that of b = 0) serves every shower (sparse_per_batch).  u = rand[b, l, n, e] when rand is given, a dense DEVICE
 * tensor (batch or 1 if per_batch, L, rows, cols) (torch.rand_like's draw, :373); otherwise the 24-bit uniform of the Philox
 * stream (as cd_randn's) at element offset + ((b L + l) rows + n) cols + e, so a batch shard passes offset + first_shower * L *
 * rows * cols and draws its slice of the global tensor.  Two launches, no atomics: the first writes (argmax n, count) per
 * (b, l, e) into count_ws, caller memory of cd_geom_sparse_workspace_bytes; the second gathers per output row.  The map needs
 * its column view (want_columns).  Nothing is allocated and the stream is not synchronised. */
/* Vector-Jacobian product of cd_geom_apply (same x, scale, shift, affine_first) for a cotangent gy (batch_rows, L, rows); the map
 * needs its transposed view.  Either output may be NULL.
 *   dx (batch_rows, L, cols):  dx[r, l, j] = sum_i M[l, i, j] gy[r, l, i], a gather over the transposed view in ascending i with
 *       fp32 FMAs, no atomics; a row does not depend on batch_rows.  The affine rides along: gy / scale first (enc form), or the
 *       sum times scale (dec form, affine_first).
 *   dm (L, rows, cols), dense:  dm[l, i, j] = sum_r gy[r, l, i] x[r, l, j] on every packed entry -- for a map over a mask, every
 *       masked entry, also where the value is 0 -- and exact zeros everywhere else, which is autograd's gradient of `mat * mask`
 *       (the slot is cleared by a memset on the stream, then one thread per packed entry writes its sum).  The batch sum is
 *       plain ascending r, fp32 FMAs, no atomics: repeated calls are bitwise equal.  x enters as cd_geom_apply reads it
 *       (x * scale + shift with affine_first) and gy as above.
 * Nothing is allocated and the stream is not synchronised. */
int cd_geom_apply_vjp(const CdGeomMap* map, const float* x, const float* gy, float* dx /* nullable */, float* dm /* nullable */,
                      int batch_rows, float scale, float shift, int affine_first, void* stream);
int cd_geom_sparse_workspace_bytes(const CdGeomMap* map, int batch, size_t* bytes);
int cd_geom_decode_sparse(const CdGeomMap* map, const float* x, float* y, int batch, int channels, int per_batch,
                          const float* rand /* nullable */, uint64_t seed, uint64_t offset, void* count_ws, void* stream);

/* HGCal forward pre-processing, cells to training batch: what DataLoaderHGCal (calodiffusion/utils/HGCal_utils.py:89-164) does
 * between reading the file and returning (showers, gen, layerE) -- x shower_scale (:125-128), NN_embed.enc (:144-145, 636-640),
 * preprocess_hgcal_shower (:20-86), the condition map (:131-132, 158) -- in one launch, one workgroup per shower.
 *   enc != NULL  showers are raw cells (batch, layers, >= cells) with `row_stride` floats between layer rows (the [:, :, :max_cells]
 *                slice of a wider file array needs no copy); each is multiplied by shower_scale in float32 and every grid value
 *                is the packed map's row sum in ascending column order with the fmaf sequence and the (y - embed_mean) / embed_std
 *                rounding of cd_geom_apply(affine_first = 0), so the result is bitwise that of cd_geom_apply into a temporary
 *                followed by the enc == NULL form.  The map is (layers, grid, cells).  The grid of a shower stays in LDS:
 *                layers * grid * 4 bytes <= 48 KB, cells <= 2048, layers <= 512, or the call fails naming these limits.
 *   enc == NULL  showers are already on the grid, (batch, layers, grid) contiguous (cells = row_stride = grid); shower_scale,
 *                embed_mean and embed_std are not used.  Any size: a grid beyond 48 KB is read twice.
 * e = gen_info[:, 0], not scaled; gen_info (batch, gen_cols), gen_cols <= 8.  Outputs: out (batch, layers, grid), layerE
 * (batch, 1 + layers) or NULL ('logit-norm'), e_out (batch, gen_cols) = (gen_info - emin) / (emax - emin) per column, in double
 * from the HOST arrays emin / emax[gen_cols] (np.array(emin) is float64, :131-132) and rounded once.
 * Numerics, as the reference forms them.  q = grid / (max_deposit e) is float32.  With layerE the reference's arrays are numpy
 * masked arrays, whose arithmetic with python scalars is float64: the layer sums, the total and their quotient are float32 (here
 * summed in fp64 in a fixed order -- a wave per layer, then the layers in layer order -- and rounded to float32 once), and
 * logit (alpha 1e-8), the normalisations of total, layers and of every voxel are float64, rounded to float32 at the end; the
 * voxels are not divided by their layer's energy.  Without layerE everything is float32.  consts = {logit_mean, logit_std,
 * totalE_mean, totalE_std, layers_mean, layers_std} as doubles (rounded to float32 by the float32 mode, as numpy rounds them).
 * logit is np.ma.log(o / (1 - o)).filled(0), o = alpha + (1 - 2 alpha) x: where the argument is not positive or the logarithm
 * not finite the value is 0 BEFORE the normalisation (negative embedded values of a set with embed_mean > 0, negative layer
 * shares); a layer without deposit is ordinary data (logit(0)), and a shower whose total is 0 has its layer shares masked the
 * same way (np.ma.divide): defined results, no error.  status: ONE device int32, zeroed by the call, then 1 + the highest index
 * of a shower with e <= 0, NaN or inf, where the reference returns whatever its masked buffers hold; such a row's outputs are
 * not written.  A row's bits do not depend on the batch.  Nothing is allocated, no atomics but the status, and the stream is
 * not synchronised: read status after the stream has finished. */
int cd_preprocess_hgcal(const CdGeomMap* enc /* nullable */, const float* showers, int64_t row_stride, const float* gen_info,
                        int gen_cols, float* out, float* layerE /* nullable */, float* e_out, int32_t* status, int batch,
                        int layers, int cells, int grid, const double consts[6], float embed_mean, float embed_std,
                        float max_deposit, const double* emin, const double* emax, float shower_scale, void* stream);

/* ---- Dataset-1 radial maps ----------------------------------------------------------------------------------------
 * The linear maps between CaloChallenge Dataset-1's irregular voxels and the regular (layer, alpha, r) grid: GeomConverter
 * (calodiffusion/utils/utils.py:659-784) with fixed matrices, NNConverter (:576-656) with trainable ones.  A flat shower
 * (V voxels) is L layers; layer i holds voxels [bound[i], bound[i+1]) as (alpha[i], rin[i]), alpha[i] either 1 or A; the grid is
 * (L, A, R).  The matrices are the `weight` tensors of the reference's nn.Linear(bias=False) layers, concatenated in layer
 * order: encoder W_i (R, rin_i) at float offset R * (rin_0 + ... + rin_{i-1}), decoder D_i (rin_i, R) at the same offset.  They
 * are DEVICE arrays passed per call (live parameters); the handle holds the layout only.
 * Every sum is a chain of fp32 FMAs in a fixed order, there are no atomics, a row b of a result depends on row b of the inputs
 * only (not on `batch`), and repeated calls are bitwise equal.  Each call is one launch; nothing is allocated and the stream is
 * not synchronised.  A workgroup keeps the matrices of one direction and one shower in LDS, which sets the limits
 *   L <= 64,   R * (rin_0 + ... + rin_{L-1}) <= 8192 floats (32 KB),   max(V, L * A * R) <= 6144 floats (24 KB);
 * a geometry beyond them is refused by cd_radial_create (Dataset-1 photons: 5 layers, 1590 and 1500 floats). */
typedef struct CdRadialMap CdRadialMap;
/* bound[L+1], alpha[L], rin[L] are HOST arrays, copied to the device here (the call allocates, and synchronises `stream`).
 * Refused with CD_EINVAL, before anything touches the device: null pointers, non-positive sizes, bound[0] != 0, a bound that is
 * not strictly increasing, an alpha[i] outside {1, A} (where the reference calls exit(1), :626-631), rin[i] <= 0, a span
 * bound[i+1] - bound[i] != alpha[i] * rin[i], and the limits above. */
int cd_radial_create(int layers, const int32_t* bound, const int32_t* alpha, const int32_t* rin, int alpha_out, int r_out,
                     CdRadialMap** out, void* stream);
int cd_radial_destroy(CdRadialMap* map);
/* NNConverter.enc (:610-633) and GeomConverter.convert of the reshaped shower (:724-732, 744-764): x (batch, V) ->
 * y (batch, 1, L, A, R);  y[b,0,i,a,:] = W_i x[b, layer i, a, :]  where alpha[i] == A, else  (W_i x[b, layer i, 0, :]) / A  in
 * every a: the dot product in ascending input bin, then the one division (:618-625). */
int cd_radial_enc(const CdRadialMap* map, const float* w, const float* x, float* y, int batch, void* stream);
/* NNConverter.dec (:635-653) and GeomConverter.unconvert + unreshape (:734-742, 766-784): g (batch, 1, L, A, R) -> x (batch, V);
 * o[b,a,:] = D_i g[b,0,i,a,:] in ascending r, and where alpha[i] == 1 the voxel is the sum of o over a in ascending a (:644). */
int cd_radial_dec(const CdRadialMap* map, const float* d, const float* g, float* x, int batch, void* stream);
/* What autograd derives from enc: dx (batch, V) = enc's transpose applied to gy (batch, 1, L, A, R) -- per a the sum over r in
 * ascending r; where alpha[i] == 1 those are summed in ascending a and divided by A once -- and, unless dw is NULL,
 * dw (as w):  dW_i[r, j] = sum_b sum_a gy[b,0,i,a,r] x[b, layer i, a, j]  (alpha[i] == 1: sum_b ((sum_a gy[b,0,i,a,r]) / A) x[b, layer
 * i, 0, j]).  The batch sum has a fixed order: 8 interleaved slices (b mod 8), each in ascending b and a, then a fixed tree over
 * the slices, inside the same launch. */
int cd_radial_enc_vjp(const CdRadialMap* map, const float* w, const float* x, const float* gy, float* dx, float* dw /* nullable */,
                      int batch, void* stream);
/* What autograd derives from dec: dg (batch, 1, L, A, R):  dg[b,0,i,a,:] = D_i^T gx[b, layer i, a, :]  (alpha[i] == 1: of
 * gx[b, layer i, 0, :], in every a), in ascending input bin, and, unless dd is NULL, dd (as d):  dD_i[j, r] = sum_b sum_a
 * gx[b, layer i, a, j] g[b,0,i,a,r]  (alpha[i] == 1: sum_b gx[b, layer i, 0, j] sum_a g[b,0,i,a,r]), reduced as dw is. */
int cd_radial_dec_vjp(const CdRadialMap* map, const float* d, const float* g, const float* gx, float* dg, float* dd /* nullable */,
                      int batch, void* stream);

/* Dataset-0/1 forward pre-processing, raw showers to a loader batch: utils.preprocess_shower (calodiffusion/utils/utils.py:
 * 315-436) and the incident-energy map of DataLoaderCaloChall (:290-312, shower_scale included) over the irregular layout of
 * `map`, one launch.  showers (batch, V) and energy (batch) are raw, both multiplied by shower_scale first; e_out (batch, 1),
 * status, shower_scale and the no-energy rule are cd_preprocess's: ONE device int32, zeroed by the call, then 1 + the highest
 * index of a shower with e <= 0, NaN or inf, or without any deposit; an empty layer of a shower that has energy elsewhere is
 * ordinary data.  consts = {logit_mean, logit_std, totalE_mean, totalE_std, layers_mean, layers_std} (utils/consts.py:4-80).
 *   conv_w == NULL  the flat form (orig_shape, :341-342, 369-380): out (batch, V) = (logit(q) - logit_mean) / logit_std,
 *                   q = showers / (max_deposit e) in float32, logit's alpha 1e-6.  layerE (batch, 1 + L) or NULL: the sum of q
 *                   over each ragged segment [bound[i], bound[i+1]) -- a wave per layer, lanes strided, a xor butterfly, in fp64
 *                   -- and their total in layer order, both rounded to float32 as the reference holds them; then, as the
 *                   reference's masked arrays promote to float64, layerE = {(total - totalE_mean) / totalE_std,
 *                   (logit(layer / total) - layers_mean) / layers_std} and every voxel's logit and normalisation in fp64,
 *                   rounded to float32 once.  Without layerE ('logit-norm') everything is float32, as cd_preprocess does it.
 *   conv_w != NULL  the grid form (:331-333): conv_w holds GeomConverter.weight_mats in cd_radial_enc's layout, out is
 *                   (batch, 1, L, A, R); layerE must be NULL (the reference's own preprocess_shower fails on a 'layer' map
 *                   here).  The steps in the reference's order: cd_radial_enc's dot products on the scaled shower, the division
 *                   by max_deposit e, logit-norm -- bitwise cd_radial_enc of the scaled showers into a temporary followed by
 *                   cd_preprocess on dims {L, A, R}.
 * A shower is staged in LDS once and has one owner workgroup, which walks showers blockIdx, blockIdx + grid, ...: a row's bits
 * do not depend on the batch.  No atomics but the status word; nothing is allocated and the stream is not synchronised. */
int cd_preprocess_ds1(const CdRadialMap* map, const float* conv_w /* nullable */, const float* showers, const float* energy,
                      float* out, float* layerE /* nullable */, float* e_out, int32_t* status, int batch, const double consts[6],
                      float max_deposit, float emin, float emax, int logE, float shower_scale, void* stream);
/* Its inverse, utils.ReverseNormCaloChall (:446-573) for Dataset 0/1; energy (batch) in physical units as for cd_reverse_norm.
 *   unconv_w == NULL  the flat form: voxels (batch, V); un-normalise and reverse_logit (alpha 1e-6); with layerE (batch, 1 + L)
 *                     negatives are clamped to 0 and every ragged segment is rescaled to its layer energy, the factor 1 where
 *                     the layer or the segment sum is below 1e-6 (:549-557); then x max_deposit x energy and the ecut threshold.
 *   unconv_w != NULL  the grid form (:562-564): voxels (batch, 1, L, A, R), unconv_w holds GeomConverter.pinv_mats in
 *                     cd_radial_dec's layout, layerE must be NULL; reverse_logit in the staging of cd_radial_dec's row program,
 *                     its dot products, then x max_deposit x energy and ecut on the flat row; negatives are not clamped.
 *                     Bitwise cd_reverse_norm_staged(stage 1), cd_radial_dec, cd_reverse_norm_staged(stage 2, dims {1, 1, V}).
 * reverse_logit where float32 exp(x) overflows (x > 88.7) is the logistic function's limit 1; the reference's exp / (1 + exp) is
 * inf / inf there, which in layer mode turns the whole layer into NaN.
 * out (batch, V).  One launch, no atomics; nothing is allocated and the stream is not synchronised. */
int cd_reverse_norm_ds1(const CdRadialMap* map, const float* unconv_w /* nullable */, const float* voxels, const float* energy,
                        const float* layerE /* nullable */, float* out, int batch, const double consts[6], float max_deposit,
                        float ecut, void* stream);

/* A plan's flat-state embedding: CaloDiffusion.forward with an NN_embed (calodiffusion/models/calodiffusion.py:86-98) runs enc
 * before and dec after the U-Net, and the EDM preconditioning, the samplers and the loss act on the flat shower.  With a map
 * set, the per-sample state of cd_denoise, cd_denoise_safe, cd_ddim_sample, cd_sampler_run, cd_loss_hybrid*, cd_train_step and
 * cd_denoise_vjp (and their workspace queries) is V = bound[L] floats, shape (batch, V), instead of the grid:
 *   denoise(x) = combine(x, dec(F(enc(c_in x))))   -- the scaling first, then enc; F on the grid; combine as CD_OBJ_* says.
 * Two launches more per denoise: embed-in before the init conv (which then does not scale again) and embed-out after the head
 * (dec, the combination and, in cd_ddim_sample, the fused sampler update).  enc_w / dec_w are DEVICE arrays in cd_radial_enc's /
 * cd_radial_dec's layout, read in place by every later call (live parameters, as the map: both must outlive their use).
 * want_grads: cd_train_step and cd_denoise_vjp (with grads) write their gradients behind the U-Net's in the flat gradient buffer --
 * cd_plan_grad_layout then takes idx = cd_plan_num_weights for enc_w and + 1 for dec_w, and its total grows -- reduced as
 * cd_radial_enc_vjp / cd_radial_dec_vjp reduce them; 0 (frozen matrices): those slots are not written and no reduction runs.
 * Refused with CD_EINVAL before anything touches the device: a map whose (L, alpha_out, r_out) is not the plan's grid, a map
 * without matrices.  map = NULL clears the embedding (the other arguments are ignored): every launch sequence is then the
 * plan's own.  cd_unet_forward is the raw network either way; cd_bns_theta_grad refuses a plan with an embedding.  Every call with a
 * map, or that clears one, synchronises `stream` and drops the cached step graphs; call cd_plan_grad_layout and the workspace queries after. */
int cd_plan_set_radial(CdPlan* plan, const CdRadialMap* map /* nullable */, const float* enc_w, const float* dec_w, int want_grads,
                       void* stream);

/* The same seam with HGCal's maps (HGCalConverter inside forward, calodiffusion.py:86-98, 113-117): the per-sample state of the
 * calls above becomes layers x cells floats, shape (batch, 1, L, cells), and
 *   denoise(x) = combine(x, dec(F(enc(c_in x))))
 * with enc = cd_geom_apply(enc_map) and dec = cd_geom_apply(dec_map), both plain (in-model the converter has no `norm`); the same
 * two launches more per denoise, embed-out with the objective's combination and cd_ddim_sample's fused update.  The maps are
 * read in place by every later call and must outlive their use; a trainable map's values are refreshed by cd_geom_refresh.
 * want_grads: two DENSE gradient slots, (L, grid, cells) for enc_map and (L, cells, grid) for dec_map, follow the U-Net's in the
 * flat gradient buffer (cd_plan_grad_layout: idx = cd_plan_num_weights and + 1), written as cd_geom_apply_vjp's dm.  0 (frozen
 * maps): the slots do not exist, no weight-gradient work runs, cd_train_step launches dec's input gradient only and
 * cd_denoise_vjp enc's too.  Refused with CD_EINVAL before anything touches the device: maps whose (layers, rows) -- enc's -- or
 * (layers, cols) -- dec's -- is not the plan's (L, alpha * r), whose cell counts disagree, or without a transposed view.
 * Setting one kind of embedding clears the other; enc_map = NULL clears this one.  Synchronises and drops the step graphs as
 * cd_plan_set_radial does; cd_bns_theta_grad refuses such a plan. */
int cd_plan_set_geom(CdPlan* plan, const CdGeomMap* enc_map /* nullable */, const CdGeomMap* dec_map, int want_grads, void* stream);

/* ---- LayerDiffusion's layer-energy model --------------------------------------------------------------------------
 * The conditional residual MLP `ResNet` (calodiffusion/models/models.py:391-457) that LayerDiffusion
 * (calodiffusion/models/layerdiffusion.py:35-38, 114-132) samples the (B, D+1) {total, per-layer} energies with.
 * Stateless: `weights` is a HOST array of n_weights = 2*(8 + 3*n_res) DEVICE pointers, (weight, bias) per nn.Linear in the
 * module's state_dict order: time_mlp.{1,3,5}, cond_mlp.{0,2,4}, in_lay, hidden_layers.i.{embeder.1, dense1.0, dense2.0},
 * out_lay; torch (out, in) row-major fp32. */
typedef struct CdLayerMlpDesc {
  uint32_t struct_size;     /* = sizeof(CdLayerMlpDesc) */
  int32_t dim_in;           /* SHAPE_FINAL[2] + 1 */
  int32_t hidden;           /* 256 */
  int32_t cond_emb;         /* 128: cat(cond_mlp, time_mlp) */
  int32_t cond_size;        /* 1 (3 for HGCal) */
  int32_t n_res;            /* num_layers - 1 ResDense blocks */
  int32_t time_embed_kind;  /* CD_TIME_* (calodiffusion.py:144-152) */
  int32_t objective;        /* CD_OBJ_* */
  float sigma_data;
} CdLayerMlpDesc;

/* ResNet.forward(x, cond, time) (models.py:444-457): x (B, dim_in), cond (B, cond_size), time (B) -> out (B, dim_in). */
int cd_layer_forward(const CdLayerMlpDesc* desc, const float* const* weights, int n_weights, int batch, const float* x,
                     const float* cond, const float* time, float* out, void* stream);
/* CaloDiffusion.denoise on the layer model (calodiffusion.py:154-169 with layerdiffusion.py:109-112): sigma (B). */
int cd_layer_denoise(const CdLayerMlpDesc* desc, const float* const* weights, int n_weights, int batch, const float* x,
                     const float* sigma, const float* cond, float* out, void* stream);
/* LayerDiffusion.sample_layers' sampler loop (layerdiffusion.py:114-132 -> models/sample.py:40-110) in ONE launch.
 * steps_dev: DEVICE (n_steps, 4) table of CdStep rows; step_noise (n_steps, B, dim_in) or NULL (deterministic);
 * xs / x0s (n_steps, B, dim_in) or NULL. */
int cd_layer_sample(const CdLayerMlpDesc* desc, const float* const* weights, int n_weights, int batch, const float* start,
                    const float* cond, const CdStep* steps_dev, int n_steps, const float* step_noise, float* x_out, float* xs,
                    float* x0s, void* stream);
/* A sampler step program (CdSamplerOp, as cd_sampler_run) on the layer model: the whole trajectory in ONE launch, one workgroup
 * per sample with the n_bufs (2..10) state vectors on chip.  Every sampler class of calodiffusion_amd/sample.py that builds a
 * program runs on the layer stage through it.
 * start (B, dim_in): buffer 0 = start * start_scale, the others start at zero.  DENOISE is cd_layer_denoise at
 * sigma = coefs[step][col] (DENOISE_PS: sample b at coefs[step][col + b]); LINCOMB / LINDIV round as cd_sampler_run's.  ops (n_ops), op_begin (NULL, or n_steps + 1 entries)
 * and coefs (n_steps, n_coef) are DEVICE arrays.  The k-th RANDN op executed takes the Philox stream elements
 * offset + k * stride + b * dim_in + i, stride = noise_stride ? noise_stride : B * dim_in (cd_sampler_run's convention, so batch
 * shards are slices of one global stream); step_noise, when given: DEVICE (RANDN ops executed, B, dim_in), tensor k instead.
 * x_out (B, dim_in); xs / x0s: NULL or (n_steps, B, dim_in), written by RECORD.
 * The op list and op_begin are checked on the host before anything is launched (kinds, 1..6 sources, buffer indices below
 * n_bufs, coefficient columns below n_coef, op_begin from 0 to n_ops and non-decreasing): a bad program is an error return.
 * That check reads them back (a few hundred bytes), so the call synchronises with `stream` once and cannot be captured into a
 * graph; it allocates nothing. */
int cd_layer_sampler_run(const CdLayerMlpDesc* desc, const float* const* weights, int n_weights, int batch, const float* start,
                         float start_scale, const float* cond, int n_bufs, int n_steps, const CdSamplerOp* ops_dev, int n_ops,
                         const int32_t* op_begin_dev, const float* coefs_dev, int n_coef, const float* step_noise, uint64_t seed,
                         uint64_t offset, uint64_t noise_stride, float* x_out, float* xs, float* x0s, void* stream);

/* Training step of the layer model (LayerDiffusion.compute_loss in the layer state, models/layerdiffusion.py:52-57, with
 * the l2 loss of models/loss.py:103-104,118-142): data = layer energies (B, dim_in), noise (B, dim_in), sigma (B),
 * cond (B, cond_size).  loss_out: one double; grads: ONE flat device buffer holding the gradient of every parameter in the
 * order of `weights` (weight, bias, weight, bias, ...), each with the parameter's element count.  The objective is the
 * descriptor's CD_OBJ_* (see cd_layer_train_step_loss).  workspace: cd_layer_train_workspace_bytes.  Nothing is allocated and
 * the stream is not synchronised. */
int cd_layer_train_workspace_bytes(const CdLayerMlpDesc* desc, int batch, size_t* bytes);
int cd_layer_train_step(const CdLayerMlpDesc* desc, const float* const* weights, int n_weights, int batch, const float* data,
                        const float* noise, const float* sigma, const float* cond, double* loss_out, float* grads,
                        void* workspace, size_t workspace_bytes, void* stream);
/* The same for every LOSS_TYPE of Loss._loss (models/loss.py:97-116; cd_layer_train_step is loss_type CD_LOSS_L2): the reference's
 * CI fixture trains the layer model with 'huber' (tests/test_execution.py:94).  Every objective of the descriptor, with pred /
 * target / weight as models/loss.py:163-210 defines them on x_noisy = data + sigma noise (the weight enters 'l2' only):
 *   CD_OBJ_HYBRID      pred = denoise(x_noisy)                                   target = data   weight 1 + sigma^-2
 *   CD_OBJ_NOISE_PRED  pred = (data - (data - sigma denoise(x_noisy))) / sigma   target = noise  weight 1
 *   CD_OBJ_MEAN_PRED   pred = denoise(x_noisy) = F                               target = data   weight sigma^-2 */
int cd_layer_train_step_loss(const CdLayerMlpDesc* desc, const float* const* weights, int n_weights, int batch, const float* data,
                             const float* noise, const float* sigma, const float* cond, int loss_type /* CD_LOSS_* */,
                             double* loss_out, float* grads, void* workspace, size_t workspace_bytes, void* stream);
/* The loss of cd_layer_train_step_loss alone (validation): the same kernel without its tape and backward, and no
 * weight-gradient launch; loss_out is bitwise the training step's.  workspace: cd_layer_train_workspace_bytes. */
int cd_layer_loss(const CdLayerMlpDesc* desc, const float* const* weights, int n_weights, int batch, const float* data,
                  const float* noise, const float* sigma, const float* cond, int loss_type /* CD_LOSS_* */, double* loss_out,
                  void* workspace, size_t workspace_bytes, void* stream);

/* Workspace of cd_layer_denoise_vjp at this batch: with_param_grads 0 sizes the input-gradient-only call (grads == NULL), 1 the
 * call that also writes grads (the per-sample tape). */
int cd_layer_vjp_workspace_bytes(const CdLayerMlpDesc* desc, int batch, int with_param_grads, size_t* bytes);
/* Vector-Jacobian product of cd_layer_denoise: given D = cd_layer_denoise(x, sigma, cond) and gy = dL/dD (B, dim_in), writes
 * dx = dL/dx (B, dim_in) and, when grads is not NULL, dL/dW of every parameter into the flat buffer of cd_layer_train_step
 * (overwritten, not accumulated; fixed-order sums: repeated calls are bitwise equal).  sigma and cond are constants.  Every
 * objective and time embedding of the descriptor.  The forward is recomputed inside the call (one launch; one more for the
 * parameter gradients).  With grads == NULL no tape is written, no parameter-gradient work is launched and dx is bitwise the dx
 * of the call with grads.  All scratch is in `workspace`; nothing is allocated and the stream is not synchronised. */
int cd_layer_denoise_vjp(const CdLayerMlpDesc* desc, const float* const* weights, int n_weights, int batch, const float* x,
                         const float* sigma, const float* cond, const float* gy, float* dx, float* grads /* nullable */,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- generator: incident energies in, physical showers out, without Python -------------------------------------------
 * A generator file (calodiffusion_amd/generator.py: export_generator; format: DESIGN.md "Generator file") holds everything
 * Diffusion.generate / LayerDiffusion.generate (calodiffusion/models/diffusion.py:118-197, layerdiffusion.py:171-235) need for one
 * model (Dataset 2 / 3 on the regular grid, HGCal with its geometry maps in the file, or Dataset 0 / 1 with its irregular layout
 * and matrices in the file; '[layer-]logit-norm'): the U-Net's descriptor, coordinate profiles and weights, LayerDiffusion's
 * layer model, each stage's compiled sampler (CdStep table or step program) and the inverse pre-processing record.
 * cd_generator_run is the launch sequence of that Python path -- start tensor from the Philox stream, (layer stage,) conditioning
 * row, U-Net sampler, cd_reverse_norm -- with the same stream offsets, so its showers are the ones generate() returns for the same
 * seed and offset (to the bit within a process; the convolutions' tilings are picked by a timer once per process and differ in the
 * last bits, so two processes agree to the bit only with CD_NO_AUTOTUNE set in both).  tools/cd_generate_example.c is a complete
 * caller.
 *
 * cd_generator_create: blob is HOST memory (the file's bytes; not needed after the call); a malformed one is CD_EINVAL with a
 * message, whatever its bytes.  It allocates the plan (cd_plan_create's device memory) and ONE device block that lives as long as
 * the handle: the layer model's weights (about 3 MB for 45 layers) and its step table or program, each rounded up to 256 bytes;
 * a model without a layer stage has no block.  A staging block of the U-Net's fp32 tensors (the sum of their sizes, each rounded
 * up to 256 bytes) is freed before create returns.  An HGCal file (format version 2) also gets its geometry maps, built from the
 * file's sparse entries by cd_geom_create_csr -- the decoder with its column view (pre-embedded), or encoder and decoder with their
 * transposed views, bound by cd_plan_set_geom (converter inside the model): device memory in proportion to the entries, never the
 * dense (layers, rows, cols) tensor.  A Dataset-0/1 file (format version 3) gets a CdRadialMap from the layout in its RADL section
 * (cd_radial_create, after the reader has checked every rule of that call on the host) and its matrices in one more device block
 * -- encoder and decoder, bound by cd_plan_set_radial with want_grads 0 (form 1: SHOWER_EMBED 'orig-NN', the sampler's state is
 * the flat shower (batch, V)), or the un-conversion matrices alone (form 0: the state is the converted grid).  The call
 * synchronises `stream`. */
typedef struct CdGenerator CdGenerator;
int cd_generator_create(const void* blob, size_t bytes, CdGenerator** out, void* stream);
int cd_generator_destroy(CdGenerator* gen);
/* The file's checksum for code that writes or verifies one: 64-bit FNV-1a of `bytes` bytes of HOST memory (everything behind the
 * 64-byte header).  Host code; touches no device. */
int cd_generator_checksum(const void* data, size_t bytes, uint64_t* out);
/* info[8] (host) = {voxels per shower (HGCal: layers x cells), layers D, energy columns, has layer stage, takes layer energies,
 * sample steps, layer steps (0 without a layer stage), format version}. */
int cd_generator_info(const CdGenerator* gen, int32_t* info);
/* geom[8] (host) = {kind of the file's geometry section: 0 none (a regular grid), 1 HGCal maps (GEOM), 2 Dataset-0/1 radial maps
 * (RADL); its form: 0 the model runs on the grid and the run converts at its end, 1 the converter is inside the model, -1 for
 * kind 0; dimensions of the sampler's per-sample state; its shape, unused entries 0 -- (1, D, H, W) on a grid, (1, layers, cells)
 * for HGCal form 1, (V) for Dataset-0/1 form 1; 0}.  A call of its own because cd_generator_info's eight entries are all taken and
 * its array cannot grow without breaking callers that pass int32_t[8]: adding an entry point leaves CD_ABI_VERSION as it is. */
int cd_generator_geometry(const CdGenerator* gen, int32_t* geom);
int cd_generator_workspace_bytes(CdGenerator* gen, int batch, size_t* bytes);
/* energy (batch, energy columns): the conditioning values e (energy_is_normalised != 0, what a loader of the Python path yields) or physical
 * incident energies in the unit of the config's EMIN / EMAX, mapped in the call as cd_preprocess maps them.  Either way the
 * energies cd_reverse_norm scales by are emin * (emax / emin)^e (logE; emin + (emax - emin) e otherwise) formed from e on the
 * device, the power correctly rounded to fp32 (numpy's float32 power, which the Python path takes on the host, may differ from it
 * in the last bit depending on the host's vector math library).
 * layers (batch, 1 + D), normalised: required for a model that conditions on layer energies and has no layer stage
 * (CaloDiffusion on a 'layer-' map), refused otherwise.  layers_out (batch, 1 + D), nullable: the layer energies the showers were
 * conditioned on (generated, or a copy of `layers`); not written for a model that takes none.
 * showers (batch, voxels): physical showers, the rows of generate()'s first return value.
 * seed / offset: the Philox stream position (model.noise_seed / model.noise_offset); *next_offset (HOST, nullable): the value
 * model.noise_offset holds after the same batch -- pass it as the next call's offset.  first_row / global_batch:
 * Diffusion.set_noise_shard's arguments, this call generates rows [first_row, first_row + batch) of a global batch; 0, batch (or
 * 0, 0) = unsharded.
 * Nothing is allocated; all scratch is in `workspace` (cd_generator_workspace_bytes at this batch).  The argument checks (a NULL
 * or unexpected `layers`, a short workspace) come before the first launch.  The call synchronises `stream` where the sampler
 * entry points do: their range fallback, and cd_layer_sampler_run's program check. */
int cd_generator_run(CdGenerator* gen, int batch, const float* energy, int energy_is_normalised, const float* layers /* nullable */,
                     uint64_t seed, uint64_t offset, int first_row, int global_batch, float* showers, float* layers_out /* nullable */,
                     uint64_t* next_offset /* nullable */, void* workspace, size_t workspace_bytes, void* stream);

/* The same run for every generator file, HGCal's (format version 2) included; cd_generator_run is this call with sparse_mode 0.
 * An HGCal file carries its geometry maps, and the run ends as ReverseNormHGCal does: cd_reverse_norm_staged stage 1, for a
 * pre-embedded model (form 0) the decode onto the cells -- cd_geom_apply with the converter's norm, or with sparse_mode != 0
 * cd_geom_decode_sparse on the decoder's own Philox stream -- and stage 2; a model with the converter inside (form 1) samples the
 * cells themselves.  energy is (batch, energy columns of cd_generator_info), showers (batch, layers * cells).  Physical energies
 * (energy_is_normalised == 0) map per column as cd_preprocess_hgcal maps them; stage 2 scales by
 * (float)(emin[0] + (emax[0] - emin[0]) * (double)e[0]).
 * sparse_mode: 0 plain decode, 1 sampled per shower, 2 sampled per batch (one selection serves the batch); != 0 needs a file
 * whose decoder has a column view (form 0), CD_EINVAL otherwise.  decode_seed / decode_offset: the position in the decoder's
 * stream (Decoder.noise_seed / noise_offset); *next_decode_offset (HOST, nullable) = decode_offset + (batch, or 1 per batch)
 * * layers * cells * grid bins, so chained calls draw what one decode of the concatenated batches draws.
 * A Dataset-0/1 file (format version 3) ends in cd_reverse_norm_ds1 with the constants of its RNRM record: the flat form with the
 * layer energies of a 'layer-' map (form 1), the grid form with the file's un-conversion matrices (form 0); one energy column,
 * mapped as for the regular grids; showers (batch, V); sparse_mode != 0 is CD_EINVAL.
 * (Tag and typedef are declared apart because the struct holds pointers, as CdHlfDesc.) */
struct CdGeneratorRun {
  uint32_t struct_size;         /* = sizeof(CdGeneratorRun) */
  int32_t batch;
  const float* energy;          /* DEVICE (batch, energy columns) */
  int32_t energy_is_normalised;
  int32_t sparse_mode;
  const float* layers;          /* DEVICE (batch, 1 + layers), nullable: as cd_generator_run */
  uint64_t seed, offset;
  int32_t first_row, global_batch;
  float* showers;               /* DEVICE (batch, voxels) */
  float* layers_out;            /* DEVICE (batch, 1 + layers), nullable */
  uint64_t* next_offset;        /* HOST, nullable */
  uint64_t decode_seed, decode_offset;
  uint64_t* next_decode_offset; /* HOST, nullable */
  void* workspace;
  size_t workspace_bytes;
  void* stream;
};
typedef struct CdGeneratorRun CdGeneratorRun;
int cd_generator_run_ex(CdGenerator* gen, const CdGeneratorRun* args);

/* ---- shower observables: the CaloChallenge high-level features -------------------------------------------------------
 * HighLevelFeatures.CalculateFeatures of the reference (calodiffusion/utils/HighLevelFeatures.py:48-89) over the voxel positions
 * XMLHandler.SetEtaAndPhiFromPolar derives (utils/XMLHandler.py:72-108): per shower and layer the deposited energy, the centre of
 * energy in eta and phi and their widths -- and the hit count and brightest voxel the reference's plots take from the same
 * showers (utils/plots.py:688, 916, 982) -- in one pass over the showers instead of one float64 temporary per product and layer.
 *
 * The descriptor holds HOST pointers, copied to the device by cd_hlf_create (the call allocates, and synchronises `stream`):
 * layer l owns voxels [layer_offset[l], layer_offset[l + 1]) of a flat shower of V = layer_offset[n_layers] voxels (the
 * `bin_edges`), eta / phi are the V positions, and with_centres[l] != 0 where centres and widths are defined (the reference:
 * l in layersBinnedInAlpha, :78-79).  A layer without voxels has no record; the R layers with voxels, in ascending l, are
 * GetRelevantLayers().  Refused with CD_EINVAL, before anything touches the device: a struct_size other than
 * sizeof(CdHlfDesc), n_layers <= 0, a null layer_offset / eta / phi / with_centres table, layer_offset[0] != 0, a
 * layer_offset that decreases, V == 0.
 * (Tag and typedef are declared apart because the struct holds pointers: a binder lays it out with its own pointer type.) */
struct CdHlfDesc {
  uint32_t struct_size;         /* = sizeof(CdHlfDesc) */
  int32_t n_layers;
  const int32_t* layer_offset;  /* [n_layers + 1] */
  const double* eta;            /* [V] */
  const double* phi;            /* [V] */
  const int32_t* with_centres;  /* [n_layers] */
};
typedef struct CdHlfDesc CdHlfDesc;
typedef struct CdHlf CdHlf;
int cd_hlf_create(const CdHlfDesc* desc, CdHlf** out, void* stream);
int cd_hlf_destroy(CdHlf* hlf);
/* showers (batch, V) fp32 on the device, in physical units.  out (batch, R, 8) fp64 = {E, EC_eta, EC_phi, var_eta, var_phi,
 * width_eta, width_phi, max_voxel} and n_hits (batch, R) int32 = the number of voxels > threshold, with (:48-68)
 *   E = sum e,   EC_c = sum c e / (E + 1e-16),   var_c = max(sum c c e / (E + 1e-16) - EC_c^2, 0),   width_c = sqrt(var_c);
 * the six centre / variance / width values of a layer without centres are 0.  Every shower element is read once.  A layer of
 * a shower is summed by 16 lanes: lane j takes the layer's voxels j, j + 16, ... in ascending order, every sum is fp64 (the
 * voxel energies enter exactly), and the lanes are combined by a fixed tree -- no atomics, so repeated calls are bitwise equal and a record does not depend on the batch it is in or on the row's alignment.
 * The grid is layers x shower slices in one dimension and is capped: any batch an int holds.  Nothing is allocated and the
 * stream is not synchronised. */
int cd_hlf_compute(const CdHlf* hlf, const float* showers, int batch, float threshold, double* out, int32_t* n_hits, void* stream);

/* ---- shower statistics: what the plot program computes before it draws ------------------------------------------------
 * The arithmetic of the reference's plot classes (calodiffusion/utils/plots.py): ELayer :567-576, SparsityLayer :684-692,
 * AverageShowerWidth :461-518, AverageER :617-625, AverageEPhi :651-658, HistEtot :884-887, HistERatio :406-418, HistNhits
 * :912-916, HistMaxE :1003-1010, HistMaxELayer :978-984, RadialEnergyHGCal :720-734, RCenterHGCal :748-779 and PhiCenterHGCal
 * :810-839.  Each of them reshapes and sums the whole shower set again; here one pass over the showers leaves the raw sums
 * they all derive from, and the divisions, masks and roots are the caller's, on (batch, layers) arrays.
 *
 * A shower is (n_layers, n_cells) fp32: a regular grid's (L, A x R) or HGCal's (L, max_ncell).  The geometry is four HOST
 * tables of n_layers * n_cells entries, copied to the device by cd_shower_stats_create (the call allocates, and synchronises
 * `stream`): r_bin in [-1, n_rbins) (-1: the cell is in no radial bin), a_bin in [-1, n_abins) or NULL with n_abins == 0,
 * r_coord and angle (radians; the cosine and sine are tabulated here).  Cells beyond a layer's real cell count are ordinary
 * cells.  Refused with CD_EINVAL, before anything touches the device: a struct_size other than sizeof(CdShowerStatsDesc),
 * n_layers outside [1, 512], n_cells outside [1, 4096], n_rbins outside [1, 256], n_abins outside [0, 256], a null r_bin /
 * r_coord / angle table, an a_bin table without n_abins or n_abins without a table, a bin index outside its range, a
 * coordinate that is not finite.
 * (Tag and typedef are declared apart because the struct holds pointers, as CdHlfDesc.) */
struct CdShowerStatsDesc {
  uint32_t struct_size;   /* = sizeof(CdShowerStatsDesc) */
  int32_t n_layers;
  int32_t n_cells;        /* cells per layer */
  int32_t n_rbins;
  int32_t n_abins;        /* 0 with a null a_bin */
  const int32_t* r_bin;   /* [n_layers * n_cells] */
  const int32_t* a_bin;   /* [n_layers * n_cells], nullable */
  const double* r_coord;  /* [n_layers * n_cells] */
  const double* angle;    /* [n_layers * n_cells] */
};
typedef struct CdShowerStatsDesc CdShowerStatsDesc;
typedef struct CdShowerStats CdShowerStats;
int cd_shower_stats_create(const CdShowerStatsDesc* desc, CdShowerStats** out, void* stream);
int cd_shower_stats_destroy(CdShowerStats* stats);
/* showers (batch, n_layers * n_cells) fp32 on the device.  Per shower and layer, with e the cell energies of the layer:
 *   records (batch, n_layers, 6) fp64 = {sum e, max e, sum e r, sum e r^2, sum e cos(angle), sum e sin(angle)}
 *   counts  (batch, n_layers, 2) int32 = {cells > hit_threshold, cells > sparsity_eps}    (fp32 against fp32, as NumPy
 *                                        compares a float32 array with a Python float)
 * and per shower, over all layers, r_profile (batch, n_rbins) and a_profile (batch, n_abins) fp64 = sum e of the cells of each
 * bin; either may be NULL and is then not computed (a_profile must be NULL for a geometry without a_bin).
 * Every shower element is read from memory once: a wave stages a layer of its showers in LDS while it takes the moment sums
 * (lane j the cells j, j + 64, ... in ascending order, combined by a fixed tree), then the lane that owns a bin adds the bin's
 * cells from LDS in ascending cell order, layer after layer.  Every sum is fp64, there are no atomics and no workspace, so the
 * outputs of a shower are the same bits in any batch, at any position and in any call.  The grid is capped: any batch an int
 * holds.  Nothing is allocated and the stream is not synchronised. */
int cd_shower_stats_compute(const CdShowerStats* stats, const float* showers, int batch, float hit_threshold, float sparsity_eps,
                            double* records, int32_t* counts, double* r_profile, double* a_profile, void* stream);
/* utils.apply_mask_conserveE of the reference (calodiffusion/utils/utils.py:1021-1032), the --EMin cut of plot.py:99-101 and
 * inference.py:293-295, in place on x (rows, row_len) fp32 on the device, a row being the LAST axis of the reference's array.
 * Per row: negatives are clamped to 0; a cell is dropped where mask (rows, row_len) uint8 is non-zero, or with a NULL mask where
 * the value before the clamp is < emin; T = the sum of the clamped row and K = the sum of its kept cells, both fp64; dropped
 * cells become 0 and kept cells are multiplied by (T + 1e-10) / (K + 1e-10) rounded once to fp32.  K is summed directly where
 * the reference forms T - lost in fp32, so a row with nothing kept is exactly zero.  emin is ignored with a mask.  16 lanes
 * take a row; row_len in [1, 4096].  Nothing is allocated and the stream is not synchronised. */
int cd_threshold_conserve(float* x, const uint8_t* mask, int64_t rows, int row_len, float emin, void* stream);

/* ---- Frechet physics distance: bootstrap moments of the feature matrix ----------------------------------------------
 * What the reference's FDP hands to jetnet.evaluation.fpd (train/evaluate.py:66-79) is a feature matrix per shower set; the
 * distance bootstraps the mean and covariance of row samples drawn with replacement.  cd_fpd_moments computes them for `sets`
 * index lists in one call.  All arrays but `counts` are on the device.
 *   x (rows, d) float64, row-major;  centre [d];  idx [sets * idx_stride] int32, set s holding its counts[s] row indices at
 *   idx[s * idx_stride + k], k < counts[s] (duplicates are normal; entries at k >= counts[s] are never read);  counts [sets]: HOST.
 * With n = counts[s], y_k = x[idx_k] - centre, S_i = sum_k y_ki and G_ij = sum_k y_ki y_kj:
 *   mean [s][i] = centre_i + S_i / n,    cov [s][i][j] = (G_ij - S_i S_j / n) / (n - 1)     (np.cov(rowvar=False) of the rows)
 * mean (sets, d) and cov (sets, d, d) float64; both triangles of cov are written, from the same registers (bitwise symmetric).
 * G runs on the fp64 matrix instruction (v_mfma_f64_16x16x4_f64) over the 16-column tiles i <= j of d + 1 columns padded to a
 * multiple of 16: column d is the constant 1, which yields S from the same products.  Rows are split into slices of
 * CD_FPD_SLICE_ROWS consecutive list positions, a workgroup each; the slices' partial Grams are summed in ascending order by a
 * second launch -- no floating-point atomics: a set's result is a function of (x, its index list, d, centre) alone, the same
 * bits alone or among other sets, at any `sets` and idx_stride.
 * Every index is checked before it is used as an address: one outside [0, rows) is never dereferenced, its set's mean and
 * cov are NaN, and *status (device int32, zeroed by the call) receives 1 + s * idx_stride + k by atomicMax -- of the one
 * offender, or of the last of several (cd_preprocess reports its rows the same way).
 * Limits: 1 <= d <= CD_FPD_MAX_D, counts[s] >= 2, sets >= 1, sets * idx_stride < 2^31 - 1.  Refused with CD_EINVAL before
 * anything touches the device: a violation of these, a null pointer, rows <= 0, idx_stride < max(counts), a workspace
 * shorter than cd_fpd_workspace_bytes(d, sets, max(counts)).  Nothing is allocated and the stream is not synchronised. */
#define CD_FPD_MAX_D 256
#define CD_FPD_SLICE_ROWS 2048
/* bytes of workspace for `sets` lists of at most max_count rows (train/evaluate.py:66-79):
 * sets * ceil(max_count / CD_FPD_SLICE_ROWS) * (T (T + 1) / 2 * 2048 + 256), T = ceil((d + 1) / 16); 0 (and cd_last_error)
 * for arguments outside the limits. */
size_t cd_fpd_workspace_bytes(int d, int sets, int max_count);
/* the bootstrap moments jetnet.evaluation.fpd takes per batch (train/evaluate.py:66-79); see above */
int cd_fpd_moments(const double* x, int64_t rows, int d, const double* centre, const int32_t* idx, int64_t idx_stride,
                   const int32_t* counts /* host */, int sets, double* mean, double* cov, int32_t* status, void* workspace,
                   size_t workspace_bytes, void* stream);

/* ---- Kernel physics distance and separation powers: the other two figures over the same feature matrix ----------------
 * The reference's metrics program (calodiffusion/tests/hgcal_metrics.py:401-432) scores one feature matrix three ways: the
 * Frechet distance above, jetnet.evaluation.kpd (:424) and a separation power per feature column (:407-415, make_hist ->
 * utils._separation_power, utils/utils.py:167-175).
 *
 * cd_kpd_sums: a batch of the kernel physics distance is an MMD estimate with the polynomial kernel
 * k(a, b) = (gamma a.b + 1)^degree over m real and n generated rows drawn with replacement.  Sets pair up: set 2 k lists the
 * real rows X and set 2 k + 1 the generated rows Y of batch k, both as rows of the one matrix x (layout of x, idx and counts
 * as for cd_fpd_moments; counts[2 k] = m and counts[2 k + 1] = n may differ).  sums (sets / 2, 3) float64 receives
 *   sums[k] = { sum_{i != j} k(X_i, X_j),   sum_{i != j} k(Y_i, Y_j),   sum_{i, j} k(X_i, Y_j) },
 * i and j being list POSITIONS: two positions that drew the same row are an ordinary pair and are counted.  The division by
 * m (m - 1), n (n - 1) and m n and the subtraction are the caller's.  The kernel matrices are never formed: a workgroup owns
 * one 64 x 64 block (CD_KPD_BLOCK) of the upper triangle of the Gram matrix of the m + n gathered rows, on
 * v_mfma_f64_16x16x4_f64 over d padded with zeros to a multiple of 4, raises gamma g + 1 to `degree` by repeated
 * multiplication, weighs each element by its region and leaves one partial triple; a second launch adds a batch's partials
 * in a fixed order that depends on (m, n) alone -- no floating-point atomics: a batch's sums are a function of (x, its two
 * lists, d, gamma, degree) alone, the same bits alone or among other batches, at any `sets` and idx_stride.
 * Indices are guarded as in cd_fpd_moments: one outside [0, rows) is never dereferenced, its batch's three sums are NaN and
 * *status (device int32, zeroed by the call) receives 1 + s * idx_stride + k by atomicMax.  Entries at k >= counts[s] are
 * never read.
 * Limits: 1 <= d <= CD_FPD_MAX_D, sets even and >= 2, 2 <= counts[s] <= CD_KPD_MAX_COUNT, 1 <= degree <= 8,
 * sets * idx_stride < 2^31 - 1.  Refused with CD_EINVAL before anything touches the device: a violation of these, a null
 * pointer, rows <= 0, idx_stride < max(counts), a workspace shorter than cd_kpd_workspace_bytes(sets, max(counts)).  Nothing
 * is allocated and the stream is not synchronised. */
#define CD_KPD_BLOCK 64
#define CD_KPD_MAX_COUNT 1048576
/* bytes of workspace for `sets` lists of at most max_count rows (hgcal_metrics.py:424): sets / 2 * nb (nb + 1) / 2 * 32,
 * nb = ceil(2 max_count / CD_KPD_BLOCK); 0 (and cd_last_error) for arguments outside the limits. */
size_t cd_kpd_workspace_bytes(int sets, int max_count);
/* the three kernel sums jetnet.evaluation.kpd takes per batch (hgcal_metrics.py:424); see above */
int cd_kpd_sums(const double* x, int64_t rows, int d, const int32_t* idx, int64_t idx_stride, const int32_t* counts /* host */,
                int sets, double gamma, int degree, double* sums, int32_t* status, void* workspace, size_t workspace_bytes,
                void* stream);
/* cd_column_histograms: np.histogram(x[row_begin : row_begin + row_count, j], bins=edges[j]) for every column j of the
 * row-major float64 matrix x (., d) in one pass, as the reference's make_hist takes them (hgcal_metrics.py:409; the arithmetic
 * on the counts, utils/utils.py:167-175, is the caller's).  edges (d, nedges) float64, ascending per column; counts
 * (d, nedges - 1) uint32.  Bin k of column j is [edges[j][k], edges[j][k + 1]), the last one closed on the right; values
 * outside [edges[j][0], edges[j][nedges - 1]] and NaN are dropped.  The bin is found arithmetically and then corrected
 * against the edges as given, so the counts are exactly those of np.histogram's binary search whatever rounding the edges
 * carry.  A workgroup counts CD_HIST_CHUNK_ROWS rows of 64 columns, whose edges it holds in LDS, into tables in LDS, every
 * thread alone writing its own row of them (no atomics); a second launch adds the workgroups' tables in ascending order.  The
 * caller guarantees that x holds row_begin + row_count rows.
 * Limits: 1 <= d <= CD_FPD_MAX_D, 2 <= nedges <= CD_HIST_MAX_EDGES (edges and tables of 64 columns fill 64 KB of LDS), row_begin >= 0,
 * 1 <= row_count < 2^32; violations, null pointers and a short workspace are CD_EINVAL before anything touches the device.
 * Nothing is allocated and the stream is not synchronised. */
#define CD_HIST_CHUNK_ROWS 256
#define CD_HIST_MAX_EDGES 64
/* ceil(row_count / CD_HIST_CHUNK_ROWS) * d * (nedges - 1) * 4 bytes (hgcal_metrics.py:409); 0 (and cd_last_error) outside the limits */
size_t cd_column_histograms_workspace_bytes(int64_t row_count, int d, int nedges);
/* the per-column counts behind the reference's separation powers (hgcal_metrics.py:407-415, utils/utils.py:167-175); see above */
int cd_column_histograms(const double* x, int64_t row_begin, int64_t row_count, int d, const double* edges, int nedges,
                         uint32_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* ---- classifier two-sample test: the reference's DNN, trained and scored on the device --------------------------------
 * The third figure of the reference's metrics program (calodiffusion/tests/hgcal_metrics.py:434-490): a DNN (:185-209) learns to
 * tell generated from Geant4 rows of the feature matrix, and its accuracy, AUC and JSD on held-out rows are the result.  The
 * network is (num_layer + 1) x [Linear -> LeakyReLU(negative_slope) -> Dropout(dropout_p)] -> Linear(hidden, 1).
 *
 * `weights`: a HOST array of 4 + 2 num_layer DEVICE pointers to fp32 tensors of nn.Linear shape, in the order of the module's
 * parameters: inputlayer.weight (hidden, input_dim), inputlayer.bias, outputlayer.weight (1, hidden), outputlayer.bias, then
 * weight (hidden, hidden) and bias of every hidden Linear.  `grads`, `exp_avg` and `exp_avg_sq` are flat fp32 device buffers
 * of cd_classifier_num_params elements holding the tensors in that order.
 *
 * Arithmetic: parameters and activations are fp32; every matrix product runs on v_mfma_f32_32x32x16_bf16 as the exact
 * three-term bf16 split of the operands (24 bits, fp32 range: features may come in any units) with fp32 accumulation.  The
 * weight gradient sums over the batch (<= CD_CLS_MAX_BATCH) inside one accumulator: no split-K, no floating-point atomics, and
 * every other reduction has a fixed order -- a step is bitwise reproducible.
 * Dropout: the decision of element (row-in-batch r, column c) of layer l at step s is word r & 3 of Philox4x32-10 at counter
 * {c, r >> 2, l, lo32(s)} under key {lo32(seed), hi32(seed) ^ hi32(s)}: dropped where the word is < floor(p 2^32), else scaled
 * by 1 / (1 - p).  It depends on the row's place in the batch, not on which matrix row sits there, and is recomputed by the
 * backward pass; this stream is this library's own, not torch's.
 * A row index outside [0, rows_total) is never dereferenced: its row is staged as NaN, so its logit (and a step's loss) is NaN.
 * Limits: 1 <= input_dim, hidden <= CD_CLS_MAX_DIM, 0 <= num_layer <= CD_CLS_MAX_LAYERS, negative_slope >= 0 (the backward pass
 * reads the activation's derivative off its output), 0 <= dropout_p < 1, 1 <= max_rows_per_call <= CD_CLS_MAX_ROWS_PER_CALL.
 * Violations, null pointers and a short or misaligned (256 bytes) workspace are CD_EINVAL before anything touches the device.
 * No entry point allocates or synchronises the stream. */
#define CD_CLS_MAX_DIM 4096
#define CD_CLS_MAX_LAYERS 8
#define CD_CLS_MAX_BATCH 256
#define CD_CLS_MAX_ROWS_PER_CALL 65536
typedef struct CdClassifierDesc {
  uint32_t struct_size;  /* = sizeof(CdClassifierDesc) */
  int32_t input_dim;
  int32_t hidden;
  int32_t num_layer;     /* hidden Linear layers after the input layer (hgcal_metrics.py:198-201) */
  float negative_slope;  /* torch.nn.LeakyReLU(): 0.01 */
  float dropout_p;
} CdClassifierDesc;
/* elements of the flat gradient / Adam buffers: the parameters of DNN (hgcal_metrics.py:185-204) */
int cd_classifier_num_params(const CdClassifierDesc* desc, int64_t* numel);
/* bytes of workspace for calls that take at most max_rows_per_call rows at a time (a training batch counts as its rows):
 * the gathered rows, num_layer + 3 activation-sized buffers and three row vectors (hgcal_metrics.py:68-84, 105-123) */
int cd_classifier_workspace_bytes(const CdClassifierDesc* desc, int max_rows_per_call, size_t* bytes);
/* model.eval() forward (hgcal_metrics.py:107-115): logits[i] for row idx[i] of x (rows_total, input_dim), or row i where idx is
 * NULL; `count` rows, any number, taken max_rows_per_call at a time (the size the workspace was asked for).  idx: device int32,
 * repeats allowed. */
int cd_classifier_forward(const CdClassifierDesc* desc, const float* const* weights, const float* x, int64_t rows_total,
                          const int32_t* idx /* nullable */, int64_t count, float* logits, int max_rows_per_call, void* workspace,
                          size_t workspace_bytes, void* stream);
/* One training step (hgcal_metrics.py:77-84): forward in train mode over the rows batch_idx[0 .. batch) of x with labels
 * labels[batch_idx[.]] (fp32, rows_total of them), dropout keyed by (seed, step); the stable BCE with logits
 * max(z, 0) - z y + log1p(exp(-|z|)), mean over the batch, into *loss (device fp64); dL/dz = (sigmoid(z) - y) / batch; the
 * gradient of every parameter into `grads`.  apply_adam != 0: then torch.optim.Adam's update (cd_adam_step, no weight decay)
 * with step number adam_step >= 1; exp_avg / exp_avg_sq may be NULL otherwise.  1 <= batch <= CD_CLS_MAX_BATCH. */
int cd_classifier_train_step(const CdClassifierDesc* desc, float* const* weights, const float* x, const float* labels, int64_t rows_total,
                             const int32_t* batch_idx, int batch, uint64_t seed, uint64_t step, float* grads, double* loss, int apply_adam,
                             float* exp_avg /* nullable */, float* exp_avg_sq /* nullable */, double lr, double beta1, double beta2, float eps,
                             int adam_step, void* workspace, size_t workspace_bytes, void* stream);
/* One epoch (train_cls, hgcal_metrics.py:68-84): perm (device int32, n_train row indices into x) is cut into batches of
 * batch_size, the last one ragged; batch k is a training step with dropout step first_step + k and Adam step number
 * first_step + k + 1, its loss in losses[k] (device fp64, ceil(n_train / batch_size) of them).  All steps are enqueued on
 * `stream`: no host synchronisation, no graph capture. */
int cd_classifier_train_epoch(const CdClassifierDesc* desc, float* const* weights, const float* x, const float* labels, int64_t rows_total,
                              const int32_t* perm, int64_t n_train, int batch_size, uint64_t seed, uint64_t first_step, float* grads,
                              float* exp_avg, float* exp_avg_sq, double lr, double beta1, double beta2, float eps, double* losses,
                              void* workspace, size_t workspace_bytes, void* stream);
/* The dropout mask of (seed, step, layer) as bytes (rows, n), 1 = kept: what torch.nn.Dropout (hgcal_metrics.py:197-201) draws
 * from its own stream, from this library's; the device function the training kernels call. */
int cd_classifier_dropout_mask(uint64_t seed, uint64_t step, int layer, float dropout_p, int rows, int n, uint8_t* mask, void* stream);

/* Arithmetic of the matrix-core kernels, process-wide: "f16x2" (default; fp32 operands as two-term fp16 splits, 3 MFMAs per
 * block, fp16 RANGE -- the 3x3x3 / strided / transposed convolutions and the fused attention's projections and products),
 * "bf16x3" (convolutions on an exact three-term bf16 split, 6 MFMAs; attention unfused on the f32-input MFMA: full fp32 range)
 * or "f32" (everything on the f32-input MFMA).  Initial value: environment variable CD_CONV_PRECISION.  Cached step graphs are
 * dropped by the next sampler call. */
int cd_set_conv_precision(const char* mode);
const char* cd_get_conv_precision(void);

/* ---- measurement ---------------------------------------------------------------------------------------------- */
/* Per-launch timing with HIP events on the launch stream (eager mode; graphs are bypassed while active).
 * cd_profile_end synchronises the device and writes a JSON object
 *   {"<kernel category>": {"launches": n, "ms": total_ms, "flops": algorithmic_per_launch, "bytes": algorithmic_per_launch,
 *                          "flops_total": sum over the launches, "bytes_total": sum over the launches}}
 * (per-launch figures are those of the category's last launch; the totals serve categories that mix shapes). */
int cd_profile_begin(void);
int cd_profile_end(char* json, int cap);

/* ---- primitives (parity tests of the individual kernels; activations CHANNELS-LAST (B, D, H, W, C)) ---- */
int cd_op_to_channels_last(const float* ncdhw, float* ndhwc, int batch, int channels, int64_t voxels, void* stream);
int cd_op_to_ncdhw(const float* ndhwc, float* ncdhw, int batch, int channels, int64_t voxels, void* stream);
/* out = data + sigma[b] * noise over `batch` rows of `per` floats: the launch with which cd_train_step, cd_train_step_target and
 * cd_loss_hybrid form the network's input, for a caller that needs those bits outside them (distill.py: the teacher's input). */
int cd_op_axpy_sigma(const float* data, const float* noise, const float* sigma, float* out, int batch, int64_t per, void* stream);
/* phi-periodic Conv3d (CylindricalConv, models.py:65-96; Downsample, :360-365). w: torch layout (Cout,Cin,kD,kH,kW).
 * kernel (kD,kH,kW) in {(3,3,3),(3,4,4),(1,1,1)}; padding 1 (z,r zero; phi circular) unless 1x1x1.
 * x0/x1: two channel-concatenated sources (c1 may be 0).  scratch: >= cd_op_scratch_bytes(). */
int cd_op_cyl_conv(const float* x0, int c0, const float* x1, int c1, const float* w, const float* bias, float* y,
                   int batch, int cout, const int32_t dims_in[3], const int32_t kernel[3], const int32_t stride[3],
                   void* scratch, void* stream);
/* The same 3x3x3 stride-1 conv, single source, through the z-slide f16x2 kernel only (an error where the grid is not eligible), every
 * sample dealt in `chunks` chunks of voxels (0: the launcher's own count).  Also returns the kernel's channel statistics of y as
 * partial sums: ch_part [batch][*units][cout][2] = {sum, sum of squares}, packed; capacity batch * ceil(voxels / 32) * cout * 2 floats. */
int cd_op_zslide_conv(const float* x, int cin, const float* w, const float* bias, float* y, float* ch_part, int* units, int batch,
                      int cout, const int32_t dims[3], int chunks, void* scratch, void* stream);
/* CylindricalConvTrans as built by Upsample (models.py:25-62, 335-348). w: (Cin,Cout,kD,4,4); padding (1, circ, 1). */
int cd_op_cyl_conv_transpose(const float* x, const float* w, const float* bias, float* y, int batch, int channels,
                             const int32_t dims_in[3], int kernel_z, int stride_z, const int32_t out_pad[3],
                             void* scratch, void* stream);
/* small-Cin planar 3x3x3 conv (init_conv, models.py:562-564): x NCDHW (B,cin,D,H,W) -> y channels-last (B,D,H,W,cout). */
int cd_op_init_conv(const float* x_ncdhw, const float* w, const float* bias, float* y, int batch, int cin, int cout,
                    const int32_t dims[3], void* scratch, void* stream);
/* The denoiser's init conv followed by the 32 -> 32 3x3x3 conv that reads it (downs[0] block 1, conv 1), as ONE launch: a
 * one-channel 5x5x5 conv of scale_b[b] * x with weights composed per boundary class, plus a table that carries the coordinate
 * channels and both biases.  x: (B, D, H, W), the data channel; w0 (32, cin, 3,3,3) / b0 and w1 (32, 32, 3,3,3) / b1: the two
 * convs; channels 1.. of w0 read the coordinate images built from r_w[W], z_d[D], phi_h[H] (use_rz: R and Z, use_phi: phi;
 * cin = 1 + 2 use_rz + use_phi).  The composed data is built in `scratch` by the call.  y: (B, D, H, W, 32); ch_part as
 * cd_op_zslide_conv's, one unit per workgroup, capacity batch * D * 64 floats; slabs: workgroups per sample (0: the launcher's
 * own count).  An error where the grid is not eligible (an axis of z or r with a single voxel, or a plane too large for LDS). */
int cd_op_init_pair_conv(const float* x, const float* w0, const float* b0, const float* w1, const float* b1, int cin, const float* r_w,
                         const float* z_d, const float* phi_h, int use_rz, int use_phi, const float* scale_b, float* y, float* ch_part,
                         int* units, int batch, const int32_t dims[3], int slabs, void* scratch, void* stream);
/* GroupNorm (+SiLU) (+ per-(b,c) additive embedding) (+ residual), Block.forward / PreNorm (models.py:160-169,321-329). */
int cd_op_group_norm(const float* x, float* y, const float* gamma, const float* beta, int batch, int channels,
                     int64_t voxels, int groups, int silu, const float* add_bc, const float* residual,
                     void* scratch, void* stream);
/* ResnetBlock.forward (models.py:172-200) on channels-last input(s) x0 (+ x1 concatenated).  w: 12 device pointers in
 * torch layout: block1.proj.conv.{weight,bias}, block1.norm.{weight,bias}, block2.proj.conv.{weight,bias},
 * block2.norm.{weight,bias}, mlp.1.{weight,bias} (NULL without conditioning), res_conv.conv.{weight,bias} (NULL if
 * cin == cout).  cond: (B, 128) or NULL. */
int cd_op_resnet_block(const float* x0, int c0, const float* x1, int c1, const float* const* w, const float* cond, float* y,
                       int batch, int cout, const int32_t dims[3], int groups, void* workspace, size_t workspace_bytes,
                       void* stream);
/* Residual(PreNorm(LinearAttention)) (models.py:111-117, 281-329).  w: 7 device pointers: fn.norm.{weight,bias},
 * fn.fn.to_qkv.conv.weight, fn.fn.to_out.0.conv.{weight,bias}, fn.fn.to_out.1.{weight,bias}. */
int cd_op_linear_attention(const float* x, const float* const* w, float* y, int batch, int channels, const int32_t dims[3],
                           void* workspace, size_t workspace_bytes, void* stream);
/* ---- backward primitives (training path; parity-tested against torch autograd on the oracle) ------------------------- */
/* Gradients of y = cyl_conv(cat(x0, x1), w) + b given dy: dx (B, vox_in, c0+c1) or NULL, dw (torch layout), db or NULL.
 * Same geometry rules as cd_op_cyl_conv (models.py:65-96, 360-365). */
int cd_op_conv_backward(const float* x0, int c0, const float* x1, int c1, const float* w, const float* dy, float* dx, float* dw,
                        float* db, int batch, int cout, const int32_t dims_in[3], const int32_t kernel[3],
                        const int32_t stride[3], void* workspace, size_t workspace_bytes, void* stream);
/* Gradients of the Upsample transposed conv (models.py:25-62, 335-348): dx, dw (cin, cout, kz, 4, 4), db. */
int cd_op_conv_transpose_backward(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int batch,
                                  int channels, const int32_t dims_in[3], int kernel_z, int stride_z, const int32_t out_pad[3],
                                  void* workspace, size_t workspace_bytes, void* stream);
/* Gradients of y = act(GroupNorm(x)) + add: dx, dgamma, dbeta, dadd (B, C) or NULL. */
int cd_op_group_norm_backward(const float* x, const float* gamma, const float* beta, const float* dy, float* dx, float* dgamma,
                              float* dbeta, float* dadd, int batch, int channels, int64_t voxels, int groups, int silu,
                              void* workspace, size_t workspace_bytes, void* stream);
size_t cd_op_scratch_bytes(int batch, int max_channels, int64_t max_voxels);
/* The classifier's layer kernels on their own -- the launches cd_classifier_train_step makes (hgcal_metrics.py:194-201).
 * y (rows, n_out) = dropout(act(x (rows, n_in) . w (n_out, n_in)^T + bias)): act != 0: LeakyReLU(negative_slope); dropout_p > 0:
 * the mask of (seed, step, layer), kept values scaled by 1 / (1 - dropout_p).  bias nullable.  rows <= CD_CLS_MAX_ROWS_PER_CALL. */
int cd_op_linear_act(const float* x, const float* w, const float* bias /* nullable */, float* y, int rows, int n_in, int n_out, int act,
                     float negative_slope, float dropout_p, uint64_t seed, uint64_t step, int layer, void* stream);
/* Its gradients for an arbitrary dy (rows, n_out): g = dy * mask * keep_scale * act'(y), y being the forward output;
 * dx (rows, n_in) = g . w (nullable), dw (n_out, n_in) = g^T . x, db = the column sums of g.  mask: bytes (rows, n_out), 1 = kept,
 * or NULL (no dropout; keep_scale is ignored).  rows <= CD_CLS_MAX_BATCH; workspace: rows * n_out * 4 bytes, 16-byte aligned. */
int cd_op_linear_act_backward(const float* x, const float* w, const float* y, const float* dy, const uint8_t* mask /* nullable */,
                              float keep_scale, int act, float negative_slope, float* dx /* nullable */, float* dw, float* db, int rows,
                              int n_in, int n_out, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CALODIFF_H */
