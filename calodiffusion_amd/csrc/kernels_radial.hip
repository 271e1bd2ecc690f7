// Dataset-1 radial maps (include/calodiff.h, "Dataset-1 radial maps"): GeomConverter / NNConverter of the reference
// (calodiffusion/utils/utils.py:576-784) as four launches -- enc, dec and the vector-Jacobian product of each -- over per-layer
// matrices that are live parameters.  Kernels and their C ABI, and the forms a plan with a flat-state embedding
// (cd_plan_set_radial) launches around its U-Net: the same row programs with the EDM preconditioning in their staging (embed-in:
// enc of c_in x) and in their epilogue (embed-out: dec, then the objective's combination and a sampler's fused update; enc's VJP:
// the direct x term).
//
// Two row programs serve the four operations, because a VJP with respect to the input is the other direction's product with the
// transposed matrix:
//   expand    flat (V) -> grid (L, A, R)   enc with W_i;  dec_vjp's dg with D_i^T
//   collapse  grid (L, A, R) -> flat (V)   dec with D_i;  enc_vjp's dx with W_i^T (and enc's division by A)
// A workgroup stages the layer table and every matrix of its direction in LDS once, k-major (the reduction index is the slow
// one), so that the lanes of a wave, which run along the output's fast index, read consecutive banks; it then walks showers
// blockIdx.x, blockIdx.x + row_blocks, ...: the shower is staged in LDS by coalesced reads and each thread forms whole output
// elements, an fmaf chain in ascending reduction index.  A result row never sees another row.
// The weight gradients ride in the same launch, in the workgroups after the row ones: a workgroup owns kRadTile consecutive
// elements of the concatenated gradient, its kRadSlices thread groups walk the showers b = slice, slice + kRadSlices, ... each in
// ascending (b, a), and a fixed tree over the slices in LDS finishes the element.  No atomics, no workspace.
//
// Dataset-0/1 pre-processing (cd_preprocess_ds1 / cd_reverse_norm_ds1; preprocess_shower and ReverseNormCaloChall of the
// reference, utils.py:315-436, 446-573) sits on the same layout.  Its grid form is the two row programs with the loader's
// arithmetic in their staging and epilogue (Ds1Args::on): expand<ENC> scales the staged shower and ends in logit-norm, collapse<DEC>
// stages reverse_logit and ends in the energy scaling and the read-out threshold.  Its flat form needs no matrices: two kernels of
// their own over the ragged segments [bound[i], bound[i+1]), a shower in LDS and a wave per layer.
#include "guarded.h"
#include "kernels_embed_head.h"
#include "kernels_geom.h"
#include "kernels_loss.h"

#include <vector>

namespace cd {
namespace {

constexpr int kRadThreads = 256;
constexpr int kRadMaxLayers = 64;     // 1 KB of layer table
constexpr int kRadMaxWeights = 8192;  // floats of one direction's matrices in LDS: 32 KB
constexpr int kRadMaxRow = 6144;      // floats of one staged shower, flat or on the grid: 24 KB
constexpr int kRadMaxRowBlocks = 1024;
constexpr int kRadTile = 32, kRadSlices = kRadThreads / kRadTile;  // weight gradient: elements per workgroup, batch slices
static_assert(kRadSlices == 8, "the tree below sums eight slices");

// The loader's arithmetic around a shower (cd_preprocess_ds1 / cd_reverse_norm_ds1)
struct Ds1Args {
  int on;                 // the row programs: 0 = the plain map
  int logE;
  const float* energy;    // (batch) forward: raw incident energies; reverse: in physical units
  float* layerE_out;      // forward, flat form: (batch, 1 + L), or null ('logit-norm')
  const float* layerE_in; // reverse, flat form: (batch, 1 + L), or null
  float* e_out;           // forward: (batch, 1)
  int32_t* status;        // forward: 0, or 1 + the highest index of a shower without energy
  float scale, max_deposit, emin, emax, ecut;
  double logit_mean, logit_std, totalE_mean, totalE_std, layers_mean, layers_std;
};

struct RadialArgs {
  const int4* lay;
  const int* vlay;
  const float* w;      // the matrices of this direction, concatenated
  const float* in;     // rows the row program reads
  float* out;          // rows it writes
  const float* other;  // weight gradient: the forward's input (`in` is then the cotangent)
  float* dw;           // weight gradient or null
  int L, A, R, V, wtotal, batch, row_blocks;
  // plan forms (null / 0: the plain maps).  scal: (batch, 4) {c_in, c_skip, c_out, sigma} of embed_kernel
  const float* scal;   // expand<ENC>: the staged row is c_in * in.  collapse: the scalars of its epilogue
  int epi;             // collapse: kEpiNone, kEpiDenoise (DEC) or kEpiDirect (enc's VJP)
  int objective;       // CD_OBJ_*
  const float* xflat;  // kEpiDenoise: the denoiser's input x (batch, V);  kEpiDirect: the caller's cotangent gy (batch, V)
  // kEpiDenoise: the sampler update of head_kernel (HeadArgs::upd_*), on the flat state
  const float* upd_stepvals;
  const float* upd_noise;
  float* upd_x_next;
  float* upd_xs;
  float* upd_x0s;
  Ds1Args pp;          // expand<ENC>: forward pre-processing around enc;  collapse<DEC>: reverse around dec
};
enum { kEpiNone = 0, kEpiDenoise = 1, kEpiDirect = 2 };

// lay_s[L] (16 bytes each), then the matrices (wtotal floats rounded up to 4) or the weight gradient's partial sums, then a row
__device__ __forceinline__ float* rad_weights(char* smem, int L) { return (float*)(smem + sizeof(int4) * (size_t)L); }
__device__ __forceinline__ float* rad_row(char* smem, int L, int wtotal) { return rad_weights(smem, L) + ((wtotal + 3) & ~3); }

__device__ __forceinline__ void rad_stage_layers(const RadialArgs& a, int4* lay_s) {
  for (int i = threadIdx.x; i < a.L; i += kRadThreads) lay_s[i] = a.lay[i];
}

// The voxel maps, written as kernels_preprocess.hip writes them (pre_voxel of preprocess_kernel, rev_logit of reverse_norm_kernel): the
// grid forms are held bitwise equal to compositions with those kernels (tests/test_gpu_ds1_preprocess.py).
constexpr float kDs1Alpha = 1e-6f;                        // utils.py:233-243; numpy rounds the python scalars to the
constexpr float kDs1LogitScale = (float)(1.0 - 2.0 * 1e-6);  // array's float32 before it multiplies
constexpr float kDs1LayerEps = 1e-6f;                     // utils.py:535

__device__ __forceinline__ float ds1_pre_voxel(float q, float mean, float std) {
  const float o = kDs1Alpha + kDs1LogitScale * q;
  return (logf(o / (1.f - o)) - mean) / std;
}
// Where expf overflows (x > 88.7: an untrained model's samples reach it) the reference's exp / (1 + exp) is inf / inf, and in
// layer mode that one NaN takes its whole layer along; here it is the logistic function's limit, 1.  Every other x: rev_logit's bits.
__device__ __forceinline__ float ds1_rev_logit(float x, float alpha) {
  const float ex = expf(x);
  const float o = isinf(ex) ? 1.f : ex / (1.f + ex);
  return (o - alpha) / (1.f - 2.f * alpha);
}
// logit of a masked array (float64, np.ma.log(o / (1 - o)).filled(0)): 0 where the argument is not positive or the log not finite
__device__ __forceinline__ double ds1_logit64(double x) {
#pragma clang fp contract(off)
  const double o = 1e-6 + (1.0 - 2.0 * 1e-6) * x;
  const double r = o / (1.0 - o);
  const double lg = log(r);
  return (r > 0.0 && isfinite(lg)) ? lg : 0.0;
}
// The incident energy of shower b in the loader's units, and its conditioning value (utils.py:290, 307-310: float32 quotient and
// float32 log10, divided by the python float log10(emax / emin)).  False: no energy, reported through status.
__device__ __forceinline__ bool ds1_energy(const Ds1Args& p, int b, float* e_scaled) {
  const float e = p.energy[b] * p.scale;
  if (!(e > 0.f) || isinf(e)) {  // uniform over the workgroup
    if (threadIdx.x == 0) atomicMax(p.status, b + 1);
    return false;
  }
  if (threadIdx.x == 0) {
    if (p.logE) p.e_out[b] = (float)((double)(float)log10((double)(e / p.emin)) / log10((double)p.emax / (double)p.emin));
    else p.e_out[b] = (e - p.emin) / (p.emax - p.emin);
  }
  *e_scaled = e;
  return true;
}

// The matrices into LDS.  TRANSPOSE: a layer's (rows, cols) row-major matrix lands column-major; otherwise a straight copy.
// ROWS_ARE_R: the source is W_i (R, rin), else D_i (rin, R).  Reads of `w` are consecutive either way.
template <bool TRANSPOSE, bool ROWS_ARE_R>
__device__ __forceinline__ void rad_stage_weights(const RadialArgs& a, const int4* lay_s, float* wt) {
  if (!TRANSPOSE) {
    for (int e = threadIdx.x; e < a.wtotal; e += kRadThreads) wt[e] = a.w[e];
    return;
  }
  for (int i = 0; i < a.L; ++i) {
    const int4 ly = lay_s[i];
    const int rows = ROWS_ARE_R ? a.R : ly.z, cols = ROWS_ARE_R ? ly.z : a.R;
    for (int e = threadIdx.x; e < rows * cols; e += kRadThreads) {
      const int r = e / cols, c = e - r * cols;
      wt[ly.w + c * rows + r] = a.w[ly.w + e];
    }
  }
}

// One element of the concatenated weight gradient per thread of a slice.  ENC: dW_i[r, j] from gy (`in`, grid rows) and x
// (`other`, flat rows); otherwise dD_i[j, r] from gx (`in`, flat rows) and g (`other`, grid rows).
template <bool ENC>
__device__ __forceinline__ void rad_weight_grad(const RadialArgs& a, const int4* lay_s, float* part, int tile) {
  const int lane = threadIdx.x & (kRadTile - 1), slice = threadIdx.x / kRadTile;
  const int e = tile * kRadTile + lane;
  float acc = 0.f;
  if (e < a.wtotal) {
    int i = 0;
    while (i + 1 < a.L && lay_s[i + 1].w <= e) ++i;
    const int4 ly = lay_s[i];
    const int local = e - ly.w;
    const int r = ENC ? local / ly.z : local % a.R, j = ENC ? local % ly.z : local / a.R;
    const int LAR = a.L * a.A * a.R;
    const float* flat = (ENC ? a.other : a.in) + ly.x + j;                  // + b V + a rin
    const float* grid = (ENC ? a.in : a.other) + (size_t)i * a.A * a.R + r;  // + b LAR + a R
    if (ly.y == a.A) {
      for (int b = slice; b < a.batch; b += kRadSlices) {
        const float* fb = flat + (size_t)b * a.V;
        const float* gb = grid + (size_t)b * LAR;
        for (int aa = 0; aa < a.A; ++aa) acc = fmaf(gb[aa * a.R], fb[aa * ly.z], acc);
      }
    } else {  // alpha 1: the grid side is summed over a first (enc: and divided by A, as the forward divides)
      for (int b = slice; b < a.batch; b += kRadSlices) {
        const float* gb = grid + (size_t)b * LAR;
        float s = 0.f;
        for (int aa = 0; aa < a.A; ++aa) s = __fadd_rn(s, gb[aa * a.R]);
        if (ENC) s = __fdiv_rn(s, (float)a.A);
        acc = fmaf(s, flat[(size_t)b * a.V], acc);
      }
    }
  }
  part[slice * kRadTile + lane] = acc;
  __syncthreads();
  if (slice == 0 && e < a.wtotal) {
    const float* p = part + lane;
    const float s01 = __fadd_rn(p[0], p[kRadTile]), s23 = __fadd_rn(p[2 * kRadTile], p[3 * kRadTile]);
    const float s45 = __fadd_rn(p[4 * kRadTile], p[5 * kRadTile]), s67 = __fadd_rn(p[6 * kRadTile], p[7 * kRadTile]);
    a.dw[e] = __fadd_rn(__fadd_rn(s01, s23), __fadd_rn(s45, s67));
  }
}

}  // namespace

// flat -> grid.  ENC: enc (W_i given as (R, rin), the alpha-1 layers divided by A); otherwise dec_vjp's dg (D_i given as (rin, R),
// which is the k-major layout already) and, in the workgroups past row_blocks, dD.
template <bool ENC>
__global__ void __launch_bounds__(kRadThreads) radial_expand_kernel(RadialArgs a) {
  extern __shared__ __attribute__((aligned(16))) char rad_smem[];
  int4* lay_s = (int4*)rad_smem;
  float* wt = rad_weights(rad_smem, a.L);  // [woff_i + j R + r]
  rad_stage_layers(a, lay_s);
  __syncthreads();
  if ((int)blockIdx.x >= a.row_blocks) {  // uniform over the workgroup
    if (!ENC) rad_weight_grad<false>(a, lay_s, wt, (int)blockIdx.x - a.row_blocks);
    return;
  }
  float* row = rad_row(rad_smem, a.L, a.wtotal);
  rad_stage_weights<ENC, true>(a, lay_s, wt);
  const int AR = a.A * a.R, LAR = a.L * AR;
  for (int b = blockIdx.x; b < a.batch; b += a.row_blocks) {
    const float* in = a.in + (size_t)b * a.V;
    float denom = 0.f;
    int nonzero = 0;
    if (ENC && a.pp.on) {  // the loader: x shower_scale first (utils.py:291), then convert (:331-333)
      float e;
      if (!ds1_energy(a.pp, b, &e)) continue;  // (before this pass's first barrier)
      denom = a.pp.max_deposit * e;
      for (int v = threadIdx.x; v < a.V; v += kRadThreads) row[v] = __fmul_rn(in[v], a.pp.scale);
    } else if (ENC && a.scal) {  // embed-in: the scaling first, then the dot product (x * scales['c_in'], then NN_embed.enc)
      const float c_in = a.scal[(size_t)b * 4];
      for (int v = threadIdx.x; v < a.V; v += kRadThreads) row[v] = __fmul_rn(in[v], c_in);
    } else {
      for (int v = threadIdx.x; v < a.V; v += kRadThreads) row[v] = in[v];
    }
    __syncthreads();  // (the first pass: the matrices too)
    float* out = a.out + (size_t)b * LAR;
    for (int o = threadIdx.x; o < LAR; o += kRadThreads) {
      const int i = o / AR, rem = o - i * AR, aa = rem / a.R, r = rem - aa * a.R;
      const int4 ly = lay_s[i];
      const bool one = ly.y != a.A;
      const float* xr = row + ly.x + (one ? 0 : aa * ly.z);
      const float* wk = wt + ly.w + r;
      float acc = 0.f;
      for (int j = 0; j < ly.z; ++j) acc = fmaf(wk[j * a.R], xr[j], acc);
      if (ENC && one) acc = __fdiv_rn(acc, (float)a.A);
      if (ENC && a.pp.on) {  // preprocess_kernel's 'logit-norm' on the grid value
        const float q = acc / denom;
        nonzero |= q != 0.f;
        acc = ds1_pre_voxel(q, (float)a.pp.logit_mean, (float)a.pp.logit_std);
      }
      out[o] = acc;
    }
    // the row is consumed before the next one is staged; a shower with no deposit at all is found here
    if (ENC && a.pp.on) {
      if (!__syncthreads_or(nonzero) && threadIdx.x == 0) atomicMax(a.pp.status, b + 1);
    } else {
      __syncthreads();
    }
  }
}

// grid -> flat.  DEC: dec (D_i given as (rin, R)); otherwise enc_vjp's dx (W_i given as (R, rin), the k-major layout already,
// the alpha-1 layers divided by A) and, in the workgroups past row_blocks, dW.
template <bool DEC>
__global__ void __launch_bounds__(kRadThreads) radial_collapse_kernel(RadialArgs a) {
  extern __shared__ __attribute__((aligned(16))) char rad_smem[];
  int4* lay_s = (int4*)rad_smem;
  float* wt = rad_weights(rad_smem, a.L);  // [woff_i + r rin + j]
  rad_stage_layers(a, lay_s);
  __syncthreads();
  if ((int)blockIdx.x >= a.row_blocks) {
    if (!DEC) rad_weight_grad<true>(a, lay_s, wt, (int)blockIdx.x - a.row_blocks);
    return;
  }
  float* row = rad_row(rad_smem, a.L, a.wtotal);
  rad_stage_weights<DEC, false>(a, lay_s, wt);
  const int AR = a.A * a.R, LAR = a.L * AR;
  for (int b = blockIdx.x; b < a.batch; b += a.row_blocks) {
    const float* in = a.in + (size_t)b * LAR;
    if (DEC && a.pp.on) {  // reverse_norm_kernel's stage 1 on the way in
      const float mean = (float)a.pp.logit_mean, std = (float)a.pp.logit_std;
      for (int o = threadIdx.x; o < LAR; o += kRadThreads) row[o] = ds1_rev_logit(in[o] * std + mean, kDs1Alpha);
    } else {
      for (int o = threadIdx.x; o < LAR; o += kRadThreads) row[o] = in[o];
    }
    __syncthreads();
    float* out = a.out + (size_t)b * a.V;
    for (int v = threadIdx.x; v < a.V; v += kRadThreads) {
      const int i = a.vlay[v];
      const int4 ly = lay_s[i];
      const bool one = ly.y != a.A;
      const int rem = v - ly.x, aa = one ? 0 : rem / ly.z, j = rem - aa * ly.z;
      const float* mk = wt + ly.w + j;
      const float* g = row + i * AR + aa * a.R;
      float res = 0.f;
      for (int s = 0; s < (one ? a.A : 1); ++s, g += a.R) {  // alpha 1: the sum over a, ascending
        float acc = 0.f;
        for (int r = 0; r < a.R; ++r) acc = fmaf(mk[r * ly.z], g[r], acc);
        res = one ? __fadd_rn(res, acc) : acc;
      }
      if (!DEC && one) res = __fdiv_rn(res, (float)a.A);
      if (a.epi == kEpiDenoise) {  // head_kernel's combination and sampler update, res in the place of the head's F
        const size_t i = (size_t)b * a.V + v;
        const float xv = a.xflat[i];
        float pred = res;
        if (a.objective == 0) pred = a.scal[b * 4 + 1] * xv + a.scal[b * 4 + 2] * pred;
        else if (a.objective == 1) pred = xv - a.scal[b * 4 + 3] * pred;
        out[v] = pred;
        if (a.upd_stepvals) {  // (DDim.__call__'s update: HeadArgs::upd_*)
          const float sigma = a.upd_stepvals[0], sprev = a.upd_stepvals[1], dsig = a.upd_stepvals[2], denom = a.upd_stepvals[3];
          const float eps = (xv - pred) / sigma;
          float r = pred + sprev * eps;
          if (a.upd_noise) r += dsig * a.upd_noise[i] / denom;
          a.upd_x_next[i] = r;
          if (a.upd_xs) a.upd_xs[i] = r;
          if (a.upd_x0s) a.upd_x0s[i] = pred;
        }
      } else if (a.epi == kEpiDirect) {  // init_dgrad_kernel's epilogue: res carries c_in already
        out[v] = a.objective == 2 ? res : fmaf(a.objective == 0 ? a.scal[b * 4 + 1] : 1.f, a.xflat[(size_t)b * a.V + v], res);
      } else if (DEC && a.pp.on) {  // reverse_norm_kernel's last loop, without a layer factor
        float d = res * a.pp.max_deposit * a.pp.energy[b];
        if (a.pp.ecut > 0.f && d < a.pp.ecut) d = 0.f;
        out[v] = d;
      } else {
        out[v] = res;
      }
    }
    __syncthreads();
  }
}

// The flat form of preprocess_shower (orig_shape: utils.py:341-342, 358-410), include/calodiff.h "cd_preprocess_ds1".  LDS: the
// layer table, L layer sums (fp64), q of one shower.
__global__ void __launch_bounds__(kRadThreads) ds1_flat_forward_kernel(RadialArgs a) {
  extern __shared__ __attribute__((aligned(16))) char rad_smem[];
  int4* lay_s = (int4*)rad_smem;
  double* lsum = (double*)(lay_s + a.L);
  float* q_s = (float*)(lsum + a.L);
  const Ds1Args& p = a.pp;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  rad_stage_layers(a, lay_s);
  __syncthreads();
  for (int b = blockIdx.x; b < a.batch; b += a.row_blocks) {
    float e;
    if (!ds1_energy(p, b, &e)) continue;  // (before this pass's first barrier)
    const float denom = p.max_deposit * e;
    const float* in = a.in + (size_t)b * a.V;
    float* out = a.out + (size_t)b * a.V;
    for (int v = tid; v < a.V; v += kRadThreads) q_s[v] = (in[v] * p.scale) / denom;
    __syncthreads();
    if (p.layerE_out) {
      for (int i = wave; i < a.L; i += kRadThreads / 64) {
        const int4 ly = lay_s[i];
        const float* seg = q_s + ly.x;
        double acc = 0.0;
        for (int k = lane; k < ly.y * ly.z; k += 64) acc += (double)seg[k];
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0) lsum[i] = acc;
      }
      __syncthreads();
      double total = 0.0;
      for (int i = 0; i < a.L; ++i) total += lsum[i];  // every thread, layer order
      if (!(total > 0.0)) {  // uniform: no deposit at all
        if (tid == 0) atomicMax(p.status, b + 1);
        __syncthreads();  // lsum is read before the next shower's sums land
        continue;
      }
      // the reference holds the sums and their quotient in float32 (:372-380, 389); from there its masked arrays are float64
      const float total32 = (float)total;
      float* le = p.layerE_out + (size_t)b * (a.L + 1);
      if (tid == 0) le[0] = (float)(((double)total32 - p.totalE_mean) / p.totalE_std);
      for (int i = tid; i < a.L; i += kRadThreads) {
        const float share = __fdiv_rn((float)lsum[i], total32);
        le[1 + i] = (float)((ds1_logit64((double)share) - p.layers_mean) / p.layers_std);
      }
      for (int v = tid; v < a.V; v += kRadThreads) out[v] = (float)((ds1_logit64((double)q_s[v]) - p.logit_mean) / p.logit_std);
      __syncthreads();
    } else {
      const float mean = (float)p.logit_mean, std = (float)p.logit_std;
      int nonzero = 0;
      for (int v = tid; v < a.V; v += kRadThreads) {
        const float q = q_s[v];
        nonzero |= q != 0.f;
        out[v] = ds1_pre_voxel(q, mean, std);
      }
      if (!__syncthreads_or(nonzero) && tid == 0) atomicMax(p.status, b + 1);
    }
  }
}

// The flat form of ReverseNormCaloChall (utils.py:494-505, 520-560, 570-571), include/calodiff.h "cd_reverse_norm_ds1", in
// reverse_norm_kernel's arithmetic.  LDS: the layer table, L layer energies, one shower.
__global__ void __launch_bounds__(kRadThreads) ds1_flat_reverse_kernel(RadialArgs a) {
  extern __shared__ __attribute__((aligned(16))) char rad_smem[];
  int4* lay_s = (int4*)rad_smem;
  float* lay_e = (float*)(lay_s + a.L);
  float* row = lay_e + a.L;
  const Ds1Args& p = a.pp;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float mean = (float)p.logit_mean, std = (float)p.logit_std;
  const float layers_mean = (float)p.layers_mean, layers_std = (float)p.layers_std;
  rad_stage_layers(a, lay_s);
  __syncthreads();
  for (int b = blockIdx.x; b < a.batch; b += a.row_blocks) {
    const float* in = a.in + (size_t)b * a.V;
    float* out = a.out + (size_t)b * a.V;
    const float en = p.energy[b];
    if (p.layerE_in && wave == 0) {
      // this shower's layer energies: reverse transform, normalise to the total deposited energy (utils.py:522-530); L <= 64
      const float* le = p.layerE_in + (size_t)b * (a.L + 1);
      const float r = lane < a.L ? ds1_rev_logit(le[1 + lane] * layers_std + layers_mean, kDs1Alpha) : 0.f;
      float sum = r;
      for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
      const float total = le[0] * (float)p.totalE_std + (float)p.totalE_mean;
      if (lane < a.L) lay_e[lane] = r / sum * total;
    }
    for (int v = tid; v < a.V; v += kRadThreads) {
      float d = ds1_rev_logit(in[v] * std + mean, kDs1Alpha);
      if (p.layerE_in) d = d < 0.f ? 0.f : d;
      row[v] = d;
    }
    __syncthreads();
    if (p.layerE_in) {
      for (int i = wave; i < a.L; i += kRadThreads / 64) {  // a wave sums its segment, then rescales it
        const int4 ly = lay_s[i];
        const int n = ly.y * ly.z;
        float prev = 0.f;
        for (int k = lane; k < n; k += 64) prev += row[ly.x + k];
        for (int o = 32; o > 0; o >>= 1) prev += __shfl_xor(prev, o);
        const float layer_e = lay_e[i];
        float fac = layer_e / (prev + 1e-10f);
        if (layer_e < kDs1LayerEps || prev < kDs1LayerEps) fac = 1.f;
        for (int k = lane; k < n; k += 64) {
          float d = row[ly.x + k] * fac * p.max_deposit * en;
          if (p.ecut > 0.f && d < p.ecut) d = 0.f;
          out[ly.x + k] = d;
        }
      }
    } else {
      for (int v = tid; v < a.V; v += kRadThreads) {
        float d = row[v] * p.max_deposit * en;
        if (p.ecut > 0.f && d < p.ecut) d = 0.f;
        out[v] = d;
      }
    }
    __syncthreads();  // the row and the layer energies are consumed before the next shower's land
  }
}

namespace {

enum RadialOp { kEnc, kDec, kEncVjp, kDecVjp };

void radial_launch(RadialOp op, const CdRadialMap* m, const float* w, const float* in, float* out, const float* other, float* dw,
                   int batch, hipStream_t s, const RadialArgs* plan_form = nullptr) {
  RadialArgs a{};
  if (plan_form) a = *plan_form;  // (scal, epi, objective, xflat, upd_*; everything else is set below)
  a.lay = m->lay; a.vlay = m->vlay; a.w = w; a.in = in; a.out = out; a.other = other; a.dw = dw;
  a.L = m->layers; a.A = m->A; a.R = m->R; a.V = m->V; a.wtotal = m->wtotal; a.batch = batch;
  a.row_blocks = batch < kRadMaxRowBlocks ? batch : kRadMaxRowBlocks;
  const int LAR = m->layers * m->A * m->R;
  const size_t table = sizeof(int4) * (size_t)m->layers;
  size_t smem = table + sizeof(float) * (size_t)(((m->wtotal + 3) & ~3) + (m->V > LAR ? m->V : LAR));
  const size_t wg = table + sizeof(float) * kRadThreads;
  if (dw && smem < wg) smem = wg;
  const dim3 grid((unsigned)(a.row_blocks + (dw ? (m->wtotal + kRadTile - 1) / kRadTile : 0)));
  switch (op) {
    case kEnc: hipLaunchKernelGGL(radial_expand_kernel<true>, grid, dim3(kRadThreads), smem, s, a); break;
    case kDec: hipLaunchKernelGGL(radial_collapse_kernel<true>, grid, dim3(kRadThreads), smem, s, a); break;
    case kEncVjp: hipLaunchKernelGGL(radial_collapse_kernel<false>, grid, dim3(kRadThreads), smem, s, a); break;
    case kDecVjp: hipLaunchKernelGGL(radial_expand_kernel<false>, grid, dim3(kRadThreads), smem, s, a); break;
  }
  CD_HIP(hipGetLastError());
}

// the flat forms: no matrices, LDS = the layer table, L sums (8 bytes cover both kernels' use) and one shower
void ds1_flat_launch(bool forward, const CdRadialMap* m, const float* in, float* out, const Ds1Args& pp, int batch, hipStream_t s) {
  RadialArgs a{};
  a.lay = m->lay; a.in = in; a.out = out; a.L = m->layers; a.A = m->A; a.R = m->R; a.V = m->V; a.batch = batch;
  a.row_blocks = batch < kRadMaxRowBlocks ? batch : kRadMaxRowBlocks;
  a.pp = pp;
  const size_t smem = (sizeof(int4) + sizeof(double)) * (size_t)m->layers + sizeof(float) * (size_t)m->V;
  if (forward) hipLaunchKernelGGL(ds1_flat_forward_kernel, dim3((unsigned)a.row_blocks), dim3(kRadThreads), smem, s, a);
  else hipLaunchKernelGGL(ds1_flat_reverse_kernel, dim3((unsigned)a.row_blocks), dim3(kRadThreads), smem, s, a);
  CD_HIP(hipGetLastError());
}

void ds1_consts(Ds1Args* p, const double consts[6]) {
  p->logit_mean = consts[0]; p->logit_std = consts[1]; p->totalE_mean = consts[2]; p->totalE_std = consts[3];
  p->layers_mean = consts[4]; p->layers_std = consts[5];
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------
// The forms of a plan with a flat-state embedding (forward.hip, train.hip)
// ------------------------------------------------------------------------------------------------------------
void radial_embed_in(const CdRadialMap* m, const float* enc_w, const float* x, const float* scal, float* g, int batch, hipStream_t s) {
  RadialArgs f{};
  f.scal = scal;
  radial_launch(kEnc, m, enc_w, x, g, nullptr, nullptr, batch, s, &f);
}

void radial_embed_out(const CdRadialMap* m, const float* dec_w, const float* F, const float* x, const float* scal, int objective,
                      float* out, const HeadArgs* upd, int batch, hipStream_t s) {
  RadialArgs f{};
  f.scal = scal; f.epi = kEpiDenoise; f.objective = objective; f.xflat = x;
  if (upd && upd->upd_stepvals) {
    CD_REQUIRE(upd->upd_x_next, "embed-out: the fused sampler update needs x_next");
    f.upd_stepvals = upd->upd_stepvals; f.upd_noise = upd->upd_noise; f.upd_x_next = upd->upd_x_next;
    f.upd_xs = upd->upd_xs; f.upd_x0s = upd->upd_x0s;
  }
  radial_launch(kDec, m, dec_w, F, out, nullptr, nullptr, batch, s, &f);
}

void radial_embed_dec_vjp(const CdRadialMap* m, const float* dec_w, const float* F, const float* gf, float* dF, float* dd, int batch,
                          hipStream_t s) {
  radial_launch(kDecVjp, m, dec_w, gf, dF, F, dd, batch, s);
}

void radial_embed_enc_vjp(const CdRadialMap* m, const float* enc_w, const float* x, const float* dg, const float* gy,
                          const float* scal, int objective, float* dx, float* dw, int batch, hipStream_t s) {
  RadialArgs f{};
  if (gy) {
    f.scal = scal; f.epi = kEpiDirect; f.objective = objective; f.xflat = gy;
  }
  radial_launch(kEncVjp, m, enc_w, dg, dx, x, dw, batch, s, &f);
}

// The cotangent of f = dec(F) on the flat state.  LOSS: head_loss_bwd_kernel's dF from the loss (x0, data, noise); otherwise
// head_vjp_kernel's dF = coef_b gy from a caller's cotangent of the denoiser output.
template <bool LOSS>
__global__ void __launch_bounds__(256) embed_cotangent_kernel(const float* __restrict__ x0, const float* __restrict__ data,
                                                              const float* __restrict__ noise, const float* __restrict__ gy,
                                                              const float* __restrict__ scal, float* __restrict__ gf, int batch,
                                                              int64_t per, int loss_type, int objective) {
  __shared__ float sNorm;
  if (LOSS) {
    if (threadIdx.x == 0) sNorm = loss_grad_norm(scal, batch, per, loss_type, objective);
    __syncthreads();
  }
  const int64_t total = (int64_t)batch * per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int b = (int)(i / per);
    const float sg = scal[b * 4 + 3];
    const float chain = objective == 0 ? scal[b * 4 + 2] : (objective == 1 ? -sg : 1.0f);
    gf[i] = LOSS ? loss_grad_dF(sNorm, x0[i], data[i], objective == 1 ? noise[i] : 0.f, sg, chain, loss_type, objective)
                 : chain * gy[i];
  }
}
void launch_embed_cotangent(const float* x0, const float* data, const float* noise, const float* gy, const float* scal, float* gf,
                            int batch, int64_t per, int loss_type, int objective, hipStream_t s) {
  int64_t blocks = ((int64_t)batch * per + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  if (gy) hipLaunchKernelGGL(embed_cotangent_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, x0, data, noise, gy, scal, gf, batch, per, loss_type, objective);
  else hipLaunchKernelGGL(embed_cotangent_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, x0, data, noise, gy, scal, gf, batch, per, loss_type, objective);
  CD_HIP(hipGetLastError());
}

}  // namespace cd

extern "C" {

int cd_radial_create(int layers, const int32_t* bound, const int32_t* alpha, const int32_t* rin, int alpha_out, int r_out,
                     CdRadialMap** out, void* stream) {
  return guarded([&] {
    CD_REQUIRE(bound && alpha && rin && out, "cd_radial_create: bound, alpha, rin and out must not be null");
    CD_REQUIRE(layers > 0 && alpha_out > 0 && r_out > 0, "cd_radial_create: layers, alpha_out and r_out must be positive");
    CD_REQUIRE(layers <= kRadMaxLayers, "cd_radial_create: at most 64 layers");
    CD_REQUIRE(bound[0] == 0, "cd_radial_create: bound[0] must be 0");
    std::vector<int4> lay((size_t)layers);
    int64_t wtotal = 0;
    for (int i = 0; i < layers; ++i)
      CD_REQUIRE(bound[i + 1] > bound[i], "cd_radial_create: bound must be strictly increasing (layer " + std::to_string(i) + ")");
    for (int i = 0; i < layers; ++i) {
      const std::string at = " (layer " + std::to_string(i) + ")";
      CD_REQUIRE(alpha[i] == 1 || alpha[i] == alpha_out,
                 "cd_radial_create: alpha must be 1 or alpha_out = " + std::to_string(alpha_out) + ", got " +
                     std::to_string(alpha[i]) + at);
      CD_REQUIRE(rin[i] > 0, "cd_radial_create: rin must be positive" + at);
      CD_REQUIRE((int64_t)bound[i + 1] - bound[i] == (int64_t)alpha[i] * rin[i],
                 "cd_radial_create: the span bound[i+1] - bound[i] must equal alpha[i] * rin[i]" + at);
      CD_REQUIRE(wtotal <= kRadMaxWeights, "cd_radial_create: the matrices of one direction exceed 8192 floats (32 KB of LDS)");
      lay[(size_t)i] = make_int4(bound[i], alpha[i], rin[i], (int)wtotal);
      wtotal += (int64_t)rin[i] * r_out;
    }
    CD_REQUIRE(wtotal <= kRadMaxWeights, "cd_radial_create: the matrices of one direction exceed 8192 floats (32 KB of LDS)");
    const int V = bound[layers];
    CD_REQUIRE(V <= kRadMaxRow && (int64_t)layers * alpha_out * r_out <= kRadMaxRow,
               "cd_radial_create: a shower exceeds 6144 floats (24 KB of LDS), flat or as layers * alpha_out * r_out");
    std::vector<int> vlay((size_t)V);
    for (int i = 0; i < layers; ++i)
      for (int v = bound[i]; v < bound[i + 1]; ++v) vlay[(size_t)v] = i;
    hipStream_t s = (hipStream_t)stream;
    struct Owner {
      CdRadialMap* m;
      ~Owner() { delete m; }
    } own{new CdRadialMap};
    CdRadialMap* m = own.m;
    m->layers = layers; m->A = alpha_out; m->R = r_out; m->V = V; m->wtotal = (int)wtotal;
    CD_HIP(hipMalloc(&m->lay, sizeof(int4) * lay.size()));
    CD_HIP(hipMalloc(&m->vlay, sizeof(int) * vlay.size()));
    CD_HIP(hipMemcpyAsync(m->lay, lay.data(), sizeof(int4) * lay.size(), hipMemcpyHostToDevice, s));
    CD_HIP(hipMemcpyAsync(m->vlay, vlay.data(), sizeof(int) * vlay.size(), hipMemcpyHostToDevice, s));
    CD_HIP(hipStreamSynchronize(s));  // the host arrays above go out of scope
    *out = m;
    own.m = nullptr;
  });
}

int cd_radial_destroy(CdRadialMap* map) {
  return guarded([&] { delete map; });
}

int cd_radial_enc(const CdRadialMap* map, const float* w, const float* x, float* y, int batch, void* stream) {
  return guarded([&] {
    CD_REQUIRE(map && w && x && y, "cd_radial_enc: map, w, x and y must not be null");
    CD_REQUIRE(batch > 0, "cd_radial_enc: batch must be positive");
    radial_launch(kEnc, map, w, x, y, nullptr, nullptr, batch, (hipStream_t)stream);
  });
}

int cd_radial_dec(const CdRadialMap* map, const float* d, const float* g, float* x, int batch, void* stream) {
  return guarded([&] {
    CD_REQUIRE(map && d && g && x, "cd_radial_dec: map, d, g and x must not be null");
    CD_REQUIRE(batch > 0, "cd_radial_dec: batch must be positive");
    radial_launch(kDec, map, d, g, x, nullptr, nullptr, batch, (hipStream_t)stream);
  });
}

int cd_radial_enc_vjp(const CdRadialMap* map, const float* w, const float* x, const float* gy, float* dx, float* dw, int batch,
                      void* stream) {
  return guarded([&] {
    CD_REQUIRE(map && w && x && gy && dx, "cd_radial_enc_vjp: map, w, x, gy and dx must not be null");
    CD_REQUIRE(batch > 0, "cd_radial_enc_vjp: batch must be positive");
    radial_launch(kEncVjp, map, w, gy, dx, x, dw, batch, (hipStream_t)stream);
  });
}

int cd_radial_dec_vjp(const CdRadialMap* map, const float* d, const float* g, const float* gx, float* dg, float* dd, int batch,
                      void* stream) {
  return guarded([&] {
    CD_REQUIRE(map && d && g && gx && dg, "cd_radial_dec_vjp: map, d, g, gx and dg must not be null");
    CD_REQUIRE(batch > 0, "cd_radial_dec_vjp: batch must be positive");
    radial_launch(kDecVjp, map, d, gx, dg, g, dd, batch, (hipStream_t)stream);
  });
}

int cd_preprocess_ds1(const CdRadialMap* map, const float* conv_w, const float* showers, const float* energy, float* out,
                      float* layerE, float* e_out, int32_t* status, int batch, const double consts[6], float max_deposit, float emin,
                      float emax, int logE, float shower_scale, void* stream) {
  return guarded([&] {
    CD_REQUIRE(map && showers && energy && out && e_out && status && consts && batch > 0, "bad argument");
    CD_REQUIRE(max_deposit > 0.f && shower_scale > 0.f && emax > emin && (!logE || emin > 0.f),
               "cd_preprocess_ds1: max_deposit and shower_scale must be positive, emax > emin (> 0 with logE)");
    CD_REQUIRE(consts[1] != 0.0 && consts[3] != 0.0 && consts[5] != 0.0, "cd_preprocess_ds1: the three std constants must not be 0");
    CD_REQUIRE(!(conv_w && layerE),
               "cd_preprocess_ds1: the grid form (conv_w) takes no layerE: the reference's own preprocess_shower fails on a "
               "'layer' map after the geometry conversion");
    hipStream_t s = (hipStream_t)stream;
    Ds1Args p{};
    p.on = 1; p.logE = logE ? 1 : 0; p.energy = energy; p.layerE_out = layerE; p.e_out = e_out; p.status = status;
    p.scale = shower_scale; p.max_deposit = max_deposit; p.emin = emin; p.emax = emax;
    ds1_consts(&p, consts);
    CD_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    if (conv_w) {
      RadialArgs f{};
      f.pp = p;
      radial_launch(kEnc, map, conv_w, showers, out, nullptr, nullptr, batch, s, &f);
    } else {
      ds1_flat_launch(true, map, showers, out, p, batch, s);
    }
  });
}

int cd_reverse_norm_ds1(const CdRadialMap* map, const float* unconv_w, const float* voxels, const float* energy, const float* layerE,
                        float* out, int batch, const double consts[6], float max_deposit, float ecut, void* stream) {
  return guarded([&] {
    CD_REQUIRE(map && voxels && energy && out && consts && batch > 0, "bad argument");
    CD_REQUIRE(max_deposit > 0.f, "cd_reverse_norm_ds1: max_deposit must be positive");
    CD_REQUIRE(!(unconv_w && layerE),
               "cd_reverse_norm_ds1: the grid form (unconv_w) takes no layerE: the reference's own preprocess_shower fails on a "
               "'layer' map after the geometry conversion, so there is nothing to invert");
    Ds1Args p{};
    p.on = 1; p.energy = energy; p.layerE_in = layerE; p.max_deposit = max_deposit; p.ecut = ecut;
    ds1_consts(&p, consts);
    if (unconv_w) {
      RadialArgs f{};
      f.pp = p;
      radial_launch(kDec, map, unconv_w, voxels, out, nullptr, nullptr, batch, (hipStream_t)stream, &f);
    } else {
      ds1_flat_launch(false, map, voxels, out, p, batch, (hipStream_t)stream);
    }
  });
}

}  // extern "C"
