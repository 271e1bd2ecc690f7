// Dataset-2/3 showers between physical and normalised space: cd_reverse_norm, cd_reverse_norm_staged and cd_preprocess.
#include "energy_map.h"
#include "guarded.h"

namespace cd {

// ------------------------------------------------------------------------------------------------------------
// Inverse pre-processing of generated showers (ReverseNormCaloChall, calodiffusion/utils/utils.py:446-573, for the regular
// grids: dataset_num 2 / 3, showerMap 'layer-logit-norm' / 'logit-norm'): un-normalise, inverse logit, (layer mode) clamp
// negatives and rescale every calorimeter layer to the layer energy given by the conditioning vector, scale to the incident
// energy, apply the read-out threshold.  One workgroup per (sample, layer z): the layer sum is a workgroup reduction.
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float rev_logit(float x, float alpha) {  // utils.py:233-237 (alpha 1e-6); HGCal_utils.py:13-17 (alpha 1e-8): always the caller's
  const float ex = expf(x);
  const float o = ex / (1.f + ex);
  return (o - alpha) / (1.f - 2.f * alpha);
}

struct ReverseNormArgs {
  const float* voxels;  // (B, 1, D, H, W) normalised-space showers
  const float* energy;  // (B) incident energies (physical units)
  const float* layerE;  // (B, 1 + D) normalised {total, layers} or null
  float* out;           // (B, D*H*W)
  int batch, D, H, W, layer_mode;
  float logit_mean, logit_std, totalE_mean, totalE_std, layers_mean, layers_std, max_deposit, ecut;
  // 0: everything (CaloChallenge regular grids); 1: un-normalise + inverse logit only; 2: layer renormalisation + scaling of
  // already-decoded showers (the two halves of ReverseNormHGCal around its geometry decode, utils/HGCal_utils.py:167-292)
  int stage = 0;
  float alpha = 1e-6f;      // reverse_logit's alpha (utils.py:233: 1e-6; HGCal_utils.py:13: 1e-8)
  float layer_eps = 1e-6f;  // "essentially zero" layer (utils.py:539-547: 1e-6; HGCal_utils.py:262-268: 1e-8)
};

__global__ void __launch_bounds__(256) reverse_norm_kernel(ReverseNormArgs a) {
  __shared__ float red[256];
  __shared__ float s_layer;
  const int b = blockIdx.y, z = blockIdx.x, tid = threadIdx.x;
  const int PV = a.H * a.W;
  float layer_e = 0.f;
  if (a.layer_mode) {
    // this sample's layer energies: reverse transform, normalise to the total deposited energy (utils.py:519-528)
    const float* le = a.layerE + (size_t)b * (a.D + 1);
    float part = 0.f;
    for (int i = tid; i < a.D; i += 256) part += rev_logit(le[1 + i] * a.layers_std + a.layers_mean, a.alpha);
    red[tid] = part;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    if (tid == 0) {
      const float total = le[0] * a.totalE_std + a.totalE_mean;
      s_layer = rev_logit(le[1 + z] * a.layers_std + a.layers_mean, a.alpha) / red[0] * total;
    }
    __syncthreads();
    layer_e = s_layer;
    __syncthreads();
  }
  const float* v = a.voxels + ((size_t)b * a.D + z) * PV;
  float* out = a.out + ((size_t)b * a.D + z) * PV;
  if (a.stage == 1) {  // un-normalise + inverse logit only: what the HGCal / Dataset-1 variants do BEFORE their geometry decode
    for (int i = tid; i < PV; i += 256) out[i] = rev_logit(v[i] * a.logit_std + a.logit_mean, a.alpha);
    return;
  }
  float part = 0.f;
  for (int i = tid; i < PV; i += 256) {
    // stage 2: the input is already in deposited-energy-fraction space (the decoded showers)
    float d = a.stage == 2 ? v[i] : rev_logit(v[i] * a.logit_std + a.logit_mean, a.alpha);
    if (a.layer_mode) d = d < 0.f ? 0.f : d;
    out[i] = d;
    part += d;
  }
  float fac = 1.f;
  if (a.layer_mode) {
    red[tid] = part;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    const float prev = red[0];
    fac = layer_e / (prev + 1e-10f);
    if (layer_e < a.layer_eps || prev < a.layer_eps) fac = 1.f;
  }
  const float en = a.energy[b];
  for (int i = tid; i < PV; i += 256) {
    float d = out[i] * fac * a.max_deposit * en;
    if (a.ecut > 0.f && d < a.ecut) d = 0.f;
    out[i] = d;
  }
}

static void launch_reverse_norm(const ReverseNormArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(reverse_norm_kernel, dim3((unsigned)a.D, (unsigned)a.batch), dim3(256), 0, s, a);
  CD_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------------------
// Forward pre-processing of raw showers (preprocess_shower, calodiffusion/utils/utils.py:315-436, and the incident-energy map of
// DataLoaderCaloChall, :290-312, for the regular grids: dataset_num 2 / 3, showerMap 'layer-logit-norm' / 'logit-norm'): the
// inverse of reverse_norm_kernel.  One workgroup per shower, so nothing depends on the batch or on how it is sharded:
//   pass 1 (layer maps only)  q = shower / (max_deposit e) in fp32, as the reference forms it; one wave per calorimeter layer
//                             sums its q in fp64 (lane-strided, then a xor butterfly: a fixed order), the total is the sum of
//                             the layer sums in layer order; layerE from those in fp64, rounded once.  q is kept in LDS when
//                             the shower fits (Dataset-2: 25.9 KB), so the voxels are read once; otherwise pass 2 reads them again.
//   pass 2                    logit (alpha 1e-6) and normalisation of every voxel, float4 wide.
// A shower without energy (e <= 0, NaN, or no deposit at all) is where the reference's masked arrays return fill values: it
// is reported through `status` instead (its layerE row is not written).
// ------------------------------------------------------------------------------------------------------------
namespace {
constexpr int kPreThreads = 512;
constexpr size_t kPreCacheBytes = 48 * 1024;  // q of one shower in LDS up to this size
constexpr float kLogitAlpha = 1e-6f;                         // utils.py:240-243; numpy rounds the python scalars to the
constexpr float kLogitScale = (float)(1.0 - 2.0 * 1e-6);     // array's float32 before it multiplies

__device__ __forceinline__ float pre_voxel(float q, float mean, float std) {
  const float o = kLogitAlpha + kLogitScale * q;
  return (logf(o / (1.f - o)) - mean) / std;
}
}  // namespace

struct PreprocessArgs {
  const float* showers;  // (B, D*H*W) raw voxel energies
  const float* energy;   // (B) raw incident energies, same unit as the showers
  float* out;            // (B, 1, D, H, W) normalised-space showers
  float* layerE;         // (B, 1 + D) normalised {total, layers}, or null: 'logit-norm'
  float* e_out;          // (B, 1) conditioning energy
  int32_t* status;       // 0, or 1 + the highest index of a shower without energy (see cd_preprocess)
  int batch, D, H, W, layer_mode, logE;
  float logit_mean, logit_std, totalE_mean, totalE_std, layers_mean, layers_std, max_deposit, emin, emax, scale;
};

__global__ void __launch_bounds__(kPreThreads) preprocess_kernel(PreprocessArgs a, int cache_q) {
  extern __shared__ double pre_smem[];  // D layer sums (padded to 16 bytes), then q when cache_q
  const int b = blockIdx.x, tid = threadIdx.x;
  const int PV = a.H * a.W, N = a.D * PV;
  const float* v = a.showers + (size_t)b * N;
  float* out = a.out + (size_t)b * N;
  const float e = a.energy[b] * a.scale;
  const float denom = a.max_deposit * e;
  if (!(e > 0.f) || isinf(e)) {  // uniform over the workgroup
    if (tid == 0) atomicMax(a.status, b + 1);
    return;
  }
  if (tid == 0) {
    a.e_out[b] = energy_to_cond(e, a.emin, a.emax, a.logE);  // utils.py:307-310
  }
  float* q_lds = (float*)(pre_smem + ((a.D + 1) & ~1));
  if (a.layer_mode) {
    const int wave = tid >> 6, lane = tid & 63;
    for (int z = wave; z < a.D; z += kPreThreads / 64) {
      double acc = 0.0;
      for (int i = lane; i < PV; i += 64) {
        const float q = (v[z * PV + i] * a.scale) / denom;
        if (cache_q) q_lds[z * PV + i] = q;
        acc += (double)q;
      }
      for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
      if (lane == 0) pre_smem[z] = acc;
    }
    __syncthreads();
    double total = 0.0;
    for (int z = 0; z < a.D; ++z) total += pre_smem[z];  // every thread, layer order
    if (!(total > 0.0)) {
      if (tid == 0) atomicMax(a.status, b + 1);
      return;
    }
    float* le = a.layerE + (size_t)b * (a.D + 1);
    if (tid == 0) le[0] = (float)((total - (double)a.totalE_mean) / (double)a.totalE_std);
    for (int z = tid; z < a.D; z += kPreThreads) {
      const double o = (double)kLogitAlpha + (double)kLogitScale * (pre_smem[z] / total);
      le[1 + z] = (float)((log(o / (1.0 - o)) - (double)a.layers_mean) / (double)a.layers_std);
    }
  }
  int nonzero = 0;
  if ((N & 3) == 0) {
    const float4* v4 = (const float4*)v;
    const float4* q4 = (const float4*)q_lds;
    float4* o4 = (float4*)out;
    for (int i = tid; i < N / 4; i += kPreThreads) {
      float4 q;
      if (cache_q) {
        q = q4[i];
      } else {
        q = v4[i];
        q.x = (q.x * a.scale) / denom; q.y = (q.y * a.scale) / denom; q.z = (q.z * a.scale) / denom; q.w = (q.w * a.scale) / denom;
      }
      nonzero |= (q.x != 0.f) | (q.y != 0.f) | (q.z != 0.f) | (q.w != 0.f);
      float4 r;
      r.x = pre_voxel(q.x, a.logit_mean, a.logit_std); r.y = pre_voxel(q.y, a.logit_mean, a.logit_std);
      r.z = pre_voxel(q.z, a.logit_mean, a.logit_std); r.w = pre_voxel(q.w, a.logit_mean, a.logit_std);
      o4[i] = r;
    }
  } else {
    for (int i = tid; i < N; i += kPreThreads) {
      const float q = cache_q ? q_lds[i] : (v[i] * a.scale) / denom;
      nonzero |= q != 0.f;
      out[i] = pre_voxel(q, a.logit_mean, a.logit_std);
    }
  }
  // 'logit-norm' has no layer sums: a shower with no deposit at all is found here
  if (!a.layer_mode && !__syncthreads_or(nonzero) && tid == 0) atomicMax(a.status, b + 1);
}

static void launch_preprocess(const PreprocessArgs& a, hipStream_t s) {
  const size_t n_bytes = (size_t)a.D * a.H * a.W * sizeof(float);
  const int cache_q = a.layer_mode && n_bytes <= kPreCacheBytes;
  const size_t lds = (size_t)((a.D + 1) & ~1) * sizeof(double) + (cache_q ? n_bytes : 0);
  CD_HIP(hipMemsetAsync(a.status, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL(preprocess_kernel, dim3((unsigned)a.batch), dim3(kPreThreads), lds, s, a, cache_q);
  CD_HIP(hipGetLastError());
}
// the grid and the normalisation constants as every entry point below is given them
template <typename Args>
static void set_grid_consts(Args& a, const int32_t dims[3], const float consts[6]) {
  a.D = dims[0]; a.H = dims[1]; a.W = dims[2];
  a.logit_mean = consts[0]; a.logit_std = consts[1]; a.totalE_mean = consts[2]; a.totalE_std = consts[3];
  a.layers_mean = consts[4]; a.layers_std = consts[5];
}

}  // namespace cd

extern "C" {

int cd_reverse_norm(const float* voxels, const float* energy, const float* layerE, float* out, int batch, const int32_t dims[3],
                    const float consts[6], float max_deposit, float ecut, void* stream) {
  return guarded([&] {
    CD_REQUIRE(voxels && energy && out && dims && consts && batch > 0, "bad argument");
    ReverseNormArgs a;
    a.voxels = voxels; a.energy = energy; a.layerE = layerE; a.out = out; a.batch = batch; a.layer_mode = layerE ? 1 : 0;
    set_grid_consts(a, dims, consts);
    a.max_deposit = max_deposit; a.ecut = ecut;
    launch_reverse_norm(a, (hipStream_t)stream);
  });
}

int cd_reverse_norm_staged(const float* voxels, const float* energy, const float* layerE, float* out, int batch,
                           const int32_t dims[3], const float consts[6], float max_deposit, float ecut, float alpha, float layer_eps,
                           int stage, void* stream) {
  return guarded([&] {
    CD_REQUIRE(voxels && out && dims && consts && batch > 0 && stage >= 0 && stage <= 2, "bad argument");
    CD_REQUIRE(stage == 1 || energy, "cd_reverse_norm_staged: stages 0 and 2 scale by the incident energies");
    ReverseNormArgs a;
    a.voxels = voxels; a.energy = energy; a.layerE = stage == 1 ? nullptr : layerE; a.out = out; a.batch = batch;
    a.layer_mode = a.layerE ? 1 : 0;
    set_grid_consts(a, dims, consts);
    a.max_deposit = max_deposit; a.ecut = ecut; a.stage = stage; a.alpha = alpha; a.layer_eps = layer_eps;
    launch_reverse_norm(a, (hipStream_t)stream);
  });
}

int cd_preprocess(const float* showers, const float* energy, float* out, float* layerE, float* e_out, int32_t* status, int batch,
                  const int32_t dims[3], const float consts[6], float max_deposit, float emin, float emax, int logE,
                  float shower_scale, void* stream) {
  return guarded([&] {
    CD_REQUIRE(showers && energy && out && e_out && status && dims && consts && batch > 0, "bad argument");
    CD_REQUIRE(dims[0] > 0 && dims[0] <= 4096 && dims[1] > 0 && dims[2] > 0 &&
                   (int64_t)dims[0] * dims[1] * dims[2] <= ((int64_t)1 << 28),
               "cd_preprocess: dims = {layers <= 4096, phi, r}, at most 2^28 voxels per shower");
    CD_REQUIRE(max_deposit > 0.f && shower_scale > 0.f && emax > emin && (!logE || emin > 0.f),
               "cd_preprocess: max_deposit and shower_scale must be positive, emax > emin (> 0 with logE)");
    PreprocessArgs a;
    a.showers = showers; a.energy = energy; a.out = out; a.layerE = layerE; a.e_out = e_out; a.status = status; a.batch = batch;
    a.layer_mode = layerE ? 1 : 0; a.logE = logE ? 1 : 0;
    set_grid_consts(a, dims, consts);
    a.max_deposit = max_deposit; a.emin = emin; a.emax = emax; a.scale = shower_scale;
    launch_preprocess(a, (hipStream_t)stream);
  });
}

}  // extern "C"
