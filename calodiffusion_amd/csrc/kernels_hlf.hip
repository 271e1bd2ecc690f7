// Shower observables (include/calodiff.h, "shower observables"): HighLevelFeatures.CalculateFeatures of the reference
// (calodiffusion/utils/HighLevelFeatures.py:48-89) as one launch.  The reference forms eta * e, eta * eta * e, phi * e,
// phi * phi * e and their sums as one float64 (N, V_layer) temporary each, per layer; here a shower element is read once and
// everything a layer needs -- five sums, the brightest voxel and the hit count -- is accumulated beside it.
//
// A workgroup belongs to one layer; its waves walk the showers.  A layer of one shower is summed by a group of 16 lanes (one DPP
// row; four groups to a wave), lane j of the group taking the layer's voxels j, j + 16, ... in ascending order, and a fixed tree
// over the group combines them.  The order of every sum is therefore a function of the layer alone -- not of the batch, the
// shower's place in it or the row's alignment.  Layers start at any element and rows have any length, so no load is wider than a
// dword: a group's load instruction reads 64 consecutive bytes of a row.
// What hides the HBM latency is the number of independent loads in flight, and a 144-voxel layer (Dataset 2) is 9 voxels a lane:
// a lane group therefore works on kHlfShowers showers at once -- the same voxel of each, up to four strides ahead, 16 loads in
// flight per lane -- and a position of the eta / phi tables (16 bytes per voxel against the shower's 4, from cache) is loaded
// once for the kHlfShowers showers.  A layer without centres does not read the tables.
// The sums are fp64: a voxel energy enters exactly and sum c^2 e / sum e - EC^2 keeps its digits for a narrow layer far from the
// axis.  What a record costs beside its voxels -- the tree and four divisions and two roots in fp64 -- is as much work as the
// voxels of a short layer, so the tree moves every sum once (below) and ends with each of a group's four records in a lane of
// its own, which finishes and stores it.  No atomics and no workspace: a record is the same bits in any batch and in any call.
// The grid is layers x shower slices, one dimension, sized for several rounds of workgroups so that the short layers' workgroups
// make room for the long ones'; it does not grow with the batch beyond that.
#include "guarded.h"

#include <vector>

// One geometry on the device (cd_hlf_create)
struct CdHlf {
  int layers = 0, R = 0, V = 0;
  int4* lay = nullptr;    // R records {first voxel, voxels, with centres, layer index}
  double* eta = nullptr;  // V
  double* phi = nullptr;  // V
  ~CdHlf() {
    if (lay) (void)hipFree(lay);
    if (eta) (void)hipFree(eta);
    if (phi) (void)hipFree(phi);
  }
};

namespace cd {
namespace {

constexpr int kHlfWaves = 4, kHlfThreads = 64 * kHlfWaves;
constexpr int kHlfShowers = 4;       // showers a lane group sums at once
constexpr int kHlfStrides = 4;       // voxels per shower and lane in flight
constexpr int kHlfGroup = 16;        // lanes that sum one layer of one shower: a DPP row
constexpr int kHlfPerTrip = kHlfShowers * (64 / kHlfGroup);  // showers of a wave's trip
constexpr int kHlfMaxBlocks = 16384; // about ten rounds of workgroups on 256 CUs

struct HlfAcc {
  double e = 0.0, ce = 0.0, pe = 0.0, cce = 0.0, ppe = 0.0;
  float mx = -INFINITY;
  int hits = 0;
};

// one voxel of one shower; eta * eta and phi * phi are formed once per voxel for the kHlfShowers showers (the reference's
// eta * eta * energy in its own order), which leaves four FMAs, an add and a conversion in fp64 per element
template <bool CENTRES>
__device__ __forceinline__ void hlf_add(HlfAcc& a, float v, double eta, double phi, double eta2, double phi2, float thr) {
  const double e = (double)v;
  a.e += e;
  if (CENTRES) {
    a.ce = fma(eta, e, a.ce);
    a.pe = fma(phi, e, a.pe);
    a.cce = fma(eta2, e, a.cce);
    a.ppe = fma(phi2, e, a.ppe);
  }
  a.mx = fmaxf(a.mx, v);
  a.hits += v > thr ? 1 : 0;
}

// the voxels j, j + G, ... of one layer of the showers row[0 .. kHlfShowers)
template <int G, bool CENTRES>
__device__ __forceinline__ void hlf_lane_sums(HlfAcc (&a)[kHlfShowers], const float* (&row)[kHlfShowers],
                                              const double* __restrict__ eta, const double* __restrict__ phi, int n, int j, float thr) {
  int i = j;
  for (; i + (kHlfStrides - 1) * G < n; i += kHlfStrides * G) {
    float v[kHlfStrides][kHlfShowers];
    double c[kHlfStrides], p[kHlfStrides];
#pragma unroll
    for (int k = 0; k < kHlfStrides; ++k) {
#pragma unroll
      for (int u = 0; u < kHlfShowers; ++u) v[k][u] = row[u][i + k * G];
      c[k] = CENTRES ? eta[i + k * G] : 0.0;
      p[k] = CENTRES ? phi[i + k * G] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < kHlfStrides; ++k) {
      const double c2 = c[k] * c[k], p2 = p[k] * p[k];
#pragma unroll
      for (int u = 0; u < kHlfShowers; ++u) hlf_add<CENTRES>(a[u], v[k][u], c[k], p[k], c2, p2, thr);
    }
  }
  for (; i < n; i += G) {
    float v[kHlfShowers];
#pragma unroll
    for (int u = 0; u < kHlfShowers; ++u) v[u] = row[u][i];
    const double c = CENTRES ? eta[i] : 0.0, p = CENTRES ? phi[i] : 0.0;
#pragma unroll
    for (int u = 0; u < kHlfShowers; ++u) hlf_add<CENTRES>(a[u], v[u], c, p, c * c, p * p, thr);
  }
}

// The tree over a group's 16 lanes, for the kHlfShowers = 4 showers each lane holds sums of.  Steps 1 and 2 pair lane j with
// j ^ 1 and j ^ 2: a lane keeps half of its showers and hands the other half to its partner, which keeps those, so a quad ends
// with one shower per lane (2 (j & 1) + (j >> 1 & 1)), summed over the quad.  Steps 3 and 4 add the lane 4 and then 8 places
// further round the row, which keeps j mod 4: lanes 0 - 3 of the group hold the four records.  Every move is a full-rate DPP
// move inside the row; each sum moves 5 times where a butterfly per shower moves it 16 times (and through the LDS crossbar, as a
// 64-lane group would need, costs a wave several cycles per dword: measured, that alone held Dataset 2 to 14 % of the stream).
template <int CTRL>
struct Dpp {
  __device__ __forceinline__ int operator()(int x) const { return __builtin_amdgcn_update_dpp(x, x, CTRL, 0xF, 0xF, true); }
};
using QuadXor1 = Dpp<0xB1>;  // quad_perm [1, 0, 3, 2]
using QuadXor2 = Dpp<0x4E>;  // quad_perm [2, 3, 0, 1]
using RowRor4 = Dpp<0x124>;
using RowRor8 = Dpp<0x128>;

template <typename P>
__device__ __forceinline__ double hlf_moved(double x, P p) {
  const long long b = __double_as_longlong(x);
  const unsigned lo = (unsigned)p((int)(unsigned)b), hi = (unsigned)p((int)(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// a += the partner's s
template <typename P>
__device__ __forceinline__ void hlf_take(HlfAcc& a, const HlfAcc& s, int centres, P p) {
  a.e += hlf_moved(s.e, p);
  if (centres) {
    a.ce += hlf_moved(s.ce, p);
    a.pe += hlf_moved(s.pe, p);
    a.cce += hlf_moved(s.cce, p);
    a.ppe += hlf_moved(s.ppe, p);
  }
  a.mx = fmaxf(a.mx, __int_as_float(p(__float_as_int(s.mx))));
  a.hits += p(s.hits);
}

__device__ __forceinline__ HlfAcc hlf_pick(bool first, const HlfAcc& x, const HlfAcc& y) {
  HlfAcc r;
  r.e = first ? x.e : y.e;
  r.ce = first ? x.ce : y.ce;
  r.pe = first ? x.pe : y.pe;
  r.cce = first ? x.cce : y.cce;
  r.ppe = first ? x.ppe : y.ppe;
  r.mx = first ? x.mx : y.mx;
  r.hits = first ? x.hits : y.hits;
  return r;
}

// One layer (L: {first voxel, voxels, with centres, layer}) of the showers this wave owns: four lane groups of kHlfShowers
// showers per trip, trips `step` showers apart
__device__ __forceinline__ void hlf_layer(const int4 L, int r, const double* __restrict__ eta, const double* __restrict__ phi,
                                          const float* __restrict__ showers, int V, int R, int batch, int first, int64_t step,
                                          float thr, double* __restrict__ out, int32_t* __restrict__ n_hits) {
  static_assert(kHlfShowers == 4 && kHlfGroup == 16, "the tree below");
  const int lane = threadIdx.x & 63, j = lane % kHlfGroup, sub = lane / kHlfGroup;
  const bool odd = j & 1, upper = j & 2;
  const int u_mine = (odd ? 2 : 0) + (upper ? 1 : 0);  // the shower whose record this lane ends with (lanes 0 - 3 of a group)
  for (int64_t b0 = (int64_t)first * kHlfPerTrip; b0 < batch; b0 += step) {
    const int64_t mine = b0 + sub * kHlfShowers;
    const float* row[kHlfShowers];
#pragma unroll
    for (int u = 0; u < kHlfShowers; ++u) {  // a shower beyond the batch reads the last one's row and stores nothing
      const int64_t b = mine + u < batch ? mine + u : batch - 1;
      row[u] = showers + b * V + L.x;
    }
    HlfAcc a[kHlfShowers];
    if (L.z) hlf_lane_sums<kHlfGroup, true>(a, row, eta + L.x, phi + L.x, L.y, j, thr);
    else hlf_lane_sums<kHlfGroup, false>(a, row, nullptr, nullptr, L.y, j, thr);
    HlfAcc k0 = hlf_pick(odd, a[2], a[0]), k1 = hlf_pick(odd, a[3], a[1]);
    hlf_take(k0, hlf_pick(odd, a[0], a[2]), L.z, QuadXor1{});
    hlf_take(k1, hlf_pick(odd, a[1], a[3]), L.z, QuadXor1{});
    HlfAcc t = hlf_pick(upper, k1, k0);
    hlf_take(t, hlf_pick(upper, k0, k1), L.z, QuadXor2{});
    hlf_take(t, t, L.z, RowRor4{});
    hlf_take(t, t, L.z, RowRor8{});
    double2 rec[4] = {{t.e, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, (double)t.mx}};
    if (L.z) {
      const double den = t.e + 1e-16;
      const double ec = t.ce / den, pc = t.pe / den;
      const double ve = fmax(t.cce / den - ec * ec, 0.0), vp = fmax(t.ppe / den - pc * pc, 0.0);
      rec[0].y = ec;
      rec[1] = {pc, ve};
      rec[2] = {vp, sqrt(ve)};
      rec[3].x = sqrt(vp);
    }
    if (j < kHlfShowers && mine + u_mine < batch) {
      const int64_t it = (mine + u_mine) * R + r;
      double2* o2 = reinterpret_cast<double2*>(out + it * 8);  // 64-byte records of a 16-byte aligned array
#pragma unroll
      for (int k = 0; k < 4; ++k) o2[k] = rec[k];
      n_hits[it] = t.hits;
    }
  }
}

// grid: blockIdx.x = slice * R + layer, so that workgroups dispatched together read neighbouring segments of the same showers
__global__ __launch_bounds__(kHlfThreads) void hlf_kernel(const int4* __restrict__ lay, const double* __restrict__ eta,
                                                          const double* __restrict__ phi, const float* __restrict__ showers,
                                                          int V, int R, int batch, int slices, float thr, double* __restrict__ out,
                                                          int32_t* __restrict__ n_hits) {
  const int r = blockIdx.x % R, slice = blockIdx.x / R;
  const int4 L = lay[r];
  const int first = slice * kHlfWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t step = (int64_t)slices * kHlfWaves * kHlfPerTrip;
  hlf_layer(L, r, eta, phi, showers, V, R, batch, first, step, thr, out, n_hits);
}

}  // namespace
}  // namespace cd

extern "C" {

int cd_hlf_create(const CdHlfDesc* desc, CdHlf** out, void* stream) {
  return guarded([&] {
    CD_REQUIRE(desc && out, "cd_hlf_create: desc and out must not be null");
    CD_REQUIRE(desc->struct_size == sizeof(CdHlfDesc), "cd_hlf_create: CdHlfDesc.struct_size is " + std::to_string(desc->struct_size) +
                                                           ", this library expects " + std::to_string(sizeof(CdHlfDesc)));
    CD_REQUIRE(desc->n_layers > 0, "cd_hlf_create: n_layers must be positive");
    CD_REQUIRE(desc->layer_offset, "cd_hlf_create: the layer_offset table is null");
    CD_REQUIRE(desc->eta, "cd_hlf_create: the eta table is null");
    CD_REQUIRE(desc->phi, "cd_hlf_create: the phi table is null");
    CD_REQUIRE(desc->with_centres, "cd_hlf_create: the with_centres table is null");
    const int n = desc->n_layers;
    const int32_t* off = desc->layer_offset;
    CD_REQUIRE(off[0] == 0, "cd_hlf_create: layer_offset[0] must be 0, got " + std::to_string(off[0]));
    std::vector<int4> lay;
    for (int l = 0; l < n; ++l) {
      CD_REQUIRE(off[l + 1] >= off[l], "cd_hlf_create: layer_offset must not decrease (layer " + std::to_string(l) + ")");
      if (off[l + 1] > off[l]) lay.push_back(make_int4(off[l], off[l + 1] - off[l], desc->with_centres[l] ? 1 : 0, l));
    }
    const int V = off[n];
    CD_REQUIRE(V > 0, "cd_hlf_create: V == 0, no layer has voxels");
    hipStream_t s = (hipStream_t)stream;
    struct Owner {
      CdHlf* m;
      ~Owner() { delete m; }
    } own{new CdHlf};
    CdHlf* m = own.m;
    m->layers = n; m->R = (int)lay.size(); m->V = V;
    CD_HIP(hipMalloc(&m->lay, sizeof(int4) * lay.size()));
    CD_HIP(hipMalloc(&m->eta, sizeof(double) * (size_t)V));
    CD_HIP(hipMalloc(&m->phi, sizeof(double) * (size_t)V));
    CD_HIP(hipMemcpyAsync(m->lay, lay.data(), sizeof(int4) * lay.size(), hipMemcpyHostToDevice, s));
    CD_HIP(hipMemcpyAsync(m->eta, desc->eta, sizeof(double) * (size_t)V, hipMemcpyHostToDevice, s));
    CD_HIP(hipMemcpyAsync(m->phi, desc->phi, sizeof(double) * (size_t)V, hipMemcpyHostToDevice, s));
    CD_HIP(hipStreamSynchronize(s));  // the host arrays may go away after the call
    *out = m;
    own.m = nullptr;
  });
}

int cd_hlf_destroy(CdHlf* hlf) {
  return guarded([&] { delete hlf; });
}

int cd_hlf_compute(const CdHlf* hlf, const float* showers, int batch, float threshold, double* out, int32_t* n_hits, void* stream) {
  return guarded([&] {
    CD_REQUIRE(hlf && showers && out && n_hits, "cd_hlf_compute: hlf, showers, out and n_hits must not be null");
    CD_REQUIRE(batch > 0, "cd_hlf_compute: batch must be positive");
    CD_REQUIRE(((uintptr_t)out & 15) == 0, "cd_hlf_compute: out must be 16-byte aligned");
    // a slice: the kHlfWaves * kHlfPerTrip showers of a workgroup's trip
    int64_t slices = ((int64_t)batch + kHlfWaves * kHlfPerTrip - 1) / (kHlfWaves * kHlfPerTrip);
    const int64_t most = kHlfMaxBlocks / hlf->R > 0 ? kHlfMaxBlocks / hlf->R : 1;
    if (slices > most) slices = most;
    hipLaunchKernelGGL(hlf_kernel, dim3((unsigned)(slices * hlf->R)), dim3(kHlfThreads), 0, (hipStream_t)stream, hlf->lay, hlf->eta,
                       hlf->phi, showers, hlf->V, hlf->R, batch, (int)slices, threshold, out, n_hits);
    CD_HIP(hipGetLastError());
  });
}

}  // extern "C"
