// Philox4x32-10 + Box-Muller unit normals, shared by cd_randn (kernels_sampler.hip) and the layer model's sampler programs
// (kernels_mlp.hip).  Element g of a stream is a pure function of (seed, g): counter = g / 4, lane = g % 4, so batch shards on
// different GPUs draw disjoint slices of one stream.
// (The reference's torch.randn CPU stream (mt19937) cannot be reproduced on device; parity tests pass noise in.)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cd {

__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// the four unit normals of counter `ctr`: stream elements 4 ctr .. 4 ctr + 3
__device__ __forceinline__ void philox_normals4(uint64_t ctr, uint64_t seed, float z[4]) {
  uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float u1 = ((float)(c[2 * p] >> 8) + 0.5f) * (1.0f / 16777216.0f);  // (0,1)
    const float u2 = ((float)(c[2 * p + 1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float rad = sqrtf(-2.f * logf(u1));
    float sn, cs;
    sincosf(6.283185307179586f * u2, &sn, &cs);
    z[2 * p] = rad * cs;
    z[2 * p + 1] = rad * sn;
  }
}

// stream element g alone
__device__ __forceinline__ float philox_normal(uint64_t g, uint64_t seed) {
  float z[4];
  philox_normals4(g >> 2, seed, z);
  const int lane = (int)(g & 3);
  return lane == 0 ? z[0] : lane == 1 ? z[1] : lane == 2 ? z[2] : z[3];
}

// stream element g as a 24-bit uniform in [0, 1) (the sparse geometry decode's draw, kernels_geom.hip)
__device__ __forceinline__ float philox_uniform(uint64_t g, uint64_t seed) {
  const uint64_t ctr = g >> 2;
  uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const int lane = (int)(g & 3);
  const uint32_t w = lane == 0 ? c[0] : lane == 1 ? c[1] : lane == 2 ? c[2] : c[3];
  return (float)(w >> 8) * (1.0f / 16777216.0f);
}

}  // namespace cd
