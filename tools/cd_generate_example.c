/* Generate showers from C: the documented example of INTEGRATION.md section B2.  Plain C against include/calodiff.h and the HIP
 * runtime's C API; calodiffusion_amd/build.py compiles it next to the library (calodiffusion_amd/lib/cd_generate_example).
 *
 *   cd_generate_example <generator file> <energies.f32> <showers.f32> <batch> [seed [offset [physical]]]
 *
 * <generator file>: written by calodiffusion_amd.generator.export_generator.  <energies.f32>: raw little-endian fp32, one
 * incident energy per shower -- the conditioning values e of a loader, or with `physical` = 1 energies in the config's unit.
 * The energies are generated `batch` at a time (a shorter last batch is fine), every call continuing the Philox stream where the
 * previous one stopped (next_offset), exactly as model.generate(loader, steps) walks it from model.noise_offset = offset.
 * <showers.f32>: raw fp32 (n, voxels) physical showers.  The model must not need layer energies from its caller. */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "calodiff.h"

static void* read_file(const char* path, size_t* bytes) {
  FILE* f = fopen(path, "rb");
  if (!f) return NULL;
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  void* p = n > 0 ? malloc((size_t)n) : NULL;
  if (p && fread(p, 1, (size_t)n, f) != (size_t)n) {
    free(p);
    p = NULL;
  }
  fclose(f);
  *bytes = p ? (size_t)n : 0;
  return p;
}

#define HIP_OK(expr)                                                              \
  do {                                                                            \
    hipError_t e_ = (expr);                                                       \
    if (e_ != hipSuccess) {                                                       \
      fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e_));                  \
      return 1;                                                                   \
    }                                                                             \
  } while (0)
#define CD_OK_OR_DIE(expr)                                                        \
  do {                                                                            \
    if ((expr) != CD_OK) {                                                        \
      fprintf(stderr, "%s: %s\n", #expr, cd_last_error());                        \
      return 1;                                                                   \
    }                                                                             \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: %s <generator file> <energies.f32> <showers.f32> <batch> [seed [offset [physical]]]\n", argv[0]);
    return 1;
  }
  const int batch = atoi(argv[4]);
  const uint64_t seed = argc > 5 ? strtoull(argv[5], NULL, 10) : 1234;
  uint64_t offset = argc > 6 ? strtoull(argv[6], NULL, 10) : 0;
  const int physical = argc > 7 ? atoi(argv[7]) : 0;
  size_t blob_bytes = 0, e_bytes = 0;
  void* blob = read_file(argv[1], &blob_bytes);
  float* energies = (float*)read_file(argv[2], &e_bytes);
  const size_t n = e_bytes / sizeof(float);
  if (!blob || !energies || batch <= 0 || n == 0) {
    fprintf(stderr, "cannot read the generator file or the energies, or batch <= 0\n");
    return 1;
  }
  if (cd_abi_version() != CD_ABI_VERSION) {
    fprintf(stderr, "library ABI %d, header ABI %d\n", cd_abi_version(), CD_ABI_VERSION);
    return 1;
  }
  CD_OK_OR_DIE(cd_device_check(NULL, 0));

  hipStream_t stream;
  HIP_OK(hipStreamCreate(&stream));
  CdGenerator* gen = NULL;
  CD_OK_OR_DIE(cd_generator_create(blob, blob_bytes, &gen, stream));
  free(blob); /* the handle keeps nothing of it */
  int32_t info[8];
  CD_OK_OR_DIE(cd_generator_info(gen, info));
  const size_t voxels = (size_t)info[0];
  if (info[4] && !info[3]) {
    fprintf(stderr, "this model takes layer energies from its caller: pass them to cd_generator_run (not part of this example)\n");
    return 1;
  }

  size_t ws_bytes = 0;
  CD_OK_OR_DIE(cd_generator_workspace_bytes(gen, batch, &ws_bytes)); /* the largest batch of the run */
  void* ws = NULL;
  float *d_e = NULL, *d_showers = NULL;
  HIP_OK(hipMalloc(&ws, ws_bytes));
  HIP_OK(hipMalloc((void**)&d_e, (size_t)batch * sizeof(float)));
  HIP_OK(hipMalloc((void**)&d_showers, (size_t)batch * voxels * sizeof(float)));
  float* showers = (float*)malloc((size_t)batch * voxels * sizeof(float));
  FILE* out = fopen(argv[3], "wb");
  if (!showers || !out) {
    fprintf(stderr, "cannot open %s\n", argv[3]);
    return 1;
  }
  for (size_t done = 0; done < n; done += (size_t)batch) {
    const int b = n - done < (size_t)batch ? (int)(n - done) : batch;
    HIP_OK(hipMemcpyAsync(d_e, energies + done, (size_t)b * sizeof(float), hipMemcpyHostToDevice, stream));
    CD_OK_OR_DIE(cd_generator_run(gen, b, d_e, !physical, NULL, seed, offset, 0, b, d_showers, NULL, &offset, ws, ws_bytes, stream));
    HIP_OK(hipMemcpyAsync(showers, d_showers, (size_t)b * voxels * sizeof(float), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    if (fwrite(showers, sizeof(float), (size_t)b * voxels, out) != (size_t)b * voxels) {
      fprintf(stderr, "short write to %s\n", argv[3]);
      return 1;
    }
  }
  fclose(out);
  printf("%zu showers of %zu voxels, next offset %llu\n", n, voxels, (unsigned long long)offset);
  CD_OK_OR_DIE(cd_generator_destroy(gen));
  HIP_OK(hipFree(ws));
  HIP_OK(hipFree(d_e));
  HIP_OK(hipFree(d_showers));
  HIP_OK(hipStreamDestroy(stream));
  free(showers);
  free(energies);
  return 0;
}
