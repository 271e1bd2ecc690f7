/* Generate showers from C: the documented example of INTEGRATION.md section B2.  Plain C against include/calodiff.h and the HIP
 * runtime's C API; calodiffusion_amd/build.py compiles it next to the library (calodiffusion_amd/lib/cd_generate_example).
 *
 *   cd_generate_example <generator file> <energies.f32> <showers.f32> <batch> [seed [offset [physical [sparse]]]]
 *
 * <generator file>: written by calodiffusion_amd.generator.export_generator.  <energies.f32>: raw little-endian fp32, one row of
 * incident-energy columns per shower (cd_generator_info's energy columns: 1 for the regular grids and Dataset 0 / 1, 3 for
 * HGCal) -- the
 * conditioning values e of a loader, or with `physical` = 1 energies in the config's unit.  `sparse` (HGCal files whose decoder
 * has a column view): 0 plain decode, 1 sampled per shower, 2 sampled per batch, on the decoder's own stream (seed 1234, chained
 * from offset 0 as generate(sparse_decoding=True) walks it from Decoder.noise_offset = 0).
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
    fprintf(stderr, "usage: %s <generator file> <energies.f32> <showers.f32> <batch> [seed [offset [physical [sparse]]]]\n", argv[0]);
    return 1;
  }
  const int batch = atoi(argv[4]);
  const uint64_t seed = argc > 5 ? strtoull(argv[5], NULL, 10) : 1234;
  uint64_t offset = argc > 6 ? strtoull(argv[6], NULL, 10) : 0;
  const int physical = argc > 7 ? atoi(argv[7]) : 0;
  const int sparse = argc > 8 ? atoi(argv[8]) : 0;
  uint64_t decode_offset = 0;
  size_t blob_bytes = 0, e_bytes = 0;
  void* blob = read_file(argv[1], &blob_bytes);
  float* energies = (float*)read_file(argv[2], &e_bytes);
  if (!blob || !energies || batch <= 0 || e_bytes < sizeof(float)) {
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
  const size_t voxels = (size_t)info[0], cols = (size_t)info[2];
  const size_t n = e_bytes / sizeof(float) / cols; /* showers: one row of `cols` energies each */
  if (n == 0) {
    fprintf(stderr, "the energies file holds no full row of %zu columns\n", cols);
    return 1;
  }
  int32_t geo[8]; /* which geometry the file carries, and the sampler's state */
  CD_OK_OR_DIE(cd_generator_geometry(gen, geo));
  static const char* const kinds[3] = {"a regular grid", "HGCal maps", "Dataset-0/1 radial maps"};
  printf("format version %d: %s", info[7], kinds[geo[0] >= 0 && geo[0] < 3 ? geo[0] : 0]);
  if (geo[0] > 0) printf(", form %d (%s)", geo[1], geo[1] ? "the converter inside the model" : "converted at the end of the run");
  printf(", state (");
  for (int i = 0; i < geo[2] && i < 4; ++i) printf(i ? ", %d" : "%d", geo[3 + i]);
  printf(")\n");
  if (info[4] && !info[3]) {
    fprintf(stderr, "this model takes layer energies from its caller: pass them to cd_generator_run (not part of this example)\n");
    return 1;
  }

  size_t ws_bytes = 0;
  CD_OK_OR_DIE(cd_generator_workspace_bytes(gen, batch, &ws_bytes)); /* the largest batch of the run */
  void* ws = NULL;
  float *d_e = NULL, *d_showers = NULL;
  HIP_OK(hipMalloc(&ws, ws_bytes));
  HIP_OK(hipMalloc((void**)&d_e, (size_t)batch * cols * sizeof(float)));
  HIP_OK(hipMalloc((void**)&d_showers, (size_t)batch * voxels * sizeof(float)));
  float* showers = (float*)malloc((size_t)batch * voxels * sizeof(float));
  FILE* out = fopen(argv[3], "wb");
  if (!showers || !out) {
    fprintf(stderr, "cannot open %s\n", argv[3]);
    return 1;
  }
  for (size_t done = 0; done < n; done += (size_t)batch) {
    const int b = n - done < (size_t)batch ? (int)(n - done) : batch;
    HIP_OK(hipMemcpyAsync(d_e, energies + done * cols, (size_t)b * cols * sizeof(float), hipMemcpyHostToDevice, stream));
    struct CdGeneratorRun run = {0};
    run.struct_size = sizeof(run);
    run.batch = b; run.energy = d_e; run.energy_is_normalised = !physical; run.sparse_mode = sparse;
    run.seed = seed; run.offset = offset; run.first_row = 0; run.global_batch = b;
    run.showers = d_showers; run.next_offset = &offset;
    run.decode_seed = 1234; run.decode_offset = decode_offset; run.next_decode_offset = &decode_offset;
    run.workspace = ws; run.workspace_bytes = ws_bytes; run.stream = stream;
    CD_OK_OR_DIE(cd_generator_run_ex(gen, &run));
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
