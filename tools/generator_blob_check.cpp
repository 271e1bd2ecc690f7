// Host-only check of a generator file: runs the reader cd_generator_create uses (csrc/generator_blob.h) and prints the section
// table, or the reader's error.  Exit status 0 (good file) or 1.
//
//   g++ -std=c++17 -O1 -I calodiffusion_amd/csrc tools/generator_blob_check.cpp -o generator_blob_check
//   ./generator_blob_check model.cdgen
#include "generator_blob.h"

#include <cstdio>
#include <fstream>
#include <iterator>

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s <generator file>\n", argv[0]);
    return 1;
  }
  std::ifstream in(argv[1], std::ios::binary);
  if (!in) {
    std::fprintf(stderr, "%s: cannot open\n", argv[1]);
    return 1;
  }
  const std::vector<char> bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  cdgen::Blob blob;
  std::string err;
  if (!cdgen::parse(bytes.data(), bytes.size(), &blob, &err)) {
    std::fprintf(stderr, "%s: %s\n", argv[1], err.c_str());
    return 1;
  }
  std::printf("%s: format version %u, %llu bytes, config '%s'\n", argv[1], blob.version, (unsigned long long)blob.total_bytes,
              blob.meta.config_name);
  for (const cdgen::Section& s : blob.sections)
    std::printf("  %s  offset %10llu  bytes %10llu\n", cdgen::detail::tag_name(s.tag).c_str(), (unsigned long long)s.off,
                (unsigned long long)s.bytes);
  std::printf("  U-Net: %zu tensors, sampler %s, %d steps\n", blob.unet.weights.size(), blob.unet_sampler.kind ? "program" : "table",
              blob.unet_sampler.n_steps);
  if (blob.meta.has_layer_stage)
    std::printf("  layer model: %zu tensors, sampler %s, %d steps\n", blob.layer.weights.size(),
                blob.layer_sampler.kind ? "program" : "table", blob.layer_sampler.n_steps);
  if (blob.geom.form >= 0) {
    const cdgen::Geom& g = blob.geom;
    std::printf("  geometry: form %d (%s), bins (%d, %d, %d), %d cells a layer, embed_mean %g, embed_std %g, %d energy columns\n", g.form,
                g.form ? "in-model" : "pre-embedded", g.layers, g.alpha, g.r, g.cells, g.embed_mean, g.embed_std, blob.rev.energy_cols);
    if (g.form == 1)
      std::printf("  encoder: %d x %d a layer, %d entries%s\n", g.enc.rows, g.enc.cols, g.enc.nnz, g.enc.is_mask ? " (a mask's pattern)" : "");
    std::printf("  decoder: %d x %d a layer, %d entries%s\n", g.dec.rows, g.dec.cols, g.dec.nnz, g.dec.is_mask ? " (a mask's pattern)" : "");
  }
  if (blob.radial.form >= 0) {
    const cdgen::Radial& g = blob.radial;
    std::printf("  radial geometry: form %d (%s), grid (%d, %d, %d), %d voxels, %d matrix floats x %d\n", g.form,
                g.form ? "in-model" : "on the converted grid", g.layers, g.alpha_out, g.r_out, g.voxels, g.wtotal, g.n_mats);
    std::printf("  layers (alpha x radial bins):");
    for (int i = 0; i < g.layers; ++i)
      std::printf(" %d x %d", cdgen::detail::rd<int32_t>(g.alpha + 4 * i), cdgen::detail::rd<int32_t>(g.rin + 4 * i));
    std::printf("\n  reverse norm: logit %.17g / %.17g, total E %.17g / %.17g, layers %.17g / %.17g, MAXDEP %g, ECUT %g\n", blob.rev.consts64[0],
                blob.rev.consts64[1], blob.rev.consts64[2], blob.rev.consts64[3], blob.rev.consts64[4], blob.rev.consts64[5],
                blob.rev.max_deposit, blob.rev.ecut);
  }
  return 0;
}
