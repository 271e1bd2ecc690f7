// Reader of the generator file (calodiffusion_amd/generator.py: export_generator; format: DESIGN.md "Generator file"), format
// versions 1 (regular grids), 2 (HGCal: a GEOM section with the geometry maps by their sparse entries) and 3 (Dataset 0 / 1: a
// RADL section with the irregular layout as cd_radial_create takes it and the matrices in cd_radial_enc / cd_radial_dec layout).
// Pure C++17, no HIP: cd_generator_create (generator.hip) and tools/generator_blob_check.cpp share it.
//
// parse() validates everything before anything is dereferenced: magic, version, total length, checksum, every section's
// offset and size against the blob length, every count against its section, with overflow-checked sums and products.  It returns
// VIEWS: byte pointers into the caller's blob (which may be unaligned: fixed records are copied out with memcpy, arrays are
// handed on as bytes for the consumer to memcpy).  A bad blob is `false` and a message, never a crash.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <string>
#include <vector>

#include "geom_csr_check.h"

namespace cdgen {

constexpr char kMagic[8] = {'C', 'D', 'G', 'E', 'N', 'B', 'L', 'B'};
constexpr uint32_t kVersion = 1;      // regular-grid files
constexpr uint32_t kVersionGeom = 2;  // HGCal files: a GEOM section, per-column EMAX / EMIN in RNRM
constexpr uint32_t kVersionRadial = 3;  // Dataset-0/1 files: a RADL section, the float64 constants of cd_reverse_norm_ds1 in RNRM
constexpr uint64_t kHeaderBytes = 64, kSectionEntryBytes = 24, kAlign = 64;
constexpr uint64_t kStepBytes = 16, kOpBytes = 40;  // sizeof(CdStep), sizeof(CdSamplerOp): generator.hip asserts both
constexpr uint64_t kWeightRecordBytes = 112, kWeightNameBytes = 96;
constexpr uint64_t kNetHeaderBytes = 32, kSamplerHeaderBytes = 64, kMetaBytes = 128, kRevNormBytes = 80;
constexpr uint64_t kRevNormGeomBytes = 96, kGeomHeaderBytes = 64, kGeomMapHeaderBytes = 64;  // version 2
constexpr int32_t kMaxEnergyCols = 8;                                                         // cd_preprocess_hgcal's limit
constexpr uint64_t kRevNormRadialBytes = 128, kRadialHeaderBytes = 64;                        // version 3
// cd_radial_create's on-chip limits (include/calodiff.h, "Dataset-1 radial maps")
constexpr int32_t kRadialMaxLayers = 64, kRadialMaxWeightFloats = 8192, kRadialMaxRowFloats = 6144;

constexpr uint32_t fourcc(char a, char b, char c, char d) {
  return (uint32_t)(uint8_t)a | (uint32_t)(uint8_t)b << 8 | (uint32_t)(uint8_t)c << 16 | (uint32_t)(uint8_t)d << 24;
}
constexpr uint32_t kTagMeta = fourcc('M', 'E', 'T', 'A'), kTagUnet = fourcc('U', 'N', 'E', 'T'), kTagLayer = fourcc('L', 'A', 'Y', 'R'),
                   kTagUnetSampler = fourcc('U', 'S', 'M', 'P'), kTagLayerSampler = fourcc('L', 'S', 'M', 'P'),
                   kTagRevNorm = fourcc('R', 'N', 'R', 'M'), kTagGeom = fourcc('G', 'E', 'O', 'M'), kTagRadial = fourcc('R', 'A', 'D', 'L');

inline uint64_t fnv1a64(const unsigned char* p, uint64_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (uint64_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
  return h;
}

struct Section {
  uint32_t tag;
  uint64_t off, bytes;
};

struct Weight {
  std::string name;
  uint64_t numel;
  const unsigned char* data;  // numel fp32, little-endian
};

// the network part of a UNET / LAYR section
struct Net {
  const unsigned char* desc = nullptr;  // CdUnetDesc / CdLayerMlpDesc bytes
  uint32_t desc_bytes = 0;
  uint32_t n_coord[3] = {0, 0, 0};  // r (W), z (D), phi (H) profile lengths
  const unsigned char* coord[3] = {nullptr, nullptr, nullptr};
  std::vector<Weight> weights;
};

struct Sampler {
  int32_t kind = 0;  // 0: CdStep table (cd_ddim_sample / cd_layer_sample); 1: step program (cd_sampler_run / cd_layer_sampler_run)
  int32_t n_steps = 0, n_ops = 0, n_coef = 0, n_bufs = 0, has_op_begin = 0, noise_tensors_drawn = 0, use_graph = 0;
  float start_scale = 1.f;
  const unsigned char* steps = nullptr;     // kind 0: n_steps CdStep
  const unsigned char* ops = nullptr;       // kind 1: n_ops CdSamplerOp
  const unsigned char* op_begin = nullptr;  // kind 1, has_op_begin: n_steps + 1 int32
  const unsigned char* coefs = nullptr;     // kind 1: n_steps * n_coef fp32
};

struct Meta {
  int32_t data_ndim = 0, data_shape[4] = {0, 0, 0, 0};
  int32_t cond_size = 0, energy_cols = 0, has_layer_stage = 0, takes_layers = 0, sample_steps = 0, layer_steps = 0, sample_offset = 0;
  uint64_t seed = 0;
  int32_t layer_dim = 0;
  char config_name[65] = {0};
};

struct RevNorm {
  int32_t dims[3] = {0, 0, 0};
  int32_t layer_map = 0, logE = 0, dataset_num = 0;
  float consts[6] = {0, 0, 0, 0, 0, 0};
  float max_deposit = 0, ecut = 0;
  double emax = 0, emin = 0;  // version 2: column 0 of the lists below
  // version 2 (HGCal); a version-1 file reads as one column, alpha and layer_eps unused
  int32_t energy_cols = 1;
  float alpha = 0, layer_eps = 0;  // cd_reverse_norm_staged's
  double emax_col[kMaxEnergyCols] = {0}, emin_col[kMaxEnergyCols] = {0};
  // version 3 (Dataset 0 / 1): cd_reverse_norm_ds1's constants, float64 as postprocess.DATASET1_PARAMS holds them
  double consts64[6] = {0, 0, 0, 0, 0, 0};
};

// one map of the GEOM section: per-layer CSR over layers * rows lines, little-endian arrays (views, possibly unaligned)
struct GeomMap {
  int32_t rows = 0, cols = 0, nnz = 0, is_mask = 0;
  const unsigned char* row_ptr = nullptr;  // layers * rows + 1 int32
  const unsigned char* col_idx = nullptr;  // nnz int32
  const unsigned char* val = nullptr;      // nnz fp32
};

struct Geom {
  int32_t form = -1;  // -1: no GEOM section; 0: pre-embedded (decoder only); 1: in-model (encoder and decoder)
  int32_t layers = 0, alpha = 0, r = 0, cells = 0, n_maps = 0;
  float embed_mean = 0, embed_std = 1;  // the converter's norm as its dec / enc apply it (0, 1: none)
  GeomMap enc, dec;
};

// the RADL section: cd_radial_create's arguments and the matrices, little-endian arrays (views, possibly unaligned)
struct Radial {
  int32_t form = -1;  // -1: no RADL section; 0: on the converted grid (the un-conversion matrices); 1: in-model (encoder, decoder)
  int32_t layers = 0, alpha_out = 0, r_out = 0, voxels = 0, n_mats = 0, wtotal = 0;
  const unsigned char* bound = nullptr;  // layers + 1 int32
  const unsigned char* alpha = nullptr;  // layers int32
  const unsigned char* rin = nullptr;    // layers int32
  const unsigned char* enc = nullptr;    // form 1: wtotal fp32 in cd_radial_enc's layout
  const unsigned char* dec = nullptr;    // wtotal fp32 in cd_radial_dec's layout (form 0: GeomConverter.pinv_mats)
};

struct Blob {
  uint32_t version = 0;
  uint64_t total_bytes = 0, checksum = 0;
  std::vector<Section> sections;
  Meta meta;
  RevNorm rev;
  Geom geom;
  Radial radial;
  Net unet, layer;
  Sampler unet_sampler, layer_sampler;
};

namespace detail {

template <typename T>
inline T rd(const unsigned char* p) {
  T v;
  memcpy(&v, p, sizeof(T));
  return v;
}
inline bool mul_ok(uint64_t a, uint64_t b, uint64_t* out) {
  if (a != 0 && b > UINT64_MAX / a) return false;
  *out = a * b;
  return true;
}
inline bool add_ok(uint64_t a, uint64_t b, uint64_t* out) {
  if (b > UINT64_MAX - a) return false;
  *out = a + b;
  return true;
}
inline std::string tag_name(uint32_t tag) {
  std::string s(4, '?');
  for (int i = 0; i < 4; ++i) {
    const char c = (char)(tag >> (8 * i) & 0xff);
    s[i] = c >= 32 && c < 127 ? c : '?';
  }
  return s;
}

// a cursor over one section: take(n) hands out the next n bytes or fails
struct Cursor {
  const unsigned char* base;
  uint64_t size, pos;
  bool take(uint64_t n, const unsigned char** out) {
    uint64_t end;
    if (!add_ok(pos, n, &end) || end > size) return false;
    *out = base + pos;
    pos = end;
    return true;
  }
  bool take_array(uint64_t count, uint64_t elem, const unsigned char** out) {
    uint64_t n;
    return mul_ok(count, elem, &n) && take(n, out);
  }
  void align(uint64_t a) {  // the next array starts on a multiple of `a` (a section's last padding may be cut)
    const uint64_t up = (pos + a - 1) / a * a;
    pos = up < size ? up : size;
  }
};

// GEOM: header {form, L, A, R, N, n_maps, embed_mean, embed_std}, then n_maps records {rows, cols, nnz, is_mask} each followed by
// row_ptr, col_idx and val, every piece on a 64-byte boundary.  Counts against the section, shapes against the bins, then the CSR
// invariants -- all before a consumer reads a record.
inline bool parse_geom(const unsigned char* sec, uint64_t size, Geom* g, std::string* err) {
  Cursor c{sec, size, 0};
  const unsigned char* h;
  if (!c.take(kGeomHeaderBytes, &h)) return *err = "GEOM: section shorter than its header", false;
  int32_t* f[6] = {&g->form, &g->layers, &g->alpha, &g->r, &g->cells, &g->n_maps};
  for (int i = 0; i < 6; ++i) *f[i] = rd<int32_t>(h + 4 * i);
  g->embed_mean = rd<float>(h + 24);
  g->embed_std = rd<float>(h + 28);
  if (g->form != 0 && g->form != 1) return g->form = -1, *err = "GEOM: unknown form (0: pre-embedded, 1: in-model)", false;
  if (g->n_maps != g->form + 1) return *err = "GEOM: form 0 holds one map (the decoder), form 1 two (encoder, decoder)", false;
  if (g->layers < 1 || g->alpha < 1 || g->r < 1 || g->cells < 1 || g->layers > 65536 || g->alpha > 65536 || g->r > 65536 ||
      (uint64_t)g->layers * (uint64_t)g->cells > (1ull << 28) || (uint64_t)g->alpha * (uint64_t)g->r > (1ull << 28))
    return *err = "GEOM: bins or cell count out of range", false;
  if (!std::isfinite(g->embed_mean) || !std::isfinite(g->embed_std) || g->embed_std == 0.f)
    return *err = "GEOM: embed_mean / embed_std must be finite and embed_std not 0", false;
  if (g->form == 1 && (g->embed_mean != 0.f || g->embed_std != 1.f)) return *err = "GEOM: an in-model converter has no norm", false;
  const int32_t grid = g->alpha * g->r;
  for (int k = 0; k < g->n_maps; ++k) {
    const bool is_enc = g->form == 1 && k == 0;
    GeomMap* m = is_enc ? &g->enc : &g->dec;
    const std::string what = is_enc ? "GEOM encoder" : "GEOM decoder";
    if (!c.take(kGeomMapHeaderBytes, &h)) return *err = what + ": record header overflows the section", false;
    m->rows = rd<int32_t>(h); m->cols = rd<int32_t>(h + 4); m->nnz = rd<int32_t>(h + 8); m->is_mask = rd<int32_t>(h + 12);
    if (m->rows != (is_enc ? grid : g->cells) || m->cols != (is_enc ? g->cells : grid))
      return *err = what + ": its shape is not that of the bins and the cell count", false;
    if (m->nnz < 0) return *err = what + ": negative entry count", false;
    if (g->form == 0 && m->is_mask) return *err = what + ": a pre-embedded file holds a frozen decoder, not a mask's pattern", false;
    uint64_t lines;
    if (!mul_ok((uint64_t)g->layers, (uint64_t)m->rows, &lines) || !add_ok(lines, 1, &lines) || !c.take_array(lines, 4, &m->row_ptr))
      return *err = what + ": row_ptr overflows the section", false;
    c.align(kAlign);
    if (!c.take_array((uint64_t)m->nnz, 4, &m->col_idx)) return *err = what + ": " + std::to_string(m->nnz) + " columns overflow the section", false;
    c.align(kAlign);
    if (!c.take_array((uint64_t)m->nnz, 4, &m->val)) return *err = what + ": " + std::to_string(m->nnz) + " values overflow the section", false;
    c.align(kAlign);
    std::string why;
    if (!cdgeom::csr_valid(m->row_ptr, m->col_idx, m->val, g->layers, m->rows, m->cols, m->nnz, &why)) return *err = what + ": " + why, false;
  }
  return true;
}

// RADL: header {form, L, A, R, V, n_mats, wtotal}, then bound[L + 1], alpha[L], rin[L] (int32) and n_mats matrices of wtotal fp32
// -- the encoder then the decoder (form 1), or the un-conversion matrices (form 0) --, every piece on a 64-byte boundary.  Counts
// against the section first, then every rule cd_radial_create has, then the values: nothing is uploaded from a file that fails.
inline bool parse_radial(const unsigned char* sec, uint64_t size, Radial* g, std::string* err) {
  Cursor c{sec, size, 0};
  const unsigned char* h;
  if (!c.take(kRadialHeaderBytes, &h)) return *err = "RADL: section shorter than its header", false;
  int32_t* f[7] = {&g->form, &g->layers, &g->alpha_out, &g->r_out, &g->voxels, &g->n_mats, &g->wtotal};
  for (int i = 0; i < 7; ++i) *f[i] = rd<int32_t>(h + 4 * i);
  if (g->form != 0 && g->form != 1) return g->form = -1, *err = "RADL: unknown form (0: on the converted grid, 1: in-model)", false;
  if (g->n_mats != g->form + 1) return *err = "RADL: form 0 holds one set of matrices (the un-conversion), form 1 two (encoder, decoder)", false;
  const int32_t L = g->layers, A = g->alpha_out, R = g->r_out;
  if (L < 1 || L > kRadialMaxLayers) return *err = "RADL: 1 to " + std::to_string(kRadialMaxLayers) + " layers (cd_radial_create's limit)", false;
  if (A < 1 || R < 1 || A > kRadialMaxRowFloats || R > kRadialMaxRowFloats || (int64_t)L * A * R > kRadialMaxRowFloats)
    return *err = "RADL: layers * alpha_out * r_out must be 1 to " + std::to_string(kRadialMaxRowFloats) + " (cd_radial_create's limit)", false;
  if (g->voxels < 1 || g->voxels > kRadialMaxRowFloats)
    return *err = "RADL: 1 to " + std::to_string(kRadialMaxRowFloats) + " voxels (cd_radial_create's limit)", false;
  if (g->wtotal < 1 || g->wtotal > kRadialMaxWeightFloats)
    return *err = "RADL: the matrices hold 1 to " + std::to_string(kRadialMaxWeightFloats) + " floats (cd_radial_create's limit)", false;
  if (!c.take_array((uint64_t)L + 1, 4, &g->bound)) return *err = "RADL: bound overflows the section", false;
  c.align(kAlign);
  if (!c.take_array((uint64_t)L, 4, &g->alpha)) return *err = "RADL: alpha overflows the section", false;
  c.align(kAlign);
  if (!c.take_array((uint64_t)L, 4, &g->rin)) return *err = "RADL: rin overflows the section", false;
  c.align(kAlign);
  int64_t sum_rin = 0;
  if (rd<int32_t>(g->bound) != 0) return *err = "RADL: bound[0] is not 0", false;
  for (int i = 0; i < L; ++i) {
    const int32_t lo = rd<int32_t>(g->bound + 4 * i), hi = rd<int32_t>(g->bound + 4 * (i + 1));
    const int32_t a = rd<int32_t>(g->alpha + 4 * i), n = rd<int32_t>(g->rin + 4 * i);
    const std::string lay = "RADL: layer " + std::to_string(i);
    if (hi <= lo) return *err = lay + ": bound is not strictly increasing", false;
    if (a != 1 && a != A) return *err = lay + ": alpha is " + std::to_string(a) + ", a layer has 1 or alpha_out angular bins", false;
    if (n < 1 || n > kRadialMaxRowFloats) return *err = lay + ": radial bin count out of range", false;
    if ((int64_t)hi - lo != (int64_t)a * n) return *err = lay + ": its span is not alpha * rin voxels", false;
    sum_rin += n;
  }
  if (rd<int32_t>(g->bound + 4 * L) != g->voxels) return *err = "RADL: the voxel count is not bound[layers]", false;
  if ((int64_t)R * sum_rin != (int64_t)g->wtotal) return *err = "RADL: the matrices' size is not r_out * sum of rin", false;
  for (int k = 0; k < g->n_mats; ++k) {
    const bool is_enc = g->form == 1 && k == 0;
    const unsigned char** m = is_enc ? &g->enc : &g->dec;
    const std::string what = is_enc ? "RADL encoder" : g->form == 1 ? "RADL decoder" : "RADL un-conversion";
    if (!c.take_array((uint64_t)g->wtotal, 4, m)) return *err = what + ": " + std::to_string(g->wtotal) + " values overflow the section", false;
    c.align(kAlign);
    for (int32_t i = 0; i < g->wtotal; ++i)
      if (!std::isfinite(rd<float>(*m + 4 * (uint64_t)i))) return *err = what + ": value " + std::to_string(i) + " is not finite", false;
  }
  return true;
}

inline bool parse_net(const unsigned char* sec, uint64_t size, const char* what, bool with_coords, Net* net, std::string* err) {
  Cursor c{sec, size, 0};
  const unsigned char* h;
  if (!c.take(kNetHeaderBytes, &h)) return *err = std::string(what) + ": section shorter than its header", false;
  net->desc_bytes = rd<uint32_t>(h);
  const uint32_t n_weights = rd<uint32_t>(h + 4);
  for (int i = 0; i < 3; ++i) net->n_coord[i] = rd<uint32_t>(h + 8 + 4 * i);
  if (net->desc_bytes < 4 || net->desc_bytes > 4096) return *err = std::string(what) + ": descriptor size out of range", false;
  if (n_weights == 0 || n_weights > 65536) return *err = std::string(what) + ": weight count out of range", false;
  if (!c.take(((uint64_t)net->desc_bytes + 7) & ~7ull, &net->desc)) return *err = std::string(what) + ": descriptor overflows its section", false;
  for (int i = 0; i < 3; ++i) {
    if (!with_coords && net->n_coord[i]) return *err = std::string(what) + ": unexpected coordinate profile", false;
    if (net->n_coord[i] > (1u << 20) || !c.take_array(net->n_coord[i], 4, &net->coord[i]))
      return *err = std::string(what) + ": coordinate profile overflows its section", false;
  }
  const unsigned char* recs;
  if (!c.take_array(n_weights, kWeightRecordBytes, &recs))
    return *err = std::string(what) + ": weight count " + std::to_string(n_weights) + " overflows its section", false;
  const uint64_t table_end = c.pos;
  uint64_t total = 0;
  net->weights.reserve(n_weights);
  for (uint32_t i = 0; i < n_weights; ++i) {
    const unsigned char* r = recs + (uint64_t)i * kWeightRecordBytes;
    if (memchr(r, 0, kWeightNameBytes) == nullptr || r[0] == 0)
      return *err = std::string(what) + ": weight " + std::to_string(i) + " has no terminated name", false;
    Weight w;
    w.name = (const char*)r;
    w.numel = rd<uint64_t>(r + kWeightNameBytes);
    const uint64_t off = rd<uint64_t>(r + kWeightNameBytes + 8);
    uint64_t nbytes, end;
    if (w.numel == 0 || !mul_ok(w.numel, 4, &nbytes) || !add_ok(off, nbytes, &end) || off < table_end || end > size || (off & 3))
      return *err = std::string(what) + ": weight '" + w.name + "' (" + std::to_string(w.numel) + " elements) overflows its section", false;
    if (!add_ok(total, nbytes, &total) || total > size)
      return *err = std::string(what) + ": weight sizes add up to more than the section", false;
    w.data = sec + off;
    net->weights.push_back(std::move(w));
  }
  return true;
}

inline bool parse_sampler(const unsigned char* sec, uint64_t size, const char* what, Sampler* s, std::string* err) {
  Cursor c{sec, size, 0};
  const unsigned char* h;
  if (!c.take(kSamplerHeaderBytes, &h)) return *err = std::string(what) + ": section shorter than its header", false;
  int32_t* f[8] = {&s->kind, &s->n_steps, &s->n_ops, &s->n_coef, &s->n_bufs, &s->has_op_begin, &s->noise_tensors_drawn, &s->use_graph};
  for (int i = 0; i < 8; ++i) *f[i] = rd<int32_t>(h + 4 * i);
  s->start_scale = rd<float>(h + 32);
  if (s->kind != 0 && s->kind != 1) return *err = std::string(what) + ": unknown sampler kind", false;
  if (s->n_steps < 1 || s->n_steps > (1 << 20)) return *err = std::string(what) + ": step count out of range", false;
  if (s->noise_tensors_drawn < 0) return *err = std::string(what) + ": negative noise tensor count", false;
  if (s->kind == 0) {
    if (!c.take_array((uint64_t)s->n_steps, kStepBytes, &s->steps))
      return *err = std::string(what) + ": step table of " + std::to_string(s->n_steps) + " rows overflows its section", false;
    return true;
  }
  if (s->n_ops < 1 || s->n_ops > (1 << 24) || s->n_coef < 1 || s->n_coef > (1 << 20) || s->n_bufs < 1 || s->n_bufs > 64)
    return *err = std::string(what) + ": program sizes out of range", false;
  if (!c.take_array((uint64_t)s->n_ops, kOpBytes, &s->ops))
    return *err = std::string(what) + ": " + std::to_string(s->n_ops) + " ops overflow their section", false;
  if (s->has_op_begin && !c.take_array((uint64_t)s->n_steps + 1, 4, &s->op_begin))
    return *err = std::string(what) + ": op_begin overflows its section", false;
  uint64_t n;
  if (!mul_ok((uint64_t)s->n_steps, (uint64_t)s->n_coef, &n) || !c.take_array(n, 4, &s->coefs))
    return *err = std::string(what) + ": coefficient table overflows its section", false;
  return true;
}

}  // namespace detail

inline const Section* find_section(const Blob& b, uint32_t tag) {
  for (const Section& s : b.sections)
    if (s.tag == tag) return &s;
  return nullptr;
}

inline bool parse(const void* blob, size_t bytes, Blob* out, std::string* err) {
  using namespace detail;
  const unsigned char* p = (const unsigned char*)blob;
  if (!p || !out || !err) return false;
  if (bytes < kHeaderBytes) return *err = "generator file: shorter than its 64-byte header", false;
  if (memcmp(p, kMagic, 8) != 0) return *err = "generator file: wrong magic (not a generator file)", false;
  out->version = rd<uint32_t>(p + 8);
  if (out->version != kVersion && out->version != kVersionGeom && out->version != kVersionRadial)
    return *err = "generator file: format version " + std::to_string(out->version) + ", this reader knows versions " + std::to_string(kVersion) +
                  ", " + std::to_string(kVersionGeom) + " and " + std::to_string(kVersionRadial), false;
  const bool v2 = out->version == kVersionGeom, v3 = out->version == kVersionRadial;
  const uint32_t n_sections = rd<uint32_t>(p + 12);
  out->total_bytes = rd<uint64_t>(p + 16);
  out->checksum = rd<uint64_t>(p + 24);
  if (out->total_bytes != (uint64_t)bytes)
    return *err = "generator file: header says " + std::to_string(out->total_bytes) + " bytes, " + std::to_string(bytes) + " given (truncated?)", false;
  if (n_sections == 0 || n_sections > 64) return *err = "generator file: section count out of range", false;
  const uint64_t table_end = kHeaderBytes + (uint64_t)n_sections * kSectionEntryBytes;
  if (table_end > (uint64_t)bytes) return *err = "generator file: section table overflows the file", false;
  out->sections.clear();
  for (uint32_t i = 0; i < n_sections; ++i) {
    const unsigned char* e = p + kHeaderBytes + (uint64_t)i * kSectionEntryBytes;
    Section s{rd<uint32_t>(e), rd<uint64_t>(e + 8), rd<uint64_t>(e + 16)};
    uint64_t end;
    if (!add_ok(s.off, s.bytes, &end) || s.off < table_end || end > (uint64_t)bytes)
      return *err = "generator file: section '" + tag_name(s.tag) + "' (offset " + std::to_string(s.off) + ", " + std::to_string(s.bytes) +
                    " bytes) lies outside the file", false;
    if (s.off % kAlign) return *err = "generator file: section '" + tag_name(s.tag) + "' is not 64-byte aligned", false;
    if (find_section(*out, s.tag)) return *err = "generator file: section '" + tag_name(s.tag) + "' appears twice", false;
    out->sections.push_back(s);
  }
  if (fnv1a64(p + kHeaderBytes, (uint64_t)bytes - kHeaderBytes) != out->checksum)
    return *err = "generator file: checksum mismatch (corrupted payload)", false;

  const Section* sm = find_section(*out, kTagMeta);
  const Section* sr = find_section(*out, kTagRevNorm);
  const Section* su = find_section(*out, kTagUnet);
  const Section* sus = find_section(*out, kTagUnetSampler);
  const Section* sg = find_section(*out, kTagGeom);
  if (v2 && !sg) return *err = "generator file: format version 2 must have a GEOM section (a version-1 payload under a version-2 header?)", false;
  if (!v2 && sg) return *err = "generator file: a GEOM section in a format version " + std::to_string(out->version) + " file", false;
  const Section* sd = find_section(*out, kTagRadial);
  if (v3 && !sd) return *err = "generator file: format version 3 must have a RADL section (another version's payload under a version-3 header?)", false;
  if (!v3 && sd) return *err = "generator file: a RADL section in a format version " + std::to_string(out->version) + " file", false;
  if (!sm || !sr || !su || !sus) return *err = "generator file: a required section (META, RNRM, UNET, USMP) is missing", false;
  if (sr->bytes < (v2 ? kRevNormGeomBytes : v3 ? kRevNormRadialBytes : kRevNormBytes)) return *err = "RNRM: section shorter than its record", false;
  if (sm->bytes < kMetaBytes) return *err = "META: section shorter than its record", false;

  Meta& m = out->meta;
  const unsigned char* q = p + sm->off;
  m.data_ndim = rd<int32_t>(q);
  for (int i = 0; i < 4; ++i) m.data_shape[i] = rd<int32_t>(q + 4 + 4 * i);
  int32_t* mf[7] = {&m.cond_size, &m.energy_cols, &m.has_layer_stage, &m.takes_layers, &m.sample_steps, &m.layer_steps, &m.sample_offset};
  for (int i = 0; i < 7; ++i) *mf[i] = rd<int32_t>(q + 20 + 4 * i);
  m.seed = rd<uint64_t>(q + 48);
  m.layer_dim = rd<int32_t>(q + 56);
  memcpy(m.config_name, q + 64, 64);
  m.config_name[64] = 0;

  RevNorm& r = out->rev;
  q = p + sr->off;
  for (int i = 0; i < 3; ++i) r.dims[i] = rd<int32_t>(q + 4 * i);
  r.layer_map = rd<int32_t>(q + 12); r.logE = rd<int32_t>(q + 16); r.dataset_num = rd<int32_t>(q + 20);
  for (int i = 0; i < 6; ++i) r.consts[i] = rd<float>(q + 24 + 4 * i);
  r.max_deposit = rd<float>(q + 48); r.ecut = rd<float>(q + 52);
  r.emax = rd<double>(q + 56); r.emin = rd<double>(q + 64);

  if (v2) {
    r.energy_cols = rd<int32_t>(q + 80);
    r.alpha = rd<float>(q + 88); r.layer_eps = rd<float>(q + 92);
    uint64_t need;
    if (r.energy_cols < 1 || r.energy_cols > kMaxEnergyCols || !mul_ok((uint64_t)r.energy_cols, 16, &need) ||
        !add_ok(need, kRevNormGeomBytes, &need) || need > sr->bytes)
      return *err = "RNRM: 1 to 8 energy columns, each with its EMAX and EMIN inside the section", false;
    for (int k = 0; k < r.energy_cols; ++k) {
      r.emax_col[k] = rd<double>(q + kRevNormGeomBytes + 8 * k);
      r.emin_col[k] = rd<double>(q + kRevNormGeomBytes + 8 * (r.energy_cols + k));
      if (!(r.emax_col[k] > r.emin_col[k]) || !std::isfinite(r.emax_col[k]) || !std::isfinite(r.emin_col[k]))
        return *err = "RNRM: EMAX must exceed EMIN in every energy column", false;
    }
    if (r.emax != r.emax_col[0] || r.emin != r.emin_col[0]) return *err = "RNRM: EMAX / EMIN are not column 0 of their lists", false;
    if (!(r.alpha >= 0.f) || !(r.alpha < 0.5f) || !(r.layer_eps >= 0.f) || !std::isfinite(r.layer_eps))
      return *err = "RNRM: the staged constants (alpha, layer eps) are out of range", false;
    if (m.energy_cols != r.energy_cols) return *err = "META: energy_cols disagrees with the RNRM record", false;
    if (!parse_geom(p + sg->off, sg->bytes, &out->geom, err)) return false;
  } else {
    r.energy_cols = 1;
    r.emax_col[0] = r.emax; r.emin_col[0] = r.emin;
  }
  if (v3) {
    for (int i = 0; i < 6; ++i) {
      r.consts64[i] = rd<double>(q + kRevNormBytes + 8 * i);
      if (!std::isfinite(r.consts64[i])) return *err = "RNRM: a constant of the Dataset-0/1 map is not finite", false;
    }
    if (r.consts64[1] == 0 || r.consts64[3] == 0 || r.consts64[5] == 0) return *err = "RNRM: a scale of the Dataset-0/1 map is 0", false;
    if (!std::isfinite(r.ecut) || r.ecut < 0) return *err = "RNRM: ECUT must be finite and not negative", false;
    if (!parse_radial(p + sd->off, sd->bytes, &out->radial, err)) return false;
  }

  // the records against each other
  uint64_t vox = 1;
  for (int i = 0; i < 3; ++i) {
    if (r.dims[i] < 1 || r.dims[i] > 65536) return *err = "RNRM: grid dimension out of range", false;
    vox *= (uint64_t)r.dims[i];
  }
  if (vox > (1ull << 28)) return *err = "RNRM: more than 2^28 voxels", false;
  const Geom& g = out->geom;
  if (v2 && (g.layers != r.dims[0] || g.alpha != r.dims[1] || g.r != r.dims[2])) return *err = "GEOM: its bins are not the RNRM grid", false;
  const Radial& rad = out->radial;
  if (v3 && (rad.layers != r.dims[0] || rad.alpha_out != r.dims[1] || rad.r_out != r.dims[2])) return *err = "RADL: its grid is not the RNRM grid", false;
  if (v3 && rad.form == 0 && r.layer_map)
    return *err = "RNRM: a 'layer' map on the converted Dataset-0/1 grid is not provided (cd_reverse_norm_ds1's grid form takes no layer energies)", false;
  if (v2 && g.form == 1) {
    if (m.data_ndim != 3 || m.data_shape[0] != 1 || m.data_shape[1] != g.layers || m.data_shape[2] != g.cells || m.data_shape[3] != 0)
      return *err = "META: the data shape of an in-model file is not (1, L, N) of its GEOM section", false;
  } else if (v3 && rad.form == 1) {
    if (m.data_ndim != 1 || m.data_shape[0] != rad.voxels || m.data_shape[1] != 0 || m.data_shape[2] != 0 || m.data_shape[3] != 0)
      return *err = "META: the data shape of an in-model Dataset-0/1 file is not (V,) of its RADL section", false;
  } else if (m.data_ndim != 4 || m.data_shape[0] != 1 || m.data_shape[1] != r.dims[0] || m.data_shape[2] != r.dims[1] || m.data_shape[3] != r.dims[2]) {
    return *err = "META: the data shape is not (1, D, H, W) of the RNRM grid", false;
  }
  if (!v2 && m.energy_cols != 1) return *err = "META: one incident-energy column is the only form of format versions 1 and 3", false;
  if (m.sample_steps < 1 || m.sample_steps > (1 << 20) || m.sample_offset < 0 || m.layer_steps < 0 || m.layer_steps > (1 << 20))
    return *err = "META: step counts out of range", false;
  if ((m.takes_layers != 0) != (r.layer_map != 0)) return *err = "META: takes_layers disagrees with the shower map", false;
  if (m.takes_layers && m.layer_dim != r.dims[0] + 1) return *err = "META: layer_dim is not D + 1", false;
  if (m.cond_size != m.energy_cols + (m.takes_layers ? m.layer_dim : 0)) return *err = "META: conditioning width disagrees with the map", false;
  if (m.has_layer_stage && !m.takes_layers) return *err = "META: a layer stage needs a 'layer-' shower map", false;
  if (!(r.emax > r.emin) || (!v2 && r.logE && !(r.emin > 0)) || !(r.max_deposit > 0))
    return *err = "RNRM: EMAX must exceed EMIN (> 0 with logE) and MAXDEP must be positive", false;

  if (!parse_net(p + su->off, su->bytes, "UNET", true, &out->unet, err)) return false;
  if (out->unet.n_coord[0] != (uint32_t)r.dims[2] || out->unet.n_coord[1] != (uint32_t)r.dims[0] || out->unet.n_coord[2] != (uint32_t)r.dims[1])
    return *err = "UNET: coordinate profile lengths are not (W, D, H) of the grid", false;
  if (!parse_sampler(p + sus->off, sus->bytes, "USMP", &out->unet_sampler, err)) return false;
  const Section* sl = find_section(*out, kTagLayer);
  const Section* sls = find_section(*out, kTagLayerSampler);
  if (m.has_layer_stage) {
    if (!sl || !sls) return *err = "generator file: the layer stage's sections (LAYR, LSMP) are missing", false;
    if (!parse_net(p + sl->off, sl->bytes, "LAYR", false, &out->layer, err)) return false;
    if (!parse_sampler(p + sls->off, sls->bytes, "LSMP", &out->layer_sampler, err)) return false;
  } else if (sl || sls) {
    return *err = "generator file: layer sections in a file without a layer stage", false;
  }
  return true;
}

}  // namespace cdgen
