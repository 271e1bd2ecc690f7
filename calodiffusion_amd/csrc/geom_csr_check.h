// The invariants of a geometry map given by its sparse entries (per-layer CSR over layers * rows lines), checked on the host
// before anything is uploaded: cd_geom_create_csr (kernels_geom.hip) and the generator file's reader (generator_blob.h) share
// this loop.  Pure C++17, no HIP.  The arrays are read as little-endian bytes (a file's may be unaligned).
#pragma once
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <string>

namespace cdgeom {

constexpr int64_t kMaxLines = (int64_t)1 << 30;  // layers * max(rows, cols): cd_geom_create's limit

// row_ptr: layers * rows + 1 int32; col_idx: nnz int32; val: nnz fp32.  row_ptr[0] == 0, non-decreasing, last == nnz; columns
// strictly ascending within a row and < cols; values finite.  Entries whose value is 0 are allowed (a mask's pattern).
inline bool csr_valid(const unsigned char* row_ptr, const unsigned char* col_idx, const unsigned char* val, int64_t layers,
                      int64_t rows, int64_t cols, int64_t nnz, std::string* err) {
  auto i32 = [](const unsigned char* p, int64_t i) {
    int32_t v;
    memcpy(&v, p + 4 * i, 4);
    return v;
  };
  if (layers < 1 || rows < 1 || cols < 1 || layers * (rows > cols ? rows : cols) > kMaxLines || layers * rows * cols > INT32_MAX)
    return *err = "geometry map: layers, rows, cols must be positive, layers * max(rows, cols) within 2^30 and layers * rows * cols below 2^31", false;
  if (nnz < 0 || nnz > INT32_MAX) return *err = "geometry map: entry count out of range", false;
  const int64_t lines = layers * rows;
  if (i32(row_ptr, 0) != 0) return *err = "geometry map: row_ptr[0] is not 0", false;
  if (i32(row_ptr, lines) != nnz)
    return *err = "geometry map: row_ptr ends at " + std::to_string(i32(row_ptr, lines)) + ", the entry count is " + std::to_string(nnz), false;
  int64_t lo = 0;
  for (int64_t r = 0; r < lines; ++r) {  // the whole of row_ptr first: no column is read through a bad range
    const int64_t hi = i32(row_ptr, r + 1);
    if (hi < lo || hi > nnz) return *err = "geometry map: row_ptr is not non-decreasing at line " + std::to_string(r), false;
    lo = hi;
  }
  lo = 0;
  for (int64_t r = 0; r < lines; ++r) {
    const int64_t hi = i32(row_ptr, r + 1);
    int64_t prev = -1;
    for (int64_t p = lo; p < hi; ++p) {
      const int64_t c = i32(col_idx, p);
      if (c < 0 || c >= cols)
        return *err = "geometry map: column " + std::to_string(c) + " of entry " + std::to_string(p) + " is outside [0, " + std::to_string(cols) + ")", false;
      if (c <= prev) return *err = "geometry map: columns are not strictly ascending in line " + std::to_string(r), false;
      prev = c;
    }
    lo = hi;
  }
  for (int64_t p = 0; p < nnz; ++p) {
    float v;
    memcpy(&v, val + 4 * p, 4);
    if (!std::isfinite(v)) return *err = "geometry map: the value of entry " + std::to_string(p) + " is not finite", false;
  }
  return true;
}

}  // namespace cdgeom
