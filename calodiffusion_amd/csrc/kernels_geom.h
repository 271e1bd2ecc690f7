// The geometry maps between flat showers and the U-Net's grid -- Dataset 1's radial matrices (kernels_radial.hip) and HGCal's
// packed maps (kernels_geom.hip) -- and the launches of a plan's flat-state embedding (kernels_radial.hip, kernels_geom_embed.hip).
#pragma once
#include "cd_common.h"

// Layout of one Dataset-1 geometry (cd_radial_create, kernels_radial.hip)
struct CdRadialMap {
  int layers = 0, A = 0, R = 0, V = 0, wtotal = 0;
  int4* lay = nullptr;  // device, per layer {bound, alpha, rin, float offset of its matrix}
  int* vlay = nullptr;  // device, layer of every voxel
  ~CdRadialMap() {
    if (lay) (void)hipFree(lay);
    if (vlay) (void)hipFree(vlay);
  }
};

// One packed HGCal map (cd_geom_create*, kernels_geom.hip).  row_ptr / col_ptr / t_ptr run over all layers: row i of layer l
// holds entries [row_ptr[l rows + i], row_ptr[l rows + i + 1])
struct CdGeomMap {
  int layers = 0, rows = 0, cols = 0, nnz = 0;
  bool masked = false;     // the pattern is a mask (a trainable map), not the values != 0
  int* row_ptr = nullptr;  // layers * rows + 1
  int* col_idx = nullptr;  // nnz, ascending within a row
  float* val = nullptr;
  int* ent_row = nullptr;  // nnz: l rows + i of every entry
  int* col_ptr = nullptr;  // layers * cols + 1, or null: no column view
  int* row_idx = nullptr;  // entries > SPARSE_EPS, ascending within a column
  float* cval = nullptr;
  int* t_ptr = nullptr;    // layers * cols + 1, or null: no transposed view
  int* t_row = nullptr;    // nnz: all entries, rows ascending within a column
  int* t_pos = nullptr;    // nnz: the entry's place in col_idx / val
  ~CdGeomMap() {
    for (void* p : {(void*)row_ptr, (void*)col_idx, (void*)val, (void*)ent_row, (void*)col_ptr, (void*)row_idx, (void*)cval,
                    (void*)t_ptr, (void*)t_row, (void*)t_pos})
      if (p) (void)hipFree(p);
  }
};

namespace cd {

struct HeadArgs;  // kernels_embed_head.h: the fused sampler update of *_embed_out

// The launches of a plan's flat-state embedding around its U-Net, one set per kind (kernels_radial.hip, kernels_geom_embed.hip).
// scal: (B, 4) of launch_embed
void radial_embed_in(const CdRadialMap* m, const float* enc_w, const float* x, const float* scal, float* g, int batch, hipStream_t s);
void radial_embed_out(const CdRadialMap* m, const float* dec_w, const float* F, const float* x, const float* scal, int objective,
                      float* out, const HeadArgs* upd, int batch, hipStream_t s);
void radial_embed_dec_vjp(const CdRadialMap* m, const float* dec_w, const float* F, const float* gf, float* dF, float* dd, int batch,
                          hipStream_t s);
void radial_embed_enc_vjp(const CdRadialMap* m, const float* enc_w, const float* x, const float* dg, const float* gy,
                          const float* scal, int objective, float* dx, float* dw, int batch, hipStream_t s);
void geom_embed_in(const CdGeomMap* enc, const float* x, const float* scal, float* g, int batch, hipStream_t s);
void geom_embed_out(const CdGeomMap* dec, const float* F, const float* x, const float* scal, int objective, float* out,
                    const HeadArgs* upd, int batch, hipStream_t s);
void geom_embed_dec_vjp(const CdGeomMap* dec, const float* F, const float* gf, float* dF, float* dd, int batch, hipStream_t s);
void geom_embed_enc_vjp(const CdGeomMap* enc, const float* x, const float* dg, const float* gy, const float* scal, int objective,
                        float* dx, float* dw, int batch, hipStream_t s);
// gf (B, V), the cotangent of dec(F): from the loss (gy null; x0, data, noise) or from a caller's cotangent gy of the output
void launch_embed_cotangent(const float* x0, const float* data, const float* noise, const float* gy, const float* scal, float* gf,
                            int batch, int64_t per, int loss_type, int objective, hipStream_t s);

}  // namespace cd
