// HGCal geometry maps, the differentiable side (include/calodiff.h, "cd_geom_apply_vjp" and "cd_plan_set_geom"): the
// vector-Jacobian product of cd_geom_apply, and the forms a plan with HGCal's flat-state embedding launches around its U-Net --
// embed-in (enc of c_in x), embed-out (dec, the objective's combination, a sampler's fused update) and the two VJPs.
//
// Two kernels serve all of it.
//   gather  out[r, l, o] = sum_p val[p] in[r, l, idx[p]] over one line of a CSR-shaped view, a lane per output element as
//           geom_apply_kernel (ascending entries, one fmaf chain, no atomics; a row never sees another row).  Over the map's rows it
//           is the forward product (embed-in, embed-out); over the transposed view -- per column the rows ascending, each entry
//           naming its place in `val` -- it is the input gradient (dec's dF, enc's dx, cd_geom_apply_vjp's dx).  The EDM
//           preconditioning rides in its staging (c_in) and its epilogue, written as radial_collapse_kernel writes them.
//   wgrad   a thread per packed entry (l, i, j): dm[l, i, j] = sum_r gy[r, l, i] x[r, l, j] in plain ascending r, written into the
//           dense slot its launcher cleared.  Entries of a row are neighbours, so gy is a broadcast and x nearly coalesced.
#include "guarded.h"
#include "kernels_embed_head.h"
#include "kernels_geom.h"

namespace cd {
namespace {

enum { kPreNone = 0, kPreCin = 1, kPreDiv = 2, kPreAffine = 3 };
enum { kEpiNone = 0, kEpiDenoise = 1, kEpiDirect = 2 };

struct GeomGatherArgs {
  const int* ptr;    // layers * n_out + 1
  const int* idx;    // input index of every entry
  const int* pos;    // place of every entry in val, or null: the entry's own
  const float* val;
  const float* in;   // (batch, layers, n_in)
  float* out;        // (batch, layers, n_out)
  int layers, n_out, n_in, batch;
  int pre;           // kPreCin: in * c_in of its row (scal);  kPreDiv: in / div
  float div, out_mul;
  const float* scal;  // (batch, 4) {c_in, c_skip, c_out, sigma} of embed_kernel
  int epi, objective;
  const float* xflat;  // kEpiDenoise: the denoiser's input x;  kEpiDirect: the caller's cotangent gy
  const float* upd_stepvals;  // kEpiDenoise: the sampler update of head_kernel (HeadArgs::upd_*), on the flat state
  const float* upd_noise;
  float* upd_x_next;
  float* upd_xs;
  float* upd_x0s;
};

__global__ void __launch_bounds__(256) geom_gather_kernel(GeomGatherArgs a) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= a.n_out) return;
  for (int l = blockIdx.y; l < a.layers; l += gridDim.y) {
    const int lo = a.ptr[l * a.n_out + o], hi = a.ptr[l * a.n_out + o + 1];
    for (int b = blockIdx.z; b < a.batch; b += gridDim.z) {
      const float* xr = a.in + ((int64_t)b * a.layers + l) * a.n_in;
      const float c_in = a.pre == kPreCin ? a.scal[(size_t)b * 4] : 1.f;
      float acc = 0.f;
      for (int p = lo; p < hi; ++p) {
        float xv = xr[a.idx[p]];
        if (a.pre == kPreCin) xv = __fmul_rn(xv, c_in);  // the scaling first, then the product (x * scales['c_in'], then enc)
        else if (a.pre == kPreDiv) xv = __fdiv_rn(xv, a.div);
        acc = fmaf(a.val[a.pos ? a.pos[p] : p], xv, acc);
      }
      const int64_t i = ((int64_t)b * a.layers + l) * a.n_out + o;
      if (a.epi == kEpiDenoise) {  // head_kernel's combination and sampler update, acc in the place of the head's F
        const float xv = a.xflat[i];
        float pred = acc;
        if (a.objective == 0) pred = a.scal[b * 4 + 1] * xv + a.scal[b * 4 + 2] * pred;
        else if (a.objective == 1) pred = xv - a.scal[b * 4 + 3] * pred;
        a.out[i] = pred;
        if (a.upd_stepvals) {  // (DDim.__call__'s update: HeadArgs::upd_*)
          const float sigma = a.upd_stepvals[0], sprev = a.upd_stepvals[1], dsig = a.upd_stepvals[2], denom = a.upd_stepvals[3];
          const float eps = (xv - pred) / sigma;
          float r = pred + sprev * eps;
          if (a.upd_noise) r += dsig * a.upd_noise[i] / denom;
          a.upd_x_next[i] = r;
          if (a.upd_xs) a.upd_xs[i] = r;
          if (a.upd_x0s) a.upd_x0s[i] = pred;
        }
      } else if (a.epi == kEpiDirect) {  // init_dgrad_kernel's epilogue: acc carries c_in already
        a.out[i] = a.objective == 2 ? acc : fmaf(a.objective == 0 ? a.scal[b * 4 + 1] : 1.f, a.xflat[i], acc);
      } else {
        a.out[i] = __fmul_rn(acc, a.out_mul);
      }
    }
  }
}

struct GeomWgradArgs {
  const int* ent_row;  // l rows + i of every entry
  const int* col_idx;
  int nnz, layers, rows, cols, batch;
  const float* gy;     // (batch, layers, rows)
  const float* x;      // (batch, layers, cols)
  float* dm;           // (layers, rows, cols), cleared by the launcher
  int gpre;            // kPreDiv: gy / div
  float div;
  int xpre;            // kPreAffine: x * scale + shift
  float scale, shift;
};

__global__ void __launch_bounds__(256) geom_wgrad_kernel(GeomWgradArgs a) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= a.nnz) return;
  const int row = a.ent_row[p], l = row / a.rows, j = a.col_idx[p];
  const float* g = a.gy + row;
  const float* x = a.x + (int64_t)l * a.cols + j;
  const int64_t g_stride = (int64_t)a.layers * a.rows, x_stride = (int64_t)a.layers * a.cols;
  float acc = 0.f;
  for (int b = 0; b < a.batch; ++b) {
    float gv = g[b * g_stride], xv = x[b * x_stride];
    if (a.gpre == kPreDiv) gv = __fdiv_rn(gv, a.div);
    if (a.xpre == kPreAffine) xv = __fadd_rn(__fmul_rn(xv, a.scale), a.shift);
    acc = fmaf(gv, xv, acc);
  }
  a.dm[(int64_t)row * a.cols + j] = acc;
}

// over the map's rows (forward) or its transposed view (input gradient); everything else of `f` is the caller's
void gather_launch(const CdGeomMap* m, bool transposed, GeomGatherArgs f, const float* in, float* out, int64_t batch, hipStream_t s) {
  f.val = m->val; f.in = in; f.out = out; f.layers = m->layers; f.batch = (int)batch;
  if (transposed) {
    f.ptr = m->t_ptr; f.idx = m->t_row; f.pos = m->t_pos; f.n_out = m->cols; f.n_in = m->rows;
  } else {
    f.ptr = m->row_ptr; f.idx = m->col_idx; f.pos = nullptr; f.n_out = m->rows; f.n_in = m->cols;
  }
  const dim3 grid((unsigned)((f.n_out + 255) / 256), (unsigned)(m->layers < 65535 ? m->layers : 65535),
                  (unsigned)(batch < 65535 ? batch : 65535));
  hipLaunchKernelGGL(geom_gather_kernel, grid, dim3(256), 0, s, f);
  CD_HIP(hipGetLastError());
}

GeomGatherArgs plain_gather() {
  GeomGatherArgs f{};
  f.out_mul = 1.f; f.div = 1.f;
  return f;
}

void wgrad_launch(const CdGeomMap* m, GeomWgradArgs w, const float* gy, const float* x, float* dm, int batch, hipStream_t s) {
  CD_HIP(hipMemsetAsync(dm, 0, sizeof(float) * (size_t)m->layers * m->rows * m->cols, s));
  if (m->nnz == 0) return;
  w.ent_row = m->ent_row; w.col_idx = m->col_idx; w.nnz = m->nnz; w.layers = m->layers; w.rows = m->rows; w.cols = m->cols;
  w.batch = batch; w.gy = gy; w.x = x; w.dm = dm;
  hipLaunchKernelGGL(geom_wgrad_kernel, dim3((unsigned)((m->nnz + 255) / 256)), dim3(256), 0, s, w);
  CD_HIP(hipGetLastError());
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------
// The forms of a plan with HGCal's flat-state embedding (forward.hip, train.hip through launch_embed_*)
// ------------------------------------------------------------------------------------------------------------
void geom_embed_in(const CdGeomMap* enc, const float* x, const float* scal, float* g, int batch, hipStream_t s) {
  GeomGatherArgs f = plain_gather();
  f.pre = kPreCin; f.scal = scal;
  gather_launch(enc, false, f, x, g, batch, s);
}

void geom_embed_out(const CdGeomMap* dec, const float* F, const float* x, const float* scal, int objective, float* out,
                    const HeadArgs* upd, int batch, hipStream_t s) {
  GeomGatherArgs f = plain_gather();
  f.scal = scal; f.epi = kEpiDenoise; f.objective = objective; f.xflat = x;
  if (upd && upd->upd_stepvals) {
    CD_REQUIRE(upd->upd_x_next, "embed-out: the fused sampler update needs x_next");
    f.upd_stepvals = upd->upd_stepvals; f.upd_noise = upd->upd_noise; f.upd_x_next = upd->upd_x_next;
    f.upd_xs = upd->upd_xs; f.upd_x0s = upd->upd_x0s;
  }
  gather_launch(dec, false, f, F, out, batch, s);
}

void geom_embed_dec_vjp(const CdGeomMap* dec, const float* F, const float* gf, float* dF, float* dd, int batch, hipStream_t s) {
  gather_launch(dec, true, plain_gather(), gf, dF, batch, s);
  if (dd) wgrad_launch(dec, GeomWgradArgs{}, gf, F, dd, batch, s);
}

void geom_embed_enc_vjp(const CdGeomMap* enc, const float* x, const float* dg, const float* gy, const float* scal, int objective,
                        float* dx, float* dw, int batch, hipStream_t s) {
  if (gy) {  // (training: the input is data, no input gradient is wanted)
    GeomGatherArgs f = plain_gather();
    f.scal = scal; f.epi = kEpiDirect; f.objective = objective; f.xflat = gy;
    gather_launch(enc, true, f, dg, dx, batch, s);
  }
  if (dw) wgrad_launch(enc, GeomWgradArgs{}, dg, x, dw, batch, s);  // (enc's input was c_in x, and dg carries that c_in)
}

}  // namespace cd

extern "C" {

int cd_geom_apply_vjp(const CdGeomMap* map, const float* x, const float* gy, float* dx, float* dm, int batch_rows, float scale,
                      float shift, int affine_first, void* stream) {
  return guarded([&] {
    CD_REQUIRE(map && gy && batch_rows > 0 && (dx || dm), "bad argument");
    CD_REQUIRE(!dm || x, "cd_geom_apply_vjp: the map's gradient needs the forward's input x");
    CD_REQUIRE(scale != 0.f, "cd_geom_apply_vjp: scale (embed_std) must not be 0");
    CD_REQUIRE(!dx || map->t_ptr, "cd_geom_apply_vjp: the map was created without its transposed view (CD_GEOM_TRANSPOSED)");
    const bool plain = scale == 1.f && shift == 0.f;  // cd_geom_apply's choice of the plain product
    if (dx) {
      GeomGatherArgs f = plain_gather();
      if (!plain && !affine_first) { f.pre = kPreDiv; f.div = scale; }
      if (!plain && affine_first) f.out_mul = scale;
      gather_launch(map, true, f, gy, dx, batch_rows, (hipStream_t)stream);
    }
    if (dm) {
      GeomWgradArgs w{};
      if (!plain && !affine_first) { w.gpre = kPreDiv; w.div = scale; }
      if (!plain && affine_first) { w.xpre = kPreAffine; w.scale = scale; w.shift = shift; }
      wgrad_launch(map, w, gy, x, dm, batch_rows, (hipStream_t)stream);
    }
  });
}

}  // extern "C"
