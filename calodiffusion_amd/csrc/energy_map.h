// The incident-energy map between physical units and the conditioning value e, one device function per direction, shared by
// cd_preprocess (kernels_preprocess.hip), cd_preprocess_hgcal (kernels_geom.hip) and the generator's conditioning kernel (generator.hip) so that their bits agree.
#pragma once
#include <hip/hip_runtime.h>

namespace cd {

// DataLoaderCaloChall's map (calodiffusion/utils/utils.py:307-310): float32 quotient and float32 log10, divided by the python float
// log10(emax / emin); or the linear form.
__device__ __forceinline__ float energy_to_cond(float e, float emin, float emax, int logE) {
  if (logE) return (float)((double)(float)log10((double)(e / emin)) / log10((double)emax / (double)emin));
  return (e - emin) / (emax - emin);
}

// Its inverse as ReverseNormCaloChall forms it on float32 arrays (utils.py:480-483): emin * (emax / emin) ** e, or
// emin + (emax - emin) * e.  base = (float)(emax / emin) and span = (float)(emax - emin), both formed in double on the host as
// python forms them.  The power is the correctly rounded float32 value (taken in double, rounded once); products and sums are
// rounded one by one, nothing fused.
__device__ __forceinline__ float cond_to_energy(float e, float emin, float base, float span, int logE) {
  if (logE) return __fmul_rn(emin, (float)pow((double)base, (double)e));
  return __fadd_rn(emin, __fmul_rn(span, e));
}

// HGCal: DataLoaderHGCal's per-column map (calodiffusion/utils/HGCal_utils.py:131-132, 158), np.array(emin) being float64: a
// double computation rounded once.  Shared by cd_preprocess_hgcal (kernels_geom.hip) and the generator's conditioning kernel.
__device__ __forceinline__ float energy_to_cond_hgcal(float e, double emin, double emax) {
  return (float)(((double)e - emin) / (emax - emin));
}

// The physical energy ReverseNormHGCal scales by (HGCal_utils.py:195-199): emin + (emax - emin) * e on float64 arrays, rounded to
// float32 at the end.  span = emax - emin formed in double on the host; product and sum are rounded one by one, nothing fused.
__device__ __forceinline__ float cond_to_energy_hgcal(float e, double emin, double span) {
  return (float)__dadd_rn(emin, __dmul_rn(span, (double)e));
}

}  // namespace cd
