// Per-curve object of the series multiplication (points_series.h): series_kernel over the scalar field of curve
// DG_CURVE and the slice loop that feeds points_mul_run of the same curve.
#include <string.h>

#include "points_series.h"

#ifndef DG_CURVE
#error "compile with -DDG_CURVE=<curve id>"
#endif

namespace dg16 {

template <>
void points_series_run<DG_CURVE>(Call& k, int group, const void* points_host, size_t n, const uint32_t* first8,
                                 const uint32_t* ratio8, uint64_t start, void* out_host, bool in_subgroup) {
  pseries::points_series_curve<DG_CURVE>(k, group, points_host, n, first8, ratio8, start, out_host, in_subgroup);
}

}  // namespace dg16
