// Per-curve object of the one-scalar point multiplication (points_scale.h): points_scale_kernel for G1 and G2 of curve
// DG_CURVE, plain and split.
#include "points_scale.h"

#ifndef DG_CURVE
#error "compile with -DDG_CURVE=<curve id>"
#endif

namespace dg16 {

template <>
void points_scale_run<DG_CURVE>(Call& k, int group, const void* points_host, const uint32_t* scalar8, size_t n,
                                void* out_host, bool in_subgroup) {
  using CT = CurveTypes<DG_CURVE>;
  if (group == 1) pscale::points_scale_typed<CT::Fq>(k, points_host, scalar8, n, out_host, in_subgroup);
  else pscale::points_scale_typed<CT::Fq2>(k, points_host, scalar8, n, out_host, in_subgroup);
}

}  // namespace dg16
