// Per-curve object of the share packing of point vectors (pss_pack.h): pss_pack_table_kernel and
// pss_pack_combine_kernel for G1 and G2 of curve DG_CURVE, plain and split.
#include "pss_pack.h"

#ifndef DG_CURVE
#error "compile with -DDG_CURVE=<curve id>"
#endif

namespace dg16 {

template <>
void pss_pack_run<DG_CURVE>(Call& k, const dg16_pss* pp, int group, const void* points, size_t n_points, void* shares,
                            bool in_subgroup) {
  using CT = CurveTypes<DG_CURVE>;
  if (group == 1) ppack::pack_points_typed<CT::Fq>(k, pp, group, points, n_points, shares, in_subgroup);
  else ppack::pack_points_typed<CT::Fq2>(k, pp, group, points, n_points, shares, in_subgroup);
}

}  // namespace dg16
