// Pippenger MSM for gfx950 -- replaces `G::msm(bases, scalars)` at dist-primitives/src/dmsm/mod.rs:82 (ark-ec
// VariableBaseMSM).  Any correct algorithm yields the same group element; parity is checked in affine form.
//
// Pipeline (DESIGN.md section 2.2 has the table; MSM_INVARIANTS.md every array's size, writer and capacity):
//   1-3 sort        scalar -> W signed c-bit digits, counted and placed per (bucket-window, bucket) by a two-level LDS-
//                   partitioned counting sort (msm_part_*; the direct atomic path msm_digits / msm_scatter for small inputs)
//   4   accumulate  one lane per SEGMENT of a bucket: XYZZ mixed additions on the reduced-radix types -- THE dominant kernels,
//                   VALU-issue-bound (msm_accumulate_kernel / _lds_kernel / _steps_kernel)
//   4b  finalize    bucket = sum of its partials (in-workgroup tree + stitch for BN254 G1, throughput finalize otherwise;
//                   buckets with > 64 partials through the giant work list)
//   5   reduce      sum_b (b + 1) B_b per bucket-window: rows of 256 buckets, then one workgroup per window (msm_reduce_impl.h)
//   6   tail        Horner over the window sums on ONE wave (fresh bases only; resident tables have one bucket set)
// What was measured and removed on the way is in CHANGELOG.md, not here.
#pragma once
#include <atomic>
#include <chrono>
#include <utility>
#include <stdio.h>

#include "glv.h"
#include "bounds.h"
#include "ctx.h"
#include "ec29.h"
#include "lane29.h"
#include "types.h"

#include "msm_geom.h"              // host planning arithmetic (plain C++: tests/test_msm_geom_host.py)
#include "msm_sort.h"              // 1-3
#include "msm_accumulate.h"        // 4: kernels
#include "msm_accumulate_steps.h"  // 4: the 14-limb G2 step loop
#include "msm_accumulate_phase.h"  // 4: buffers and launch
#include "msm_chains.h"            // one-wave chains; 6: Horner tail
#include "msm_finalize.h"          // 4b
#include "msm_glv.h"               // plain MSM: GLV and msm_run
#include "msm_table.h"             // resident tables, synthetic bases

// Translation units that only CALL the MSM phases of a curve (the prover) declare them extern so that the kernels are
// compiled once, in msm_group.hip / msm_reduce.hip:  namespace dg16 { DG16_MSM_EXTERN(CurveTypes<0>) }
#define DG16_MSM_EXTERN_GROUP(F)                                                                                  \
  extern template void msm_accumulate_phase<F>(hipStream_t, const MsmSort&, const MsmBuffers<F>&, const void* const*); \
  extern template void msm_finalize_phase<F>(hipStream_t, const MsmSort&, const MsmBuffers<F>&);                   \
  extern template void msm_tail_phase<F>(hipStream_t, const MsmSort&, const MsmBuffers<F>&, bool, void*);         \
  extern template void* msm_build_table<F>(hipStream_t, const void*, size_t, unsigned, unsigned);
#define DG16_MSM_EXTERN(CT)                                                                                       \
  DG16_MSM_EXTERN_GROUP(CT::Fq)                                                                                   \
  DG16_MSM_EXTERN_GROUP(CT::Fq2)                                                                                  \
  extern template MsmSort msm_sort_on<CT::Fr, CT::SCALAR_BITS>(hipStream_t, Channel&, const void*, size_t, unsigned, bool, \
                                                              unsigned, unsigned);
