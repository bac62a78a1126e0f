// The slice rule of every "n points times something" call: dg16_points_mul, dg16_points_scale, dg16_points_mul_series,
// dg16_group_ntt, dg16_pss_pack_points and dg16_points_check cut their work into launches of at most
// dg16_ctx_set_points_mul_slice lanes, so the per-lane workspace of a launch (for the products: a table of 8 XYZZ) is
// bounded whatever n is.  Host and device text; nothing here but integers.
#pragma once
#include <stddef.h>

#ifndef DG_HD      // fp.h's idiom, word for word; under hipcc the includer brings the HIP runtime header (fp.h does)
#if defined(__HIPCC__)
#define DG_HD __host__ __device__ __forceinline__
#else
#define DG_HD inline
#endif
#endif

namespace dg16 {

constexpr size_t kSliceDefault = (size_t)1 << 16;   // lanes per launch where the context sets none

DG_HD size_t round_slice(size_t v) { return (v + 63) / 64 * 64; }
// lanes per launch under the context's setting: 0 = the default; rounded up to whole waves
DG_HD size_t slice_lanes(size_t ctx_slice) { return round_slice(ctx_slice ? ctx_slice : kSliceDefault); }
// lanes of the largest launch of a call over n lanes: what its workspace is sized for and the stride of its tables
DG_HD size_t launch_stride(size_t n, size_t slice) { return n < slice ? round_slice(n) : slice; }
DG_HD size_t slice_count(size_t n, size_t slice) { return (n + slice - 1) / slice; }

}  // namespace dg16
