// A geometric series of scalars times n points: out[i] = (first * ratio^(start + i) mod r) * P_i
// (dg16_points_mul_series) and, on top of it, phase 1 of the key ceremony: one contribution to a powers-of-tau
// transcript (dg16_srs_contribute) and the decision whether one transcript is a contribution to another
// (dg16_srs_verify_contribution).
//
//   products   the n independent products k_i P_i are points_mul.h's: every lane holds another scalar, which is what its
//              regular windows and its per-lane recoding are for.  Nothing of that loop is repeated here.
//   scalars    NEW on the device: the k_i never exist on the host.  series_kernel writes a slice's terms in Montgomery
//              form straight into the workspace slot points_mul_run reads (mode bit 0 = Montgomery scalars), so the call
//              uploads 64 bytes of scalars whatever n is.
//   chunks     a lane owns kChunk consecutive exponents: it raises ratio to the first of them by square and multiply
//              over the 64 bits of the exponent (term) and multiplies on from there (fill_chunk).  kChunk = 16: at most
//              127 + 16 field products per 16 terms, about nine per term, against the roughly 330 GROUP operations of the
//              product the term feeds.  Fusing the series into points_mul_kernel would save one 32-byte read per product.
//   exponents  the exponent of element i of the slice that starts at lo is start + lo + i, a full 64-bit number: slices
//              (SlicePlan) and chunks carry it as uint64_t, and the C entry point refuses a start + n that wraps.
//   edge cases ratio = 0: pow_u64(0) is one, so the term of exponent 0 is `first` and every other term is 0 (the
//              identity); first = 0: all identities; ratio = 1: every term is `first`.
//   slices     of the size dg16_ctx_set_points_mul_slice sets, by slices.h's rule (slice_lanes): the device copy of
//              a slice's points (slot 2) and its scalars (slot 1) come from channel 0's workspace; points_mul_run adds
//              its slots 20 .. 22.
//
// The term function, the chunk loop and the slice plan are host and device text: tests/host_arith/host_points_series.cpp
// runs them on a CPU against Python's pow().  The decision function of dg16_srs_verify_contribution is with the
// transcript verifier's, in points_check.h.
//
// Out of scope: the contribution hashes and the hash-to-G2 of a challenge (host work, the caller's protocol), a .ptau
// reader, and device-pointer forms of these calls.
#pragma once
#include "points_scale.h"

namespace dg16 {
namespace pseries {

constexpr unsigned kChunk = 16;     // consecutive exponents per lane

// stored words below r (a canonical integer; zero included)
template <class Fr>
DG_HD bool below_modulus(const Fr& x) {
  for (int i = Fr::NL - 1; i >= 0; i--)
    if (x.l[i] != Fr::Params::P[i]) return x.l[i] < Fr::Params::P[i];
  return false;
}

// first * ratio^e, all three in Montgomery form; ratio^0 = 1 also for ratio = 0
template <class Fr>
DG_HD Fr term(const Fr& first_m, const Fr& ratio_m, uint64_t e) {
  return first_m * ratio_m.pow_u64(e);
}

// out[j] = first * ratio^(e0 + j), j < cnt: one power, then cnt - 1 products
template <class Fr>
DG_HD void fill_chunk(const Fr& first_m, const Fr& ratio_m, uint64_t e0, unsigned cnt, Fr* out) {
  Fr v = term(first_m, ratio_m, e0);
  for (unsigned j = 0; j < cnt; j++) {
    out[j] = v;
    v = v * ratio_m;
  }
}

// slice `index` of a call over n points: elements [lo, lo + cnt), the exponent of its first element, its chunks
struct SlicePlan {
  size_t lo, cnt;
  uint64_t exp0;
  size_t chunks;
};
using dg16::round_slice;      // (slices.h's, under the names the plan has been tested by)
using dg16::slice_count;
// slice: a multiple of 64 (slices.h: slice_lanes); start + n does not wrap
DG_HD SlicePlan plan_slice(size_t n, size_t slice, uint64_t start, size_t index) {
  SlicePlan p;
  p.lo = index * slice;
  p.cnt = n - p.lo < slice ? n - p.lo : slice;
  p.exp0 = start + (uint64_t)p.lo;
  p.chunks = (p.cnt + kChunk - 1) / kChunk;
  return p;
}
// chunk c of a slice: elements [i0, i0 + len) of the slice
DG_HD size_t chunk_begin(size_t c) { return c * kChunk; }
DG_HD unsigned chunk_len(const SlicePlan& p, size_t c) {
  const size_t left = p.cnt - chunk_begin(c);
  return left < kChunk ? (unsigned)left : kChunk;
}

}  // namespace pseries
}  // namespace dg16

#if defined(__HIPCC__)
// ---- device side ----------------------------------------------------------------------------------------------------------
#include <string.h>

namespace dg16 {
namespace pseries {

// out[i] = first * ratio^(exp0 + i) (Montgomery), i < cnt; one chunk per lane
template <class Fr>
__global__ void __launch_bounds__(64) series_kernel(Fr* __restrict__ out, SlicePlan p, Fr first_m, Fr ratio_m) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= p.chunks) return;
  const size_t i0 = chunk_begin(c);
  fill_chunk(first_m, ratio_m, p.exp0 + (uint64_t)i0, chunk_len(p, c), out + i0);
}

// out_host[i] = (first * ratio^(start + i)) * points_host[i] (affine); out_host may be points_host.  first8, ratio8:
// canonical integers below r (the caller checked them).  Workspace slots of channel 0: 1 (the slice's scalars), 2 (its
// points, then its products) and those of points_mul_run.
template <int CURVE>
void points_series_curve(Call& k, int group, const void* points_host, size_t n, const uint32_t* first8,
                         const uint32_t* ratio8, uint64_t start, void* out_host, bool in_subgroup) {
  if (!n) return;
  using Fr = typename CurveTypes<CURVE>::Fr;
  static_assert(sizeof(Fr) == 32, "scalar size");
  Fr first, ratio;
  memcpy(&first, first8, 32);
  memcpy(&ratio, ratio8, 32);
  const Fr first_m = first.to_mont(), ratio_m = ratio.to_mont();
  const size_t slice = slice_lanes(k.ctx->points_mul_slice), stride = launch_stride(n, slice);
  const size_t pb = affine_bytes(CURVE, group);
  Fr* scal = (Fr*)ws(k.c, 1, stride * sizeof(Fr));
  char* pts = (char*)ws(k.c, 2, stride * pb);
  const unsigned mode = 1u | (in_subgroup ? 2u : 0u);      // Montgomery scalars; the split rule of dg16_msm
  for (size_t s = 0, ns = slice_count(n, slice); s < ns; s++) {
    const SlicePlan p = plan_slice(n, slice, start, s);
    // the scalars first: the kernel is one serial chain of about forty field products per lane (35 us measured at 2^14
    // terms) and can run while the host stages the copy of the points behind it.  (Both are ordered behind the previous
    // slice's kernels on the stream.)
    hipLaunchKernelGGL(series_kernel<Fr>, dim3((unsigned)((p.chunks + 63) / 64)), dim3(64), 0, k.s(), scal, p, first_m,
                       ratio_m);
    DG_HIP(hipGetLastError());
    DG_HIP(hipMemcpyAsync(pts, (const char*)points_host + p.lo * pb, p.cnt * pb, hipMemcpyHostToDevice, k.s()));
    points_mul_run<CURVE>(k, group, pts, scal, p.cnt, mode, pts);
    DG_HIP(hipMemcpyAsync((char*)out_host + p.lo * pb, pts, p.cnt * pb, hipMemcpyDeviceToHost, k.s()));
  }
  DG_HIP(hipStreamSynchronize(k.s()));
}

}  // namespace pseries

// host pointers; first8, ratio8: canonical integers below r
template <int CURVE>
void points_series_run(Call& k, int group, const void* points_host, size_t n, const uint32_t* first8,
                       const uint32_t* ratio8, uint64_t start, void* out_host, bool in_subgroup);
// (defined in the per-curve objects points_series_<curve>.o)
template <> void points_series_run<0>(Call&, int, const void*, size_t, const uint32_t*, const uint32_t*, uint64_t, void*, bool);
template <> void points_series_run<1>(Call&, int, const void*, size_t, const uint32_t*, const uint32_t*, uint64_t, void*, bool);
template <> void points_series_run<2>(Call&, int, const void*, size_t, const uint32_t*, const uint32_t*, uint64_t, void*, bool);

}  // namespace dg16
#endif
