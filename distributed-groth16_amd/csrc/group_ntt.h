// Radix-2 transform over GROUP elements (dg16_group_ntt) and, on top of it, the preparation of a reference string from
// the monomial powers of a ceremony (dg16_srs_prepare): arkworks' Radix2EvaluationDomain::{fft, ifft} on a Vec<G>,
// snarkjs' `powersoftau prepare phase2`.
//
//   schedule   constant geometry, decimation in time.  Stage s = 1 .. k of a transform of n = 2^k points has n / 2 lanes;
//              lane j reads the pair (2j, 2j + 1) of the stage's source -- in stage 1 the pair (rev(j), rev(j) + n / 2)
//              of the caller's array, rev the reversal of k - 1 bits, which is the bit-reversed load of a decimation in
//              time -- and writes a + w b to j and a - w b to j + n / 2 of the stage's destination, w = w_n^e with
//              e = (j >> (k - s)) << (k - s).  After stage s position (t << (k - s)) | g holds frequency t of the
//              size-2^s transform of the inputs g, g + 2^(k - s), ..: natural order after stage k.  Source and
//              destination alternate between two buffers; a lane writes only what belongs to it.
//   launches   e = 0 exactly for the lanes j < n / 2^s: they come FIRST in every stage and run in an add/sub launch of
//              their own (all of stage 1); the lanes from n / 2^s on multiply.  A wave never holds both kinds.
//   slices     each of the two lane ranges of a stage is cut into runs of at most `slice` lanes
//              (dg16_ctx_set_points_mul_slice; slices.h: slice_lanes, launch_stride): the table of a slice is 8 XYZZ per
//              lane, whatever n is.  The XYZZ results of a stage lie as the destination does (lane j's at j and
//              j + n / 2), so ONE launch of fixed_base_impl.h's batched inversion converts a whole stage in place.
//   butterfly  t = w b through pmul::product_split (every input is in the order-r subgroup by the call's contract, so the
//              split path is always taken where an endomorphism is wired), then a + t and a - t through the complete
//              addition law: a = w b, a = -w b and identity operands are ordinary inputs here (all points equal, one
//              point and identities, ..).
//   budget     multiplications: sum_s (n / 2 - n / 2^s) = (n / 2) k - (n - 1) for a forward transform; the inverse runs
//              the same stages with w^-1 and then one pass of n products by n^-1.
//
// The schedule and the butterfly are host and device text: tests/host_arith/host_group_ntt.cpp runs them on a CPU, on
// field elements and on points, through the Ops parameter, and counts.
#pragma once
#include <vector>

#include "points_mul.h"

namespace dg16 {
namespace gntt {

constexpr unsigned kMaxLog = 27;                     // dg16_ntt's limit

enum Launch : int { kAddSub = 0, kMul = 1 };

DG_HD size_t bit_reverse(size_t x, unsigned bits) {
  size_t r = 0;
  for (unsigned i = 0; i < bits; i++) {
    r = (r << 1) | (x & 1);
    x >>= 1;
  }
  return r;
}

// lane j of stage s: dst[lo] = src[a] + w_n^tw src[b], dst[hi] = src[a] - w_n^tw src[b]
struct Pair {
  size_t a, b, lo, hi, tw;
};
DG_HD Pair pair_of(unsigned log_n, unsigned s, size_t j) {
  const size_t half = (size_t)1 << (log_n - 1);
  Pair p;
  if (s == 1) {
    p.a = bit_reverse(j, log_n - 1);
    p.b = p.a + half;
  } else {
    p.a = 2 * j;
    p.b = 2 * j + 1;
  }
  p.lo = j;
  p.hi = j + half;
  p.tw = (j >> (log_n - s)) << (log_n - s);
  return p;
}
// the lanes [0, trivial_lanes) of stage s have w = 1
DG_HD size_t trivial_lanes(unsigned log_n, unsigned s) { return (size_t)1 << (log_n - s); }
DG_HD Launch launch_of(unsigned log_n, unsigned s, size_t j) { return j < trivial_lanes(log_n, s) ? kAddSub : kMul; }

using dg16::slice_lanes;      // (slices.h's, under the names the plan has been tested by)
using dg16::launch_stride;

struct Slice {      // lanes [lo, lo + cnt) of one stage, all of one kind
  Launch kind;
  size_t lo, cnt;
};
// the launches of stage s in order; slice from slices.h's slice_lanes()
inline std::vector<Slice> stage_slices(unsigned log_n, unsigned s, size_t slice) {
  std::vector<Slice> out;
  const size_t half = (size_t)1 << (log_n - 1), triv = trivial_lanes(log_n, s);
  for (size_t lo = 0; lo < triv; lo += slice) out.push_back(Slice{kAddSub, lo, triv - lo < slice ? triv - lo : slice});
  for (size_t lo = triv; lo < half; lo += slice) out.push_back(Slice{kMul, lo, half - lo < slice ? half - lo : slice});
  return out;
}
// the scaling pass of the inverse (and the twiddled pass of srs_prepare): n lanes, lane j multiplies element j
inline std::vector<Slice> scale_slices(size_t n, size_t slice) {
  std::vector<Slice> out;
  for (size_t lo = 0; lo < n; lo += slice) out.push_back(Slice{kMul, lo, n - lo < slice ? n - lo : slice});
  return out;
}
DG_HD size_t forward_products(unsigned log_n) {
  return log_n ? ((size_t)log_n << (log_n - 1)) - (((size_t)1 << log_n) - 1) : 0;
}

// The butterfly.  Ops names the element types and the group operations:
//   In, Out, Scalar;  Out lift(In);  Out mul(In, Scalar) (the product w b);  Out add(Out, Out);  Out neg(Out)
// combine() is its second half, for a caller that fetches a only after the product.
template <class Ops>
DG_HD void combine(Ops& ops, const typename Ops::In& a, const typename Ops::Out& t, typename Ops::Out* sum,
                   typename Ops::Out* diff) {
  const typename Ops::Out l = ops.lift(a);
  *sum = ops.add(l, t);
  *diff = ops.add(l, ops.neg(t));
}
template <class Ops>
DG_HD void butterfly(Ops& ops, const typename Ops::In& a, const typename Ops::In& b, const typename Ops::Scalar& w,
                     typename Ops::Out* sum, typename Ops::Out* diff) {
  combine(ops, a, ops.mul(b, w), sum, diff);
}
// a lane of the add/sub launch: w = 1
template <class Ops>
DG_HD void butterfly_trivial(Ops& ops, const typename Ops::In& a, const typename Ops::In& b, typename Ops::Out* sum,
                             typename Ops::Out* diff) {
  combine(ops, a, ops.lift(b), sum, diff);
}

// w^e (* scale) as a plain integer from a split power table in Montgomery form (ctx.h: TwiddleSet lo, hi, n_inv)
template <class Fr>
DG_HD Fr twiddle(const Fr* lo, const Fr* hi, unsigned lb, size_t e, const Fr* scale) {
  Fr w = lo[e & (((size_t)1 << lb) - 1)] * hi[e >> lb];
  if (scale) w = w * *scale;
  return w.from_mont();
}

// the group operations on points: affine in, XYZZ out, the products through points_mul.h's loops over table `Tab`
struct Words8 {
  uint32_t l[8];
};
template <class F, class Inner, class Tab>
struct PointOps {
  using In = Affine<F>;
  using Out = XYZZ<F>;
  using Scalar = Words8;
  Inner& inner;
  Tab& tab;
  DG_HD Out lift(const In& p) { return XYZZ<F>::from_affine(p); }
  DG_HD Out mul(const In& p, const Scalar& k) {
    if constexpr (GlvOf<F>::enabled) return pmul::product_split<F>(p, k.l, inner, tab);
    else return pmul::product_plain<F>(p, k.l, inner, tab);
  }
  DG_HD Out add(const Out& a, const Out& b) { return inner.add(a, b); }
  DG_HD Out neg(const Out& a) { return a.neg(); }
};

}  // namespace gntt
}  // namespace dg16

#if defined(__HIPCC__)
// ---- device side ----------------------------------------------------------------------------------------------------------
namespace dg16 {

// All pointers are device buffers of affine points of `group`.  (defined in the per-curve objects group_ntt_<curve>.o)
//
// x: 2^log_n points, y: as many (scratch).  Returns the one of the two that holds the transform; the other is clobbered.
// scale = false leaves the n^-1 of an inverse transform out.
template <int CURVE>
void* group_ntt_run(Call& k, int group, void* x, void* y, unsigned log_n, int inverse, bool scale);
// G1: out[j] = src[j + a_off] - src[j + b_off], j < n
template <int CURVE>
void group_diff_run(Call& k, const void* src, size_t a_off, size_t b_off, size_t n, void* out);
// G1: out[j] = (w_2m^-j / 2m) src[j], j < m = 2^log_m (the twiddled pass in front of the odd half of a size-2m inverse)
template <int CURVE>
void group_twist_run(Call& k, const void* src, unsigned log_m, void* out);
template <> void* group_ntt_run<0>(Call&, int, void*, void*, unsigned, int, bool);
template <> void* group_ntt_run<1>(Call&, int, void*, void*, unsigned, int, bool);
template <> void* group_ntt_run<2>(Call&, int, void*, void*, unsigned, int, bool);
template <> void group_diff_run<0>(Call&, const void*, size_t, size_t, size_t, void*);
template <> void group_diff_run<1>(Call&, const void*, size_t, size_t, size_t, void*);
template <> void group_diff_run<2>(Call&, const void*, size_t, size_t, size_t, void*);
template <> void group_twist_run<0>(Call&, const void*, unsigned, void*);
template <> void group_twist_run<1>(Call&, const void*, unsigned, void*);
template <> void group_twist_run<2>(Call&, const void*, unsigned, void*);

}  // namespace dg16
#endif
