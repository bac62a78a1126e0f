// One scalar, n points: out[i] = k * P_i (dg16_points_scale) and, on top of it, a phase-2 contribution to a Groth16 key
// (dg16_groth16_contribute: l_query and h_query times delta^-1).
//
//   why not points_mul.h   its regular windows, its dummy addition for a zero digit, its per-lane recoding and its table
//              of eight consecutive multiples exist because every lane holds another scalar.  Here every lane holds the
//              SAME one, so the digit stream is uniform over the wave -- over the whole launch -- and a sliding form
//              costs no divergence.
//   schedule   made on the host once per call (make_schedule): k is split with the group's endomorphism where the rule of
//              dg16_msm allows it (pmul::may_split: cofactor one, or the caller's in_subgroup), every part is recoded as a
//              width-w non-adjacent form (wnaf.h: recode_wnaf) -- digits odd or zero, |d| < 2^(w-1), two non-zero digits
//              at least w positions apart -- and the part's sign is folded into its digits.  One 32-bit word per position holds the signed
//              bytes of the (up to four) parts; the rows run from position 0 to the highest position that holds a
//              non-zero digit of any part.
//   loop       the kernel reads the row of a position at an address that depends on the position alone: a uniform load,
//              and every "is this digit zero" branch is uniform.  Per position ONE doubling and, for each part with a
//              non-zero digit, one addition of psi^j(T[|d|]), y negated for d < 0; the endomorphism is applied to the
//              table entry on the fly (GlvOf<F>::endo_xyzz), as in points_mul.h.  A zero position is a doubling and
//              nothing else: no dummy addition, no select.  The chain starts at the top row, so no identity is doubled.
//   table      the odd multiples P, 3P, .. (2^(w-1) - 1) P only: one doubling and 2^(w-2) - 1 additions (wnaf.h:
//              build_odd_table).
//   width      w = 5, by the count (density of a width-w NAF: one non-zero digit in w + 1 positions), table included:
//                 path      bits x parts   w = 4: additions      w = 5: additions      dg16_points_mul
//                 plain     255 x 1        3 + 255 / 5 = 54      7 + 255 / 6 = 49.5    67
//                 DIM = 2   127 x 2        3 + 254 / 5 = 53.8    7 + 254 / 6 = 49.3    67
//                 DIM = 4    66 x 4        3 + 264 / 5 = 55.8    7 + 264 / 6 = 51      71
//              w = 6 pays 15 table additions for 255 / 7 = 36.4: 51.4, no better, with twice the table.  At w = 5 the
//              table is eight entries, the size and the layout of points_mul.h's (pmul::GlobalTab), and the worst case
//              (a non-zero digit every w positions) is 7 + ceil(256 / 5) = 59 additions, 7 + 2 * 26 = 59, 7 + 4 * 14 = 63.
//   budget     doublings: 1 (table) + the top position: at most 256 / 128 / 68.
//   slices     of slices.h's rule, as dg16_points_mul's.
//   affine     the accumulators of a slice go through fixed_base_impl.h's batched inversion (fb_to_affine).
//
// Exceptional cases of the addition law.  All additions are XYZZ::add, which is complete (identity, equal and opposite
// operands); nothing is proven away.  They do occur: the accumulator is the identity until the first non-zero digit, an
// identity input makes every table entry the identity, k = r on a point of order r ends in (r - d) P + d P, and a point
// outside the subgroup (plain path) can meet its own multiples anywhere -- a point of order two already in the table.
//
// The schedule and the loops are host and device text: tests/host_arith/host_points_scale.cpp runs them on a CPU against
// the oracle and counts the group operations through the Ops parameter.
#pragma once
#include "points_mul.h"
#include "wnaf.h"

namespace dg16 {
namespace pscale {

constexpr int kWidth = 5;
constexpr int kTable = 1 << (kWidth - 2);      // entries 1P, 3P, .. 15P
using wnaf::kMaxRows;
using wnaf::row_digit;

// rows[i]: byte j = the signed digit of part j at position i (the part's sign folded in)
struct Schedule {
  int dim;                 // 1 (plain), 2 or 4
  int len;                 // rows; 0 for k = 0
  uint32_t rows[kMaxRows];
};

// k: 8 words, below 2^255.  split: use the group's endomorphism (the caller applied pmul::may_split)
template <class F>
inline void make_schedule(const uint32_t* k, bool split, Schedule& s) {
  int8_t dig[4][kMaxRows];
  s.dim = 1;
  s.len = 0;
  bool done = false;
  if constexpr (GlvOf<F>::enabled) {
    if (split) {
      pmul::SplitScalar<F> parts;
      pmul::split_scalar<F>(k, parts);
      s.dim = GlvOf<F>::DIM;
      for (int j = 0; j < GlvOf<F>::DIM; j++) {
        const int len = wnaf::recode_wnaf<kWidth>(parts.mag[j], parts.neg[j], dig[j]);
        s.len = len > s.len ? len : s.len;
      }
      done = true;
    }
  }
  if (!done) s.len = wnaf::recode_wnaf<kWidth>(k, false, dig[0]);
  for (int i = 0; i < kMaxRows; i++) {
    s.rows[i] = 0u;
    for (int j = 0; j < s.dim; j++) s.rows[i] |= (uint32_t)(uint8_t)dig[j][i] << (8 * j);
  }
}

// acc + d psi^ENDO(p), d odd
template <int ENDO, class F, class Ops, class Tab>
DG_HD XYZZ<F> digit_add(const XYZZ<F>& acc, int d, Ops& ops, Tab& tab) {
  const int m = d < 0 ? -d : d;
  XYZZ<F> e = tab.get((m >> 1) + 1);
  if constexpr (ENDO > 0) {
#pragma unroll
    for (int t = 0; t < ENDO; t++) GlvOf<F>::endo_xyzz(e);
  }
  if (d < 0) e.y = e.y.neg();
  return ops.add(acc, e);
}

// k p under the schedule's rows; DIM = 1 for ANY point of the curve, DIM = 2 / 4 for p in the order-r subgroup
template <int DIM, class F, class Ops, class Tab>
DG_HD XYZZ<F> product(const Affine<F>& p, const uint32_t* rows, int len, Ops& ops, Tab& tab) {
  wnaf::build_odd_table<kTable>(p, ops, tab);
  XYZZ<F> acc = XYZZ<F>::inf();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int i = len - 1; i >= 0; i--) {
    if (i != len - 1) acc = ops.dbl(acc);
    const uint32_t row = rows[i];
    if (!row) continue;
    if (const int d = row_digit(row, 0)) acc = digit_add<0>(acc, d, ops, tab);
    if constexpr (DIM >= 2) {
      if (const int d = row_digit(row, 1)) acc = digit_add<1>(acc, d, ops, tab);
    }
    if constexpr (DIM == 4) {
      if (const int d = row_digit(row, 2)) acc = digit_add<2>(acc, d, ops, tab);
      if (const int d = row_digit(row, 3)) acc = digit_add<3>(acc, d, ops, tab);
    }
  }
  return acc;
}

// d^-1 mod r as a plain integer, for 1 <= d < r (pmul::rr_scalar_ok)
template <class Fr>
inline void invert_scalar(const Fr& d, uint32_t* out8) {
  const Fr inv = d.to_mont().inv().from_mont();
  for (int i = 0; i < 8; i++) out8[i] = inv.l[i];
}

}  // namespace pscale
}  // namespace dg16

#if defined(__HIPCC__)
// ---- device side ----------------------------------------------------------------------------------------------------------
namespace dg16 {
namespace pscale {

// acc_out[i] = k * points[i], i < n <= stride, k as `len` rows; table: kTable * W * stride words (pmul::GlobalTab)
template <class F, int DIM>
__global__ void __launch_bounds__(64) points_scale_kernel(const Affine<F>* __restrict__ points,
                                                           const uint32_t* __restrict__ rows, int len, size_t n,
                                                           uint32_t* __restrict__ table, size_t stride,
                                                           XYZZ<F>* __restrict__ acc_out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Affine<F> p = fb_load(points + i);
  pmul::GlobalTab<F> tab{table + i, stride};
  pmul::PlainOps<F> ops;
  fb_store(acc_out + i, product<DIM, F>(p, rows, len, ops, tab));
}

// out_host[i] = k * points_host[i] (affine), in slices of the context's points_mul_slice; out_host may be points_host.
// Workspace slots of channel 0: 1 (rows), 2 (the slice's points, then its products), and those of pmul::points_mul_typed,
// with the same sizes: 20 (tables), 21 (accumulators), 22 (prefix products).
template <class F>
void points_scale_typed(Call& k, const void* points_host, const uint32_t* scalar8, size_t n, void* out_host,
                        bool in_subgroup) {
  if (!n) return;
  Schedule s;
  make_schedule<F>(scalar8, pmul::may_split<F>(in_subgroup), s);
  const size_t slice = slice_lanes(k.ctx->points_mul_slice), stride = launch_stride(n, slice);
  constexpr size_t W = sizeof(XYZZ<F>) / 4;
  const uint32_t* rows = (const uint32_t*)ws(k.c, 1, sizeof s.rows);
  Affine<F>* p = (Affine<F>*)ws(k.c, 2, stride * sizeof(Affine<F>));
  uint32_t* table = (uint32_t*)ws(k.c, 20, (size_t)kTable * W * stride * 4);
  XYZZ<F>* acc = (XYZZ<F>*)ws(k.c, 21, stride * sizeof(XYZZ<F>));
  F* pref = (F*)ws(k.c, 22, stride * sizeof(F));
  DG_HIP(hipMemcpyAsync((void*)rows, s.rows, sizeof s.rows, hipMemcpyHostToDevice, k.s()));
  k.begin_dominant();
  for (size_t lo = 0; lo < n; lo += slice) {
    const size_t cnt = n - lo < slice ? n - lo : slice;
    const dim3 grid((unsigned)((cnt + 63) / 64)), block(64);
    // (the copy is ordered behind the previous slice's kernels on the stream)
    DG_HIP(hipMemcpyAsync(p, (const Affine<F>*)points_host + lo, cnt * sizeof(Affine<F>), hipMemcpyHostToDevice, k.s()));
    if (s.dim == 1)
      hipLaunchKernelGGL((points_scale_kernel<F, 1>), grid, block, 0, k.s(), p, rows, s.len, cnt, table, stride, acc);
    else
      hipLaunchKernelGGL((points_scale_kernel<F, GlvOf<F>::DIM>), grid, block, 0, k.s(), p, rows, s.len, cnt, table,
                         stride, acc);
    DG_HIP(hipGetLastError());
    fb_to_affine(k, acc, pref, cnt, p);
    DG_HIP(hipMemcpyAsync((Affine<F>*)out_host + lo, p, cnt * sizeof(Affine<F>), hipMemcpyDeviceToHost, k.s()));
  }
  k.end_dominant();
  DG_HIP(hipStreamSynchronize(k.s()));
}

}  // namespace pscale

// host pointers; scalar8: a plain integer below 2^255 (the caller checked it)
template <int CURVE>
void points_scale_run(Call& k, int group, const void* points_host, const uint32_t* scalar8, size_t n, void* out_host,
                      bool in_subgroup);
// (defined in the per-curve objects points_scale_<curve>.o)
template <> void points_scale_run<0>(Call&, int, const void*, const uint32_t*, size_t, void*, bool);
template <> void points_scale_run<1>(Call&, int, const void*, const uint32_t*, size_t, void*, bool);
template <> void points_scale_run<2>(Call&, int, const void*, const uint32_t*, size_t, void*, bool);

}  // namespace dg16
#endif
