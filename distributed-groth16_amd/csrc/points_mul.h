// Batched variable-base point multiplication out[i] = k_i * P_i (dg16_points_mul) and, on top of it, Groth16 proof
// re-randomization (dg16_groth16_rerandomize; ark_groth16::Groth16::rerandomize_proof).
//
//   recoding   every scalar becomes a REGULAR signed fixed-window form, w = 4: k = sum_i d_i 16^i, d_i in [-8, 8], one
//              digit per window whatever the scalar is.  d_i = raw_i + c_i - 16 c_(i+1) with raw_i the i-th nibble and
//              the carry c_(i+1) = [raw_i + c_i > 8]; the carries of a scalar are one bit mask (recode_carries), so the
//              loop, which runs from the top window down, needs no digit array.
//   loop       per window: four doublings, then ONE table addition -- T[|d|] from the table 1P .. 8P, its y negated by
//              a select for d < 0; for d = 0 the lane adds T[1] and keeps the old accumulator by a select.  Every lane of
//              a wave runs the same sequence of group operations; only the branches of the complete addition law (ec.h:
//              identity operand, equal or opposite operands) can make lanes part, and those are rare by construction.
//   split      where the group's endomorphism may be used (GlvOf<F>, glv_endo.h; the rule of dg16_msm: cofactor one, or
//              the caller's DG16_F_BASES_IN_SUBGROUP) the scalar is split into DIM parts (glv.h) that share one
//              doubling chain: per window DIM additions of psi^j(T[|d_j|]), the endomorphism applied to the table
//              entry on the fly (one table, of P).  DIM = 2: two halves < 2^127, 32 windows; DIM = 4 (G2 of the BLS12
//              curves): four quarters < 2^66, 17 windows.
//   budget     plain: 64 windows, 4 + 63 * 4 = 256 doublings and 3 + 64 = 67 additions (table included);
//              DIM = 2: 4 + 31 * 4 = 128 doublings, 3 + 64 = 67 additions; DIM = 4: 4 + 16 * 4 = 68, 3 + 68 = 71.
//   table      eight XYZZ entries per product (1 KB for BN254 G1, 3 KB for a BLS12 G2) live in the channel's workspace,
//              word-major and lane-minor: word t of entry j of lane l at ((j - 1) * W + t) * stride + l, so the lanes of
//              a wave that read the same entry read consecutive words.
//   affine     the accumulators of a slice go through fixed_base_impl.h's batched inversion (fb_affine_kernel).
//
// Exceptional cases of the addition law.  The accumulator is 16 v P and the addend d P, |d| <= 8, v the part of the
// scalar above the window.  For a point of order r and the plain path they coincide only in the LAST window, when
// 16 v = r + e with e = +-d: k = r (16 v = r - 1, d = 1: P - P), k = r - 2 (d = -1: -P - P, a doubling) -- r = 1 mod 16
// on all three curves -- and their analogues around 2 r, 3 r, .. below 2^255.  Small scalars leave the accumulator at
// the identity for the leading windows, k = 0 to the end, and an identity input makes every table entry the identity.
// A point outside the subgroup (cofactor groups, plain path) can meet its own multiples anywhere.  With the split on
// subgroup points the parts are short vectors of a lattice whose nonzero vectors are longer than a window, so only the
// identity cases occur.  All of it goes through XYZZ::add, which is complete; nothing is proven away.
//
// The recoding and the loops are host and device text: tests/host_arith/host_points_mul.cpp runs them on a CPU against
// the oracle and counts the group operations through the Ops parameter.
#pragma once
#include "glv_endo.h"
#include "slices.h"
#include "types.h"

namespace dg16 {
namespace pmul {

constexpr int kWindowBits = 4;
constexpr int kTable = 1 << (kWindowBits - 1);     // entries 1P .. 8P
constexpr int kWinPlain = 64;                      // scalars below 2^255
constexpr int kWinHalf = 32;                       // |k1|, |k2| < 2^127 (msm_geom.h: kGlvBits)
constexpr int kWinQuarter = 17;                    // quarters < 2^66 (kGlv4Bits = 65 and a spare bit), < 2^67 needed

template <class F> constexpr int split_windows() { return GlvOf<F>::DIM == 2 ? kWinHalf : kWinQuarter; }
// the rule of dg16_msm (msm_glv.h): split where an endomorphism is wired and phi(P) = LAMBDA P is known to hold
template <class F> DG_HD bool may_split(bool in_subgroup) {
  if constexpr (GlvOf<F>::enabled) return GlvCofactorOne<F>::value || in_subgroup;
  else return false;
}

// nibble i of an 8-word integer; a chain of selects, so k stays in registers under a run-time i
DG_HD uint32_t raw_digit(const uint32_t* k, int i) {
  const int wi = i >> 3;
  uint32_t w = k[0];
#pragma unroll
  for (int j = 1; j < 8; j++) w = wi == j ? k[j] : w;
  return (w >> ((i & 7) * 4)) & 15u;
}
// bit i = the carry INTO window i.  The carry out of the top window is zero for k < 2^(4 nwin - 1).
DG_HD uint64_t recode_carries(const uint32_t* k, int nwin) {
  uint64_t c = 0;
  uint32_t carry = 0;
  for (int i = 0; i < nwin; i++) {
    c |= (uint64_t)carry << i;
    carry = raw_digit(k, i) + carry > 8u ? 1u : 0u;
  }
  return c;
}
// d_i in [-8, 8]
DG_HD int digit(const uint32_t* k, uint64_t carries, int i, int nwin) {
  const int cin = (int)((carries >> i) & 1u);
  const int cout = i + 1 < nwin ? (int)((carries >> (i + 1)) & 1u) : 0;
  return (int)raw_digit(k, i) + cin - 16 * cout;
}

// what the loops call for a group operation; the host tests pass a counting one
template <class F>
struct PlainOps {
  DG_HD XYZZ<F> dbl(const XYZZ<F>& a) { return a.dbl(); }
  DG_HD XYZZ<F> add(const XYZZ<F>& a, const XYZZ<F>& b) { return a.add(b); }
};

template <class F>
DG_HD XYZZ<F> select(bool c, const XYZZ<F>& a, const XYZZ<F>& b) {
  return {F::select(c, a.x, b.x), F::select(c, a.y, b.y), F::select(c, a.zz, b.zz), F::select(c, a.zzz, b.zzz)};
}

// T[j] = j p, j = 1 .. 8: four doublings, three additions
template <class F, class Ops, class Tab>
DG_HD void build_table(const Affine<F>& p, Ops& ops, Tab& tab) {
  const XYZZ<F> t1 = XYZZ<F>::from_affine(p);
  tab.put(1, t1);
  const XYZZ<F> t2 = ops.dbl(t1);
  tab.put(2, t2);
  const XYZZ<F> t3 = ops.add(t2, t1);
  tab.put(3, t3);
  const XYZZ<F> t4 = ops.dbl(t2);
  tab.put(4, t4);
  const XYZZ<F> t6 = ops.dbl(t3);
  tab.put(6, t6);
  tab.put(5, ops.add(t4, t1));
  tab.put(8, ops.dbl(t4));
  tab.put(7, ops.add(t6, t1));
}

// acc + (flip ? -d : d) psi^ENDO(p): one addition whatever d is
template <int ENDO, class F, class Ops, class Tab>
DG_HD XYZZ<F> window_add(const XYZZ<F>& acc, int d, bool flip, Ops& ops, Tab& tab) {
  int m = d < 0 ? -d : d;
  m = m > kTable ? kTable : m;       // only a scalar outside the contract (>= 2^255) gets here: a wrong point, never a wild read
  const bool neg = (d < 0) != flip;
  XYZZ<F> e = tab.get(m ? m : 1);
  if constexpr (ENDO > 0) {
#pragma unroll
    for (int t = 0; t < ENDO; t++) GlvOf<F>::endo_xyzz(e);
  }
  e.y = F::select(neg, e.y.neg(), e.y);
  const XYZZ<F> s = ops.add(acc, e);
  return select(m != 0, s, acc);
}

// k p for an 8-word integer k < 2^255 and ANY point p of the curve
template <class F, class Ops, class Tab>
DG_HD XYZZ<F> product_plain(const Affine<F>& p, const uint32_t* k, Ops& ops, Tab& tab) {
  build_table(p, ops, tab);
  const uint64_t carries = recode_carries(k, kWinPlain);
  XYZZ<F> acc = XYZZ<F>::inf();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int i = kWinPlain - 1; i >= 0; i--) {
    if (i != kWinPlain - 1) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
      for (int j = 0; j < kWindowBits; j++) acc = ops.dbl(acc);
    }
    acc = window_add<0>(acc, digit(k, carries, i, kWinPlain), false, ops, tab);
  }
  return acc;
}

// the parts of k under the group's split: magnitudes (8 words each), signs and carry masks
template <class F>
struct SplitScalar {
  static constexpr int DIM = GlvOf<F>::DIM;
  uint32_t mag[DIM][8];
  bool neg[DIM];
  uint64_t carries[DIM];
};
template <class F>
DG_HD void split_scalar(const uint32_t* k, SplitScalar<F>& s) {
  using GC = typename GlvOf<F>::C;
  constexpr int DIM = GlvOf<F>::DIM;
  if constexpr (DIM == 2) glv::split<GC>(k, s.mag[0], s.mag[1]);
  else glv::split4<GC>(k, s.mag[0], s.mag[1], s.mag[2], s.mag[3]);
#pragma unroll
  for (int j = 0; j < DIM; j++) {
    s.neg[j] = (s.mag[j][7] >> 31) != 0;
    s.mag[j][7] &= 0x7fffffffu;
    s.carries[j] = recode_carries(s.mag[j], split_windows<F>());
  }
}

// k p for p in the order-r subgroup: k = sum_j k_j LAMBDA^j, one doubling chain, DIM additions per window
template <class F, class Ops, class Tab>
DG_HD XYZZ<F> product_split(const Affine<F>& p, const uint32_t* k, Ops& ops, Tab& tab) {
  constexpr int DIM = GlvOf<F>::DIM;
  constexpr int NW = split_windows<F>();
  build_table(p, ops, tab);
  SplitScalar<F> s;
  split_scalar<F>(k, s);
  XYZZ<F> acc = XYZZ<F>::inf();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int i = NW - 1; i >= 0; i--) {
    if (i != NW - 1) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
      for (int j = 0; j < kWindowBits; j++) acc = ops.dbl(acc);
    }
    acc = window_add<0>(acc, digit(s.mag[0], s.carries[0], i, NW), s.neg[0], ops, tab);
    acc = window_add<1>(acc, digit(s.mag[1], s.carries[1], i, NW), s.neg[1], ops, tab);
    if constexpr (DIM == 4) {
      acc = window_add<2>(acc, digit(s.mag[2], s.carries[2], i, NW), s.neg[2], ops, tab);
      acc = window_add<3>(acc, digit(s.mag[3], s.carries[3], i, NW), s.neg[3], ops, tab);
    }
  }
  return acc;
}

// ---- re-randomization: the arithmetic of one proof ---------------------------------------------------------------------
template <class Fq, class Fq2>
struct RrProof {           // the proof layout of dg16_groth16_verify_batch
  Affine<Fq> a;
  Affine<Fq2> b;
  Affine<Fq> c;
};
// 1 <= x < r on the stored words (a Montgomery form is canonical too, and zero exactly when the value is)
template <class Fr>
DG_HD bool rr_scalar_ok(const Fr& x) {
  if (x.is_zero()) return false;
  for (int i = Fr::NL - 1; i >= 0; i--) {
    if (x.l[i] < Fr::Params::P[i]) return true;
    if (x.l[i] > Fr::Params::P[i]) return false;
  }
  return false;
}
// the four multipliers of one proof as plain integers: 1 / r1 (for A), r2 (for A, into C), r1 (for B), r1 r2 (for delta)
template <class Fr>
DG_HD void rr_scalars(const Fr& r1, const Fr& r2, bool mont, Fr* r1_inv, Fr* r2_int, Fr* r1_int, Fr* r1_r2) {
  const Fr m1 = mont ? r1 : r1.to_mont(), m2 = mont ? r2 : r2.to_mont();
  *r1_inv = m1.inv().from_mont();
  *r2_int = mont ? r2.from_mont() : r2;
  *r1_int = mont ? r1.from_mont() : r1;
  *r1_r2 = (m1 * m2).from_mont();
}
// (A', B', C') = (r1^-1 A, r1 B + r1 r2 delta, C + r2 A) from the four products; ok = false writes three identities
template <class Fq, class Fq2>
DG_HD RrProof<Fq, Fq2> rr_combine(bool ok, const Affine<Fq>& a_inv, const Affine<Fq>& a_r2, const Affine<Fq>& c,
                                   const Affine<Fq2>& b_r1, const Affine<Fq2>& delta_r12) {
  if (!ok) return {Affine<Fq>::inf(), Affine<Fq2>::inf(), Affine<Fq>::inf()};
  return {a_inv, XYZZ<Fq2>::from_affine(b_r1).madd(delta_r12, false).to_affine(),
          XYZZ<Fq>::from_affine(c).madd(a_r2, false).to_affine()};
}

}  // namespace pmul
}  // namespace dg16

#if defined(__HIPCC__)
// ---- device side ----------------------------------------------------------------------------------------------------------
#include "fixed_base_impl.h"
#include "verify_batch.h"

namespace dg16 {
namespace pmul {

// the table of one lane in the slice's buffer: word-major, lane-minor (see the header comment)
template <class F>
struct GlobalTab {
  static constexpr int W = (int)(sizeof(XYZZ<F>) / 4);
  uint32_t* base;      // the buffer, offset by the lane
  size_t stride;       // lanes of the slice
  __device__ __forceinline__ void put(int j, const XYZZ<F>& e) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(&e);
    uint32_t* dst = base + (size_t)(j - 1) * W * stride;
#pragma unroll
    for (int t = 0; t < W; t++) dst[(size_t)t * stride] = w[t];
  }
  __device__ __forceinline__ XYZZ<F> get(int j) const {
    XYZZ<F> e;
    uint32_t* w = reinterpret_cast<uint32_t*>(&e);
    const uint32_t* src = base + (size_t)(j - 1) * W * stride;
#pragma unroll
    for (int t = 0; t < W; t++) w[t] = src[(size_t)t * stride];
    return e;
  }
};

// acc_out[i] = scalars[i] * points[i], i < n <= stride; table: kTable * W * stride words
template <class F, class Fr, bool SPLIT>
__global__ void __launch_bounds__(64) points_mul_kernel(const Affine<F>* points, const Fr* __restrict__ scalars, size_t n,
                                                         int mont, uint32_t* __restrict__ table, size_t stride,
                                                         XYZZ<F>* __restrict__ acc_out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fr k = fb_load(scalars + i);
  if (mont) k = k.from_mont();
  const Affine<F> p = fb_load(points + i);
  GlobalTab<F> tab{table + i, stride};
  PlainOps<F> ops;
  XYZZ<F> acc;
  if constexpr (SPLIT) acc = product_split<F>(p, k.l, ops, tab);
  else acc = product_plain<F>(p, k.l, ops, tab);
  fb_store(acc_out + i, acc);
}

// out_dev[i] = scalars_dev[i] * points_dev[i] (affine), in slices of `slice` products.  out_dev may be points_dev.
// Workspace slots of the channel: 20 (tables), 21 (accumulators), 22 (prefix products).
template <class F, class Fr>
void points_mul_typed(Call& k, const void* points_dev, const void* scalars_dev, size_t n, unsigned mode, void* out_dev) {
  if (!n) return;
  static_assert(sizeof(Fr) == 32, "scalar size");
  const size_t slice = slice_lanes(k.ctx->points_mul_slice);
  const size_t first = launch_stride(n, slice);      // the stride of every launch of this call
  constexpr size_t W = sizeof(XYZZ<F>) / 4;
  uint32_t* table = (uint32_t*)ws(k.c, 20, (size_t)kTable * W * first * 4);
  XYZZ<F>* acc = (XYZZ<F>*)ws(k.c, 21, first * sizeof(XYZZ<F>));
  F* pref = (F*)ws(k.c, 22, first * sizeof(F));
  const bool split = may_split<F>(mode & 2u);
  k.begin_dominant();
  for (size_t lo = 0; lo < n; lo += slice) {
    const size_t cnt = n - lo < slice ? n - lo : slice;
    const dim3 grid((unsigned)((cnt + 63) / 64)), block(64);
    const Affine<F>* p = (const Affine<F>*)points_dev + lo;
    const Fr* s = (const Fr*)scalars_dev + lo;
    if (split)
      hipLaunchKernelGGL((points_mul_kernel<F, Fr, true>), grid, block, 0, k.s(), p, s, cnt, (int)(mode & 1u), table,
                         first, acc);
    else
      hipLaunchKernelGGL((points_mul_kernel<F, Fr, false>), grid, block, 0, k.s(), p, s, cnt, (int)(mode & 1u), table,
                         first, acc);
    DG_HIP(hipGetLastError());
    fb_to_affine(k, acc, pref, cnt, (Affine<F>*)out_dev + lo);
  }
  k.end_dominant();
}

}  // namespace pmul

// mode: ctx.h's msm_mode (bit 0 = Montgomery scalars, bit 1 = DG16_F_BASES_IN_SUBGROUP); device pointers
template <int CURVE>
void points_mul_run(Call& k, int group, const void* points_dev, const void* scalars_dev, size_t n, unsigned mode,
                    void* out_dev);
// proofs_dev -> out_dev (may be the same buffer) under r1_r2_dev; BN254 and BLS12-381
template <int CURVE>
void rerandomize_run(Call& k, const VkData& vk, const void* proofs_dev, size_t n, const void* r1_r2_dev, bool mont,
                     void* out_dev);
// (defined in the per-curve objects points_mul_<curve>.o)
template <> void points_mul_run<0>(Call&, int, const void*, const void*, size_t, unsigned, void*);
template <> void points_mul_run<1>(Call&, int, const void*, const void*, size_t, unsigned, void*);
template <> void points_mul_run<2>(Call&, int, const void*, const void*, size_t, unsigned, void*);
template <> void rerandomize_run<0>(Call&, const VkData&, const void*, size_t, const void*, bool, void*);
template <> void rerandomize_run<1>(Call&, const VkData&, const void*, size_t, const void*, bool, void*);

}  // namespace dg16
#endif
