// The latency-bound chains of the MSM and the prover on ONE wave: wave-cooperative group operations in the 32-bit and the
// reduced-radix form, k P by interleaved NAFs (with the endomorphism split), their limb-per-lane forms (lane29.h), sums of
// a few points, and phase 6, the Horner tail.  Pipeline: msm_impl.h.
#pragma once
#include "ec29.h"
#include "glv.h"
#include "lane29.h"
#include "msm_accumulate_phase.h"
#include "types.h"

#ifndef DG16_CHAIN_PRIO
#define DG16_CHAIN_PRIO 3       // priority of the one-wave chain kernels (Horner tail, scalar multiples, assembly)
#endif

namespace dg16 {

// ---- wave-cooperative group operations (single-chain phases: Horner tail, s*A / r*B1) ------------------------
// A lone lane takes ~10 us (G1) / ~40 us (G2) per dependent group operation; these phases are chains of such
// operations with little parallelism, so one WAVE runs each chain and spreads the independent products of an
// operation over its lanes: the operands are uniform across the wave, slot = lane / 4 picks the product, an Fq2
// product is itself split over three lanes of the quad (Karatsuba), results are shared with readlane.
template <class P>
__device__ __forceinline__ Fp<P> lane_bcast(const Fp<P>& v, int src) {   // src: wave-uniform lane index
  Fp<P> r;
#pragma unroll
  for (int i = 0; i < Fp<P>::NL; i++) r.l[i] = (uint32_t)__builtin_amdgcn_readlane((int)v.l[i], src);
  return r;
}
template <class F>
__device__ __forceinline__ Fp2<F> lane_bcast(const Fp2<F>& v, int src) {
  return {lane_bcast(v.c0, src), lane_bcast(v.c1, src)};
}
template <class P>
__device__ __forceinline__ Fp<P> lane_get(const Fp<P>& v, int src) {     // src: per-lane index
  Fp<P> r;
#pragma unroll
  for (int i = 0; i < Fp<P>::NL; i++) r.l[i] = (uint32_t)__shfl((int)v.l[i], src);
  return r;
}
// product per slot (slot = lane / 4; the operands must be equal across the quad).  The product is a CALL
// (Fp::mul_call): these chains run once per proof on one wave, so their cost is dependent issue + instruction fetch
// of cold code -- with every product inlined the s*A kernel was 180 KB and the proof assembly 210 KB of straight-line
// code (0.46 ms for ~40 us of arithmetic); a call keeps an addition at ~4 KB.
template <class P>
__device__ __forceinline__ Fp<P> slot_mul(const Fp<P>& a, const Fp<P>& b) { return Fp<P>::mul_call(a, b); }
template <class F>
__device__ __forceinline__ Fp2<F> slot_mul(const Fp2<F>& a, const Fp2<F>& b) {
  const unsigned q = __lane_id() & 3;
  const F x = F::select(q == 0, a.c0, F::select(q == 1, a.c1, a.c0 + a.c1));
  const F y = F::select(q == 0, b.c0, F::select(q == 1, b.c1, b.c0 + b.c1));
  const F t = F::mul_call(x, y);
  const int base = (int)(__lane_id() & ~3u);
  const F t0 = lane_get(t, base), t1 = lane_get(t, base + 1), t2 = lane_get(t, base + 2);
  return {t0 - fq2_beta_mul(t1), t2 - t0 - t1};      // u^2 = -BETA (fp2.h)
}
// 2 * p with p (and the result) uniform across the wave                 (dbl-2008-s-1, a = 0)
template <class F>
__device__ __forceinline__ XYZZ<F> dbl_wave(const XYZZ<F>& p) {
  if (p.is_inf()) return p;
  const unsigned slot = __lane_id() >> 2;
  const F u = p.y.dbl();
  // level 1: v = u^2 | xx = x^2
  const F a1 = F::select(slot == 0, u, p.x);
  const F r1 = slot_mul(a1, a1);
  const F v = lane_bcast(r1, 0), xx = lane_bcast(r1, 4);
  const F m = xx.dbl() + xx;
  // level 2: w = u v | s = x v | m^2 | zz' = v zz
  const F a2 = F::select(slot == 0, u, F::select(slot == 1, p.x, F::select(slot == 2, m, v)));
  const F b2 = F::select(slot <= 1, v, F::select(slot == 2, m, p.zz));
  const F r2 = slot_mul(a2, b2);
  const F w = lane_bcast(r2, 0), sv = lane_bcast(r2, 4), mm = lane_bcast(r2, 8), zz3 = lane_bcast(r2, 12);
  const F x3 = mm - sv.dbl();
  // level 3: m (s - x3) | w y | zzz' = w zzz
  const F a3 = F::select(slot == 0, m, w);
  const F b3 = F::select(slot == 0, sv - x3, F::select(slot == 1, p.y, p.zzz));
  const F r3 = slot_mul(a3, b3);
  const F y3 = lane_bcast(r3, 0) - lane_bcast(r3, 4);
  return {x3, y3, zz3, lane_bcast(r3, 8)};
}

// p + o, both (and the result) uniform across the wave: 14 products in 4 levels       (add-2008-s)
template <class F>
__device__ __forceinline__ XYZZ<F> add_wave(const XYZZ<F>& p, const XYZZ<F>& o) {
  if (o.is_inf()) return p;
  if (p.is_inf()) return o;
  const unsigned slot = __lane_id() >> 2;
  // level 1: u1 = x1 zz2 | u2 = x2 zz1 | s1 = y1 zzz2 | s2 = y2 zzz1
  const F a1 = F::select(slot == 0, p.x, F::select(slot == 1, o.x, F::select(slot == 2, p.y, o.y)));
  const F b1 = F::select(slot == 0, o.zz, F::select(slot == 1, p.zz, F::select(slot == 2, o.zzz, p.zzz)));
  const F r1 = slot_mul(a1, b1);
  const F u1 = lane_bcast(r1, 0), u2 = lane_bcast(r1, 4), s1 = lane_bcast(r1, 8), s2 = lane_bcast(r1, 12);
  const F pd = u2 - u1, rd = s2 - s1;
  if (pd.is_zero()) {
    if (rd.is_zero()) return dbl_wave(p);
    return XYZZ<F>::inf();
  }
  // level 2: pp = p^2 | rr = r^2 | zz1 zz2 | zzz1 zzz2
  const F a2 = F::select(slot == 0, pd, F::select(slot == 1, rd, F::select(slot == 2, p.zz, p.zzz)));
  const F b2 = F::select(slot == 0, pd, F::select(slot == 1, rd, F::select(slot == 2, o.zz, o.zzz)));
  const F r2 = slot_mul(a2, b2);
  const F pp = lane_bcast(r2, 0), rr = lane_bcast(r2, 4), zzp = lane_bcast(r2, 8), zzzp = lane_bcast(r2, 12);
  // level 3: ppp = p pp | q = u1 pp | zz3 = (zz1 zz2) pp
  const F a3 = F::select(slot == 0, pd, F::select(slot == 1, u1, zzp));
  const F r3 = slot_mul(a3, pp);
  const F ppp = lane_bcast(r3, 0), q = lane_bcast(r3, 4), zz3 = lane_bcast(r3, 8);
  const F x3 = rr - ppp - q.dbl();
  // level 4: r (q - x3) | s1 ppp | zzz3 = (zzz1 zzz2) ppp
  const F a4 = F::select(slot == 0, rd, F::select(slot == 1, s1, zzzp));
  const F b4 = F::select(slot == 0, q - x3, ppp);
  const F r4 = slot_mul(a4, b4);
  return {x3, lane_bcast(r4, 0) - lane_bcast(r4, 4), zz3, lane_bcast(r4, 8)};
}
// k * p by double-and-add on one wave; k = NW little-endian 32-bit words (plain integer), uniform
template <class F, int NW>
__device__ __forceinline__ XYZZ<F> scalar_mul_wave(const XYZZ<F>& p, const uint32_t* k) {
  XYZZ<F> acc = XYZZ<F>::inf();
  for (int i = NW * 32 - 1; i >= 0; i--) {
    acc = dbl_wave(acc);
    if ((k[i / 32] >> (i % 32)) & 1) acc = add_wave(acc, p);
  }
  return acc;
}

// ---- the same wave-cooperative operations on the reduced-radix types (XYZZ29, internal Montgomery form) -------------
// A level is ONE 162-mad (392 for 14 limbs) column-chain product (fp29_asm_gen.h) per lane instead of the 454-slot out-of-line
// 32-bit product of the forms above; coordinates stay below the storage bound BS p between levels (fit<BS>), so every
// slot's operand has the same static type.
// bcast29<SRC>: the value lane SRC (< 16) of every row of 16 lanes holds -> all lanes of the row, v_mov_b32_dpp
// row_newbcast:SRC, one VALU instruction per limb (the operands of these chains are uniform across the wave and every row
// holds the same four slots, so a row-local broadcast is a wave-wide one).  The moves are ONE OPAQUE asm statement per
// element ON PURPOSE -- two wait states first (a DPP read needs them after the VALU write of its source and hipcc cannot
// see a DPP inside an asm), then a v_mov_b32_dpp per limb: through __builtin_amdgcn_update_dpp hipcc's DPP combiner folds
// the broadcast into a consuming subtraction, v_subrev_u32_dpp ... row_newbcast, which does not compute S1 - dpp(S0) on
// gfx950 (the v_readlane form before it ran the glue on the scalar unit: CHANGELOG.md, round 4).
template <int SRC, class P, int B>
__device__ __forceinline__ Fe<P, B, 1> bcast29(const Fe<P, B, 1>& v) {
  static_assert(SRC >= 0 && SRC < 16, "row_newbcast takes a lane of the row");
  static_assert(RR<P>::N == 9 || RR<P>::N == 14, "limb count");
  Fe<P, B, 1> r;
  if constexpr (RR<P>::N == 9) {
    asm volatile(
        "s_nop 1\n\t"
        "v_mov_b32_dpp %0, %9 row_newbcast:%18 row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %1, %10 row_newbcast:%18 row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %2, %11 row_newbcast:%18 row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %3, %12 row_newbcast:%18 row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %4, %13 row_newbcast:%18 row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %5, %14 row_newbcast:%18 row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %6, %15 row_newbcast:%18 row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %7, %16 row_newbcast:%18 row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %8, %17 row_newbcast:%18 row_mask:0xf bank_mask:0xf"
        : "=&v"(r.l[0]), "=&v"(r.l[1]), "=&v"(r.l[2]), "=&v"(r.l[3]), "=&v"(r.l[4]), "=&v"(r.l[5]), "=&v"(r.l[6]),
          "=&v"(r.l[7]), "=&v"(r.l[8])
        : "v"(v.l[0]), "v"(v.l[1]), "v"(v.l[2]), "v"(v.l[3]), "v"(v.l[4]), "v"(v.l[5]), "v"(v.l[6]), "v"(v.l[7]),
          "v"(v.l[8]), "n"(SRC));
  } else {
    asm volatile(
        "s_nop 1\n\t"
        "v_mov_b32_dpp %0, %14 row_newbcast:%28 row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %1, %15 row_newbcast:%28 row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %2, %16 row_newbcast:%28 row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %3, %17 row_newbcast:%28 row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %4, %18 row_newbcast:%28 row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %5, %19 row_newbcast:%28 row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %6, %20 row_newbcast:%28 row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %7, %21 row_newbcast:%28 row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %8, %22 row_newbcast:%28 row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %9, %23 row_newbcast:%28 row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %10, %24 row_newbcast:%28 row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %11, %25 row_newbcast:%28 row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %12, %26 row_newbcast:%28 row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %13, %27 row_newbcast:%28 row_mask:0xf bank_mask:0xf"
        : "=&v"(r.l[0]), "=&v"(r.l[1]), "=&v"(r.l[2]), "=&v"(r.l[3]), "=&v"(r.l[4]), "=&v"(r.l[5]), "=&v"(r.l[6]),
          "=&v"(r.l[7]), "=&v"(r.l[8]), "=&v"(r.l[9]), "=&v"(r.l[10]), "=&v"(r.l[11]), "=&v"(r.l[12]), "=&v"(r.l[13])
        : "v"(v.l[0]), "v"(v.l[1]), "v"(v.l[2]), "v"(v.l[3]), "v"(v.l[4]), "v"(v.l[5]), "v"(v.l[6]), "v"(v.l[7]),
          "v"(v.l[8]), "v"(v.l[9]), "v"(v.l[10]), "v"(v.l[11]), "v"(v.l[12]), "v"(v.l[13]), "n"(SRC));
  }
  return r;
}
template <int SRC, class P, int B>
__device__ __forceinline__ Fe2<P, B, 1> bcast29(const Fe2<P, B, 1>& v) {
  return {bcast29<SRC>(v.c0), bcast29<SRC>(v.c1)};
}
template <class P, int B>
__device__ __forceinline__ Fe<P, B, 1> lane_get29(const Fe<P, B, 1>& v, int src) {   // src: per-lane index
  Fe<P, B, 1> r;
#pragma unroll
  for (int i = 0; i < RR<P>::N; i++) r.l[i] = (uint32_t)__shfl((int)v.l[i], src);
  return r;
}
// product per slot (slot = lane / 4; operands equal across the quad); an Fq2 product is three base-field products on
// three lanes of the quad (Karatsuba), joined with ds_bpermute
template <class P, int B>
__device__ __forceinline__ Fe<P, B, 1> slot_mul29(const Fe<P, B, 1>& a, const Fe<P, B, 1>& b) { return fit<B>(a * b); }
// (BM: the base-field product of the three lanes -- inline, or behind a call: SlotMulCall in prover_impl.h)
template <class BM, class P, int B>
__device__ __forceinline__ Fe2<P, B, 1> slot_mul29_fe2(const Fe2<P, B, 1>& a, const Fe2<P, B, 1>& b) {
  constexpr int BETA = Fq2Beta<P>::value;
  const unsigned q = __lane_id() & 3;
  const Fe<P, B, 1> sa = fit<B>(a.c0 + a.c1), sb = fit<B>(b.c0 + b.c1);
  const Fe<P, B, 1> x = select(q == 0, a.c0, select(q == 1, a.c1, sa));
  const Fe<P, B, 1> y = select(q == 0, b.c0, select(q == 1, b.c1, sb));
  const Fe<P, B, 1> t = BM::mul(x, y);
  const int base = (int)(__lane_id() & ~3u);
  const Fe<P, B, 1> t0 = lane_get29(t, base), t1 = lane_get29(t, base + 1), t2 = lane_get29(t, base + 2);
  if constexpr (BETA == 1) return {fit<B>(t0 - t1), fit<B>(t2 - (t0 + t1))};          // u^2 = -BETA (fp2.h)
  else return {fit<B>(t0 - mul_small<BETA>(t1)), fit<B>(t2 - (t0 + t1))};
}
// M: how a level's product is issued -- inline (the chains that loop: Horner tail, scalar multiples, tree steps) or behind
// a call (prover_impl.h: SlotMulCall -- chains that run ONCE per proof, whose cost is the fetch of cold code)
struct SlotMulInline {
  template <class P, int B>
  static __device__ __forceinline__ Fe<P, B, 1> mul(const Fe<P, B, 1>& a, const Fe<P, B, 1>& b) { return fit<B>(a * b); }
  template <class P, int B>
  static __device__ __forceinline__ Fe2<P, B, 1> mul(const Fe2<P, B, 1>& a, const Fe2<P, B, 1>& b) {
    return slot_mul29_fe2<SlotMulInline>(a, b);
  }
};
template <class P, int B>
__device__ __forceinline__ Fe2<P, B, 1> slot_mul29(const Fe2<P, B, 1>& a, const Fe2<P, B, 1>& b) {
  return slot_mul29_fe2<SlotMulInline>(a, b);
}
// 2 p, p (and the result) uniform across the wave                       (dbl-2008-s-1, a = 0)
template <class F, class M = SlotMulInline>
__device__ __forceinline__ XYZZ29<F> dbl_wave29(const XYZZ29<F>& p) {
  constexpr int BS = XYZZ29<F>::BS;
  if (p.is_inf()) return p;
  const unsigned slot = (__lane_id() & 15) >> 2;     // four slots per row of 16 lanes (the same in every row)
  const auto u = fit<BS>(dbl(p.y));
  if constexpr (HasOrderTwoPoint<F>::value) {          // (ec29.h) 2 T = the identity, with zero limbs
    if (is_zero_up_to_bound(u)) return XYZZ29<F>::inf();
  }
  // level 1: v = u^2 | xx = x^2
  const auto a1 = select(slot == 0, u, p.x);
  const auto r1 = M::mul(a1, a1);
  const auto v = bcast29<0>(r1), xx = bcast29<4>(r1);
  const auto m = fit<BS>(dbl(xx) + xx);
  // level 2: w = u v | s = x v | m^2 | zz' = v zz
  const auto a2 = select(slot == 0, u, select(slot == 1, p.x, select(slot == 2, m, v)));
  const auto b2 = select(slot <= 1, v, select(slot == 2, m, p.zz));
  const auto r2 = M::mul(a2, b2);
  const auto w = bcast29<0>(r2), sv = bcast29<4>(r2), mm = bcast29<8>(r2), zz3 = bcast29<12>(r2);
  const auto x3 = fit<BS>(mm - dbl(sv));
  // level 3: m (s - x3) | w y | zzz' = w zzz
  const auto a3 = select(slot == 0, m, w);
  const auto b3 = select(slot == 0, fit<BS>(sv - x3), select(slot == 1, p.y, p.zzz));
  const auto r3 = M::mul(a3, b3);
  const auto y3 = fit<BS>(bcast29<0>(r3) - bcast29<4>(r3));
  return {x3, y3, zz3, bcast29<8>(r3)};
}
// p + o, both (and the result) uniform across the wave: 14 products in 4 levels       (add-2008-s)
template <class F, class M = SlotMulInline>
__device__ __forceinline__ XYZZ29<F> add_wave29(const XYZZ29<F>& p, const XYZZ29<F>& o) {
  constexpr int BS = XYZZ29<F>::BS;
  if (o.is_inf()) return p;
  if (p.is_inf()) return o;
  const unsigned slot = (__lane_id() & 15) >> 2;     // four slots per row of 16 lanes (the same in every row)
  // level 1: u1 = x1 zz2 | u2 = x2 zz1 | s1 = y1 zzz2 | s2 = y2 zzz1
  const auto a1 = select(slot == 0, p.x, select(slot == 1, o.x, select(slot == 2, p.y, o.y)));
  const auto b1 = select(slot == 0, o.zz, select(slot == 1, p.zz, select(slot == 2, o.zzz, p.zzz)));
  const auto r1 = M::mul(a1, b1);
  const auto u1 = bcast29<0>(r1), u2 = bcast29<4>(r1), s1 = bcast29<8>(r1), s2 = bcast29<12>(r1);
  const auto pd = fit<BS>(u2 - u1), rd = fit<BS>(s2 - s1);
  if (is_zero(pd)) {
    if (is_zero(rd)) return dbl_wave29<F, M>(p);
    return XYZZ29<F>::inf();
  }
  // level 2: pp = p^2 | rr = r^2 | zz1 zz2 | zzz1 zzz2
  const auto a2 = select(slot == 0, pd, select(slot == 1, rd, select(slot == 2, p.zz, p.zzz)));
  const auto b2 = select(slot == 0, pd, select(slot == 1, rd, select(slot == 2, o.zz, o.zzz)));
  const auto r2 = M::mul(a2, b2);
  const auto pp = bcast29<0>(r2), rr = bcast29<4>(r2), zzp = bcast29<8>(r2), zzzp = bcast29<12>(r2);
  // level 3: ppp = p pp | q = u1 pp | zz3 = (zz1 zz2) pp
  const auto a3 = select(slot == 0, pd, select(slot == 1, u1, zzp));
  const auto r3 = M::mul(a3, pp);
  const auto ppp = bcast29<0>(r3), q = bcast29<4>(r3), zz3 = bcast29<8>(r3);
  const auto x3 = fit<BS>(rr - (ppp + dbl(q)));
  // level 4: r (q - x3) | s1 ppp | zzz3 = (zzz1 zzz2) ppp
  const auto a4 = select(slot == 0, rd, select(slot == 1, s1, zzzp));
  const auto b4 = select(slot == 0, fit<BS>(q - x3), ppp);
  const auto r4 = M::mul(a4, b4);
  return {x3, fit<BS>(bcast29<0>(r4) - bcast29<4>(r4)), zz3, bcast29<8>(r4)};
}
// ---- k p on one wave: interleaved width-4 NAFs, and the endomorphism split where the group allows it -----------------
// The plain double-and-add chain (round 4) ran NW * 32 doublings and ~NW * 16 additions -- 254 x 3 + 127 x 4 = 1 270
// dependent product levels for s A' / r B1' of a proof: 0.52 ms of an 8-shard rank's 3.0 ms.  Here the scalar is recoded
// as a width-4 NAF (digits 0, +-1, +-3, +-5, +-7, one nonzero digit in five on average) over the odd multiples P, 3P, 5P,
// 7P kept in LDS, and for a group of cofactor one (BN254 G1: phi(P) = LAMBDA P holds for EVERY point of the curve;
// GlvCofactorOne below) k is first split k = k1 + k2 LAMBDA with 127-bit halves (glv.h) whose NAFs are interleaved
// over (P, phi P) (Straus): 127 doublings + ~51 additions + the table = ~600 levels.  Groups with a cofactor keep the
// unsplit scalar (a key's A' / B1' are in the order-r subgroup only if the key is valid, and a proof must equal
// arkworks' for any key): 254 doublings + ~51 additions = ~980 levels.
template <class F> struct GlvOf;
template <class F> struct GlvCofactorOne;
constexpr int kNafMax = 8 * 32 + 8;        // digits of one NAF (an NW-word integer has at most NW * 32 + 1)
template <class F>
struct ScalarMulLds {                      // per chain (one wave)
  XYZZ29<F> tab[8];                        // (2 j + 1) P, j < 4; then phi of them
  signed char naf[2][kNafMax];
};
// width-4 NAF of the NB-bit integer k[0 .. NW) (little-endian words): out[i] in {0, +-1, +-3, +-5, +-7}, i <= NB; returns
// the number of digits (highest nonzero position + 1).  One bit of carry instead of a multi-word subtraction: the window
// at a set bit is taken with the carry added, a window value >= 8 becomes value - 16 and carries into the bit after it.
template <int NW>
__device__ __forceinline__ int wnaf4_words(const uint32_t* k, int nbits, bool negate, signed char* out) {
  auto bits = [&](int at, int cnt) -> unsigned {      // k[at .. at + cnt), cnt <= 4 (bits past the top are zero)
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < NW; j++) {
      lo = (at >> 5) == j ? k[j] : lo;
      hi = (at >> 5) + 1 == j ? k[j] : hi;
    }
    const uint64_t v = ((uint64_t)hi << 32 | lo) >> (at & 31);
    return (unsigned)v & ((1u << cnt) - 1u);
  };
  int len = 0;
  unsigned carry = 0;
  for (int i = 0; i <= nbits + 4; i++) out[i] = 0;
  int bit = 0;
  while (bit <= nbits) {
    if (bits(bit, 1) == carry) { bit++; continue; }
    int word = (int)(bits(bit, 4) + carry);
    carry = (unsigned)(word >> 3) & 1u;
    word -= (int)(carry << 4);
    out[bit] = (signed char)(negate ? -word : word);
    len = bit + 1;
    bit += 4;
  }
  return len;
}
// k p; p, k (NW canonical little-endian words) and the result uniform across the wave; `lds` is this wave's alone
// ALLOW_SPLIT = false: never split (a caller whose points need not be in the order-r subgroup of a cofactor-one group
// either -- there is none today -- or that wants one code path for all groups).
// Several waves of one workgroup may run chains side by side, each on its own `lds`: the two barriers below are WORKGROUP
// barriers, reached by every wave exactly twice whatever its point and scalar (no early return in front of them).
template <class F, int NW, bool ALLOW_SPLIT>
__device__ __forceinline__ XYZZ29<F> scalar_mul_lane29(const XYZZ29<F>& p_in, const uint32_t* k, ScalarMulLds<F>* lds);
template <class F, int NW>
__device__ __forceinline__ XYZZ29<F> scalar_mul_two_waves_lane29(const XYZZ29<F>& p_in, const uint32_t* k,
                                                                 ScalarMulLds<F>* lds, XYZZ29<F>* xchg);
template <class F, int NW, bool ALLOW_SPLIT = true>
__device__ __forceinline__ XYZZ29<F> scalar_mul_wave29(const XYZZ29<F>& p_in, const uint32_t* k, ScalarMulLds<F>* lds) {
  if constexpr (lane29::enabled<F>()) return scalar_mul_lane29<F, NW, ALLOW_SPLIT>(p_in, k, lds);   // (lane29.h)
  constexpr int BS = XYZZ29<F>::BS;
  constexpr bool SPLIT = ALLOW_SPLIT && GlvOf<F>::enabled && GlvCofactorOne<F>::value && NW == 8;
  const unsigned lane = __lane_id();
  const bool p_inf = p_in.is_inf();
  // (the identity runs the chain on a stand-in so that the barriers are reached; the result is discarded)
  XYZZ29<F> p = p_in;
  if (p_inf) { p.x = FieldOf<F>::one(); p.y = FieldOf<F>::one(); p.zz = FieldOf<F>::one(); p.zzz = FieldOf<F>::one(); }
  // the table of odd multiples (a doubling and three additions on the wave)
  {
    const XYZZ29<F> p2 = dbl_wave29(p);
    XYZZ29<F> m = p;
#pragma unroll 1
    for (int j = 0; j < 4; j++) {
      if (j) m = add_wave29(m, p2);
      if (lane == 0) lds->tab[j] = m;
    }
  }
  int len = 0;
  if constexpr (SPLIT) {
    using GC = typename GlvOf<F>::C;
    uint32_t h[2][8];
    glv::split<GC>(k, h[0], h[1]);
    // lanes 0 and 1 recode one half each; phi(x, y) = (BETA x, y): x_affine = X / ZZ, so only X changes
    if (lane < 2) {
      uint32_t w[5];
#pragma unroll
      for (int i = 0; i < 4; i++) w[i] = lane ? h[1][i] : h[0][i];
      w[4] = 0;
      const bool neg_half = ((lane ? h[1][7] : h[0][7]) >> 31) != 0;
      len = wnaf4_words<5>(w, 128, neg_half, lds->naf[lane]);
    }
    __syncthreads();
    {
      Fp<typename FieldOf<F>::Params> beta32;
#pragma unroll
      for (int i = 0; i < Fp<typename FieldOf<F>::Params>::NL; i++) beta32.l[i] = GC::BETA[i];
      const auto beta = FieldOf<F>::from32(beta32);
      const unsigned slot = (lane & 15) >> 2;
      const XYZZ29<F> t = lds->tab[slot];
      const auto bx = fit<BS>(t.x * beta);
      if ((lane & 3) == 0 && lane < 16) {
        XYZZ29<F> e = t;
        e.x = bx;
        lds->tab[4 + slot] = e;
      }
    }
    len = max(__shfl(len, 0), __shfl(len, 1));
  } else {
    if (lane == 0) len = wnaf4_words<NW>(k, NW * 32, false, lds->naf[0]);
    len = __shfl(len, 0);
  }
  __syncthreads();
  XYZZ29<F> acc = XYZZ29<F>::inf();
#pragma unroll 1
  for (int i = len - 1; i >= 0; i--) {
    acc = dbl_wave29(acc);
#pragma unroll 1
    for (int hf = 0; hf < (SPLIT ? 2 : 1); hf++) {
      const int d = lds->naf[hf][i];
      if (d == 0) continue;
      XYZZ29<F> o = lds->tab[4 * hf + ((d < 0 ? -d : d) >> 1)];
      const auto ny = fit<BS>(neg(o.y));
      o.y = select(d < 0, ny, o.y);
      acc = add_wave29(acc, o);
    }
  }
  return p_inf ? p_in : acc;
}

// The same product on TWO waves of one workgroup, for a group whose scalars split (GlvOf + GlvCofactorOne): wave h runs the
// NAF chain of half h alone -- 127 doublings + ~25 additions each instead of 127 + ~51 on one wave -- over its own table (wave
// 1's entries are phi of wave 0's: X times BETA), and wave 0 adds the two results.  The chain was the critical path of a
// small proof (BASELINE config 4: prover_stage1_g1_kernel 0.61 of 1.95 ms, profiles/r6f_timeline_config4.md).
// Both waves call this with the same arguments; the result is valid in wave 0 (threadIdx.x < 64).
template <class F>
constexpr bool scalar_mul_splits() {
  return GlvOf<F>::enabled && GlvCofactorOne<F>::value;
}
template <class F, int NW>
__device__ __forceinline__ XYZZ29<F> scalar_mul_two_waves29(const XYZZ29<F>& p_in, const uint32_t* k, ScalarMulLds<F>* lds,
                                                            XYZZ29<F>* xchg) {
  static_assert(NW == 8, "eight-word scalars");
  if constexpr (lane29::enabled<F>()) return scalar_mul_two_waves_lane29<F, NW>(p_in, k, lds, xchg);   // (lane29.h)
  constexpr int BS = XYZZ29<F>::BS;
  using GC = typename GlvOf<F>::C;
  const unsigned lane = __lane_id(), h = (threadIdx.x >> 6) & 1u;
  const bool p_inf = p_in.is_inf();
  XYZZ29<F> p = p_in;      // (the identity runs the chain on a stand-in so that the barriers are reached)
  if (p_inf) { p.x = FieldOf<F>::one(); p.y = FieldOf<F>::one(); p.zz = FieldOf<F>::one(); p.zzz = FieldOf<F>::one(); }
  {
    Fp<typename FieldOf<F>::Params> beta32;
#pragma unroll
    for (int i = 0; i < Fp<typename FieldOf<F>::Params>::NL; i++) beta32.l[i] = GC::BETA[i];
    const auto beta = FieldOf<F>::from32(beta32);
    const XYZZ29<F> p2 = dbl_wave29(p);
    XYZZ29<F> m = p;
#pragma unroll 1
    for (int j = 0; j < 4; j++) {
      if (j) m = add_wave29(m, p2);
      XYZZ29<F> e = m;
      const auto bx = fit<BS>(m.x * beta);            // phi(x, y) = (BETA x, y): x_affine = X / ZZ, so only X changes
      e.x = select(h != 0, bx, m.x);
      if (lane == 0) lds->tab[4 * h + j] = e;
    }
  }
  uint32_t hv[2][8];
  glv::split<GC>(k, hv[0], hv[1]);
  int len = 0;
  if (lane == 0) {
    uint32_t w[5];
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = h ? hv[1][i] : hv[0][i];
    w[4] = 0;
    len = wnaf4_words<5>(w, 128, ((h ? hv[1][7] : hv[0][7]) >> 31) != 0, lds->naf[h]);
  }
  len = __shfl(len, 0);
  __syncthreads();
  XYZZ29<F> acc = XYZZ29<F>::inf();
#pragma unroll 1
  for (int i = len - 1; i >= 0; i--) {
    acc = dbl_wave29(acc);
    const int d = lds->naf[h][i];
    if (d == 0) continue;
    XYZZ29<F> o = lds->tab[4 * h + ((d < 0 ? -d : d) >> 1)];
    const auto ny = fit<BS>(neg(o.y));
    o.y = select(d < 0, ny, o.y);
    acc = add_wave29(acc, o);
  }
  if (h == 1 && lane == 0) *xchg = acc;
  __syncthreads();
  if (h == 0) acc = add_wave29(acc, *xchg);
  return p_inf ? p_in : acc;
}

// ---- the same chains in LIMB-PER-LANE form (lane29.h) for the nine-limb base fields ----------------------------------
// One register per coordinate, a column-parallel product on each row of 16 lanes, the four products of a level on the four
// rows: a doubling 0.85 us instead of 2.1, an addition ~1.1 instead of 3.2 (profiles/r6l_lane29_probe.txt).  The table
// of odd multiples lives in the same LDS slots in raw lane form (lane29::store_pt_raw); p_in, k and the result are what
// the forms above take and return.
template <class F, int NW, bool ALLOW_SPLIT>
__device__ __forceinline__ XYZZ29<F> scalar_mul_lane29(const XYZZ29<F>& p_in, const uint32_t* k, ScalarMulLds<F>* lds) {
  using P = typename FieldOf<F>::Params;
  using FO = lane29::Ops<F>;
  using LPt = lane29::Pt<FO>;
  constexpr bool SPLIT = ALLOW_SPLIT && GlvOf<F>::enabled && GlvCofactorOne<F>::value && NW == 8 && !FO::EXT;
  const unsigned lane = __lane_id();
  typename FO::KT kc;
  kc.init();
  const bool p_inf = p_in.is_inf();
  LPt p = lane29::to_pt<F>(kc, p_in);
  if (p_inf) p = {FO::one(kc), FO::one(kc), FO::one(kc), FO::one(kc), false};   // (stand-in: the barriers below must be reached)
  {
    const LPt p2 = lane29::dbl_pt<FO>(kc, p);
    LPt m = p;
#pragma unroll 1
    for (int j = 0; j < 4; j++) {
      if (j) m = lane29::add_pt<FO>(kc, m, p2);
      lane29::store_pt_raw<F>(kc, &lds->tab[j], m);
    }
  }
  int len = 0;
  if constexpr (SPLIT) {
    using GC = typename GlvOf<F>::C;
    uint32_t h[2][8];
    glv::split<GC>(k, h[0], h[1]);
    if (lane < 2) {
      uint32_t w[5];
#pragma unroll
      for (int i = 0; i < 4; i++) w[i] = lane ? h[1][i] : h[0][i];
      w[4] = 0;
      const bool neg_half = ((lane ? h[1][7] : h[0][7]) >> 31) != 0;
      len = wnaf4_words<5>(w, 128, neg_half, lds->naf[lane]);
    }
    __syncthreads();
    {
      // phi(x, y) = (BETA x, y): row j of the wave takes entry j -- one product for the four entries
      Fp<P> beta32;
#pragma unroll
      for (int i = 0; i < Fp<P>::NL; i++) beta32.l[i] = GC::BETA[i];
      const uint32_t beta = FO::template from_regs<XYZZ29<F>::BS>(kc, FieldOf<F>::from32(beta32));
      const uint32_t* src = reinterpret_cast<const uint32_t*>(&lds->tab[kc.row]);
      uint32_t* dst = reinterpret_cast<uint32_t*>(&lds->tab[4 + kc.row]);
      const bool on = kc.l16 < 9u;
      const unsigned i = on ? kc.l16 : 0u;
      const uint32_t bx = lane29::mul(kc, on ? src[i] : 0u, beta);
      if (on) {
        dst[i] = bx;
        dst[9 + i] = src[9 + i];
        dst[18 + i] = src[18 + i];
        dst[27 + i] = src[27 + i];
      }
    }
    len = max(__shfl(len, 0), __shfl(len, 1));
  } else {
    if (lane == 0) len = wnaf4_words<NW>(k, NW * 32, false, lds->naf[0]);
    len = __shfl(len, 0);
  }
  __syncthreads();
  LPt acc = lane29::inf_pt<FO>(kc);
#pragma unroll 1
  for (int i = len - 1; i >= 0; i--) {
    acc = lane29::dbl_pt<FO>(kc, acc);
#pragma unroll 1
    for (int hf = 0; hf < (SPLIT ? 2 : 1); hf++) {
      const int d = lds->naf[hf][i];
      if (d == 0) continue;
      LPt o = lane29::load_pt<F>(kc, &lds->tab[4 * hf + ((d < 0 ? -d : d) >> 1)]);
      if (d < 0) o = lane29::neg_pt<FO>(kc, o);
      acc = lane29::add_pt<FO>(kc, acc, o);
    }
  }
  return p_inf ? p_in : lane29::from_pt<F>(kc, acc);
}
template <class F, int NW>
__device__ __forceinline__ XYZZ29<F> scalar_mul_two_waves_lane29(const XYZZ29<F>& p_in, const uint32_t* k,
                                                                 ScalarMulLds<F>* lds, XYZZ29<F>* xchg) {
  using P = typename FieldOf<F>::Params;
  using GC = typename GlvOf<F>::C;
  using FO = lane29::Ops<F>;
  using LPt = lane29::Pt<FO>;
  static_assert(!FO::EXT, "the endomorphism split of a cofactor-one G1");
  const unsigned lane = __lane_id(), h = (threadIdx.x >> 6) & 1u;
  typename FO::KT kc;
  kc.init();
  const bool p_inf = p_in.is_inf();
  LPt p = lane29::to_pt<F>(kc, p_in);
  if (p_inf) p = {FO::one(kc), FO::one(kc), FO::one(kc), FO::one(kc), false};
  {
    Fp<P> beta32;
#pragma unroll
    for (int i = 0; i < Fp<P>::NL; i++) beta32.l[i] = GC::BETA[i];
    const uint32_t beta = FO::template from_regs<XYZZ29<F>::BS>(kc, FieldOf<F>::from32(beta32));
    if (h) p.x = lane29::mul(kc, p.x, beta);          // wave 1 runs its chain over phi(P) = (BETA x, y)
    const LPt p2 = lane29::dbl_pt<FO>(kc, p);
    LPt m = p;
#pragma unroll 1
    for (int j = 0; j < 4; j++) {
      if (j) m = lane29::add_pt<FO>(kc, m, p2);
      lane29::store_pt_raw<F>(kc, &lds->tab[4 * h + j], m);
    }
  }
  uint32_t hv[2][8];
  glv::split<GC>(k, hv[0], hv[1]);
  int len = 0;
  if (lane == 0) {
    uint32_t w[5];
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = h ? hv[1][i] : hv[0][i];
    w[4] = 0;
    len = wnaf4_words<5>(w, 128, ((h ? hv[1][7] : hv[0][7]) >> 31) != 0, lds->naf[h]);
  }
  len = __shfl(len, 0);
  __syncthreads();
  LPt acc = lane29::inf_pt<FO>(kc);
#pragma unroll 1
  for (int i = len - 1; i >= 0; i--) {
    acc = lane29::dbl_pt<FO>(kc, acc);
    const int d = lds->naf[h][i];
    if (d == 0) continue;
    LPt o = lane29::load_pt<F>(kc, &lds->tab[4 * h + ((d < 0 ? -d : d) >> 1)]);
    if (d < 0) o = lane29::neg_pt<FO>(kc, o);
    acc = lane29::add_pt<FO>(kc, acc, o);
  }
  if (h == 1) lane29::store_pt_raw<F>(kc, xchg, acc);
  __syncthreads();
  if (h == 0) acc = lane29::add_pt<FO>(kc, acc, lane29::load_pt<F>(kc, xchg));
  return p_inf ? p_in : lane29::from_pt<F>(kc, acc);
}
// sum of n points in memory (proper XYZZ29s), uniform result: the chains that only add (the king's combination, the
// terms of prove::A / B / C)
template <class F>
__device__ __forceinline__ XYZZ29<F> sum_points_wave(const XYZZ29<F>* pts, unsigned n) {
  if constexpr (lane29::enabled<F>()) {
    using FO = lane29::Ops<F>;
    typename FO::KT kc;
    kc.init();
    lane29::Pt<FO> acc = lane29::inf_pt<FO>(kc);
#pragma unroll 1
    for (unsigned i = 0; i < n; i++) acc = lane29::add_pt<FO>(kc, acc, lane29::load_pt<F>(kc, &pts[i]));
    return lane29::from_pt<F>(kc, acc);
  } else {
    XYZZ29<F> acc = XYZZ29<F>::inf();
#pragma unroll 1
    for (unsigned i = 0; i < n; i++) acc = add_wave29(acc, pts[i]);
    return acc;
  }
}

// the same sum as an affine point (the king's combination hands affine points to the parties)
template <class F>
__device__ __forceinline__ Affine<F> sum_points_affine_wave(const XYZZ29<F>* pts, unsigned n) {
  if constexpr (lane29::enabled<F>()) {
    using FO = lane29::Ops<F>;
    typename FO::KT kc;
    kc.init();
    lane29::Pt<FO> acc = lane29::inf_pt<FO>(kc);
#pragma unroll 1
    for (unsigned i = 0; i < n; i++) acc = lane29::add_pt<FO>(kc, acc, lane29::load_pt<F>(kc, &pts[i]));
    return lane29::to_affine<F>(kc, acc);
  } else {
    return sum_points_wave<F>(pts, n).to_xyzz32().to_affine();
  }
}

// ---- 6: Horner tail ---------------------------------------------------------------------------------
// W*c dependent doublings: inherently serial in the group, but not inside one doubling.  One wave runs the
// chain; the 9 multiplications of an XYZZ doubling form 3 dependency levels (2 | 4 | 3 products), each level
// is evaluated by different lanes at once and shared with readlane.  An Fq2 product is itself spread over three
// lanes of a quad (Karatsuba).  One thread per MSM took 2.5 ms (G1) / 10.2 ms (G2) for the 256 doublings of a
// 2^20-point MSM, as long as the bucket accumulation itself.  (Round 4: the chain runs on the reduced-radix types.)
template <class F>
__global__ void __launch_bounds__(64) msm_tail_kernel(const XYZZ29<F>* __restrict__ window_sums, MsmGeom g,
                                                       int affine, F* __restrict__ out) {
  __builtin_amdgcn_s_setprio(DG16_CHAIN_PRIO);   // latency-bound chain: issue ahead of the accumulation waves sharing the SIMD
  // one wave per MSM instance (blockIdx.x), every lane carries the same running total (internal form: dbl_wave29)
  window_sums += (size_t)blockIdx.x * g.bw;
  out += (size_t)blockIdx.x * (affine ? 2 : 3);
  XYZZ29<F> acc = XYZZ29<F>::inf();
  if constexpr (lane29::enabled<F>()) {          // limb-per-lane chain (lane29.h): 0.85 us per doubling instead of 2.1
    using FO = lane29::Ops<F>;
    typename FO::KT kc;
    kc.init();
    lane29::Pt<FO> a = lane29::inf_pt<FO>(kc);
#pragma unroll 1
    for (int w = (int)g.bw - 1; w >= 0; w--) {
#pragma unroll 1
      for (unsigned k = 0; k < g.c; k++) a = lane29::dbl_pt<FO>(kc, a);
      a = lane29::add_pt<FO>(kc, a, lane29::load_pt<F>(kc, &window_sums[w]));
    }
    if (affine) {            // (X / ZZ, Y / ZZZ) with the inversion in lane form as well (lane29::to_affine)
      const Affine<F> r = lane29::to_affine<F>(kc, a);
      if (threadIdx.x == 0) {
        out[0] = r.x;
        out[1] = r.y;
      }
      return;
    }
    acc = lane29::from_pt<F>(kc, a);
  } else {
#pragma unroll 1
    for (int w = (int)g.bw - 1; w >= 0; w--) {
#pragma unroll 1
      for (unsigned k = 0; k < g.c; k++) acc = dbl_wave29(acc);
      acc = add_wave29(acc, window_sums[w]);
    }
  }
  if (threadIdx.x != 0) return;
  using FO = FieldOf<F>;
  if (affine) {
    Affine<F> a = acc.to_xyzz32().to_affine();
    out[0] = a.x;
    out[1] = a.y;
  } else if (acc.is_inf()) {
    out[0] = F::one();
    out[1] = F::one();
    out[2] = F::zero();
  } else {
    // (X ZZ, Y ZZZ, ZZ) is the same point in Jacobian coordinates with Z = ZZ (ec.h: XYZZ::to_jacobian)
    out[0] = FO::to32(fit<FO::BS>(acc.x * acc.zz));
    out[1] = FO::to32(fit<FO::BS>(acc.y * acc.zzz));
    out[2] = FO::to32(acc.zz);
  }
}

// Launched by msm_bucket_phase (msm_reduce.hip) but INSTANTIATED in msm_group.hip: the chain's products stay inline for
// every group (a call per level cost the G2 tail 8 us per operation against 3 for G1's inline form).
template <class F>
void msm_tail_phase(hipStream_t s, const MsmSort& st, const MsmBuffers<F>& b, bool out_affine, void* out_dev) {
  hipLaunchKernelGGL(msm_tail_kernel<F>, dim3(b.ninst), dim3(64), 0, s, b.window_sums, st.g, (int)out_affine, (F*)out_dev);
}

}  // namespace dg16
