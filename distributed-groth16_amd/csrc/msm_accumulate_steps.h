// MSM phase 4 for the G2 of the 14-limb curves: the accumulation as a step loop over three product sites, with the
// temporaries parked in the accumulation-register file through asm (DG_ACC_* / AccReg; tools/check_agpr_file.py guards
// that file).  xyzz_add_into_steps is shared with msm_finalize_lds_kernel (msm_finalize.h).  Pipeline: msm_impl.h.
#pragma once
#include "msm_accumulate.h"

namespace dg16 {

// ---- 4 (G2 of the 14-limb curves): the same accumulation as a STEP LOOP over three product sites ---------------------
// Inlined, an Fq2 mixed addition of a 14-limb curve is a 100-KB loop (eleven Fq2 products) run by one wave per SIMD against
// the 64-KB instruction cache two CUs share: 9 ms per 2^20-point launch on some boxes of the pool, 18 on others, same
// binary; products behind calls cost a dozen scratch accesses each (14.4 ms everywhere).  Here a mixed addition is a loop
// of NINE steps over THREE sites -- one Fq2 product (visited six times), one Fq2 square (twice) and the fused
// Y3 = R (Q - X3) - PPP Y1 (once) -- with a wave-uniform switch in front of a site to route its operands and one behind it
// to route the result:
//     0  P = x2 ZZ - X1      1  R = y2 ZZZ - Y1      2  PP = P^2      3  PPP = P PP      4  ZZ <- ZZ PP
//     5  ZZZ <- ZZZ PPP      6  Q = X1 PP            7  X3 = R^2 - PPP - 2 Q (-> X1), T = Q - X3      8  Y1 <- R T - PPP Y1
// The same 10 584 v_mad_u64_u32 per addition as the straight-line form, in a loop that stays in the instruction cache;
// values and the order of operations inside a product are those of the straight-line form (parity tests unchanged).
// The accumulator (X1, Y1, ZZ, ZZZ) lives in LDS columns; the four temporaries (P -> Q, R, PP -> T, PPP) in a FILE of
// accumulation registers at FIXED numbers a[kAccFileBase + 28 slot + i] named in asm statements (gfx950: 256 AGPRs next to
// the 256 VGPRs of a wave at one wave per SIMD) -- machine state the compiler does not see: as C++ values (in VGPRs, or in
// AGPRs through "=a" / "+a" operands) the step switch turned them into phis that hipcc merged with 270-330 copies per visit
// of a site against the 84 the routing needs.
constexpr int kAccFileBase = 144;
// Round 6 -- what round 5's abort was: a clobber list is NOT a reservation.  The first form named
// two registers ("a144", "a255": enough for the resource accounting) and hipcc, which needed 160 spill registers in the
// step-loop form of the 14-limb G2 FINALIZE, put sixteen of its own values -- hoisted operand addresses -- into
// a[144..159]; acc_set<0> then overwrote them and the next reload used field limbs as an address
// (HSA_STATUS_ERROR_MEMORY_APERTURE_VIOLATION; reproduced at the first call on the all-equal-points shape of
// dmsm/mod.rs:155-159, profiles/r6a_*).  tests/test_kernel_isa.py could not see it: in a disassembly the compiler's
// v_accvgpr_write looks like acc_set's.  Now (i) every write NAMES its register as clobbered, so the compiler never keeps a
// value of its own in a file register across an acc_set; (ii) the kernel declares all 112; (iii) tools/check_agpr_file.py
// reads the compiler's assembly (-save-temps), where the asm statements are bracketed by ASMSTART / ASMEND, and FAILS THE
// BUILD (csrc/Makefile) if any instruction of the compiler's own touches a[144..255] in a kernel that uses the file.
#define DG_ACC_REGS_LO(X) X(144) X(145) X(146) X(147) X(148) X(149) X(150) X(151) X(152) X(153) X(154) X(155) X(156) X(157) X(158) X(159) X(160) X(161) X(162) X(163) X(164) X(165) X(166) X(167) X(168) X(169) X(170) X(171) X(172) X(173) X(174) X(175) X(176) X(177) X(178) X(179) X(180) X(181) X(182) X(183) X(184) X(185) X(186) X(187) X(188) X(189) X(190) X(191) X(192) X(193) X(194) X(195) X(196) X(197) X(198) X(199)
#define DG_ACC_REGS_HI(X) X(200) X(201) X(202) X(203) X(204) X(205) X(206) X(207) X(208) X(209) X(210) X(211) X(212) X(213) X(214) X(215) X(216) X(217) X(218) X(219) X(220) X(221) X(222) X(223) X(224) X(225) X(226) X(227) X(228) X(229) X(230) X(231) X(232) X(233) X(234) X(235) X(236) X(237) X(238) X(239) X(240) X(241) X(242) X(243) X(244) X(245) X(246) X(247) X(248) X(249) X(250) X(251) X(252) X(253) X(254)
// -DDG16_ACC_CLOBBER_R5: round 5's declaration (two registers named, nothing on the writes) -- the NEGATIVE CONTROL of
// tools/abort_hunt.sh and tests/test_kernel_isa.py: built that way the 14-limb G2 finalize collides again, and
// tools/check_agpr_file.py must say so (the Makefile then refuses the object: pass AGPR_CHECK=../../tools/true.py to get the
// library anyway).
#ifdef DG16_ACC_CLOBBER_R5
#define DG_ACC_WRITE_CLOBBER(n)
#else
#define DG_ACC_WRITE_CLOBBER(n) : "a" #n
#endif
template <int R> struct AccReg;
#define X(n)                                                                                             \
  template <> struct AccReg<n> {                                                                         \
    static __device__ __forceinline__ void w(uint32_t v) {                                               \
      asm volatile("v_accvgpr_write_b32 a" #n ", %0" ::"v"(v) DG_ACC_WRITE_CLOBBER(n));                  \
    }                                                                                                    \
    static __device__ __forceinline__ uint32_t r() {                                                     \
      uint32_t v;                                                                                        \
      asm volatile("v_accvgpr_read_b32 %0, a" #n : "=v"(v));                                             \
      return v;                                                                                          \
    }                                                                                                    \
  };
DG_ACC_REGS_LO(X) DG_ACC_REGS_HI(X) X(255)
#undef X
// all registers of the file, for the kernel's one declaration (resource accounting: the wave is allocated them)
#define X(n) "a" #n,
#ifdef DG16_ACC_CLOBBER_R5
#define DG_ACC_FILE_CLOBBERS "a144", "a255"
#else
#define DG_ACC_FILE_CLOBBERS DG_ACC_REGS_LO(X) DG_ACC_REGS_HI(X) "a255"
#endif
template <int BASE, int N, class P, int B, int... I>
__device__ __forceinline__ void acc_set_seq(const Fe2<P, B, 1>& v, std::integer_sequence<int, I...>) {
  ((AccReg<BASE + I>::w(v.c0.l[I]), AccReg<BASE + N + I>::w(v.c1.l[I])), ...);
}
template <int BASE, int N, class P, int B, int... I>
__device__ __forceinline__ void acc_get_seq(Fe2<P, B, 1>& v, std::integer_sequence<int, I...>) {
  ((v.c0.l[I] = AccReg<BASE + I>::r(), v.c1.l[I] = AccReg<BASE + N + I>::r()), ...);
}
template <int SLOT, class P, int B>
__device__ __forceinline__ void acc_set(const Fe2<P, B, 1>& v) {
  constexpr int N = RR<P>::N;
  static_assert(kAccFileBase + 2 * N * (SLOT + 1) <= 256, "slot inside the file");
  acc_set_seq<kAccFileBase + 2 * N * SLOT, N>(v, std::make_integer_sequence<int, N>{});
}
template <int SLOT, class P, int B>
__device__ __forceinline__ Fe2<P, B, 1> acc_get() {
  constexpr int N = RR<P>::N;
  Fe2<P, B, 1> v;
  acc_get_seq<kAccFileBase + 2 * N * SLOT, N>(v, std::make_integer_sequence<int, N>{});
  return v;
}
// d += b (full XYZZ addition, XYZZ29::add_into) as a STEP LOOP over the same three product sites: the 14-limb G2 finalize
// (msm_finalize_lds_kernel: two lanes per bucket summing the bucket's partials) inlined a 144-KB addition -- 35 900
// instructions with its doubling branch -- and ran at 16 % of its issue rate on the slow boxes of the pool.
//     0  U1 = X1 ZZ2 -> X1      1  S1 = Y1 ZZZ2 -> Y1      2  P = X2 ZZ1 - U1      3  R = Y2 ZZZ1 - S1
//     4  PP = P^2               5  PPP = P PP              6  T = ZZ1 ZZ2          7  ZZ3 = T PP
//     8  T = ZZZ1 ZZZ2          9  ZZZ3 = T PPP           10  Q = U1 PP           11  X3 = R^2 - PPP - 2 Q
//    12  Y3 = R (Q - X3) - PPP S1
// d: accumulator in LDS columns (get / put); b: read-only operand behind an accessor (memory or LDS), intact throughout, so
// the rare d == b case doubles b.  Needs the accumulation-register file of the calling kernel (kAccFileBase).
template <class F, class D, class B>
__device__ __forceinline__ void xyzz_add_into_steps(const D& d, const B& b_) {
  using FO = FieldOf<F>;
  using P = typename FO::Params;
  constexpr int BS = FO::BS;
  constexpr int BG = 640;
  using G = Fe2<P, BG, 1>;
  if (limbs_all_zero(b_.get(2))) return;
  if (limbs_all_zero(d.get(2))) {
    d.put(0, b_.get(0)); d.put(1, b_.get(1)); d.put(2, b_.get(2)); d.put(3, b_.get(3));
    return;
  }
  B b = b_;
  auto dg = [&](int c) { return d.get(c).template as<BG, 1>(); };
  auto bg = [&](int c) { return b.get(c).template as<BG, 1>(); };
  int special = 0;
  bool p_zero = false;
#pragma unroll 1
  for (int step = 0; step < 13; step++) {
    asm volatile("" : "+s"(step));          // opaque: the sites must not be cloned per step
    b.launder();                            // ... and the operand's 112 word addresses not hoisted out of the loop (they
                                            // were: 224 registers of pointers, 932 B of scratch per lane)
    if (step == 4 || step == 11) {
      const G a = step == 4 ? acc_get<0, P, BG>() : acc_get<1, P, BG>();
      const auto c = sqr(a);
      if (step == 4) {
        acc_set<2>(c.template as<BG, 1>());                             // PP
      } else {
        const auto ppp = acc_get<3, P, 128>(), q_ = acc_get<0, P, 128>();
        const auto x3 = fit<BS>(c - (ppp + dbl(q_)));
        d.put(0, x3);
        acc_set<2>(fit<BG>(q_ - x3));                                   // Q - X3
      }
    } else if (step == 12) {
      const auto r_ = acc_get<1, P, BG>(), t_ = acc_get<2, P, BG>();
      const auto ppp = acc_get<3, P, 128>();
      d.put(1, fit<BS>(mul_sub(r_, t_, ppp, d.get(1))));                // R (Q - X3) - PPP S1
    } else {
      G a, bb;
      switch (step) {
        case 0: a = dg(0); bb = bg(2); break;                            // X1 ZZ2
        case 1: a = dg(1); bb = bg(3); break;                            // Y1 ZZZ2
        case 2: a = bg(0); bb = dg(2); break;                            // X2 ZZ1
        case 3: a = bg(1); bb = dg(3); break;                            // Y2 ZZZ1
        case 5: a = acc_get<0, P, BG>(); bb = acc_get<2, P, BG>(); break;   // P PP
        case 6: a = dg(2); bb = bg(2); break;                            // ZZ1 ZZ2
        case 7: a = acc_get<0, P, BG>(); bb = acc_get<2, P, BG>(); break;   // (ZZ1 ZZ2) PP
        case 8: a = dg(3); bb = bg(3); break;                            // ZZZ1 ZZZ2
        case 9: a = acc_get<0, P, BG>(); bb = acc_get<3, P, BG>(); break;   // (ZZZ1 ZZZ2) PPP
        default: a = dg(0); bb = acc_get<2, P, BG>(); break;             // U1 PP
      }
      const auto c = a * bb;
      switch (step) {
        case 0: d.put(0, c.template as<BS, 1>()); break;                 // U1
        case 1: d.put(1, c.template as<BS, 1>()); break;                 // S1
        case 2: {
          const auto p_ = fit<BG>(c - d.get(0));
          p_zero = is_zero_compact(p_);
          acc_set<0>(p_);
          break;
        }
        case 3: {
          const auto r_ = fit<BG>(c - d.get(1));
          if (p_zero) special = is_zero_compact(r_) ? 1 : 2;
          acc_set<1>(r_);
          break;
        }
        case 5: acc_set<3>(c.template as<BG, 1>()); break;               // PPP
        case 6: acc_set<0>(c.template as<BG, 1>()); break;
        case 7: d.put(2, c.template as<BS, 1>()); break;                 // ZZ3
        case 8: acc_set<0>(c.template as<BG, 1>()); break;
        case 9: d.put(3, c.template as<BS, 1>()); break;                 // ZZZ3
        default: acc_set<0>(c.template as<BG, 1>()); break;              // Q
      }
      if (special) break;
    }
  }
  if (special == 1) {
    const XYZZ29<F> t = XYZZ29<F>{b.get(0), b.get(1), b.get(2), b.get(3)}.dbl_pt();
    d.put(0, t.x); d.put(1, t.y); d.put(2, t.zz); d.put(3, t.zzz);
  } else if (special == 2) {
    d.put(2, FO::zero());                                              // the identity: zz = 0
  }
}

template <class F, int BLOCK>
__global__ void __launch_bounds__(BLOCK, 1)
msm_accumulate_steps_kernel(MsmBases bases, size_t n, MsmGeom g,
                            const unsigned* __restrict__ offsets, const unsigned* __restrict__ counts,
                            const unsigned* __restrict__ seg_off, const unsigned* __restrict__ seg_total,
                            const unsigned* __restrict__ entries, XYZZ29<F>* __restrict__ seg_sum,
                            XYZZ29<F>* __restrict__ buckets, unsigned long long* __restrict__ clk) {
  ClkProbe probe;
  probe.begin(clk);
  using FO = FieldOf<F>;
  using P = typename FO::Params;
  using S = typename FO::Store;
  constexpr int BS = FO::BS;
  constexpr int BG = 640;                    // every operand of a site is below 10 p (P, R, Q - X3: < 9.3 p)
  using G = Fe2<P, BG, 1>;
  static_assert(kAccFileBase + 4 * 2 * RR<P>::N <= 256, "four temporaries in the accumulation registers");
  constexpr int WORDS = sizeof(S) / 4;
  __shared__ uint32_t sh[4 * WORDS][BLOCK];
  const unsigned lane = threadIdx.x;
  auto ld = [&](int coord) {
    S v;
    uint32_t* w = reinterpret_cast<uint32_t*>(&v);
#pragma unroll
    for (int i = 0; i < WORDS; i++) w[i] = sh[coord * WORDS + i][lane];
    return v;
  };
  auto ldg = [&](int coord) { return ld(coord).template as<BG, 1>(); };
  auto st = [&](int coord, const S& v) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(&v);
#pragma unroll
    for (int i = 0; i < WORDS; i++) sh[coord * WORDS + i][lane] = w[i];
  };
  const unsigned w = blockIdx.y % g.bw;
  const uint32_t* __restrict__ base_tab = bases.p[blockIdx.y / g.bw];
  const unsigned t = blockIdx.x * BLOCK + threadIdx.x;
  const bool live = t < seg_total[w];
  SegRange sr{};
  if (live) sr = msm_segment(g, w, t, counts, seg_off);
  const unsigned cnt = live && DG_OK(2, (size_t)offsets[sr.bslot] + sr.first + sr.cnt, g.region + 1) ? sr.cnt : 0u;
  const unsigned* e = entries + (size_t)w * g.region + (live ? offsets[sr.bslot] + sr.first : 0u);
  asm volatile("" ::: DG_ACC_FILE_CLOBBERS);   // the temporaries' registers belong to this wave (acc_set / acc_get)
  bool inf = true;
  unsigned cur = cnt ? e[0] : 0u;
  for (unsigned j = 0; j < cnt; j++) {
    const unsigned nxt = (j + 1 < cnt) ? e[j + 1] : 0u;
    const unsigned ent = cur;
    cur = nxt;
    const bool negate = ent >> 31;
    {
      const Affine29<F> q = load_internal<F>(base_tab, DG_IDX(3, ent & 0x7fffffffu, g.region));
      if (q.is_inf()) continue;
      const auto nqy = neg(q.y);
      const auto qy = select(negate, nqy, q.y.template as<decltype(nqy)::Bound, decltype(nqy)::Limb>());
      if (inf) {
        st(0, q.x.template as<BS, 1>()); st(1, fit<BS>(qy)); st(2, FO::one()); st(3, FO::one());
        inf = false;
        continue;
      }
      acc_set<0>(q.x.template as<BG, 1>());
      acc_set<1>(fit<BG>(qy));
    }
    int special = 0;                          // 1: the same point again (double it), 2: its inverse (identity)
    bool p_zero = false;
#pragma unroll 1
    for (int step = 0; step < 9; step++) {
      asm volatile("" : "+s"(step));          // opaque: the sites must not be cloned per step
      if (step == 2 || step == 7) {
        // ---- the squaring site: PP = P^2, then X3 = R^2 - PPP - 2 Q
        const G a = step == 2 ? acc_get<0, P, BG>() : acc_get<1, P, BG>();
        const auto c = sqr(a);
        if (step == 2) {
          acc_set<2>(c.template as<BG, 1>());
        } else {
          const auto ppp = acc_get<3, P, 128>(), q_ = acc_get<0, P, 128>();   // products: below 2 p
          const auto x3 = fit<BS>(c - (ppp + dbl(q_)));
          st(0, x3);
          acc_set<2>(fit<BG>(q_ - x3));                                 // Q - X3
        }
      } else if (step == 8) {
        // ---- the fused site: Y3 = R (Q - X3) - PPP Y1, one reduction per component
        const auto r_ = acc_get<1, P, BG>(), d_ = acc_get<2, P, BG>();
        const auto ppp = acc_get<3, P, 128>();
        st(1, fit<BS>(mul_sub(r_, d_, ppp, ld(1))));
      } else {
        // ---- the product site
        G a, b;
        switch (step) {
          case 0: a = acc_get<0, P, BG>(); b = ldg(2); break;              // x2 ZZ
          case 1: a = acc_get<1, P, BG>(); b = ldg(3); break;              // y2 ZZZ
          case 3: a = acc_get<0, P, BG>(); b = acc_get<2, P, BG>(); break;  // P PP
          case 4: a = ldg(2); b = acc_get<2, P, BG>(); break;              // ZZ PP
          case 5: a = ldg(3); b = acc_get<3, P, BG>(); break;              // ZZZ PPP
          default: a = ldg(0); b = acc_get<2, P, BG>(); break;             // X1 PP
        }
        const auto c = a * b;
        switch (step) {
          case 0: {
            const auto p_ = fit<BG>(c - ld(0));                           // P = U2 - X1
            p_zero = is_zero_compact(p_);
            acc_set<0>(p_);
            break;
          }
          case 1: {
            const auto r_ = fit<BG>(c - ld(1));                           // R = S2 - Y1
            if (p_zero) special = is_zero_compact(r_) ? 1 : 2;
            acc_set<1>(r_);
            break;
          }
          case 3: acc_set<3>(c.template as<BG, 1>()); break;            // PPP
          case 4: st(2, c.template as<BS, 1>()); break;                   // ZZ3
          case 5: st(3, c.template as<BS, 1>()); break;                   // ZZZ3
          default: acc_set<0>(c.template as<BG, 1>()); break;           // Q
        }
        if (special) break;
      }
    }
    if (special == 1) {
      const Affine29<F> q2 = load_internal<F>(base_tab, ent & 0x7fffffffu);
      const auto nq2 = neg(q2.y);
      const auto qy2 = select(negate, nq2, q2.y.template as<decltype(nq2)::Bound, decltype(nq2)::Limb>());
      const XYZZ29<F> d = XYZZ29<F>::dbl_affine(q2.x, qy2);
      st(0, d.x); st(1, d.y); st(2, d.zz); st(3, d.zzz);
      if constexpr (HasOrderTwoPoint<F>::value) inf = d.is_inf();       // (ec29.h) twice the point of order two
    } else if (special == 2) {
      inf = true;
    }
  }
  if (live) {
    XYZZ29<F> out = XYZZ29<F>::inf();
    if (!inf) out = XYZZ29<F>{ld(0), ld(1), ld(2), ld(3)};
    if (sr.k == 1) buckets[((size_t)blockIdx.y << g.log_nb) + (sr.bslot & (((size_t)1 << g.log_nb) - 1))] = out;
    else seg_sum[(size_t)blockIdx.y * g.seg_cap + DG_IDX(4, t, g.seg_cap)] = out;
  }
  probe.end(clk);
}

}  // namespace dg16
