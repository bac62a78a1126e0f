// The endomorphisms of the six groups (GlvOf): which groups have one wired, its dimension, its constants and its action
// on a point.  Host and device text (no kernels): the plain MSM (msm_glv.h) and the batched point multiplication
// (points_mul.h) both split scalars with it, and the host tests instantiate it with the host compiler.
#pragma once
#include "consts_gen.h"
#include "ec.h"
#include "glv.h"

namespace dg16 {

// ---- GLV for the plain G1 MSM (glv.h): 2n points (P_i, phi(P_i)), 127-bit half scalars, half the windows ------------
template <class F> struct GlvOf { static constexpr bool enabled = false; };
// phi(P) = LAMBDA P (psi(P) = LAMBDA P) holds for P in the order-r subgroup ONLY.  A group of cofactor one is that subgroup
// (BN254 G1); for every other group the split needs the caller's word that the bases are in it
// (DG16_F_BASES_IN_SUBGROUP) -- an on-curve point outside the subgroup (decoded with validate = 0, say) must still give
// the group element VariableBaseMSM::msm gives, so without the flag those groups run the unsplit path.
template <class F> struct GlvCofactorOne { static constexpr bool value = false; };
template <> struct GlvCofactorOne<Fp<bn254_fq_params>> { static constexpr bool value = true; };
// G1 of the three curves (j = 0): phi(x, y) = (BETA x, y)
template <class P, class GC>
struct GlvG1 {
  static constexpr bool enabled = true;
  static constexpr int DIM = 2;
  using C = GC;
  DG_HD static void endo(Affine<Fp<P>>& p) {
    Fp<P> beta;
#pragma unroll
    for (int k = 0; k < Fp<P>::NL; k++) beta.l[k] = GC::BETA[k];
    p.x = p.x * beta;
  }
  // the same map on a projective point: x = X / ZZ, so BETA scales X alone (the identity stays the identity)
  DG_HD static void endo_xyzz(XYZZ<Fp<P>>& p) {
    Fp<P> beta;
#pragma unroll
    for (int k = 0; k < Fp<P>::NL; k++) beta.l[k] = GC::BETA[k];
    p.x = p.x * beta;
  }
};
template <> struct GlvOf<Fp<bn254_fq_params>> : GlvG1<bn254_fq_params, bn254_glv_consts> {};
template <> struct GlvOf<Fp<bls12_381_fq_params>> : GlvG1<bls12_381_fq_params, bls12_381_glv_consts> {};
template <> struct GlvOf<Fp<bls12_377_fq_params>> : GlvG1<bls12_377_fq_params, bls12_377_glv_consts> {};
// G2 of the three curves: psi(x, y) = (GAMMA_X conj(x), GAMMA_Y conj(y)) = LAMBDA (x, y) (untwist, Frobenius, twist),
// LAMBDA a root of x^4 - x^2 + 1 mod r.  DIM = 4: the four-dimensional split (glv.h: split4) -- 4n points P, psi P,
// psi^2 P, psi^3 P and quarters of at most 65 bits; DIM = 2: split() over psi alone.
template <class P, class GC, int D>
struct GlvG2 {
  static constexpr bool enabled = true;
  static constexpr int DIM = D;
  using C = GC;
  using Fq = Fp<P>;
  DG_HD static void endo(Affine<Fp2<Fq>>& p) {
    if (p.is_inf()) return;
    Fp2<Fq> gx, gy;
#pragma unroll
    for (int k = 0; k < Fq::NL; k++) {
      gx.c0.l[k] = GC::GAMMA_X_C0[k]; gx.c1.l[k] = GC::GAMMA_X_C1[k];
      gy.c0.l[k] = GC::GAMMA_Y_C0[k]; gy.c1.l[k] = GC::GAMMA_Y_C1[k];
    }
    p.x = Fp2<Fq>{p.x.c0, p.x.c1.neg()} * gx;
    p.y = Fp2<Fq>{p.y.c0, p.y.c1.neg()} * gy;
  }
  // the same map on a projective point: conjugation is a field automorphism, so it goes through X / ZZ and Y / ZZZ
  // coordinate by coordinate (ZZ = 0 stays 0: the identity maps to itself)
  DG_HD static void endo_xyzz(XYZZ<Fp2<Fq>>& p) {
    Fp2<Fq> gx, gy;
#pragma unroll
    for (int k = 0; k < Fq::NL; k++) {
      gx.c0.l[k] = GC::GAMMA_X_C0[k]; gx.c1.l[k] = GC::GAMMA_X_C1[k];
      gy.c0.l[k] = GC::GAMMA_Y_C0[k]; gy.c1.l[k] = GC::GAMMA_Y_C1[k];
    }
    p.x = Fp2<Fq>{p.x.c0, p.x.c1.neg()} * gx;
    p.y = Fp2<Fq>{p.y.c0, p.y.c1.neg()} * gy;
    p.zz.c1 = p.zz.c1.neg();
    p.zzz.c1 = p.zzz.c1.neg();
  }
};
// BN254: LAMBDA ~ 2^127, so the TWO-dimensional split over psi alone is balanced too, and it is the faster one there
// (2^20 points: 6.93 ms against 7.24 for the four-dimensional form, same call -- twice the points to sort and convert
// and a fifth, nearly empty window cost more than the shorter tail saves: profiles/r4n_glv4_ab.txt).  A BLS12 curve has
// q = u mod r, 64 bits: only the four-dimensional form is balanced (BLS12-381 2^20: 19.8 -> 16.2 ms).
template <> struct GlvOf<Fp2<Fp<bn254_fq_params>>> : GlvG2<bn254_fq_params, bn254_g2_glv_consts, 2> {};
template <> struct GlvOf<Fp2<Fp<bls12_381_fq_params>>> : GlvG2<bls12_381_fq_params, bls12_381_g2_glv4_consts, 4> {};
template <> struct GlvOf<Fp2<Fp<bls12_377_fq_params>>> : GlvG2<bls12_377_fq_params, bls12_377_g2_glv4_consts, 4> {};
// (kGlvBits, kGlv4Bits -- the widths of the halves and quarters -- are in msm_geom.h)

}  // namespace dg16
