// Curve and subgroup membership of affine points (dg16_points_check) and, on top of it, the checks of a powers-of-tau
// transcript (dg16_srs_verify).
//
//   decision   classify(p, subgroup): the identity (all-zero bytes) is good; a coordinate that is not reduced (>= q) is
//              bad; a point off y^2 = x^3 + b (b of the curve or of its twist) is bad; with `subgroup`, r P != O is bad.
//              The first two tests run on the 32-bit-limb words as they arrive (fp.h); only a reduced point of the curve
//              reaches the multiplication.
//   r P        one point per lane on the 29-bit-limb arithmetic (fp29.h, ec29.h).  r is a public constant, so the lane
//              needs neither a table nor a regular recoding: the non-adjacent form of r is two bit masks computed at
//              compile time (naf_of), the accumulator starts at P (the top digit of a NAF is +1) and every digit below is
//              one doubling and, where it is not zero, one MIXED addition of +-P (madd: 8M + 2S against the 12M + 2S of a
//              table entry in XYZZ).  Every lane of every wave takes the same branches -- the digits are the same for all
//              -- but for the exceptional cases of the addition law, which XYZZ29 handles (ec29.h: identity, equal and
//              opposite operands; a point of order two through HasOrderTwoPoint: T = (q - 1, 0) of BLS12-377 G1 doubles
//              to the identity and r T = T is reported bad).  For a point of order r the last addition is -P + P.
//              BN254: 254 doublings + 73 additions.  BLS12-381: 255 + 59.  BLS12-377: 252 + 68 (NafOf<..>::v; the host
//              test counts them).
//   no shortcut  BN254 G1 has cofactor one: every reduced point of the curve is in the subgroup and `subgroup` changes
//              nothing there.  The other five groups ship r P.  An endomorphism test (phi(P) = lambda P on G1, psi(P) =
//              x P on G2 of the BLS12 curves) is a fraction of the work, but it may replace r P only with a cited proof of
//              equivalence per curve; none is wired here.
//
// classify and the chain are host and device text: tests/host_arith/host_points_check.cpp runs them on a CPU under the
// address and undefined-behaviour sanitizers against plain-Python decisions.
#pragma once
#include "ec29.h"
#include "slices.h"
#include "types.h"

namespace dg16 {
namespace pchk {

enum Verdict : int { kGood = 0, kUnreduced = 1, kOffCurve = 2, kOffSubgroup = 3 };

// the non-adjacent form of an odd 8-word integer below 2^255: bit i of pos / neg = digit i is +1 / -1
struct Naf {
  uint32_t pos[8];
  uint32_t neg[8];
  int top;       // index of the highest digit (always +1)
  int adds;      // non-zero digits below the top
};
constexpr Naf naf_of(const uint32_t (&m)[8]) {
  uint32_t k[9] = {m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], 0};
  Naf out = {{0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}, 0, 0};
  for (int i = 0; i < 256; i++) {
    if (k[0] & 1u) {
      if ((k[0] & 3u) == 1u) {
        out.pos[i >> 5] |= 1u << (i & 31);
        k[0] -= 1u;                                   // odd: no borrow
      } else {
        out.neg[i >> 5] |= 1u << (i & 31);
        for (int j = 0; j < 9; j++) {                 // k += 1
          k[j] += 1u;
          if (k[j] != 0u) break;
        }
      }
      out.top = i;
      out.adds++;
    }
    for (int j = 0; j < 9; j++) k[j] = (k[j] >> 1) | (j + 1 < 9 ? k[j + 1] << 31 : 0u);
  }
  out.adds--;
  return out;
}
template <class RP>
struct NafOf {
  static constexpr Naf v = naf_of(RP::P);
};

// the six groups: coordinate field, scalar-field parameters, b
template <int CURVE, int GROUP>
struct GroupOf;
template <int CURVE>
struct GroupOf<CURVE, 1> {
  using CT = CurveTypes<CURVE>;
  using F = typename CT::Fq;
  using RP = typename CT::Fr::Params;
  static constexpr bool kCofactorOne = CURVE == 0;
  DG_HD static F b() {
    F v;
#pragma unroll
    for (int i = 0; i < F::NL; i++) v.l[i] = CT::G1c::B[i];
    return v;
  }
};
template <int CURVE>
struct GroupOf<CURVE, 2> {
  using CT = CurveTypes<CURVE>;
  using F = typename CT::Fq2;
  using RP = typename CT::Fr::Params;
  static constexpr bool kCofactorOne = false;
  DG_HD static F b() {
    F v;
#pragma unroll
    for (int i = 0; i < CT::Fq::NL; i++) {
      v.c0.l[i] = CT::G2c::B_C0[i];
      v.c1.l[i] = CT::G2c::B_C1[i];
    }
    return v;
  }
};

// stored words < q (a Montgomery form is reduced exactly when its value is)
template <class P>
DG_HD bool reduced(const Fp<P>& v) {
  for (int i = P::NL - 1; i >= 0; i--)
    if (v.l[i] != P::P[i]) return v.l[i] < P::P[i];
  return false;
}
template <class B>
DG_HD bool reduced(const Fp2<B>& v) { return reduced(v.c0) && reduced(v.c1); }

// what the chain calls for a group operation; the host test passes a counting one
template <class F>
struct ChainOps {
  DG_HD XYZZ29<F> dbl(const XYZZ29<F>& a) { return a.dbl_pt(); }
  DG_HD XYZZ29<F> madd(const XYZZ29<F>& a, const Affine29<F>& q, bool negate) { return a.madd(q, negate); }
};

// r p == O for a reduced point p of the curve, not the identity; r the modulus RP
template <class F, class RP, class Ops>
DG_HD bool order_divides_r(const Affine<F>& p32, Ops& ops) {
  using FO = FieldOf<F>;
  using X = XYZZ29<F>;
  const Affine29<F> p = {FO::canon_of(FO::from32(p32.x)), FO::canon_of(FO::from32(p32.y))};
  X acc = {p.x.template as<X::BS, 1>(), p.y.template as<X::BS, 1>(), FO::one(), FO::one()};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int i = NafOf<RP>::v.top - 1; i >= 0; i--) {
    acc = ops.dbl(acc);
    const uint32_t bit = 1u << (i & 31);
    const bool pos = NafOf<RP>::v.pos[i >> 5] & bit, neg = NafOf<RP>::v.neg[i >> 5] & bit;
    if (pos || neg) acc = ops.madd(acc, p, neg);
  }
  return acc.is_inf();
}

template <int CURVE, int GROUP, class Ops>
DG_HD int classify(const Affine<typename GroupOf<CURVE, GROUP>::F>& p, bool subgroup, Ops& ops) {
  using G = GroupOf<CURVE, GROUP>;
  using F = typename G::F;
  if (p.is_inf()) return kGood;
  if (!reduced(p.x) || !reduced(p.y)) return kUnreduced;
  if (!(p.y.sqr() == p.x.sqr() * p.x + G::b())) return kOffCurve;
  if constexpr (G::kCofactorOne) return kGood;
  if (!subgroup) return kGood;
  return order_divides_r<F, typename G::RP>(p, ops) ? kGood : kOffSubgroup;
}

// ---- dg16_srs_verify: the bits of dg16_srs_report::failed and the sizes of the five arrays --------------------------------
constexpr unsigned kMaxLogM = 26;
struct SrsShape {
  size_t m, n_tau_g1, n_g2, n_long, n_short;     // 2^log_m, 2m - 1, m, 2m - 2 terms, m - 1 terms
};
inline SrsShape srs_shape(unsigned log_m) {
  const size_t m = (size_t)1 << log_m;
  return {m, 2 * m - 1, m, 2 * m - 2, m - 1};
}

// ---- dg16_srs_verify_contribution: from the outcomes of the checks to the word ------------------------------------------
// (the values of the DG16_P1_* bits of include/dg16.h; points_check.hip holds the static_asserts)
constexpr uint32_t kP1After = 1u, kP1BadPoint = 2u, kP1Identity = 4u, kP1Base = 8u, kP1FirstRelation = 16u;
constexpr int kP1Relations = 8;     // KEY_TAU, KEY_ALPHA, KEY_BETA, LINK_TAU_G1, LINK_TAU_G2, LINK_ALPHA, LINK_BETA, LINK_BETA_G2
constexpr uint32_t kSrsBadPoint = 1u, kSrsIdentity = 2u;      // DG16_SRS_BAD_POINT, DG16_SRS_IDENTITY

struct P1Outcomes {
  uint32_t after_failed;            // dg16_srs_report::failed of `after`
  bool bad_point, identity;         // among the key, the challenge and the heads of `before`
  bool base_differs;                // tau_g1[0] or tau_g2[0]
  bool relation_fails[kP1Relations];
};
// the pairings assume subgroup points that are not the identity: without that they are not run
DG_HD bool p1_relations_skipped(uint32_t after_failed, bool bad_point, bool identity) {
  return bad_point || identity || (after_failed & (kSrsBadPoint | kSrsIdentity)) != 0;
}
DG_HD uint32_t p1_decide(const P1Outcomes& o) {
  uint32_t w = 0;
  if (o.after_failed) w |= kP1After;
  if (o.bad_point) w |= kP1BadPoint;
  if (o.identity) w |= kP1Identity;
  if (o.base_differs) w |= kP1Base;
  if (!p1_relations_skipped(o.after_failed, o.bad_point, o.identity))
    for (int j = 0; j < kP1Relations; j++)
      if (o.relation_fails[j]) w |= kP1FirstRelation << j;
  return w;
}

}  // namespace pchk
}  // namespace dg16

#if defined(__HIPCC__)
// ---- device side ----------------------------------------------------------------------------------------------------------
#include "ctx.h"
#include "fixed_base_impl.h"

namespace dg16 {
namespace pchk {

struct CheckResult {              // device words of one call: bad points, the smallest bad index (n when none)
  unsigned long long n_bad;
  unsigned long long first_bad;
};

// one point per lane, points[i] with global index index0 + i, i < n
template <int CURVE, int GROUP>
__global__ void __launch_bounds__(64) points_check_kernel(const Affine<typename GroupOf<CURVE, GROUP>::F>* __restrict__ points,
                                                           size_t n, size_t index0, int subgroup,
                                                           CheckResult* __restrict__ res) {
  using F = typename GroupOf<CURVE, GROUP>::F;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Affine<F> p = fb_load(points + i);
  ChainOps<F> ops;
  if (classify<CURVE, GROUP>(p, subgroup != 0, ops) != kGood) {
    atomicAdd(&res->n_bad, 1ull);
    atomicMin(&res->first_bad, (unsigned long long)(index0 + i));
  }
}

template <int CURVE, int GROUP>
void points_check_typed(Call& k, const void* points_dev, size_t n, size_t index0, int subgroup, CheckResult* res_dev) {
  if (!n) return;
  using F = typename GroupOf<CURVE, GROUP>::F;
  hipLaunchKernelGGL((points_check_kernel<CURVE, GROUP>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, k.s(),
                     (const Affine<F>*)points_dev, n, index0, subgroup, res_dev);
  DG_HIP(hipGetLastError());
}

}  // namespace pchk

// points_dev[0 .. n) with global indices from index0; res_dev is updated, not initialised.  n < 2^31 * 64.
template <int CURVE>
void points_check_run(Call& k, int group, const void* points_dev, size_t n, size_t index0, int subgroup,
                      pchk::CheckResult* res_dev);
// the transcript checks behind dg16_srs_verify (BN254, BLS12-381); argument checks are the caller's
template <int CURVE>
void srs_verify_run(Call& k, unsigned log_m, const dg16_srs_powers* powers, const void* coeffs, dg16_srs_report* report);
// (defined in the per-curve objects points_check_<curve>.o)
template <> void points_check_run<0>(Call&, int, const void*, size_t, size_t, int, pchk::CheckResult*);
template <> void points_check_run<1>(Call&, int, const void*, size_t, size_t, int, pchk::CheckResult*);
template <> void points_check_run<2>(Call&, int, const void*, size_t, size_t, int, pchk::CheckResult*);
template <> void srs_verify_run<0>(Call&, unsigned, const dg16_srs_powers*, const void*, dg16_srs_report*);
template <> void srs_verify_run<1>(Call&, unsigned, const dg16_srs_powers*, const void*, dg16_srs_report*);
// the checks behind dg16_groth16_verify_contribution (BN254, BLS12-381), beside srs_verify_run whose membership stage,
// sums and pairing equality they share; argument checks are the caller's
template <int CURVE>
void phase2_verify_run(Call& k, size_t num_inputs, size_t num_vars, size_t domain_size, const dg16_groth16_key* before,
                       const dg16_groth16_key* after, const void* coeffs, dg16_phase2_report* report);
template <> void phase2_verify_run<0>(Call&, size_t, size_t, size_t, const dg16_groth16_key*, const dg16_groth16_key*,
                                      const void*, dg16_phase2_report*);
template <> void phase2_verify_run<1>(Call&, size_t, size_t, size_t, const dg16_groth16_key*, const dg16_groth16_key*,
                                      const void*, dg16_phase2_report*);
// the checks behind dg16_srs_verify_contribution (BN254, BLS12-381): srs_verify_run on `after`, membership of the key,
// the challenge and the heads of `before`, and eight pairing equalities; argument checks are the caller's
template <int CURVE>
void phase1_verify_run(Call& k, unsigned log_m, const dg16_srs_powers* before, const dg16_srs_powers* after,
                       const void* key, const void* challenge_g2, const void* coeffs,
                       dg16_srs_contribution_report* report);
template <> void phase1_verify_run<0>(Call&, unsigned, const dg16_srs_powers*, const dg16_srs_powers*, const void*,
                                      const void*, const void*, dg16_srs_contribution_report*);
template <> void phase1_verify_run<1>(Call&, unsigned, const dg16_srs_powers*, const dg16_srs_powers*, const void*,
                                      const void*, const void*, dg16_srs_contribution_report*);

}  // namespace dg16
#endif
