// Test-only: the recoding, the per-product loops and the re-randomization arithmetic of
// distributed-groth16_amd/csrc/points_mul.h compiled with the HOST compiler, so that the CPU tests
// (tests/test_points_mul_host.py) run exactly the text the kernel runs and count its group operations.
// Never part of the product.
#include <stdint.h>
#include <string.h>
#include "../../distributed-groth16_amd/csrc/points_mul.h"

using namespace dg16;

namespace {

template <class F>
struct LocalTab {
  XYZZ<F> t[pmul::kTable];
  void put(int j, const XYZZ<F>& e) { t[j - 1] = e; }
  XYZZ<F> get(int j) const { return t[j - 1]; }
};

// counts what the loop executes; an addition whose operands are the same point (a doubling inside add) or opposite
// points is counted apart, whether or not the loop keeps its result
template <class F>
struct CountOps {
  uint32_t n[4] = {0, 0, 0, 0};   // doublings, additions, equal operands, opposite operands
  XYZZ<F> dbl(const XYZZ<F>& a) { n[0]++; return a.dbl(); }
  XYZZ<F> add(const XYZZ<F>& a, const XYZZ<F>& b) {
    n[1]++;
    if (!a.is_inf() && !b.is_inf() && a.x * b.zz == b.x * a.zz) n[a.y * b.zzz == b.y * a.zzz ? 2 : 3]++;
    return a.add(b);
  }
};

template <class F>
void mul(int split, const void* points, const void* scalars, size_t n, void* out, uint32_t* counts) {
  const Affine<F>* p = (const Affine<F>*)points;
  const uint32_t* k = (const uint32_t*)scalars;
  Affine<F>* o = (Affine<F>*)out;
  for (size_t i = 0; i < n; i++) {
    LocalTab<F> tab;
    CountOps<F> ops;
    XYZZ<F> acc = split ? pmul::product_split<F>(p[i], k + 8 * i, ops, tab) : pmul::product_plain<F>(p[i], k + 8 * i, ops, tab);
    o[i] = acc.to_affine();
    memcpy(counts + 4 * i, ops.n, sizeof ops.n);
  }
}

template <class F>
int split_digits(const uint32_t* k, uint32_t* mags, int32_t* negs, int8_t* digits, int* nwin) {
  pmul::SplitScalar<F> s;
  pmul::split_scalar<F>(k, s);
  constexpr int DIM = GlvOf<F>::DIM, NW = pmul::split_windows<F>();
  for (int j = 0; j < DIM; j++) {
    memcpy(mags + 8 * j, s.mag[j], 32);
    negs[j] = s.neg[j];
    for (int i = 0; i < NW; i++) digits[j * NW + i] = (int8_t)pmul::digit(s.mag[j], s.carries[j], i, NW);
  }
  *nwin = NW;
  return DIM;
}

template <int CURVE>
void rerandomize(const void* proof, const void* delta, const void* r1_r2, int mont, void* out) {
  using CT = CurveTypes<CURVE>;
  using Fq = typename CT::Fq;
  using Fq2 = typename CT::Fq2;
  using Fr = typename CT::Fr;
  pmul::RrProof<Fq, Fq2> pr;
  Affine<Fq2> d;
  Fr r[2], m[4];
  memcpy(&pr, proof, sizeof pr);
  memcpy(&d, delta, sizeof d);
  memcpy(r, r1_r2, sizeof r);
  const bool ok = pmul::rr_scalar_ok(r[0]) && pmul::rr_scalar_ok(r[1]);
  for (auto& x : m) x = Fr::zero();
  if (ok) pmul::rr_scalars(r[0], r[1], mont != 0, &m[0], &m[1], &m[2], &m[3]);
  pmul::PlainOps<Fq> o1;
  pmul::PlainOps<Fq2> o2;
  LocalTab<Fq> t1;
  LocalTab<Fq2> t2;
  const Affine<Fq> a_inv = pmul::product_split<Fq>(pr.a, m[0].l, o1, t1).to_affine();
  const Affine<Fq> a_r2 = pmul::product_split<Fq>(pr.a, m[1].l, o1, t1).to_affine();
  const Affine<Fq2> b_r1 = pmul::product_split<Fq2>(pr.b, m[2].l, o2, t2).to_affine();
  const Affine<Fq2> d_12 = pmul::product_plain<Fq2>(d, m[3].l, o2, t2).to_affine();   // (the library: fixed-base table)
  const pmul::RrProof<Fq, Fq2> res = pmul::rr_combine<Fq, Fq2>(ok, a_inv, a_r2, pr.c, b_r1, d_12);
  memcpy(out, &res, sizeof res);
}

}  // namespace

#define BY_GROUP(gid, CALL)                                           \
  switch (gid) {                                                      \
    case 0: { using F = CurveTypes<0>::Fq; CALL; break; }             \
    case 1: { using F = CurveTypes<0>::Fq2; CALL; break; }            \
    case 2: { using F = CurveTypes<1>::Fq; CALL; break; }             \
    case 3: { using F = CurveTypes<1>::Fq2; CALL; break; }            \
    case 4: { using F = CurveTypes<2>::Fq; CALL; break; }             \
    case 5: { using F = CurveTypes<2>::Fq2; CALL; break; }            \
    default: return -1;                                               \
  }

extern "C" {

// window width, table entries, windows of the plain path
void hp_params(int* out) { out[0] = pmul::kWindowBits; out[1] = pmul::kTable; out[2] = pmul::kWinPlain; }
// digits[i], i < kWinPlain, of the 8-word integer k
void hp_digits(const uint32_t* k, int8_t* digits) {
  const uint64_t c = pmul::recode_carries(k, pmul::kWinPlain);
  for (int i = 0; i < pmul::kWinPlain; i++) digits[i] = (int8_t)pmul::digit(k, c, i, pmul::kWinPlain);
}
// gid = 2 * curve + group - 1.  Returns DIM; mags: DIM x 8 words, negs: DIM, digits: DIM x *nwin
int hp_split(int gid, const uint32_t* k, uint32_t* mags, int32_t* negs, int8_t* digits, int* nwin) {
  BY_GROUP(gid, return split_digits<F>(k, mags, negs, digits, nwin));
  return -1;
}
// LAMBDA of the group's split (8 words): k = sum_j +-mag_j LAMBDA^j mod r
int hp_lambda(int gid, uint32_t* out) {
  BY_GROUP(gid, memcpy(out, GlvOf<F>::C::LAMBDA, 32));
  return 0;
}
// 1 where the library would split for this group and flag
int hp_may_split(int gid, int in_subgroup) {
  BY_GROUP(gid, return pmul::may_split<F>(in_subgroup != 0) ? 1 : 0);
  return -1;
}
// out[i] = scalars[i] (8 words, plain integer) * points[i]; counts: n x 4 (CountOps)
int hp_mul(int gid, int split, const void* points, const void* scalars, size_t n, void* out, uint32_t* counts) {
  BY_GROUP(gid, mul<F>(split, points, scalars, n, out, counts));
  return 0;
}
int hp_rerandomize(int curve, const void* proof, const void* delta, const void* r1_r2, int mont, void* out) {
  if (curve == 0) rerandomize<0>(proof, delta, r1_r2, mont, out);
  else if (curve == 1) rerandomize<1>(proof, delta, r1_r2, mont, out);
  else return -1;
  return 0;
}

}  // extern "C"
