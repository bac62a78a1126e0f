// Test-only: the schedule and the per-product loop of distributed-groth16_amd/csrc/points_scale.h compiled with the HOST
// compiler, so that the CPU tests (tests/test_points_scale_host.py) run exactly the text the kernel runs and count its
// group operations.  Never part of the product.
#include <stdint.h>
#include <string.h>
#include "../../distributed-groth16_amd/csrc/points_scale.h"

using namespace dg16;

namespace {

template <class F>
struct LocalTab {
  XYZZ<F> t[pscale::kTable];
  void put(int j, const XYZZ<F>& e) { t[j - 1] = e; }
  XYZZ<F> get(int j) const { return t[j - 1]; }
};

template <class F>
struct CountOps {
  uint32_t n[2] = {0, 0};   // doublings, additions
  XYZZ<F> dbl(const XYZZ<F>& a) { n[0]++; return a.dbl(); }
  XYZZ<F> add(const XYZZ<F>& a, const XYZZ<F>& b) { n[1]++; return a.add(b); }
};

// one scalar, n points; counts: n x 2
template <class F>
void scale(int split, const void* points, const uint32_t* k, size_t n, void* out, uint32_t* counts) {
  const Affine<F>* p = (const Affine<F>*)points;
  Affine<F>* o = (Affine<F>*)out;
  pscale::Schedule s;
  pscale::make_schedule<F>(k, split != 0, s);
  for (size_t i = 0; i < n; i++) {
    LocalTab<F> tab;
    CountOps<F> ops;
    XYZZ<F> acc;
    if (s.dim == 1) acc = pscale::product<1, F>(p[i], s.rows, s.len, ops, tab);
    else acc = pscale::product<GlvOf<F>::DIM, F>(p[i], s.rows, s.len, ops, tab);
    o[i] = acc.to_affine();
    memcpy(counts + 2 * i, ops.n, sizeof ops.n);
  }
}

template <class F>
int schedule(int split, const uint32_t* k, int8_t* digits, int* len) {
  pscale::Schedule s;
  pscale::make_schedule<F>(k, split != 0, s);
  for (int j = 0; j < 4; j++)
    for (int i = 0; i < pscale::kMaxRows; i++)
      digits[j * pscale::kMaxRows + i] = j < s.dim && i < s.len ? (int8_t)pscale::row_digit(s.rows[i], j) : 0;
  *len = s.len;
  return s.dim;
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

// width, table entries, rows of a schedule
void hs_params(int* out) { out[0] = pscale::kWidth; out[1] = pscale::kTable; out[2] = pscale::kMaxRows; }
// gid = 2 * curve + group - 1.  Returns the number of parts (1, 2, 4); digits: 4 x kMaxRows signed digits (the parts'
// signs folded in), *len the rows in use
int hs_schedule(int gid, int split, const uint32_t* k, int8_t* digits, int* len) {
  BY_GROUP(gid, return schedule<F>(split, k, digits, len));
  return -1;
}
// wnaf.h's recoder alone at width w (5 or 7) on the 8-word integer m: digits = kMaxRows signed digits of m, or of -m
// where neg; returns the length, -1 for another width
int hs_recode(int w, const uint32_t* m, int neg, int8_t* digits) {
  if (w == 5) return wnaf::recode_wnaf<5>(m, neg != 0, digits);
  if (w == 7) return wnaf::recode_wnaf<7>(m, neg != 0, digits);
  return -1;
}
// LAMBDA of the group's split (8 words): k = sum_j part_j LAMBDA^j mod r
int hs_lambda(int gid, uint32_t* out) {
  BY_GROUP(gid, memcpy(out, GlvOf<F>::C::LAMBDA, 32));
  return 0;
}
// out[i] = k * points[i] (k: 8 words, a plain integer below 2^255); counts: n x 2 (doublings, additions)
int hs_scale(int gid, int split, const void* points, const uint32_t* k, size_t n, void* out, uint32_t* counts) {
  BY_GROUP(gid, scale<F>(split, points, k, n, out, counts));
  return 0;
}
// d^-1 mod r (8 words each); -1 where d is zero or not below r
int hs_invert(int curve, const uint32_t* d, uint32_t* out) {
  if (curve == 0) {
    bn254_fr v;
    memcpy(&v, d, 32);
    if (!pmul::rr_scalar_ok(v)) return -1;
    pscale::invert_scalar(v, out);
  } else if (curve == 1) {
    bls12_381_fr v;
    memcpy(&v, d, 32);
    if (!pmul::rr_scalar_ok(v)) return -1;
    pscale::invert_scalar(v, out);
  } else {
    bls12_377_fr v;
    memcpy(&v, d, 32);
    if (!pmul::rr_scalar_ok(v)) return -1;
    pscale::invert_scalar(v, out);
  }
  return 0;
}

}  // extern "C"

#if defined(HOST_POINTS_SCALE_MAIN)
// A stand-alone program for a sanitizer build (tests/test_points_scale_host.py): host_points_scale <file of 8-word
// integers>.  Per integer one line: the length of the recoder's digits at w = 5, 7 for m and for -m, then, for an integer
// below 2^255, parts:rows of make_schedule for the six groups on the plain and the split path.
#include <stdio.h>

int main(int argc, char** argv) {
  FILE* f = argc == 2 ? fopen(argv[1], "rb") : nullptr;
  if (!f) {
    fprintf(stderr, "usage: host_points_scale <file of 8-word integers>\n");
    return 2;
  }
  uint32_t m[8];
  int8_t digits[4 * pscale::kMaxRows];
  while (fread(m, 4, 8, f) == 8) {
    for (int w = 5; w <= 7; w += 2)
      for (int neg = 0; neg < 2; neg++) printf("%d ", hs_recode(w, m, neg, digits));
    for (int id = 0; id < 12 && !(m[7] >> 31); id++) {
      int len = 0;
      const int dim = hs_schedule(id / 2, id % 2, m, digits, &len);
      printf("%d:%d ", dim, len);
    }
    printf("\n");
  }
  fclose(f);
  return 0;
}
#endif
