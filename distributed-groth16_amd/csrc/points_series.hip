// C ABI of the series multiplication and of a phase-1 contribution (include/dg16.h): dg16_points_mul_series,
// dg16_srs_contribute.  Argument checks, the scalar arithmetic of a contribution's key and the dispatch on the curve; the
// series kernel and the slice loop live in points_series.h and the per-curve objects (points_series_curve.hip).  Both
// calls take host pointers only, run on channel 0 and are synchronous.  (dg16_srs_verify_contribution sits with the
// transcript verifier it extends, in points_check.hip.)
#include <string.h>

#include <vector>

#include "points_series.h"

using namespace dg16;

namespace {

constexpr unsigned kTwoAdicity[3] = {28, 32, 47};

void series(Call& k, int curve, int group, const void* points, size_t n, const uint32_t* first8, const uint32_t* ratio8,
            uint64_t start, void* out, bool in_subgroup) {
  switch (curve) {
    case 0: points_series_run<0>(k, group, points, n, first8, ratio8, start, out, in_subgroup); break;
    case 1: points_series_run<1>(k, group, points, n, first8, ratio8, start, out, in_subgroup); break;
    default: points_series_run<2>(k, group, points, n, first8, ratio8, start, out, in_subgroup); break;
  }
}

void scale(Call& k, int curve, int group, const void* points, const uint32_t* scalar8, size_t n, void* out) {
  switch (curve) {
    case 0: points_scale_run<0>(k, group, points, scalar8, n, out, true); break;
    case 1: points_scale_run<1>(k, group, points, scalar8, n, out, true); break;
    default: points_scale_run<2>(k, group, points, scalar8, n, out, true); break;
  }
}

// every one of the `count` 32-byte integers at p is below r, and -- with nonzero -- not zero
template <class Fr>
bool scalars_ok_typed(const void* p, int count, bool nonzero) {
  for (int j = 0; j < count; j++) {
    Fr v;
    memcpy(&v, (const char*)p + 32 * j, 32);
    if (!pseries::below_modulus(v) || (nonzero && v.is_zero())) return false;
  }
  return true;
}
bool scalars_ok(int curve, const void* p, int count, bool nonzero) {
  return curve == 0   ? scalars_ok_typed<bn254_fr>(p, count, nonzero)
         : curve == 1 ? scalars_ok_typed<bls12_381_fr>(p, count, nonzero)
                      : scalars_ok_typed<bls12_377_fr>(p, count, nonzero);
}

// a * b mod r on canonical integers
template <class Fr>
void mul_mod_typed(const uint32_t* a8, const uint32_t* b8, uint32_t* out8) {
  Fr a, b;
  memcpy(&a, a8, 32);
  memcpy(&b, b8, 32);
  const Fr p = (a.to_mont() * b.to_mont()).from_mont();
  memcpy(out8, &p, 32);
}
void mul_mod(int curve, const uint32_t* a8, const uint32_t* b8, uint32_t* out8) {
  if (curve == 0) mul_mod_typed<bn254_fr>(a8, b8, out8);
  else if (curve == 1) mul_mod_typed<bls12_381_fr>(a8, b8, out8);
  else mul_mod_typed<bls12_377_fr>(a8, b8, out8);
}

}  // namespace

extern "C" {

int dg16_points_mul_series(dg16_ctx* ctx, int curve, int group, const void* points_affine, size_t n, const void* first,
                           const void* ratio, uint64_t start, void* out_affine, int in_subgroup) {
  if (!ctx) return DG16_ERR_BAD_ARG;
  return guarded(ctx, [&] {
    DG_REQUIRE(curve >= 0 && curve <= 2, DG16_ERR_BAD_CURVE, "unknown curve id");
    DG_REQUIRE(group == 1 || group == 2, DG16_ERR_BAD_ARG, "group must be 1 (G1) or 2 (G2)");
    DG_REQUIRE(n == 0 || (points_affine && first && ratio && out_affine), DG16_ERR_BAD_ARG, "null operand");
    DG_REQUIRE(n < ((size_t)1 << 30), DG16_ERR_BAD_ARG, "n must be < 2^30");
    DG_REQUIRE(start <= UINT64_MAX - (uint64_t)n, DG16_ERR_BAD_ARG, "start + n must not overflow 64 bits");
    if (!n) return;
    DG_REQUIRE(scalars_ok(curve, first, 1, false) && scalars_ok(curve, ratio, 1, false), DG16_ERR_BAD_ARG,
               "first and ratio must be below r");
    uint32_t f8[8], r8[8];
    memcpy(f8, first, 32);
    memcpy(r8, ratio, 32);
    Call k(ctx, 0);
    series(k, curve, group, points_affine, n, f8, r8, start, out_affine, in_subgroup != 0);
    k.finish();
  });
}

int dg16_srs_contribute(dg16_ctx* ctx, int curve, unsigned log_m, const dg16_srs_powers* powers, const void* secrets,
                        const void* blinds, const void* challenge_g2, const dg16_srs_powers_out* out, void* key_out) {
  if (!ctx) return DG16_ERR_BAD_ARG;
  return guarded(ctx, [&] {
    DG_REQUIRE(curve >= 0 && curve <= 2, DG16_ERR_BAD_CURVE, "unknown curve id");
    DG_REQUIRE(powers && powers->tau_g1 && powers->tau_g2 && powers->alpha_tau_g1 && powers->beta_tau_g1 &&
                   powers->beta_g2,
               DG16_ERR_BAD_ARG, "null powers");
    DG_REQUIRE(out && out->tau_g1 && out->tau_g2 && out->alpha_tau_g1 && out->beta_tau_g1 && out->beta_g2,
               DG16_ERR_BAD_ARG, "null output");
    DG_REQUIRE(secrets, DG16_ERR_BAD_ARG, "null secrets");
    DG_REQUIRE((blinds != nullptr) == (challenge_g2 != nullptr) && (blinds != nullptr) == (key_out != nullptr),
               DG16_ERR_BAD_ARG, "blinds, challenge_g2 and key_out come together or not at all");
    DG_REQUIRE(log_m + 1 <= kTwoAdicity[curve] && log_m <= 26, DG16_ERR_BAD_ARG,
               "domain larger than the field's 2-adic subgroup (PolynomialDegreeTooLarge)");
    DG_REQUIRE(scalars_ok(curve, secrets, 3, true), DG16_ERR_BAD_ARG, "a secret is zero or not below r");
    DG_REQUIRE(!blinds || scalars_ok(curve, blinds, 3, true), DG16_ERR_BAD_ARG, "a blind is zero or not below r");
    const size_t m = (size_t)1 << log_m;
    const size_t g1b = affine_bytes(curve, 1), g2b = affine_bytes(curve, 2);
    uint32_t x8[3][8];      // tau, alpha, beta
    memcpy(x8, secrets, sizeof x8);
    const uint32_t one8[8] = {1u, 0, 0, 0, 0, 0, 0, 0};
    Call k(ctx, 0);
    if (blinds) {
      // read G = tau_g1[0] and the challenge before any output is written: an output may be its input
      std::vector<char> key(3 * (2 * g1b + g2b));
      uint32_t s8[3][8];
      memcpy(s8, blinds, sizeof s8);
      for (int j = 0; j < 3; j++) {
        char* kx = &key[j * (2 * g1b + g2b)];
        uint32_t sx8[8];
        mul_mod(curve, s8[j], x8[j], sx8);
        scale(k, curve, 1, powers->tau_g1, s8[j], 1, kx);
        scale(k, curve, 1, powers->tau_g1, sx8, 1, kx + g1b);
        scale(k, curve, 2, (const char*)challenge_g2 + j * g2b, x8[j], 1, kx + 2 * g1b);
      }
      memcpy(key_out, key.data(), key.size());
    }
    series(k, curve, 1, powers->tau_g1, 2 * m - 1, one8, x8[0], 0, out->tau_g1, true);
    series(k, curve, 2, powers->tau_g2, m, one8, x8[0], 0, out->tau_g2, true);
    series(k, curve, 1, powers->alpha_tau_g1, m, x8[1], x8[0], 0, out->alpha_tau_g1, true);
    series(k, curve, 1, powers->beta_tau_g1, m, x8[2], x8[0], 0, out->beta_tau_g1, true);
    scale(k, curve, 2, powers->beta_g2, x8[2], 1, out->beta_g2);
    k.finish();
  });
}

}  // extern "C"
