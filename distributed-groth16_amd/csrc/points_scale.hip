// C ABI of the one-scalar point multiplication and of the phase-2 contribution (include/dg16.h): dg16_points_scale,
// dg16_groth16_contribute.  Argument checks, the scalar arithmetic of a contribution and the dispatch on the curve; the
// schedule, the kernel and the device copies live in points_scale.h and the per-curve objects (points_scale_curve.hip).
// Both calls take host pointers only, run on channel 0 and are synchronous.
#include <string.h>

#include <vector>

#include "points_scale.h"

using namespace dg16;

namespace {

void scale(Call& k, int curve, int group, const void* points, const uint32_t* scalar8, size_t n, void* out,
           bool in_subgroup) {
  switch (curve) {
    case 0: points_scale_run<0>(k, group, points, scalar8, n, out, in_subgroup); break;
    case 1: points_scale_run<1>(k, group, points, scalar8, n, out, in_subgroup); break;
    default: points_scale_run<2>(k, group, points, scalar8, n, out, in_subgroup); break;
  }
}

// 1 <= d < r, and then d^-1 mod r as a plain integer
template <class Fr>
bool invert(const void* d32, uint32_t* inv8) {
  Fr d;
  memcpy(&d, d32, 32);
  if (!pmul::rr_scalar_ok(d)) return false;
  pscale::invert_scalar(d, inv8);
  return true;
}

}  // namespace

extern "C" {

int dg16_points_scale(dg16_ctx* ctx, int curve, int group, const void* points_affine, const void* scalar, size_t n,
                      void* out_affine, int in_subgroup) {
  if (!ctx) return DG16_ERR_BAD_ARG;
  return guarded(ctx, [&] {
    DG_REQUIRE(curve >= 0 && curve <= 2, DG16_ERR_BAD_CURVE, "unknown curve id");
    DG_REQUIRE(group == 1 || group == 2, DG16_ERR_BAD_ARG, "group must be 1 (G1) or 2 (G2)");
    DG_REQUIRE(n == 0 || (points_affine && scalar && out_affine), DG16_ERR_BAD_ARG, "null operand");
    DG_REQUIRE(n < ((size_t)1 << 30), DG16_ERR_BAD_ARG, "n must be < 2^30");
    if (!n) return;
    uint32_t k8[8];
    memcpy(k8, scalar, 32);
    DG_REQUIRE(!(k8[7] >> 31), DG16_ERR_BAD_ARG, "the scalar must be below 2^255");
    Call k(ctx, 0);
    scale(k, curve, group, points_affine, k8, n, out_affine, in_subgroup != 0);
    k.finish();
  });
}

int dg16_groth16_contribute(dg16_ctx* ctx, int curve, size_t n_l, size_t n_h, const void* l_query, const void* h_query,
                            const void* fixed_points, const void* delta, void* l_out, void* h_out, void* fixed_out) {
  if (!ctx) return DG16_ERR_BAD_ARG;
  return guarded(ctx, [&] {
    DG_REQUIRE(curve >= 0 && curve <= 2, DG16_ERR_BAD_CURVE, "unknown curve id");
    DG_REQUIRE(fixed_points && delta && fixed_out, DG16_ERR_BAD_ARG, "null argument");
    DG_REQUIRE(n_l == 0 || (l_query && l_out), DG16_ERR_BAD_ARG, "null l_query");
    DG_REQUIRE(n_h == 0 || (h_query && h_out), DG16_ERR_BAD_ARG, "null h_query");
    DG_REQUIRE(n_l < ((size_t)1 << 30) && n_h < ((size_t)1 << 30), DG16_ERR_BAD_ARG, "n_l and n_h must be < 2^30");
    uint32_t d8[8], inv8[8];
    memcpy(d8, delta, 32);
    const bool ok = curve == 0   ? invert<bn254_fr>(delta, inv8)
                    : curve == 1 ? invert<bls12_381_fr>(delta, inv8)
                                 : invert<bls12_377_fr>(delta, inv8);
    DG_REQUIRE(ok, DG16_ERR_BAD_ARG, "delta is zero or not below r");
    const size_t g1b = affine_bytes(curve, 1), g2b = affine_bytes(curve, 2);
    // alpha_g1 | beta_g1 | delta_g1 | beta_g2 | delta_g2: the deltas times d, the rest as it is (fixed_out may be the input)
    std::vector<char> fixed((const char*)fixed_points, (const char*)fixed_points + 3 * g1b + 2 * g2b);
    Call k(ctx, 0);
    scale(k, curve, 1, &fixed[2 * g1b], d8, 1, &fixed[2 * g1b], true);
    scale(k, curve, 2, &fixed[3 * g1b + g2b], d8, 1, &fixed[3 * g1b + g2b], true);
    scale(k, curve, 1, l_query, inv8, n_l, l_out, true);
    scale(k, curve, 1, h_query, inv8, n_h, h_out, true);
    memcpy(fixed_out, fixed.data(), fixed.size());
    k.finish();
  });
}

}  // extern "C"
