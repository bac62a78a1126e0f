// C ABI of the membership check, of the transcript verifier and of the verifiers of a phase-2 and of a phase-1
// contribution (include/dg16.h): dg16_points_check, dg16_srs_verify, dg16_groth16_verify_contribution,
// dg16_srs_verify_contribution.
// Argument checks, the device copies of the host arrays and the dispatch on the curve; the kernel and the transcript
// checks live in the per-curve objects (points_check_curve.hip).  All calls take host pointers only, run on channel 0
// and are synchronous; their device buffers are freed on every path.
#include "points_check.h"

using namespace dg16;

static_assert(pchk::kP1After == DG16_P1_AFTER && pchk::kP1BadPoint == DG16_P1_BAD_POINT &&
                  pchk::kP1Identity == DG16_P1_IDENTITY && pchk::kP1Base == DG16_P1_BASE &&
                  pchk::kP1FirstRelation == DG16_P1_KEY_TAU &&
                  (pchk::kP1FirstRelation << (pchk::kP1Relations - 1)) == DG16_P1_LINK_BETA_G2,
              "points_check.h and include/dg16.h disagree on the DG16_P1_* bits");
static_assert(pchk::kSrsBadPoint == DG16_SRS_BAD_POINT && pchk::kSrsIdentity == DG16_SRS_IDENTITY,
              "points_check.h and include/dg16.h disagree on the DG16_SRS_* bits");

namespace {

constexpr unsigned kTwoAdicity[3] = {28, 32, 47};

struct DeviceBuffer {
  void* p = nullptr;
  explicit DeviceBuffer(size_t bytes) { DG_HIP(hipMalloc(&p, bytes ? bytes : 16)); }
  ~DeviceBuffer() {      // (hipFree waits for the kernels that still use the buffer)
    if (p) (void)hipFree(p);
  }
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
};

void check(Call& k, int curve, int group, const void* dev, size_t n, size_t index0, int subgroup,
           pchk::CheckResult* res) {
  switch (curve) {
    case 0: points_check_run<0>(k, group, dev, n, index0, subgroup, res); break;
    case 1: points_check_run<1>(k, group, dev, n, index0, subgroup, res); break;
    default: points_check_run<2>(k, group, dev, n, index0, subgroup, res); break;
  }
}

}  // namespace

extern "C" {

int dg16_points_check(dg16_ctx* ctx, int curve, int group, const void* points_affine, size_t n, int subgroup,
                      size_t* n_bad, size_t* first_bad) {
  if (!ctx) return DG16_ERR_BAD_ARG;
  return guarded(ctx, [&] {
    DG_REQUIRE(curve >= 0 && curve <= 2, DG16_ERR_BAD_CURVE, "unknown curve id");
    DG_REQUIRE(group == 1 || group == 2, DG16_ERR_BAD_ARG, "group must be 1 (G1) or 2 (G2)");
    DG_REQUIRE(n_bad && first_bad && (n == 0 || points_affine), DG16_ERR_BAD_ARG, "null argument");
    DG_REQUIRE(n < ((size_t)1 << 30), DG16_ERR_BAD_ARG, "n must be < 2^30");
    *n_bad = 0;
    *first_bad = n;
    if (!n) return;
    size_t slice = slice_lanes(ctx->points_mul_slice);      // points per launch and per temporary device copy
    if (slice > n) slice = n;
    const size_t pb = affine_bytes(curve, group);
    Call k(ctx, 0);
    DeviceBuffer pts(slice * pb), dres(sizeof(pchk::CheckResult));
    pchk::CheckResult res = {0ull, (unsigned long long)n};
    DG_HIP(hipMemcpyAsync(dres.p, &res, sizeof res, hipMemcpyHostToDevice, k.s()));
    k.begin_dominant();
    for (size_t lo = 0; lo < n; lo += slice) {
      const size_t cnt = n - lo < slice ? n - lo : slice;
      // (the copy is ordered behind the previous slice's kernel on the stream)
      DG_HIP(hipMemcpyAsync(pts.p, (const char*)points_affine + lo * pb, cnt * pb, hipMemcpyHostToDevice, k.s()));
      check(k, curve, group, pts.p, cnt, lo, subgroup != 0, (pchk::CheckResult*)dres.p);
    }
    k.end_dominant();
    DG_HIP(hipMemcpyAsync(&res, dres.p, sizeof res, hipMemcpyDeviceToHost, k.s()));
    k.finish();
    DG_HIP(hipStreamSynchronize(k.s()));
    *n_bad = (size_t)res.n_bad;
    *first_bad = (size_t)res.first_bad;
  });
}

int dg16_srs_verify(dg16_ctx* ctx, int curve, unsigned log_m, const dg16_srs_powers* powers, const void* coeffs,
                    dg16_srs_report* report) {
  if (!ctx) return DG16_ERR_BAD_ARG;
  return guarded(ctx, [&] {
    DG_REQUIRE(curve >= 0 && curve <= 2, DG16_ERR_BAD_CURVE, "unknown curve id");
    DG_REQUIRE(curve != DG16_BLS12_377, DG16_ERR_UNSUPPORTED, "transcript verification: BN254 and BLS12-381 only");
    DG_REQUIRE(powers && powers->tau_g1 && powers->tau_g2 && powers->alpha_tau_g1 && powers->beta_tau_g1 &&
                   powers->beta_g2,
               DG16_ERR_BAD_ARG, "null powers");
    DG_REQUIRE(coeffs && report, DG16_ERR_BAD_ARG, "null argument");
    DG_REQUIRE(log_m >= 1 && log_m <= pchk::kMaxLogM && log_m + 1 <= kTwoAdicity[curve], DG16_ERR_BAD_ARG,
               "need 1 <= log_m <= 26 and a domain of 2m inside the field's 2-adic subgroup");
    const pchk::SrsShape sh = pchk::srs_shape(log_m);
    const uint8_t* c = (const uint8_t*)coeffs;
    for (size_t j = 0; j < sh.n_long; j++) {
      uint8_t any = 0;
      for (int b = 0; b < 16; b++) any |= c[16 * j + b];
      DG_REQUIRE(any, DG16_ERR_BAD_ARG, "a coefficient is zero");
    }
    Call k(ctx, 0);
    if (curve == DG16_BN254) srs_verify_run<0>(k, log_m, powers, coeffs, report);
    else srs_verify_run<1>(k, log_m, powers, coeffs, report);
    k.finish();
    DG_HIP(hipStreamSynchronize(k.s()));
  });
}

int dg16_groth16_verify_contribution(dg16_ctx* ctx, int curve, size_t num_inputs, size_t num_vars, size_t domain_size,
                                     const dg16_groth16_key* before, const dg16_groth16_key* after, const void* coeffs,
                                     dg16_phase2_report* report) {
  if (!ctx) return DG16_ERR_BAD_ARG;
  return guarded(ctx, [&] {
    DG_REQUIRE(curve >= 0 && curve <= 2, DG16_ERR_BAD_CURVE, "unknown curve id");
    DG_REQUIRE(curve != DG16_BLS12_377, DG16_ERR_UNSUPPORTED, "contribution verification: BN254 and BLS12-381 only");
    DG_REQUIRE(before && after && coeffs && report, DG16_ERR_BAD_ARG, "null argument");
    constexpr size_t kMax = (size_t)1 << 28;
    DG_REQUIRE(num_inputs >= 1 && num_inputs <= num_vars && num_vars < kMax && domain_size >= 1 && domain_size < kMax,
               DG16_ERR_BAD_ARG, "need 1 <= num_inputs <= num_vars < 2^28 and 1 <= domain_size < 2^28");
    const size_t n_l = num_vars - num_inputs;
    for (const dg16_groth16_key* key : {before, after})
      DG_REQUIRE(key->a_query && key->b_g1_query && key->b_g2_query && key->h_query && (key->l_query || !n_l) &&
                     key->fixed_points && key->gamma_g2 && key->gamma_abc_g1,
                 DG16_ERR_BAD_ARG, "null array in a key");
    const size_t n_coeff = n_l > domain_size ? n_l : domain_size;
    const uint8_t* c = (const uint8_t*)coeffs;
    for (size_t j = 0; j < n_coeff; j++) {
      uint8_t any = 0;
      for (int b = 0; b < 16; b++) any |= c[16 * j + b];
      DG_REQUIRE(any, DG16_ERR_BAD_ARG, "a coefficient is zero");
    }
    Call k(ctx, 0);
    if (curve == DG16_BN254) phase2_verify_run<0>(k, num_inputs, num_vars, domain_size, before, after, coeffs, report);
    else phase2_verify_run<1>(k, num_inputs, num_vars, domain_size, before, after, coeffs, report);
    k.finish();
    DG_HIP(hipStreamSynchronize(k.s()));
  });
}

int dg16_srs_verify_contribution(dg16_ctx* ctx, int curve, unsigned log_m, const dg16_srs_powers* before,
                                 const dg16_srs_powers* after, const void* key, const void* challenge_g2,
                                 const void* coeffs, dg16_srs_contribution_report* report) {
  if (!ctx) return DG16_ERR_BAD_ARG;
  return guarded(ctx, [&] {
    DG_REQUIRE(curve >= 0 && curve <= 2, DG16_ERR_BAD_CURVE, "unknown curve id");
    DG_REQUIRE(curve != DG16_BLS12_377, DG16_ERR_UNSUPPORTED, "contribution verification: BN254 and BLS12-381 only");
    for (const dg16_srs_powers* pw : {before, after})
      DG_REQUIRE(pw && pw->tau_g1 && pw->tau_g2 && pw->alpha_tau_g1 && pw->beta_tau_g1 && pw->beta_g2, DG16_ERR_BAD_ARG,
                 "null powers");
    DG_REQUIRE(key && challenge_g2 && coeffs && report, DG16_ERR_BAD_ARG, "null argument");
    DG_REQUIRE(log_m >= 1 && log_m <= pchk::kMaxLogM && log_m + 1 <= kTwoAdicity[curve], DG16_ERR_BAD_ARG,
               "need 1 <= log_m <= 26 and a domain of 2m inside the field's 2-adic subgroup");
    const pchk::SrsShape sh = pchk::srs_shape(log_m);
    const uint8_t* c = (const uint8_t*)coeffs;
    for (size_t j = 0; j < sh.n_long; j++) {
      uint8_t any = 0;
      for (int b = 0; b < 16; b++) any |= c[16 * j + b];
      DG_REQUIRE(any, DG16_ERR_BAD_ARG, "a coefficient is zero");
    }
    Call k(ctx, 0);
    if (curve == DG16_BN254) phase1_verify_run<0>(k, log_m, before, after, key, challenge_g2, coeffs, report);
    else phase1_verify_run<1>(k, log_m, before, after, key, challenge_g2, coeffs, report);
    k.finish();
    DG_HIP(hipStreamSynchronize(k.s()));
  });
}

}  // extern "C"
