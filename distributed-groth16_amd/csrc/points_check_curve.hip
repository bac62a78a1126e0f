// Per-curve object of the membership check (points_check.h): points_check_kernel for G1 and G2 of curve DG_CURVE, and --
// for the curves that have a pairing here (BN254, BLS12-381) -- the transcript checks of dg16_srs_verify.
//
//   membership   the five arrays are copied to the device whole (the sums read them anyway) and checked with
//                subgroup = 1, one result pair per array; the seven heads are compared with the identity on the host
//   sums         the coefficients widened to 32-byte integers once; msm_launch eight times (six sums in G1, two in G2)
//                on the call's stream, canonical scalars, bases known to be in the subgroup (checked above): the second
//                sum of a pair reads the same array one point further on.  The eight affine results come back in one
//                copy.
//   equalities   e(P1, Q1) = e(P2, Q2) as is_one(final_exp(miller(P1, Q1) miller(-P2, Q2))) with Pairing<DG_CURVE> on
//                the host, five times
#include <string.h>

#include <vector>

#include "points_check.h"
#if DG_CURVE < 2
#include "pairing.h"
#endif

#ifndef DG_CURVE
#error "compile with -DDG_CURVE=<curve id>"
#endif

namespace dg16 {

template <>
void points_check_run<DG_CURVE>(Call& k, int group, const void* points_dev, size_t n, size_t index0, int subgroup,
                                pchk::CheckResult* res_dev) {
  if (group == 1) pchk::points_check_typed<DG_CURVE, 1>(k, points_dev, n, index0, subgroup, res_dev);
  else pchk::points_check_typed<DG_CURVE, 2>(k, points_dev, n, index0, subgroup, res_dev);
}

#if DG_CURVE < 2
namespace {

using P = Pairing<DG_CURVE>;
using Fq = P::Fq;
using Fq2 = P::Fq2;

struct DeviceBuffers {
  std::vector<void*> owned;
  ~DeviceBuffers() {
    for (void* p : owned) (void)hipFree(p);
  }
  void* get(size_t bytes) {
    void* p = nullptr;
    DG_HIP(hipMalloc(&p, bytes ? bytes : 16));
    owned.push_back(p);
    return p;
  }
};

bool all_zero(const void* p, size_t bytes) {
  const uint8_t* b = (const uint8_t*)p;
  for (size_t i = 0; i < bytes; i++)
    if (b[i]) return false;
  return true;
}

// e(p1, q1) == e(p2, q2); subgroup points, any of them may be the identity
bool pairings_equal(const Affine<Fq>& p1, const Affine<Fq2>& q1, const Affine<Fq>& p2, const Affine<Fq2>& q2) {
  const Affine<Fq> n2 = p2.is_inf() ? p2 : Affine<Fq>{p2.x, p2.y.neg()};
  return P::is_one12(P::final_exp(P::mul12(P::miller(p1, q1), P::miller(n2, q2))));
}

}  // namespace

template <>
void srs_verify_run<DG_CURVE>(Call& k, unsigned log_m, const dg16_srs_powers* pw, const void* coeffs,
                              dg16_srs_report* report) {
  const pchk::SrsShape sh = pchk::srs_shape(log_m);
  constexpr size_t g1b = sizeof(Affine<Fq>), g2b = sizeof(Affine<Fq2>);
  const void* host[5] = {pw->tau_g1, pw->tau_g2, pw->alpha_tau_g1, pw->beta_tau_g1, pw->beta_g2};
  const size_t count[5] = {sh.n_tau_g1, sh.n_g2, sh.m, sh.m, 1};
  const int group[5] = {1, 2, 1, 1, 2};
  memset(report, 0, sizeof *report);

  DeviceBuffers buf;
  void* dev[5];
  for (int a = 0; a < 5; a++) {
    const size_t bytes = count[a] * (group[a] == 1 ? g1b : g2b);
    dev[a] = buf.get(bytes);
    DG_HIP(hipMemcpyAsync(dev[a], host[a], bytes, hipMemcpyHostToDevice, k.s()));
  }
  // ---- membership ----
  pchk::CheckResult res[5];
  for (int a = 0; a < 5; a++) res[a] = {0ull, (unsigned long long)count[a]};
  pchk::CheckResult* dres = (pchk::CheckResult*)buf.get(sizeof res);
  DG_HIP(hipMemcpyAsync(dres, res, sizeof res, hipMemcpyHostToDevice, k.s()));
  k.begin_dominant();
  for (int a = 0; a < 5; a++) points_check_run<DG_CURVE>(k, group[a], dev[a], count[a], 0, 1, dres + a);
  k.end_dominant();
  DG_HIP(hipMemcpyAsync(res, dres, sizeof res, hipMemcpyDeviceToHost, k.s()));
  DG_HIP(hipStreamSynchronize(k.s()));
  bool found = false;
  for (int a = 0; a < 5; a++) {
    report->n_bad_points += res[a].n_bad;
    if (res[a].n_bad && !found) {
      found = true;
      report->bad_array = (uint32_t)a;
      report->bad_index = res[a].first_bad;
    }
  }
  if (found) report->failed |= DG16_SRS_BAD_POINT;
  const char* t = (const char*)pw->tau_g1;
  const char* u = (const char*)pw->tau_g2;
  if (all_zero(t, g1b) || all_zero(t + g1b, g1b) || all_zero(u, g2b) || all_zero(u + g2b, g2b) ||
      all_zero(pw->alpha_tau_g1, g1b) || all_zero(pw->beta_tau_g1, g1b) || all_zero(pw->beta_g2, g2b))
    report->failed |= DG16_SRS_IDENTITY;
  if (report->failed) return;

  // ---- the eight sums ----
  std::vector<uint32_t> wide(sh.n_long * 8, 0u);
  for (size_t j = 0; j < sh.n_long; j++) memcpy(&wide[8 * j], (const char*)coeffs + 16 * j, 16);
  void* dscal = buf.get(sh.n_long * 32);
  DG_HIP(hipMemcpyAsync(dscal, wide.data(), sh.n_long * 32, hipMemcpyHostToDevice, k.s()));
  char* dsum = (char*)buf.get(6 * g1b + 2 * g2b);
  // slots: 0, 1 T | 2, 3 A | 4, 5 B (G1, lo and shifted) | then U lo, U shifted (G2)
  const struct { int array; size_t terms; } g1_sums[3] = {{0, sh.n_long}, {2, sh.n_short}, {3, sh.n_short}};
  for (int s = 0; s < 3; s++)
    for (int shift = 0; shift < 2; shift++)
      msm_launch(k, DG_CURVE, 1, (const char*)dev[g1_sums[s].array] + shift * g1b, dscal, g1_sums[s].terms, 2u, true,
                 dsum + (2 * s + shift) * g1b);
  for (int shift = 0; shift < 2; shift++)
    msm_launch(k, DG_CURVE, 2, (const char*)dev[1] + shift * g2b, dscal, sh.n_short, 2u, true,
               dsum + 6 * g1b + shift * g2b);
  struct Sums {
    Affine<Fq> g1[6];
    Affine<Fq2> g2[2];
  } sums;
  static_assert(sizeof(Sums) == 6 * g1b + 2 * g2b, "layout of the sums");
  DG_HIP(hipMemcpyAsync(&sums, dsum, sizeof sums, hipMemcpyDeviceToHost, k.s()));
  DG_HIP(hipStreamSynchronize(k.s()));

  // ---- the five equalities ----
  Affine<Fq> t0, t1, b0;
  Affine<Fq2> u0, u1, bg2;
  memcpy(&t0, t, g1b);
  memcpy(&t1, t + g1b, g1b);
  memcpy(&b0, pw->beta_tau_g1, g1b);
  memcpy(&u0, u, g2b);
  memcpy(&u1, u + g2b, g2b);
  memcpy(&bg2, pw->beta_g2, g2b);
  if (!pairings_equal(sums.g1[0], u1, sums.g1[1], u0)) report->failed |= DG16_SRS_TAU_G1;
  if (!pairings_equal(t1, sums.g2[0], t0, sums.g2[1])) report->failed |= DG16_SRS_TAU_G2;
  if (!pairings_equal(sums.g1[2], u1, sums.g1[3], u0)) report->failed |= DG16_SRS_ALPHA;
  if (!pairings_equal(sums.g1[4], u1, sums.g1[5], u0)) report->failed |= DG16_SRS_BETA;
  if (!pairings_equal(b0, u0, t0, bg2)) report->failed |= DG16_SRS_BETA_G2;
}
#endif

}  // namespace dg16
