// Per-curve object of the membership check (points_check.h): points_check_kernel for G1 and G2 of curve DG_CURVE, and --
// for the curves that have a pairing here (BN254, BLS12-381) -- the transcript checks of dg16_srs_verify and the checks
// of a phase-2 contribution (dg16_groth16_verify_contribution), which run the same three stages, and the checks of a
// phase-1 contribution (dg16_srs_verify_contribution): the transcript checks on `after` and eight more equalities.
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

// dg16_groth16_verify_contribution: membership of the eight arrays a contribution rewrites, the byte comparison of the
// ones it does not, four sums (msm_launch) and three equalities -- the stages of srs_verify_run on another statement
template <>
void phase2_verify_run<DG_CURVE>(Call& k, size_t num_inputs, size_t num_vars, size_t domain_size,
                                 const dg16_groth16_key* before, const dg16_groth16_key* after, const void* coeffs,
                                 dg16_phase2_report* report) {
  constexpr size_t g1b = sizeof(Affine<Fq>), g2b = sizeof(Affine<Fq2>);
  const size_t n_l = num_vars - num_inputs, n_h = domain_size;
  const dg16_groth16_key* key[2] = {before, after};
  memset(report, 0, sizeof *report);

  // L, H, D1, D2 of `before`, then of `after`
  const void* host[8];
  const size_t count[8] = {n_l, n_h, 1, 1, n_l, n_h, 1, 1};
  const int group[8] = {1, 1, 1, 2, 1, 1, 1, 2};
  for (int s = 0; s < 2; s++) {
    const char* f = (const char*)key[s]->fixed_points;
    host[4 * s] = key[s]->l_query;
    host[4 * s + 1] = key[s]->h_query;
    host[4 * s + 2] = f + 2 * g1b;
    host[4 * s + 3] = f + 3 * g1b + g2b;
  }
  DeviceBuffers buf;
  void* dev[8];
  for (int a = 0; a < 8; a++) {
    const size_t bytes = count[a] * (group[a] == 1 ? g1b : g2b);
    dev[a] = buf.get(bytes);
    if (bytes) DG_HIP(hipMemcpyAsync(dev[a], host[a], bytes, hipMemcpyHostToDevice, k.s()));
  }
  // ---- membership ----
  pchk::CheckResult res[8];
  for (int a = 0; a < 8; a++) res[a] = {0ull, (unsigned long long)count[a]};
  pchk::CheckResult* dres = (pchk::CheckResult*)buf.get(sizeof res);
  DG_HIP(hipMemcpyAsync(dres, res, sizeof res, hipMemcpyHostToDevice, k.s()));
  k.begin_dominant();
  for (int a = 0; a < 8; a++) points_check_run<DG_CURVE>(k, group[a], dev[a], count[a], 0, 1, dres + a);
  k.end_dominant();
  DG_HIP(hipMemcpyAsync(res, dres, sizeof res, hipMemcpyDeviceToHost, k.s()));
  DG_HIP(hipStreamSynchronize(k.s()));
  bool found = false;
  for (int a = 0; a < 8; a++) {
    report->n_bad_points += res[a].n_bad;
    if (res[a].n_bad && !found) {
      found = true;
      report->bad_array = (uint32_t)a;
      report->bad_index = res[a].first_bad;
    }
  }
  if (found) report->failed |= DG16_P2_BAD_POINT;
  if (all_zero(host[2], g1b) || all_zero(host[3], g2b) || all_zero(host[6], g1b) || all_zero(host[7], g2b))
    report->failed |= DG16_P2_IDENTITY;
  // ---- what a contribution leaves alone ----
  const char* f0 = (const char*)before->fixed_points;
  const char* f1 = (const char*)after->fixed_points;
  if (memcmp(before->a_query, after->a_query, num_vars * g1b) ||
      memcmp(before->b_g1_query, after->b_g1_query, num_vars * g1b) ||
      memcmp(before->b_g2_query, after->b_g2_query, num_vars * g2b) ||
      memcmp(before->gamma_g2, after->gamma_g2, g2b) ||
      memcmp(before->gamma_abc_g1, after->gamma_abc_g1, num_inputs * g1b) || memcmp(f0, f1, 2 * g1b) ||
      memcmp(f0 + 3 * g1b, f1 + 3 * g1b, g2b))
    report->failed |= DG16_P2_CHANGED;
  if (report->failed & (DG16_P2_BAD_POINT | DG16_P2_IDENTITY)) return;

  // ---- the four sums: rho L, rho H, rho L', rho H' ----
  const size_t n_coeff = n_l > n_h ? n_l : n_h;
  std::vector<uint32_t> wide(n_coeff * 8, 0u);
  for (size_t j = 0; j < n_coeff; j++) memcpy(&wide[8 * j], (const char*)coeffs + 16 * j, 16);
  void* dscal = buf.get(n_coeff * 32);
  DG_HIP(hipMemcpyAsync(dscal, wide.data(), n_coeff * 32, hipMemcpyHostToDevice, k.s()));
  char* dsum = (char*)buf.get(4 * g1b);
  Affine<Fq> sums[4];
  const int sum_of[4] = {0, 1, 4, 5};
  for (int s = 0; s < 4; s++)
    if (count[sum_of[s]]) msm_launch(k, DG_CURVE, 1, dev[sum_of[s]], dscal, count[sum_of[s]], 2u, true, dsum + s * g1b);
  DG_HIP(hipMemcpyAsync(sums, dsum, sizeof sums, hipMemcpyDeviceToHost, k.s()));
  DG_HIP(hipStreamSynchronize(k.s()));

  // ---- the three equalities ----
  Affine<Fq> d1[2];
  Affine<Fq2> d2[2];
  for (int s = 0; s < 2; s++) {
    memcpy(&d1[s], host[4 * s + 2], g1b);
    memcpy(&d2[s], host[4 * s + 3], g2b);
  }
  if (!pairings_equal(d1[1], d2[0], d1[0], d2[1])) report->failed |= DG16_P2_DELTA;
  if (n_l && !pairings_equal(sums[2], d2[1], sums[0], d2[0])) report->failed |= DG16_P2_L;
  if (!pairings_equal(sums[3], d2[1], sums[1], d2[0])) report->failed |= DG16_P2_H;
}

// dg16_srs_verify_contribution: srs_verify_run on `after`, then membership of the 19 loose points (one launch per
// group), the byte comparison of the bases and eight equalities; pchk::p1_decide makes the word
template <>
void phase1_verify_run<DG_CURVE>(Call& k, unsigned log_m, const dg16_srs_powers* before, const dg16_srs_powers* after,
                                 const void* key, const void* challenge_g2, const void* coeffs,
                                 dg16_srs_contribution_report* report) {
  constexpr size_t g1b = sizeof(Affine<Fq>), g2b = sizeof(Affine<Fq2>);
  memset(report, 0, sizeof *report);
  srs_verify_run<DG_CURVE>(k, log_m, after, coeffs, &report->after);

  struct Key {
    Affine<Fq> g1_s, g1_sx;
    Affine<Fq2> g2_spx;
  } kx[3];      // tau, alpha, beta
  static_assert(sizeof(Key) == 2 * g1b + g2b, "layout of a key");
  Affine<Fq2> sp[3];
  memcpy(kx, key, sizeof kx);
  memcpy(sp, challenge_g2, sizeof sp);
  // T0, T1, A0, B0 | U0, U1, beta_g2 of `before`; T0, T1, A0, B0 | U0, U1, beta_g2 of `after`
  Affine<Fq> h1[2][4];
  Affine<Fq2> h2[2][3];
  const dg16_srs_powers* pw[2] = {before, after};
  for (int s = 0; s < 2; s++) {
    memcpy(&h1[s][0], pw[s]->tau_g1, 2 * g1b);
    memcpy(&h1[s][2], pw[s]->alpha_tau_g1, g1b);
    memcpy(&h1[s][3], pw[s]->beta_tau_g1, g1b);
    memcpy(&h2[s][0], pw[s]->tau_g2, 2 * g2b);
    memcpy(&h2[s][2], pw[s]->beta_g2, g2b);
  }
  // ---- membership: 6 + 4 points of G1, 3 + 3 + 3 of G2 ----
  Affine<Fq> c1[10];
  Affine<Fq2> c2[9];
  for (int j = 0; j < 3; j++) {
    c1[2 * j] = kx[j].g1_s;
    c1[2 * j + 1] = kx[j].g1_sx;
    c2[j] = kx[j].g2_spx;
    c2[3 + j] = sp[j];
    c2[6 + j] = h2[0][j];
  }
  for (int j = 0; j < 4; j++) c1[6 + j] = h1[0][j];
  DeviceBuffers buf;
  void* d1 = buf.get(sizeof c1);
  void* d2 = buf.get(sizeof c2);
  pchk::CheckResult res[2] = {{0ull, 10ull}, {0ull, 9ull}};
  pchk::CheckResult* dres = (pchk::CheckResult*)buf.get(sizeof res);
  DG_HIP(hipMemcpyAsync(d1, c1, sizeof c1, hipMemcpyHostToDevice, k.s()));
  DG_HIP(hipMemcpyAsync(d2, c2, sizeof c2, hipMemcpyHostToDevice, k.s()));
  DG_HIP(hipMemcpyAsync(dres, res, sizeof res, hipMemcpyHostToDevice, k.s()));
  points_check_run<DG_CURVE>(k, 1, d1, 10, 0, 1, dres);
  points_check_run<DG_CURVE>(k, 2, d2, 9, 0, 1, dres + 1);
  DG_HIP(hipMemcpyAsync(res, dres, sizeof res, hipMemcpyDeviceToHost, k.s()));
  DG_HIP(hipStreamSynchronize(k.s()));
  report->n_bad_points = (uint32_t)(res[0].n_bad + res[1].n_bad);

  pchk::P1Outcomes o = {};
  o.after_failed = report->after.failed;
  o.bad_point = report->n_bad_points != 0;
  for (const Affine<Fq>& p : c1) o.identity |= all_zero(&p, g1b);
  for (const Affine<Fq2>& p : c2) o.identity |= all_zero(&p, g2b);
  o.base_differs = memcmp(&h1[0][0], &h1[1][0], g1b) != 0 || memcmp(&h2[0][0], &h2[1][0], g2b) != 0;
  if (!pchk::p1_relations_skipped(o.after_failed, o.bad_point, o.identity)) {
    // R(a, b; c, d): e(a, d) = e(b, c)
    const auto fails = [](const Affine<Fq>& a, const Affine<Fq>& b, const Affine<Fq2>& c, const Affine<Fq2>& d) {
      return !pairings_equal(a, d, b, c);
    };
    for (int j = 0; j < 3; j++) o.relation_fails[j] = fails(kx[j].g1_s, kx[j].g1_sx, sp[j], kx[j].g2_spx);
    o.relation_fails[3] = fails(h1[0][1], h1[1][1], sp[0], kx[0].g2_spx);
    o.relation_fails[4] = fails(kx[0].g1_s, kx[0].g1_sx, h2[0][1], h2[1][1]);
    o.relation_fails[5] = fails(h1[0][2], h1[1][2], sp[1], kx[1].g2_spx);
    o.relation_fails[6] = fails(h1[0][3], h1[1][3], sp[2], kx[2].g2_spx);
    o.relation_fails[7] = fails(kx[2].g1_s, kx[2].g1_sx, h2[0][2], h2[1][2]);
  }
  report->failed = pchk::p1_decide(o);
}
#endif

}  // namespace dg16
