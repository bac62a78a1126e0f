// C ABI of the group transform and of the reference-string preparation (include/dg16.h): dg16_group_ntt,
// dg16_srs_prepare.  Argument checks, the device copies of the host arrays and the dispatch on the curve; the kernels and
// the stage loop live in the per-curve objects (group_ntt_curve.hip).  Both calls take host pointers only, run on
// channel 0 and are synchronous; their device buffers are freed on every path.
#include <string.h>

#include <vector>

#include "group_ntt.h"

using namespace dg16;

namespace {

constexpr unsigned kTwoAdicity[3] = {28, 32, 47};

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

void* transform(Call& k, int curve, int group, void* x, void* y, unsigned log_n, int inverse, bool scale) {
  switch (curve) {
    case 0: return group_ntt_run<0>(k, group, x, y, log_n, inverse, scale);
    case 1: return group_ntt_run<1>(k, group, x, y, log_n, inverse, scale);
    default: return group_ntt_run<2>(k, group, x, y, log_n, inverse, scale);
  }
}
void diff(Call& k, int curve, const void* src, size_t a_off, size_t b_off, size_t n, void* out) {
  switch (curve) {
    case 0: group_diff_run<0>(k, src, a_off, b_off, n, out); break;
    case 1: group_diff_run<1>(k, src, a_off, b_off, n, out); break;
    default: group_diff_run<2>(k, src, a_off, b_off, n, out); break;
  }
}
void twist(Call& k, int curve, const void* src, unsigned log_m, void* out) {
  switch (curve) {
    case 0: group_twist_run<0>(k, src, log_m, out); break;
    case 1: group_twist_run<1>(k, src, log_m, out); break;
    default: group_twist_run<2>(k, src, log_m, out); break;
  }
}

// host -> x, inverse transform of size 2^log_m, -> host
void lagrange(Call& k, int curve, int group, const void* powers, unsigned log_m, void* x, void* y, void* out) {
  const size_t bytes = affine_bytes(curve, group) << log_m;
  DG_HIP(hipMemcpyAsync(x, powers, bytes, hipMemcpyHostToDevice, k.s()));
  const void* res = transform(k, curve, group, x, y, log_m, 1, true);
  DG_HIP(hipMemcpyAsync(out, res, bytes, hipMemcpyDeviceToHost, k.s()));
  DG_HIP(hipStreamSynchronize(k.s()));
}

}  // namespace

extern "C" {

int dg16_group_ntt(dg16_ctx* ctx, int curve, int group, void* points_affine, unsigned log_n, int inverse) {
  if (!ctx) return DG16_ERR_BAD_ARG;
  return guarded(ctx, [&] {
    DG_REQUIRE(curve >= 0 && curve <= 2, DG16_ERR_BAD_CURVE, "unknown curve id");
    DG_REQUIRE(group == 1 || group == 2, DG16_ERR_BAD_ARG, "group must be 1 (G1) or 2 (G2)");
    DG_REQUIRE(points_affine, DG16_ERR_BAD_ARG, "null operand");
    DG_REQUIRE(log_n <= kTwoAdicity[curve] && log_n <= gntt::kMaxLog, DG16_ERR_BAD_ARG,
               "log_n beyond the field's 2-adic subgroup or 27");
    if (!log_n) return;
    const size_t bytes = affine_bytes(curve, group) << log_n;
    Call k(ctx, 0);
    DeviceBuffers buf;
    void* x = buf.get(bytes);
    void* y = buf.get(bytes);
    DG_HIP(hipMemcpyAsync(x, points_affine, bytes, hipMemcpyHostToDevice, k.s()));
    const void* res = transform(k, curve, group, x, y, log_n, inverse != 0, true);
    DG_HIP(hipMemcpyAsync(points_affine, res, bytes, hipMemcpyDeviceToHost, k.s()));
    k.finish();
    DG_HIP(hipStreamSynchronize(k.s()));
  });
}

int dg16_srs_prepare(dg16_ctx* ctx, int curve, unsigned log_m, int reduction, const dg16_srs_powers* powers,
                     dg16_srs_prepared* out) {
  if (!ctx) return DG16_ERR_BAD_ARG;
  return guarded(ctx, [&] {
    DG_REQUIRE(curve >= 0 && curve <= 2, DG16_ERR_BAD_CURVE, "unknown curve id");
    DG_REQUIRE(reduction == 0 || reduction == 1, DG16_ERR_BAD_ARG, "reduction must be 0 (circom) or 1 (libsnark)");
    DG_REQUIRE(powers && powers->tau_g1 && powers->tau_g2 && powers->alpha_tau_g1 && powers->beta_tau_g1 &&
                   powers->beta_g2,
               DG16_ERR_BAD_ARG, "null powers");
    DG_REQUIRE(out && out->lag_g1 && out->lag_g2 && out->alpha_lag_g1 && out->beta_lag_g1 && out->h_g1 && out->fixed,
               DG16_ERR_BAD_ARG, "null output");
    DG_REQUIRE(log_m + 1 <= kTwoAdicity[curve] && log_m <= 26, DG16_ERR_BAD_ARG,
               "domain larger than the field's 2-adic subgroup (PolynomialDegreeTooLarge)");
    const size_t m = (size_t)1 << log_m;
    const size_t g1b = affine_bytes(curve, 1), g2b = affine_bytes(curve, 2);
    Call k(ctx, 0);
    DeviceBuffers buf;
    void* x = buf.get(2 * m * g1b);        // 2m G1 points hold m G2 points too
    void* y = buf.get(2 * m * g1b);
    lagrange(k, curve, 1, powers->tau_g1, log_m, x, y, out->lag_g1);
    lagrange(k, curve, 2, powers->tau_g2, log_m, x, y, out->lag_g2);
    lagrange(k, curve, 1, powers->alpha_tau_g1, log_m, x, y, out->alpha_lag_g1);
    lagrange(k, curve, 1, powers->beta_tau_g1, log_m, x, y, out->beta_lag_g1);
    // the h basis from p = tau_g1[0 .. 2m - 1) | identity
    DG_HIP(hipMemcpyAsync(x, powers->tau_g1, (2 * m - 1) * g1b, hipMemcpyHostToDevice, k.s()));
    DG_HIP(hipMemsetAsync((char*)x + (2 * m - 1) * g1b, 0, g1b, k.s()));
    const void* h;
    if (reduction == 0) {
      // odd outputs of the size-2m inverse: q_j = (w_2m^-j / 2m) (p_j - p_(j+m)), then the size-m inverse without 1 / m
      diff(k, curve, x, 0, m, m, y);
      twist(k, curve, y, log_m, x);
      h = transform(k, curve, 1, x, y, log_m, 1, false);
    } else {
      diff(k, curve, x, m, 0, m, y);       // tau^(i+m) - tau^i; the last entry is the identity
      DG_HIP(hipMemsetAsync((char*)y + (m - 1) * g1b, 0, g1b, k.s()));
      h = y;
    }
    DG_HIP(hipMemcpyAsync(out->h_g1, h, m * g1b, hipMemcpyDeviceToHost, k.s()));
    k.finish();
    DG_HIP(hipStreamSynchronize(k.s()));
    char* f = (char*)out->fixed;
    memcpy(f, powers->alpha_tau_g1, g1b);
    memcpy(f + g1b, powers->beta_tau_g1, g1b);
    memcpy(f + 2 * g1b, powers->tau_g1, g1b);
    memcpy(f + 3 * g1b, powers->beta_g2, g2b);
    memcpy(f + 3 * g1b + g2b, powers->tau_g2, g2b);
  });
}

}  // extern "C"
