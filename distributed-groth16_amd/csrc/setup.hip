// C ABI of the key generator (include/dg16.h): dg16_fixed_base_mul, dg16_fixed_base_window_bits, dg16_groth16_setup,
// dg16_groth16_setup_srs, dg16_setup_srs_limits.  Argument checks, staging of host-pointer calls and the dispatch on
// the curve; the kernels live in the per-curve objects (setup_curve.hip, setup_srs_curve.hip).
#include <vector>

#include "fixed_base_impl.h"
#include "setup.h"
#include "setup_srs_plan.h"

namespace dg16 {
namespace {

void fixed_base_dispatch(Call& k, int curve, int group, const void* base, const void* scalars, size_t n, bool mont,
                         void* out) {
  switch (curve) {
    case 0: fixed_base_run<0>(k, group, base, scalars, n, mont, out); break;
    case 1: fixed_base_run<1>(k, group, base, scalars, n, mont, out); break;
    default: fixed_base_run<2>(k, group, base, scalars, n, mont, out); break;
  }
}

}  // namespace
}  // namespace dg16

using namespace dg16;

extern "C" {

unsigned dg16_fixed_base_window_bits(size_t n) { return fixed_base_window_bits(n); }

int dg16_fixed_base_mul(dg16_ctx* ctx, int curve, int group, const void* base, const void* scalars, size_t n,
                        void* out_affine, unsigned flags, int channel) {
  int rc = guard_channel(ctx, channel);
  if (rc) return rc;
  return guarded(ctx, [&] {
    DG_REQUIRE(curve >= 0 && curve <= 2, DG16_ERR_BAD_CURVE, "unknown curve id");
    DG_REQUIRE(group == 1 || group == 2, DG16_ERR_BAD_ARG, "group must be 1 (G1) or 2 (G2)");
    DG_REQUIRE(n == 0 || (scalars && out_affine), DG16_ERR_BAD_ARG, "null operand");
    DG_REQUIRE(n < ((size_t)1 << 30), DG16_ERR_BAD_ARG, "n must be < 2^30");
    if (!n) return;
    const bool dev = flags & DG16_F_DEVICE_PTRS;
    const size_t pb = affine_bytes(curve, group);
    Call k(ctx, channel);
    const void* dscal = stage_in(k, 1, scalars, n * 32, dev);
    void* dout = dev ? out_affine : ws(k.c, 0, n * pb);
    fixed_base_dispatch(k, curve, group, base, dscal, n, flags & DG16_F_SCALARS_MONT, dout);
    if (!dev) stage_out(k, out_affine, dout, n * pb, false);
    k.finish();
    if (!dev) DG_HIP(hipStreamSynchronize(k.s()));
  });
}

int dg16_groth16_setup(dg16_ctx* ctx, int curve, size_t num_constraints, size_t num_inputs, size_t num_vars,
                       unsigned log_m, const uint32_t* a_row_ptr, const uint32_t* a_col, const void* a_coeff,
                       const uint32_t* b_row_ptr, const uint32_t* b_col, const void* b_coeff,
                       const uint32_t* c_row_ptr, const uint32_t* c_col, const void* c_coeff, const void* trapdoor,
                       const void* generators, void* a_query, void* b_g1_query, void* b_g2_query, void* h_query,
                       void* l_query, void* fixed_points, void* gamma_g2, void* gamma_abc_g1, unsigned flags) {
  if (!ctx) return DG16_ERR_BAD_ARG;
  return guarded(ctx, [&] {
    DG_REQUIRE(curve >= 0 && curve <= 2, DG16_ERR_BAD_CURVE, "unknown curve id");
    const size_t nc = num_constraints, ni = num_inputs, nv = num_vars;
    DG_REQUIRE(a_row_ptr && b_row_ptr && c_row_ptr && trapdoor, DG16_ERR_BAD_ARG, "null operand");
    DG_REQUIRE(a_query && b_g1_query && b_g2_query && h_query && fixed_points && gamma_g2 && gamma_abc_g1 &&
                   (l_query || nv == ni),
               DG16_ERR_BAD_ARG, "null output");
    const unsigned two_adicity[3] = {28, 32, 47};
    DG_REQUIRE(log_m + 1 <= two_adicity[curve] && log_m <= 26, DG16_ERR_BAD_ARG,
               "domain larger than the field's 2-adic subgroup (PolynomialDegreeTooLarge)");
    const size_t m = (size_t)1 << log_m;
    // D::new(num_constraints + num_inputs): the domain must hold both
    DG_REQUIRE(ni >= 1 && ni <= nv && nc + ni <= m && nv < ((size_t)1 << 30), DG16_ERR_BAD_ARG,
               "need 1 <= num_inputs <= num_vars and num_constraints + num_inputs <= 2^log_m");
    const bool dev = flags & DG16_F_DEVICE_PTRS;
    Call k(ctx, 0);
    if (dev) DG_HIP(hipStreamSynchronize(k.s()));   // behind the producers on channel 0's stream, before row_ptr[nc] is read
    SetupArgs s{};
    s.nc = nc; s.ni = ni; s.nv = nv; s.log_m = log_m;
    s.trapdoor = trapdoor;
    s.generators = generators;
    s.libsnark = flags & DG16_F_QAP_LIBSNARK;
    const uint32_t* rp[3] = {a_row_ptr, b_row_ptr, c_row_ptr};
    const uint32_t* cl[3] = {a_col, b_col, c_col};
    const void* cf[3] = {a_coeff, b_coeff, c_coeff};
    // staged copies of host-pointer calls (freed on every path)
    std::vector<void*> owned;
    struct Free {
      std::vector<void*>& v;
      ~Free() { for (void* p : v) (void)hipFree(p); }
    } free_owned{owned};
    auto dmalloc = [&](size_t bytes) {
      void* p = nullptr;
      DG_HIP(hipMalloc(&p, bytes ? bytes : 16));
      owned.push_back(p);
      return p;
    };
    for (int j = 0; j < 3; j++) {
      uint32_t last = 0;
      if (dev) {
        if (nc) DG_HIP(hipMemcpy(&last, rp[j] + nc, sizeof last, hipMemcpyDeviceToHost));
      } else {
        // matrix indices are checked before anything reaches the device, as dg16_qap does
        for (size_t i = 0; i < nc; i++)
          DG_REQUIRE(rp[j][i] <= rp[j][i + 1], DG16_ERR_BAD_ARG, "row_ptr is not non-decreasing");
        last = nc ? rp[j][nc] : 0;
        DG_REQUIRE(!last || (cl[j] && cf[j]), DG16_ERR_BAD_ARG, "null matrix");
        for (size_t e = nc ? rp[j][0] : 0; e < last; e++)
          DG_REQUIRE(cl[j][e] < nv, DG16_ERR_BAD_ARG, "matrix column >= num_vars");
      }
      DG_REQUIRE(!last || (cl[j] && cf[j]), DG16_ERR_BAD_ARG, "null matrix");
      s.nnz[j] = last;
      if (dev) {
        s.row_ptr[j] = rp[j]; s.col[j] = cl[j]; s.coeff[j] = cf[j];
      } else {
        void* p = dmalloc((nc + 1) * 4);
        void* c = dmalloc((size_t)last * 4);
        void* v = dmalloc((size_t)last * 32);
        DG_HIP(hipMemcpyAsync(p, rp[j], (nc + 1) * 4, hipMemcpyHostToDevice, k.s()));
        if (last) {
          DG_HIP(hipMemcpyAsync(c, cl[j], (size_t)last * 4, hipMemcpyHostToDevice, k.s()));
          DG_HIP(hipMemcpyAsync(v, cf[j], (size_t)last * 32, hipMemcpyHostToDevice, k.s()));
        }
        s.row_ptr[j] = (const unsigned*)p; s.col[j] = (const unsigned*)c; s.coeff[j] = v;
      }
    }
    const size_t g1b = affine_bytes(curve, 1), g2b = affine_bytes(curve, 2);
    void* host_out[8] = {a_query, b_g1_query, b_g2_query, h_query, l_query, fixed_points, gamma_g2, gamma_abc_g1};
    const size_t out_bytes[8] = {nv * g1b, nv * g1b, nv * g2b, m * g1b, (nv - ni) * g1b, 3 * g1b + 2 * g2b, g2b, ni * g1b};
    void* d[8];
    for (int j = 0; j < 8; j++) d[j] = dev ? host_out[j] : dmalloc(out_bytes[j]);
    s.a_query = d[0]; s.b_g1_query = d[1]; s.b_g2_query = d[2]; s.h_query = d[3]; s.l_query = d[4];
    s.fixed_points = d[5]; s.gamma_g2 = d[6]; s.gamma_abc_g1 = d[7];
    switch (curve) {
      case 0: groth16_setup_run<0>(k, s); break;
      case 1: groth16_setup_run<1>(k, s); break;
      default: groth16_setup_run<2>(k, s); break;
    }
    if (!dev)
      for (int j = 0; j < 8; j++)
        if (out_bytes[j]) DG_HIP(hipMemcpy(host_out[j], d[j], out_bytes[j], hipMemcpyDeviceToHost));
    k.finish();
  });
}

void dg16_setup_srs_limits(unsigned* wave_from, unsigned* msm_from) {
  if (wave_from) *wave_from = srs::kWaveFrom;
  if (msm_from) *msm_from = srs::kMsmFrom;
}

int dg16_groth16_setup_srs(dg16_ctx* ctx, int curve, size_t num_constraints, size_t num_inputs, size_t num_vars,
                           unsigned log_m, const uint32_t* a_row_ptr, const uint32_t* a_col, const void* a_coeff,
                           const uint32_t* b_row_ptr, const uint32_t* b_col, const void* b_coeff,
                           const uint32_t* c_row_ptr, const uint32_t* c_col, const void* c_coeff, const dg16_srs* srs_in,
                           void* a_query, void* b_g1_query, void* b_g2_query, void* h_query, void* l_query,
                           void* fixed_points, void* gamma_g2, void* gamma_abc_g1, unsigned flags) {
  if (!ctx) return DG16_ERR_BAD_ARG;
  return guarded(ctx, [&] {
    DG_REQUIRE(curve >= 0 && curve <= 2, DG16_ERR_BAD_CURVE, "unknown curve id");
    const size_t nc = num_constraints, ni = num_inputs, nv = num_vars;
    DG_REQUIRE(a_row_ptr && b_row_ptr && c_row_ptr, DG16_ERR_BAD_ARG, "null operand");
    DG_REQUIRE(srs_in && srs_in->lag_g1 && srs_in->lag_g2 && srs_in->alpha_lag_g1 && srs_in->beta_lag_g1 &&
                   srs_in->h_g1 && srs_in->fixed,
               DG16_ERR_BAD_ARG, "null reference string");
    DG_REQUIRE(a_query && b_g1_query && b_g2_query && h_query && fixed_points && gamma_g2 && gamma_abc_g1 &&
                   (l_query || nv == ni),
               DG16_ERR_BAD_ARG, "null output");
    DG_REQUIRE(log_m <= 26, DG16_ERR_BAD_ARG, "domain larger than 2^26");
    const size_t m = (size_t)1 << log_m;
    DG_REQUIRE(ni >= 1 && ni <= nv && nc + ni <= m && nv < ((size_t)1 << 30), DG16_ERR_BAD_ARG,
               "need 1 <= num_inputs <= num_vars and num_constraints + num_inputs <= 2^log_m");
    const bool dev = flags & DG16_F_DEVICE_PTRS;
    Call k(ctx, 0);
    if (dev) DG_HIP(hipStreamSynchronize(k.s()));   // behind the producers on channel 0's stream, before row_ptr[nc] is read
    SrsSetupArgs s{};
    s.nc = nc; s.ni = ni; s.nv = nv; s.log_m = log_m;
    s.in_subgroup = flags & DG16_F_BASES_IN_SUBGROUP;
    const uint32_t* rp[3] = {a_row_ptr, b_row_ptr, c_row_ptr};
    const uint32_t* cl[3] = {a_col, b_col, c_col};
    const void* cf[3] = {a_coeff, b_coeff, c_coeff};
    std::vector<void*> owned;      // staged copies of host-pointer calls (freed on every path)
    struct Free {
      std::vector<void*>& v;
      ~Free() { for (void* p : v) (void)hipFree(p); }
    } free_owned{owned};
    auto dmalloc = [&](size_t bytes) {
      void* p = nullptr;
      DG_HIP(hipMalloc(&p, bytes ? bytes : 16));
      owned.push_back(p);
      return p;
    };
    for (int j = 0; j < 3; j++) {
      uint32_t last = 0;
      if (dev) {
        if (nc) DG_HIP(hipMemcpy(&last, rp[j] + nc, sizeof last, hipMemcpyDeviceToHost));
      } else {
        // matrix indices are checked before anything reaches the device, as dg16_groth16_setup does
        for (size_t i = 0; i < nc; i++)
          DG_REQUIRE(rp[j][i] <= rp[j][i + 1], DG16_ERR_BAD_ARG, "row_ptr is not non-decreasing");
        last = nc ? rp[j][nc] : 0;
        DG_REQUIRE(!last || (cl[j] && cf[j]), DG16_ERR_BAD_ARG, "null matrix");
        for (size_t e = nc ? rp[j][0] : 0; e < last; e++)
          DG_REQUIRE(cl[j][e] < nv, DG16_ERR_BAD_ARG, "matrix column >= num_vars");
      }
      DG_REQUIRE(!last || (cl[j] && cf[j]), DG16_ERR_BAD_ARG, "null matrix");
      s.nnz[j] = last;
      if (dev) {
        s.row_ptr[j] = rp[j]; s.col[j] = cl[j]; s.coeff[j] = cf[j];
      } else {
        void* p = dmalloc((nc + 1) * 4);
        void* c = dmalloc((size_t)last * 4);
        void* v = dmalloc((size_t)last * 32);
        DG_HIP(hipMemcpyAsync(p, rp[j], (nc + 1) * 4, hipMemcpyHostToDevice, k.s()));
        if (last) {
          DG_HIP(hipMemcpyAsync(c, cl[j], (size_t)last * 4, hipMemcpyHostToDevice, k.s()));
          DG_HIP(hipMemcpyAsync(v, cf[j], (size_t)last * 32, hipMemcpyHostToDevice, k.s()));
        }
        s.row_ptr[j] = (const unsigned*)p; s.col[j] = (const unsigned*)c; s.coeff[j] = v;
      }
    }
    // the entries of one output are numbered in 32 bits (K takes all three matrices and the instance terms)
    DG_REQUIRE(s.nnz[0] + s.nnz[1] + s.nnz[2] + ni < ((size_t)1 << 32), DG16_ERR_BAD_ARG, "more than 2^32 matrix entries");
    const size_t g1b = affine_bytes(curve, 1), g2b = affine_bytes(curve, 2);
    // the reference string: five arrays of m points
    const void* tabs[5] = {srs_in->lag_g1, srs_in->lag_g2, srs_in->alpha_lag_g1, srs_in->beta_lag_g1, srs_in->h_g1};
    const size_t tab_bytes[5] = {m * g1b, m * g2b, m * g1b, m * g1b, m * g1b};
    const void* dt[5];
    for (int j = 0; j < 5; j++) {
      if (dev) { dt[j] = tabs[j]; continue; }
      void* p = dmalloc(tab_bytes[j]);
      DG_HIP(hipMemcpyAsync(p, tabs[j], tab_bytes[j], hipMemcpyHostToDevice, k.s()));
      dt[j] = p;
    }
    s.lag_g1 = dt[0]; s.lag_g2 = dt[1]; s.alpha_lag_g1 = dt[2]; s.beta_lag_g1 = dt[3];
    void* host_out[8] = {a_query, b_g1_query, b_g2_query, h_query, l_query, fixed_points, gamma_g2, gamma_abc_g1};
    const size_t out_bytes[8] = {nv * g1b, nv * g1b, nv * g2b, m * g1b, (nv - ni) * g1b, 3 * g1b + 2 * g2b, g2b, ni * g1b};
    void* d[8];
    for (int j = 0; j < 8; j++) d[j] = dev ? host_out[j] : dmalloc(out_bytes[j]);
    s.a_query = d[0]; s.b_g1_query = d[1]; s.b_g2_query = d[2]; s.l_query = d[4]; s.gamma_abc_g1 = d[7];
    switch (curve) {
      case 0: groth16_setup_srs_run<0>(k, s); break;
      case 1: groth16_setup_srs_run<1>(k, s); break;
      default: groth16_setup_srs_run<2>(k, s); break;
    }
    // the copies: h_query = h_g1; fixed_points = alpha_g1 | beta_g1 | g1 | beta_g2 | g2 (delta = 1); gamma_g2 = g2
    DG_HIP(hipMemcpyAsync(d[3], dt[4], m * g1b, hipMemcpyDeviceToDevice, k.s()));
    DG_HIP(hipMemcpyAsync(d[5], srs_in->fixed, 3 * g1b + 2 * g2b, hipMemcpyHostToDevice, k.s()));
    DG_HIP(hipMemcpyAsync(d[6], (const char*)srs_in->fixed + 3 * g1b + g2b, g2b, hipMemcpyHostToDevice, k.s()));
    DG_HIP(hipStreamSynchronize(k.s()));
    if (!dev)
      for (int j = 0; j < 8; j++)
        if (out_bytes[j]) DG_HIP(hipMemcpy(host_out[j], d[j], out_bytes[j], hipMemcpyDeviceToHost));
    k.finish();
  });
}

}  // extern "C"
