// C ABI of the batched point multiplication and of proof re-randomization (include/dg16.h): dg16_points_mul,
// dg16_ctx_set_points_mul_slice, dg16_groth16_rerandomize.  Argument checks, staging of host-pointer calls and the
// dispatch on the curve; the kernels live in the per-curve objects (points_mul_curve.hip).
#include <string.h>

#include "points_mul.h"

using namespace dg16;

namespace {

// 1 <= x < r on the stored 32-byte words (host side of pmul::rr_scalar_ok)
bool host_scalar_ok(int curve, const uint8_t* x) {
  if (curve == DG16_BN254) {
    bn254_fr v;
    memcpy(&v, x, 32);
    return pmul::rr_scalar_ok(v);
  }
  bls12_381_fr v;
  memcpy(&v, x, 32);
  return pmul::rr_scalar_ok(v);
}

}  // namespace

extern "C" {

int dg16_ctx_set_points_mul_slice(dg16_ctx* ctx, size_t products) {
  if (!ctx) return DG16_ERR_BAD_ARG;
  return guarded(ctx, [&] {
    DG_REQUIRE(products <= ((size_t)1 << 20), DG16_ERR_BAD_ARG, "slice must be <= 2^20 products (0 = default)");
    std::lock_guard<std::mutex> g(ctx->mu);
    ctx->points_mul_slice = products;
  });
}

int dg16_points_mul(dg16_ctx* ctx, int curve, int group, const void* points_affine, const void* scalars, size_t n,
                    void* out_affine, unsigned flags, int channel) {
  int rc = guard_channel(ctx, channel);
  if (rc) return rc;
  return guarded(ctx, [&] {
    DG_REQUIRE(curve >= 0 && curve <= 2, DG16_ERR_BAD_CURVE, "unknown curve id");
    DG_REQUIRE(group == 1 || group == 2, DG16_ERR_BAD_ARG, "group must be 1 (G1) or 2 (G2)");
    DG_REQUIRE(n == 0 || (points_affine && scalars && out_affine), DG16_ERR_BAD_ARG, "null operand");
    DG_REQUIRE(n < ((size_t)1 << 30), DG16_ERR_BAD_ARG, "n must be < 2^30");
    if (!n) return;
    const bool dev = flags & DG16_F_DEVICE_PTRS;
    const size_t pb = affine_bytes(curve, group);
    Call k(ctx, channel);
    const void* dscal = stage_in(k, 1, scalars, n * 32, dev);
    const void* dpts = stage_in(k, 2, points_affine, n * pb, dev);
    void* dout = dev ? out_affine : ws(k.c, 0, n * pb);
    const unsigned mode = msm_mode(flags);
    switch (curve) {
      case 0: points_mul_run<0>(k, group, dpts, dscal, n, mode, dout); break;
      case 1: points_mul_run<1>(k, group, dpts, dscal, n, mode, dout); break;
      default: points_mul_run<2>(k, group, dpts, dscal, n, mode, dout); break;
    }
    if (!dev) stage_out(k, out_affine, dout, n * pb, false);
    k.finish();
    if (!dev) DG_HIP(hipStreamSynchronize(k.s()));
  });
}

int dg16_groth16_rerandomize(dg16_ctx* ctx, const dg16_vk* vk, const void* proofs_affine, size_t n_proofs,
                             const void* r1_r2, unsigned flags, void* proofs_out, int channel) {
  int rc = guard_channel(ctx, channel);
  if (rc) return rc;
  return guarded(ctx, [&] {
    DG_REQUIRE(vk && vk->ctx == ctx, DG16_ERR_BAD_ARG, "verifying key belongs to another context");
    DG_REQUIRE(!(flags & ~(unsigned)(DG16_F_DEVICE_PTRS | DG16_F_SCALARS_MONT)), DG16_ERR_BAD_ARG,
               "dg16_groth16_rerandomize takes DG16_F_SCALARS_MONT and DG16_F_DEVICE_PTRS only");
    if (!n_proofs) return;
    DG_REQUIRE(proofs_affine && r1_r2 && proofs_out, DG16_ERR_BAD_ARG, "null argument");
    DG_REQUIRE(n_proofs < ((size_t)1 << 28), DG16_ERR_BAD_ARG, "n_proofs must be < 2^28");
    const bool dev = flags & DG16_F_DEVICE_PTRS;
    if (!dev) {
      const uint8_t* r = (const uint8_t*)r1_r2;
      for (size_t i = 0; i < 2 * n_proofs; i++)
        DG_REQUIRE(host_scalar_ok(vk->curve, r + 32 * i), DG16_ERR_BAD_ARG, "r1 or r2 is zero or not below r");
    }
    const size_t pb = 2 * affine_bytes(vk->curve, 1) + affine_bytes(vk->curve, 2);
    Call k(ctx, channel);
    const void* dr = stage_in(k, 1, r1_r2, n_proofs * 64, dev);
    const void* dp = stage_in(k, 2, proofs_affine, n_proofs * pb, dev);
    void* dout = dev ? proofs_out : ws(k.c, 0, n_proofs * pb);
    const bool mont = flags & DG16_F_SCALARS_MONT;
    if (vk->curve == DG16_BN254) rerandomize_run<0>(k, vk->d, dp, n_proofs, dr, mont, dout);
    else rerandomize_run<1>(k, vk->d, dp, n_proofs, dr, mont, dout);
    if (!dev) stage_out(k, proofs_out, dout, n_proofs * pb, false);
    k.finish();
    if (!dev) DG_HIP(hipStreamSynchronize(k.s()));
  });
}

}  // extern "C"
