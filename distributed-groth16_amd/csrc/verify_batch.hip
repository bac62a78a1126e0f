// C ABI of the batch verifier (include/dg16.h): dg16_vk_create, dg16_vk_destroy, dg16_groth16_verify_batch.
// Argument checks, staging of host-pointer calls and the dispatch on the curve; the pairing arithmetic and the
// kernels live in the per-curve objects (pairing_curve.hip).  The single-proof host verifier (verify.hip) is a
// separate, older path and shares nothing with this one.
#include <vector>

#include "verify_batch.h"

using namespace dg16;

extern "C" {

int dg16_vk_create(dg16_ctx* ctx, int curve, const void* alpha_g1, const void* beta_g2, const void* gamma_g2,
                   const void* delta_g2, const void* ic, size_t n_ic, unsigned flags, dg16_vk** out) {
  if (!ctx) return DG16_ERR_BAD_ARG;
  return guarded(ctx, [&] {
    DG_REQUIRE(out, DG16_ERR_BAD_ARG, "null output");
    *out = nullptr;
    DG_REQUIRE(curve >= 0 && curve <= 2, DG16_ERR_BAD_CURVE, "unknown curve id");
    DG_REQUIRE(curve != DG16_BLS12_377, DG16_ERR_UNSUPPORTED, "batch verification: BN254 and BLS12-381 only");
    DG_REQUIRE(alpha_g1 && beta_g2 && gamma_g2 && delta_g2 && ic, DG16_ERR_BAD_ARG, "null argument");
    DG_REQUIRE(n_ic >= 1 && n_ic < ((size_t)1 << 24), DG16_ERR_BAD_ARG, "need 1 <= n_ic < 2^24");
    DG_REQUIRE(!(flags & ~(unsigned)DG16_F_DEVICE_PTRS), DG16_ERR_BAD_ARG, "dg16_vk_create takes DG16_F_DEVICE_PTRS only");
    DG_HIP(hipSetDevice(ctx->device));
    const size_t g1b = affine_bytes(curve, 1), g2b = affine_bytes(curve, 2);
    // the per-key work runs on the host: a key on the device comes back first
    std::vector<uint8_t> host;
    const void* src[5] = {alpha_g1, beta_g2, gamma_g2, delta_g2, ic};
    if (flags & DG16_F_DEVICE_PTRS) {
      sync_channel0(ctx);   // the blocking copies below run on the NULL stream: wait for the key's producers first
      const size_t bytes[5] = {g1b, g2b, g2b, g2b, n_ic * g1b};
      host.resize(g1b + 3 * g2b + n_ic * g1b);
      size_t off = 0;
      for (int j = 0; j < 5; j++) {
        DG_HIP(hipMemcpy(host.data() + off, src[j], bytes[j], hipMemcpyDeviceToHost));
        src[j] = host.data() + off;
        off += bytes[j];
      }
    }
    dg16_vk* vk = new dg16_vk;
    vk->ctx = ctx;
    vk->curve = curve;
    bool ok;
    try {
      ok = curve == DG16_BN254 ? vk_prepare<0>(src[0], src[1], src[2], src[3], src[4], n_ic, &vk->d)
                               : vk_prepare<1>(src[0], src[1], src[2], src[3], src[4], n_ic, &vk->d);
    } catch (...) {
      delete vk;
      throw;
    }
    if (!ok) {
      delete vk;
      throw StatusError{DG16_ERR_BAD_ARG,
                        "malformed verifying key (non-reduced coordinate, point off its curve or outside the subgroup)"};
    }
    *out = vk;
  });
}

void dg16_vk_destroy(dg16_vk* vk) {
  if (!vk) return;
  if (vk->ctx && hipSetDevice(vk->ctx->device) == hipSuccess) {
    (void)hipDeviceSynchronize();   // a stream-ordered batch may still read the tables
    vk_release(vk->d);
  }
  delete vk;
}

int dg16_groth16_verify_batch(dg16_ctx* ctx, const dg16_vk* vk, const void* public_inputs, size_t n_public,
                              const void* proofs_affine, size_t n_proofs, unsigned flags, uint8_t* verdict,
                              int channel) {
  int rc = guard_channel(ctx, channel);
  if (rc) return rc;
  return guarded(ctx, [&] {
    DG_REQUIRE(vk && vk->ctx == ctx, DG16_ERR_BAD_ARG, "verifying key belongs to another context");
    DG_REQUIRE(n_public + 1 == vk->d.n_ic, DG16_ERR_LENGTH_MISMATCH,
               "public input count does not match the verification key");
    if (!n_proofs) return;
    DG_REQUIRE(proofs_affine && verdict && (public_inputs || !n_public), DG16_ERR_BAD_ARG, "null argument");
    DG_REQUIRE(n_proofs < ((size_t)1 << 30), DG16_ERR_BAD_ARG, "n_proofs must be < 2^30");
    const bool dev = flags & DG16_F_DEVICE_PTRS;
    const size_t pb = 2 * affine_bytes(vk->curve, 1) + affine_bytes(vk->curve, 2);
    Call k(ctx, channel);
    const void* dx = stage_in(k, 1, public_inputs, n_proofs * n_public * 32, dev);
    const void* dp = stage_in(k, 2, proofs_affine, n_proofs * pb, dev);
    uint8_t* dv = dev ? verdict : (uint8_t*)ws(k.c, 0, n_proofs);
    const bool mont = flags & DG16_F_SCALARS_MONT;
    if (vk->curve == DG16_BN254) verify_batch_run<0>(k, vk->d, dx, n_public, mont, dp, n_proofs, dv);
    else verify_batch_run<1>(k, vk->d, dx, n_public, mont, dp, n_proofs, dv);
    if (!dev) stage_out(k, verdict, dv, n_proofs, false);
    k.finish();
    if (!dev) DG_HIP(hipStreamSynchronize(k.s()));
  });
}

}  // extern "C"
