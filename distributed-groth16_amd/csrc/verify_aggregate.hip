// C ABI of the aggregate verifier (include/dg16.h): dg16_groth16_verify_aggregate -- one verdict for a batch of proofs
// under caller-supplied coefficients.  Argument checks, staging of host-pointer calls and the dispatch on the curve;
// the kernels live in the per-curve objects (aggregate_curve.hip), the key handle is the batch verifier's
// (verify_batch.hip: dg16_vk_create).
#include "verify_batch.h"

using namespace dg16;

extern "C" {

int dg16_groth16_verify_aggregate(dg16_ctx* ctx, const dg16_vk* vk, const void* public_inputs, size_t n_public,
                                  const void* proofs_affine, size_t n_proofs, const void* coeffs, unsigned flags,
                                  uint8_t* accepted, int channel) {
  int rc = guard_channel(ctx, channel);
  if (rc) return rc;
  return guarded(ctx, [&] {
    DG_REQUIRE(vk && vk->ctx == ctx, DG16_ERR_BAD_ARG, "verifying key belongs to another context");
    DG_REQUIRE(!(flags & ~(unsigned)(DG16_F_SCALARS_MONT | DG16_F_DEVICE_PTRS)), DG16_ERR_BAD_ARG,
               "dg16_groth16_verify_aggregate takes DG16_F_SCALARS_MONT and DG16_F_DEVICE_PTRS only");
    DG_REQUIRE(n_public + 1 == vk->d.n_ic, DG16_ERR_LENGTH_MISMATCH,
               "public input count does not match the verification key");
    DG_REQUIRE(accepted, DG16_ERR_BAD_ARG, "null argument");
    DG_REQUIRE(!n_proofs || (proofs_affine && coeffs && (public_inputs || !n_public)), DG16_ERR_BAD_ARG, "null argument");
    DG_REQUIRE(n_proofs < ((size_t)1 << 30), DG16_ERR_BAD_ARG, "n_proofs must be < 2^30");
    const bool dev = flags & DG16_F_DEVICE_PTRS;
    const size_t pb = 2 * affine_bytes(vk->curve, 1) + affine_bytes(vk->curve, 2);
    Call k(ctx, channel);
    uint8_t* dv = dev ? accepted : (uint8_t*)ws(k.c, 0, 1);
    if (!n_proofs) {          // the empty product is one
      DG_HIP(hipMemsetAsync(dv, 1, 1, k.s()));
    } else {
      const void* dx = stage_in(k, 1, public_inputs, n_proofs * n_public * 32, dev);
      const void* dp = stage_in(k, 2, proofs_affine, n_proofs * pb, dev);
      const void* dc = stage_in(k, 3, coeffs, n_proofs * 16, dev);
      const bool mont = flags & DG16_F_SCALARS_MONT;
      if (vk->curve == DG16_BN254) verify_aggregate_run<0>(k, vk->d, dx, n_public, mont, dp, n_proofs, dc, dv);
      else verify_aggregate_run<1>(k, vk->d, dx, n_public, mont, dp, n_proofs, dc, dv);
    }
    if (!dev) stage_out(k, accepted, dv, 1, false);
    k.finish();
    if (!dev) DG_HIP(hipStreamSynchronize(k.s()));
  });
}

}  // extern "C"
