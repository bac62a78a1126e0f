// Groth16 prover instantiated for curve id 2 (bls12_377).
#include "msm_impl.h"

namespace dg16 {
DG16_MSM_EXTERN(CurveTypes<2>)   // compiled in msm_group.hip / msm_reduce.hip
}  // namespace dg16

#include "prover_impl.h"

namespace dg16 {
void pk_build_bls12_377(dg16_ctx* ctx, PkDev& d, const void* a, const void* b1, const void* b2, const void* h, const void* l,
                 const void* fx, bool dev) { pk_build<2>(ctx, d, a, b1, b2, h, l, fx, dev); }
void prove_bls12_377(dg16_ctx* ctx, const PkDev& pk, const void* a, const void* b, const void* c, const void* w,
              const void* rs, bool mont, bool dev, void* out, bool overlap, bool libsnark) {
  prove_typed<2>(ctx, pk, a, b, c, w, rs, mont, dev, out, overlap, libsnark);
}
void msms_bls12_377(dg16_ctx* ctx, Call& k0, Call& k1, Call& k2, const PkDev& pk, const void* a, const void* b, const void* c,
             const void* w, const void* rs, bool mont, bool dev, uint8_t* res, const dg16_comm* comm, const void* h_given) {
  msms_typed<2>(ctx, k0, k1, k2, pk, a, b, c, w, rs, mont, dev, res, comm, h_given);
}
void prove_dist_bls12_377(dg16_ctx* ctx, const PkDev& pk, const dg16_comm* comm, const void* a, const void* b, const void* c,
              const void* w, const void* rs, bool mont, bool dev, void* out, bool overlap) {
  prove_dist_typed<2>(ctx, pk, comm, a, b, c, w, rs, mont, dev, out, overlap);
}
void assemble_bls12_377(Call& k0, const uint8_t* gathered, size_t n_shards, uint8_t* proof) {
  assemble_typed<2>(k0, gathered, n_shards, proof);
}
size_t results_bytes_bls12_377() { return msm_results_bytes<2>(); }
size_t proof_bytes_bls12_377() {
  using CT = CurveTypes<2>;
  return 2 * sizeof(Jacobian<CT::Fq>) + sizeof(Jacobian<CT::Fq2>);
}
}  // namespace dg16
