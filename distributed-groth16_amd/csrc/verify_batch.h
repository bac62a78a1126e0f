// Batched Groth16 verification (dg16_vk_create, dg16_groth16_verify_batch, dg16_groth16_verify_aggregate): what
// verify_batch.hip and verify_aggregate.hip (C ABI, curve dispatch) need from the per-curve objects pairing_<curve>.o
// (pairing_curve.hip) and aggregate_<curve>.o (aggregate_curve.hip), each compiled once per curve id.
#pragma once
#include "ctx.h"

namespace dg16 {

struct VkData {            // a prepared verifying key: device memory owned by the dg16_vk handle
  size_t n_ic = 0;
  void* ic = nullptr;          // n_ic affine G1 points
  void* gamma = nullptr;       // the Miller-loop lines of gamma_g2 (null: gamma is the identity)
  void* delta = nullptr;
  void* alpha_beta = nullptr;  // the Miller value of (-alpha_g1, beta_g2), one Fq12
  // what the aggregate verifier pairs instead of alpha_beta (its pair is (-s_0 alpha, beta), s_0 known per call)
  void* beta = nullptr;        // the Miller-loop lines of beta_g2 (null: beta is the identity)
  void* neg_alpha = nullptr;   // -alpha_g1, one affine G1 point
  // delta_g2 itself (affine, host memory; 192 bytes hold the larger curve's): dg16_groth16_rerandomize multiplies it
  alignas(16) uint8_t delta_point[192] = {};
};

// Validates the key (host pointers), does the per-key work on the host and uploads it; false = malformed key.
template <int CURVE>
bool vk_prepare(const void* alpha_g1, const void* beta_g2, const void* gamma_g2, const void* delta_g2, const void* ic,
                size_t n_ic, VkData* out);
// verdict_dev[i] for n proofs on the call's stream (device pointers); temporaries come from the channel's workspace
template <int CURVE>
void verify_batch_run(Call& k, const VkData& vk, const void* inputs_dev, size_t n_public, bool mont,
                      const void* proofs_dev, size_t n, uint8_t* verdict_dev);
// *accepted_dev for the whole batch under the coefficients coeffs_dev (n x 16 bytes), n >= 1, on the call's stream
// (device pointers); temporaries and the two MSMs use the channel's workspace
template <int CURVE>
void verify_aggregate_run(Call& k, const VkData& vk, const void* inputs_dev, size_t n_public, bool mont,
                          const void* proofs_dev, size_t n, const void* coeffs_dev, uint8_t* accepted_dev);
// (defined in the per-curve objects)
template <> bool vk_prepare<0>(const void*, const void*, const void*, const void*, const void*, size_t, VkData*);
template <> bool vk_prepare<1>(const void*, const void*, const void*, const void*, const void*, size_t, VkData*);
template <> void verify_batch_run<0>(Call&, const VkData&, const void*, size_t, bool, const void*, size_t, uint8_t*);
template <> void verify_batch_run<1>(Call&, const VkData&, const void*, size_t, bool, const void*, size_t, uint8_t*);
template <> void verify_aggregate_run<0>(Call&, const VkData&, const void*, size_t, bool, const void*, size_t, const void*,
                                         uint8_t*);
template <> void verify_aggregate_run<1>(Call&, const VkData&, const void*, size_t, bool, const void*, size_t, const void*,
                                         uint8_t*);

inline void vk_release(VkData& d) {
  for (void** p : {&d.ic, &d.gamma, &d.delta, &d.alpha_beta, &d.beta, &d.neg_alpha}) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
  }
}

}  // namespace dg16

struct dg16_vk {
  dg16_ctx* ctx = nullptr;
  int curve = 0;
  dg16::VkData d;
};
