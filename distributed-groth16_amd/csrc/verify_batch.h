// Batched Groth16 verification (dg16_vk_create, dg16_groth16_verify_batch): what verify_batch.hip (C ABI, curve
// dispatch) needs from the per-curve objects pairing_<curve>.o (pairing_curve.hip compiled once per curve id).
#pragma once
#include "ctx.h"

namespace dg16 {

struct VkData {            // a prepared verifying key: device memory owned by the dg16_vk handle
  size_t n_ic = 0;
  void* ic = nullptr;          // n_ic affine G1 points
  void* gamma = nullptr;       // the Miller-loop lines of gamma_g2 (null: gamma is the identity)
  void* delta = nullptr;
  void* alpha_beta = nullptr;  // the Miller value of (-alpha_g1, beta_g2), one Fq12
};

// Validates the key (host pointers), does the per-key work on the host and uploads it; false = malformed key.
template <int CURVE>
bool vk_prepare(const void* alpha_g1, const void* beta_g2, const void* gamma_g2, const void* delta_g2, const void* ic,
                size_t n_ic, VkData* out);
// verdict_dev[i] for n proofs on the call's stream (device pointers); temporaries come from the channel's workspace
template <int CURVE>
void verify_batch_run(Call& k, const VkData& vk, const void* inputs_dev, size_t n_public, bool mont,
                      const void* proofs_dev, size_t n, uint8_t* verdict_dev);
// (defined in the per-curve objects)
template <> bool vk_prepare<0>(const void*, const void*, const void*, const void*, const void*, size_t, VkData*);
template <> bool vk_prepare<1>(const void*, const void*, const void*, const void*, const void*, size_t, VkData*);
template <> void verify_batch_run<0>(Call&, const VkData&, const void*, size_t, bool, const void*, size_t, uint8_t*);
template <> void verify_batch_run<1>(Call&, const VkData&, const void*, size_t, bool, const void*, size_t, uint8_t*);

inline void vk_release(VkData& d) {
  for (void** p : {&d.ic, &d.gamma, &d.delta, &d.alpha_beta}) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
  }
}

}  // namespace dg16
