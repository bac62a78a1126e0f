// Key generation (dg16_fixed_base_mul, dg16_groth16_setup, dg16_groth16_setup_srs): what setup.hip (C ABI, curve
// dispatch) needs from the per-curve objects setup_<curve>.o and setup_srs_<curve>.o (setup_curve.hip and
// setup_srs_curve.hip compiled once per curve id, the way prover_bn254.hip etc. are).
#pragma once
#include "ctx.h"

namespace dg16 {

struct SetupArgs {
  size_t nc, ni, nv;
  unsigned log_m;
  const unsigned *row_ptr[3], *col[3];      // A, B, C as CSR by constraint (device pointers)
  const void* coeff[3];                     // Montgomery form (device pointers)
  size_t nnz[3];
  const void* trapdoor;                     // host: alpha | beta | gamma | delta | tau, canonical
  const void* generators;                   // host: g1 affine | g2 affine, or null
  bool libsnark;                            // DG16_F_QAP_LIBSNARK: h_query = [tau^i Z(tau) / delta]_{i < m-1} | identity
  // device outputs
  void *a_query, *b_g1_query, *b_g2_query, *h_query, *l_query, *fixed_points, *gamma_g2, *gamma_abc_g1;
};

// dg16_groth16_setup_srs: the same key from the Lagrange-basis points of a ceremony (setup_srs_curve.hip)
struct SrsSetupArgs {
  size_t nc, ni, nv;
  unsigned log_m;
  const unsigned *row_ptr[3], *col[3];      // A, B, C as CSR by constraint (device pointers)
  const void* coeff[3];                     // Montgomery form (device pointers)
  size_t nnz[3];
  const void *lag_g1, *lag_g2, *alpha_lag_g1, *beta_lag_g1;      // [m] affine points (device pointers)
  bool in_subgroup;                         // DG16_F_BASES_IN_SUBGROUP: the endomorphism split may be used
  // device outputs: the four sums over the matrices' columns (h_query and the fixed points are copies: setup.hip)
  void *a_query, *b_g1_query, *b_g2_query, *l_query, *gamma_abc_g1;
};

// out_dev[i] = scalars_dev[i] * base (affine); base_host null = the standard generator
template <int CURVE>
void fixed_base_run(Call& k, int group, const void* base_host, const void* scalars_dev, size_t n, bool mont,
                    void* out_dev);
// the whole generator on the call's stream; synchronises before it returns (it owns temporary device memory)
template <int CURVE>
void groth16_setup_run(Call& k, const SetupArgs& a);
// the four sparse transposed matrix x point-vector products on the call's stream; synchronises before it returns
template <int CURVE>
void groth16_setup_srs_run(Call& k, const SrsSetupArgs& a);
// (defined in the per-curve objects)
template <> void fixed_base_run<0>(Call&, int, const void*, const void*, size_t, bool, void*);
template <> void fixed_base_run<1>(Call&, int, const void*, const void*, size_t, bool, void*);
template <> void fixed_base_run<2>(Call&, int, const void*, const void*, size_t, bool, void*);
template <> void groth16_setup_run<0>(Call&, const SetupArgs&);
template <> void groth16_setup_run<1>(Call&, const SetupArgs&);
template <> void groth16_setup_run<2>(Call&, const SetupArgs&);
template <> void groth16_setup_srs_run<0>(Call&, const SrsSetupArgs&);
template <> void groth16_setup_srs_run<1>(Call&, const SrsSetupArgs&);
template <> void groth16_setup_srs_run<2>(Call&, const SrsSetupArgs&);

}  // namespace dg16
