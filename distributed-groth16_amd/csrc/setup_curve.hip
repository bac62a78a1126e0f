// Per-curve object of the key generator: the fixed-base kernels (fixed_base_impl.h) for G1 and G2 of curve DG_CURVE and
// the scalar side of dg16_groth16_setup -- LibsnarkReduction::instance_map_with_evaluation (reached through
// ark-circom/src/circom/qap.rs:20-25) and CircomReduction::h_query_scalars (qap.rs:94-110), all on the device.
//
//   u = L_i(tau), i < m        inverse NTT of [tau^j]: L_i(tau) = (1/m) sum_j (tau w^-i)^j
//   a_k, b_k, c_k = (M^T u)_k  the three CSR matrices are transposed by a counting sort over the columns (count,
//                              scan, fill: setup_transpose.h); one lane per wire then GATHERS its column -- there
//                              is no atomic add in Fr
//   abc_k = beta a_k + alpha b_k + c_k, / gamma for the instance wires, / delta for the witness wires
//   h                          inverse NTT of size 2 m of [tau^j / delta]_{j < 2m-1} | 0, odd-indexed entries
//                              (DG16_F_QAP_LIBSNARK: the geometric sequence tau^i Z(tau) / delta, i < m - 1, then 0)
//   seven fixed-base calls     a, b (G1), b (G2), h, l, gamma_abc, and the six fixed points
#include <string.h>

#include "fixed_base_impl.h"
#include "setup.h"
#include "setup_transpose.h"

#ifndef DG_CURVE
#error "compile with -DDG_CURVE=<curve id>"
#endif

namespace dg16 {
namespace {

using CT = CurveTypes<DG_CURVE>;
using Fr = CT::Fr;

// out[j] = scale * base^j for j < count, zero for count <= j < total
__global__ void __launch_bounds__(256) setup_powers_kernel(Fr* __restrict__ out, size_t count, size_t total,
                                                            const Fr* __restrict__ base, const Fr* __restrict__ scale) {
  size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= total) return;
  out[j] = j < count ? base->pow_u64((uint64_t)j) * *scale : Fr::zero();
}

// out[j] = scale * base^j for j < count, zero for count <= j < total, as a chunked power ladder: a lane raises base to
// the start of its kGeoChunk consecutive exponents once (log2 steps) and multiplies its way through them
constexpr unsigned kGeoChunk = 16;
__global__ void __launch_bounds__(256) setup_geometric_kernel(Fr* __restrict__ out, size_t count, size_t total,
                                                               const Fr* __restrict__ base, const Fr* __restrict__ scale) {
  const size_t j0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * kGeoChunk;
  if (j0 >= total) return;
  const Fr g = *base;
  Fr v = j0 < count ? g.pow_u64((uint64_t)j0) * *scale : Fr::zero();
  for (size_t j = j0; j < j0 + kGeoChunk && j < total; j++) {
    out[j] = j < count ? v : Fr::zero();
    v = v * g;
  }
}

__global__ void __launch_bounds__(256) setup_odd_kernel(const Fr* __restrict__ in, size_t m, Fr* __restrict__ out) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) out[i] = in[2 * i + 1];
}

using TCsr = TCsrT<Fr>;      // setup_transpose.h
__device__ __forceinline__ Fr setup_column(const TCsr& M, size_t k, const Fr* __restrict__ u) {
  Fr acc = Fr::zero();
  for (unsigned p = M.ptr[k], e = M.ptr[k + 1]; p < e; p++) acc = acc + M.coeff[M.t_src[p]] * u[M.t_row[p]];
  return acc;
}
// consts: alpha | beta | 1/gamma | 1/delta (Montgomery).  One lane per wire.
__global__ void __launch_bounds__(256) setup_wire_kernel(TCsr A, TCsr B, TCsr Cm, const Fr* __restrict__ u,
                                                          const Fr* __restrict__ consts, size_t nc, size_t ni, size_t nv,
                                                          Fr* __restrict__ a_s, Fr* __restrict__ b_s,
                                                          Fr* __restrict__ gamma_abc_s, Fr* __restrict__ l_s) {
  size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nv) return;
  Fr a = setup_column(A, k, u), b = setup_column(B, k, u), c = setup_column(Cm, k, u);
  if (k < ni) a = a + u[nc + k];
  a_s[k] = a;
  b_s[k] = b;
  const Fr abc = consts[1] * a + consts[0] * b + c;
  if (k < ni) gamma_abc_s[k] = abc * consts[2];
  else l_s[k - ni] = abc * consts[3];
}

bool host_canonical_nonzero(const Fr& x) {
  bool nz = false;
  for (int i = 0; i < Fr::NL; i++) nz |= x.l[i] != 0;
  if (!nz) return false;
  for (int i = Fr::NL - 1; i >= 0; i--) {
    if (x.l[i] < Fr::Params::P[i]) return true;
    if (x.l[i] > Fr::Params::P[i]) return false;
  }
  return false;      // == r
}

}  // namespace

template <>
void fixed_base_run<DG_CURVE>(Call& k, int group, const void* base_host, const void* scalars_dev, size_t n, bool mont,
                              void* out_dev) {
  if (group == 1) fixed_base_typed<CT::Fq, CT::G1c, Fr, CT::SCALAR_BITS>(k, base_host, scalars_dev, n, mont, out_dev);
  else fixed_base_typed<CT::Fq2, CT::G2c, Fr, CT::SCALAR_BITS>(k, base_host, scalars_dev, n, mont, out_dev);
}

template <>
void groth16_setup_run<DG_CURVE>(Call& k, const SetupArgs& s) {
  const size_t m = (size_t)1 << s.log_m, nc = s.nc, ni = s.ni, nv = s.nv;
  // ---- trapdoor (host): canonical, non-zero, tau outside the domain (Z(tau) = tau^m - 1 != 0) ----------------
  Fr td[5];
  memcpy(td, s.trapdoor, sizeof td);
  for (int i = 0; i < 5; i++) {
    DG_REQUIRE(host_canonical_nonzero(td[i]), DG16_ERR_BAD_ARG, "trapdoor element is zero or not below r");
    td[i] = td[i].to_mont();
  }
  const Fr alpha = td[0], beta = td[1], gamma = td[2], delta = td[3], tau = td[4];
  Fr zt = tau;
  for (unsigned i = 0; i < s.log_m; i++) zt = zt.sqr();
  DG_REQUIRE(zt != Fr::one(), DG16_ERR_BAD_ARG, "tau lies in the evaluation domain (tau^m = 1)");
  const Fr dinv = delta.inv(), ginv = gamma.inv();
  // device constants: 0 alpha | 1 beta | 2 1/gamma | 3 1/delta | 4 tau | 5 one | 6..8 alpha beta delta | 9..11 beta delta gamma
  //                   12 Z(tau) / delta
  const Fr host_consts[13] = {alpha, beta, ginv, dinv, tau, Fr::one(), alpha, beta, delta, beta, delta, gamma,
                              (zt - Fr::one()) * dinv};
  DevBuf consts(sizeof host_consts + 16);
  Fr* cd = consts.as<Fr>();
  unsigned* flag = (unsigned*)(cd + 13);
  DG_HIP(hipMemcpyAsync(cd, host_consts, sizeof host_consts, hipMemcpyHostToDevice, k.s()));
  DG_HIP(hipMemsetAsync(flag, 0, 16, k.s()));
  DG_HIP(hipStreamSynchronize(k.s()));          // host_consts is a stack buffer

  const size_t g1b = sizeof(Affine<CT::Fq>), g2b = sizeof(Affine<CT::Fq2>);
  const char* gens = (const char*)s.generators;
  const void* g1 = gens;
  const void* g2 = gens ? gens + g1b : nullptr;

  // ---- scalars ------------------------------------------------------------------------------------------------
  DevBuf a_s(nv * sizeof(Fr)), b_s(nv * sizeof(Fr)), gabc_s(ni * sizeof(Fr)), l_s((nv - ni) * sizeof(Fr)),
      h_s(m * sizeof(Fr));
  {
    DevBuf u(m * sizeof(Fr)), big(s.libsnark ? 0 : 2 * m * sizeof(Fr));
    hipLaunchKernelGGL(setup_powers_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, k.s(), u.as<Fr>(), m, m,
                       cd + 4, cd + 5);
    ntt_launch(k, DG_CURVE, u.p, s.log_m, 1, nullptr);
    if (s.libsnark) {
      const size_t lanes = (m + kGeoChunk - 1) / kGeoChunk;
      hipLaunchKernelGGL(setup_geometric_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, k.s(), h_s.as<Fr>(),
                         m - 1, m, cd + 4, cd + 12);
    } else {
      hipLaunchKernelGGL(setup_powers_kernel, dim3((unsigned)((2 * m + 255) / 256)), dim3(256), 0, k.s(), big.as<Fr>(),
                         2 * m - 1, 2 * m, cd + 4, cd + 3);
      ntt_launch(k, DG_CURVE, big.p, s.log_m + 1, 1, nullptr);
      hipLaunchKernelGGL(setup_odd_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, k.s(), big.as<Fr>(), m,
                         h_s.as<Fr>());
    }
    Transposes<Fr> tr(k, s.row_ptr, s.col, s.coeff, s.nnz, nc, nv, flag);
    const TCsr* t = tr.t;
    hipLaunchKernelGGL(setup_wire_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, k.s(), t[0], t[1], t[2],
                       u.as<Fr>(), cd, nc, ni, nv, a_s.as<Fr>(), b_s.as<Fr>(), gabc_s.as<Fr>(), l_s.as<Fr>());
    DG_HIP(hipGetLastError());
    DG_HIP(hipStreamSynchronize(k.s()));
    unsigned bad = 0;
    DG_HIP(hipMemcpy(&bad, flag, sizeof bad, hipMemcpyDeviceToHost));
    DG_REQUIRE(!bad, DG16_ERR_BAD_ARG, "dg16_groth16_setup: matrix entry out of range (column >= num_vars or bad row_ptr)");
  }   // (u, the size-2m buffer and the transposes are freed before the point tables are built)

  // ---- points -------------------------------------------------------------------------------------------------
  fixed_base_run<DG_CURVE>(k, 1, g1, a_s.p, nv, true, s.a_query);
  fixed_base_run<DG_CURVE>(k, 1, g1, b_s.p, nv, true, s.b_g1_query);
  fixed_base_run<DG_CURVE>(k, 2, g2, b_s.p, nv, true, s.b_g2_query);
  fixed_base_run<DG_CURVE>(k, 1, g1, h_s.p, m, true, s.h_query);
  fixed_base_run<DG_CURVE>(k, 1, g1, l_s.p, nv - ni, true, s.l_query);
  fixed_base_run<DG_CURVE>(k, 1, g1, gabc_s.p, ni, true, s.gamma_abc_g1);
  DevBuf fixed2(3 * g2b);
  fixed_base_run<DG_CURVE>(k, 1, g1, cd + 6, 3, true, s.fixed_points);                    // alpha_g1 | beta_g1 | delta_g1
  fixed_base_run<DG_CURVE>(k, 2, g2, cd + 9, 3, true, fixed2.p);                          // beta_g2 | delta_g2 | gamma_g2
  DG_HIP(hipMemcpyAsync((char*)s.fixed_points + 3 * g1b, fixed2.p, 2 * g2b, hipMemcpyDeviceToDevice, k.s()));
  DG_HIP(hipMemcpyAsync(s.gamma_g2, (char*)fixed2.p + 2 * g2b, g2b, hipMemcpyDeviceToDevice, k.s()));
  DG_HIP(hipStreamSynchronize(k.s()));
}

}  // namespace dg16
