// The kernels of the batch verifier for ONE curve id (-DDG_CURVE=0 BN254, 1 BLS12-381): pairing_<curve>.o.
// One proof per lane, two launches per batch:
//   verify_prepare_kernel  the input checks (reduced coordinates, on the curve, order-r subgroup; public inputs < r)
//                          and acc = IC_0 + sum_j x_j IC_(j+1) by double-and-add, negated and affine
//   verify_decide_kernel   three Miller loops with one squaring chain -- (A, B) with B's lines computed in the loop,
//                          (-acc, gamma) and (-C, delta) from the key's line tables --, times the key's Miller value of
//                          (-alpha, beta), one final exponentiation, compare with one
// Blocks of one wave, so a batch spreads over as many compute units as it has waves: a lane's pairing is a long
// latency chain with its Fq12 values in scratch memory (pairing.h), and what a batch gains from the GPU
// is the number of such chains in flight.
#include <string.h>

#include <vector>

#include "pairing.h"
#include "verify_batch.h"

#ifndef DG_CURVE
#error "compile with -DDG_CURVE=0 or 1"
#endif

namespace dg16 {
namespace {

using P = Pairing<DG_CURVE>;
using Fq = P::Fq;
using Fq2 = P::Fq2;
using Fr = P::Fr;
constexpr int kLanes = 64;

__global__ __launch_bounds__(kLanes) void verify_prepare_kernel(P::Key key, const Fr* inputs, size_t n_public, bool mont,
                                                                const P::Proof* proofs, size_t n, Affine<Fq>* nacc,
                                                                uint8_t* ok) {
  const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
  if (i >= n) return;
  P::Proof pr = proofs[i];
  Affine<Fq> s = Affine<Fq>::inf();
  ok[i] = P::prepare_one(key, inputs + i * n_public, n_public, mont, pr, &s) ? 1 : 0;
  nacc[i] = s;
}

__global__ __launch_bounds__(kLanes) void verify_decide_kernel(P::Key key, const P::Proof* proofs, size_t n,
                                                               const Affine<Fq>* nacc, const uint8_t* ok,
                                                               uint8_t* verdict) {
  const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
  if (i >= n) return;
  uint8_t v = 0;
  if (ok[i]) {
    P::Proof pr = proofs[i];
    Affine<Fq> s = nacc[i];
    v = P::decide_one(key, pr, s) ? 1 : 0;
  }
  verdict[i] = v;
}

void* upload(const void* src, size_t bytes) {
  void* d = nullptr;
  DG_HIP(hipMalloc(&d, bytes));
  hipError_t e = hipMemcpy(d, src, bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    DG_HIP(e);
  }
  return d;
}

}  // namespace

template <>
bool vk_prepare<DG_CURVE>(const void* alpha_g1, const void* beta_g2, const void* gamma_g2, const void* delta_g2,
                          const void* ic, size_t n_ic, VkData* out) {
  Affine<Fq> alpha;
  Affine<Fq2> beta, gamma, delta;
  memcpy(&alpha, alpha_g1, sizeof alpha);
  memcpy(&beta, beta_g2, sizeof beta);
  memcpy(&gamma, gamma_g2, sizeof gamma);
  memcpy(&delta, delta_g2, sizeof delta);
  std::vector<Affine<Fq>> icv(n_ic);
  memcpy(icv.data(), ic, n_ic * sizeof(Affine<Fq>));
  std::vector<P::Line> tg(P::N_LINES), td(P::N_LINES);
  P::Fq12 ab;
  if (!P::prepare_key(alpha, beta, gamma, delta, icv.data(), n_ic, tg.data(), td.data(), &ab)) return false;
  // the aggregate verifier's third pair (aggregate_curve.hip): beta's lines and -alpha
  std::vector<P::Line> tb(P::N_LINES);
  if (!beta.is_inf()) P::prepare_g2(beta, tb.data());
  Affine<Fq> nalpha = alpha.is_inf() ? alpha : Affine<Fq>{alpha.x, alpha.y.neg()};
  VkData d;
  try {
    d.n_ic = n_ic;
    static_assert(sizeof delta <= sizeof d.delta_point, "delta_g2 does not fit VkData::delta_point");
    memcpy(d.delta_point, &delta, sizeof delta);
    d.ic = upload(icv.data(), n_ic * sizeof(Affine<Fq>));
    if (!gamma.is_inf()) d.gamma = upload(tg.data(), tg.size() * sizeof(P::Line));
    if (!delta.is_inf()) d.delta = upload(td.data(), td.size() * sizeof(P::Line));
    d.alpha_beta = upload(&ab, sizeof ab);
    if (!beta.is_inf()) d.beta = upload(tb.data(), tb.size() * sizeof(P::Line));
    d.neg_alpha = upload(&nalpha, sizeof nalpha);
  } catch (...) {
    vk_release(d);
    throw;
  }
  *out = d;
  return true;
}

template <>
void verify_batch_run<DG_CURVE>(Call& k, const VkData& vk, const void* inputs_dev, size_t n_public, bool mont,
                                const void* proofs_dev, size_t n, uint8_t* verdict_dev) {
  Affine<Fq>* nacc = (Affine<Fq>*)ws(k.c, 3, n * sizeof(Affine<Fq>));
  uint8_t* ok = (uint8_t*)ws(k.c, 4, n);
  P::Key key = {(const Affine<Fq>*)vk.ic, (const P::Line*)vk.gamma, (const P::Line*)vk.delta,
                (const P::Fq12*)vk.alpha_beta};
  const unsigned blocks = (unsigned)((n + kLanes - 1) / kLanes);
  k.begin_dominant();
  hipLaunchKernelGGL(verify_prepare_kernel, dim3(blocks), dim3(kLanes), 0, k.s(), key, (const Fr*)inputs_dev, n_public,
                     mont, (const P::Proof*)proofs_dev, n, nacc, ok);
  DG_HIP(hipGetLastError());
  hipLaunchKernelGGL(verify_decide_kernel, dim3(blocks), dim3(kLanes), 0, k.s(), key, (const P::Proof*)proofs_dev, n,
                     (const Affine<Fq>*)nacc, (const uint8_t*)ok, verdict_dev);
  DG_HIP(hipGetLastError());
  k.end_dominant();
}

}  // namespace dg16
