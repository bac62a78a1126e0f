// The kernels of the aggregate verifier for ONE curve id (-DDG_CURVE=0 BN254, 1 BLS12-381): aggregate_<curve>.o.
// One verdict for a batch: with caller-supplied coefficients rho_i (include/dg16.h) the small-exponent test
//   prod_i e(rho_i A_i, B_i) e(-sum_j s_j IC_j, gamma) e(-sum_i rho_i C_i, delta) e(-s_0 alpha, beta) == 1,
//   s_j = sum_i rho_i x_ij mod r, x_i0 = 1
// in stages whose only single-lane serial one is the final exponentiation:
//   aggregate_check_kernel    one proof per lane: the input checks of the batch verifier (pairing.h: valid_g1 / valid_g2,
//                             inputs < r) plus rho_i != 0; rho_i A_i by a 128-bit double-and-add; a sanitised C_i and
//                             rho_i (identity and zero for a proof that failed) for the MSM; an ok byte per proof
//   aggregate_colsum_kernel   s_j: workgroups over slices of the proofs per column, summed through LDS; a second launch
//                             of the same shape adds the slices
//   (msm_launch, twice)       ACC = sum_j s_j IC_j and CS = sum_i rho_i C_i: the library's MSM on the call's stream
//   aggregate_miller_kernel   (rho_i A_i, B_i) per lane with B's lines computed in the loop; one more workgroup runs the
//                             three key-side pairs (-ACC, gamma), (-CS, delta), (-s_0 alpha, beta) from the key's line
//                             tables, a lane each; every one-wave workgroup multiplies its values down to one through LDS
//   aggregate_product_kernel  the product tree over the workgroups' values, 64 to one per level
//   aggregate_decide_kernel   one lane: final exponentiation, compare with one, AND with "no proof failed a check"
// Fq12 multiplication is exactly associative and commutative, so the order of the tree changes nothing.
#include <algorithm>

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
using Fq12 = P::Fq12;
constexpr int kLanes = 64;
constexpr int kSumThreads = 256;
constexpr unsigned kSumSlices = 256;   // at most this many workgroups per column in the first pass

__global__ __launch_bounds__(kLanes) void aggregate_check_kernel(const Fr* inputs, size_t n_public, bool mont,
                                                                  const P::Proof* proofs, const uint32_t* coeffs,
                                                                  size_t n, Affine<Fq>* ra, Affine<Fq>* cs, Fr* rho,
                                                                  Fr* rk, uint8_t* ok, unsigned* bad) {
  const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
  if (i >= n) return;
  P::Proof pr = proofs[i];
  Fr r = Fr::zero();
  for (int w = 0; w < 4; w++) r.l[w] = coeffs[4 * i + w];
  bool good = !r.is_zero();                      // a zero coefficient would skip the proof
  good = good && P::valid_g1(pr.a) && P::valid_g2(pr.b) && P::valid_g1(pr.c);
  for (size_t j = 0; good && j < n_public; j++) good = P::canonical(inputs[i * n_public + j]);
  Affine<Fq> a = Affine<Fq>::inf(), c = Affine<Fq>::inf();
  Fr k = Fr::zero();
  if (good) {
    a = scalar_mul<Fq, 4>(XYZZ<Fq>::from_affine(pr.a), r.l).to_affine();
    c = pr.c;
    // the factor that turns an input as it was given into rho x as a plain integer under one Montgomery product
    k = mont ? r : r.to_mont();
  } else {
    r = Fr::zero();
    atomicOr(bad, 1u);
  }
  ra[i] = a;
  cs[i] = c;
  rho[i] = r;
  rk[i] = k;
  ok[i] = good ? 1 : 0;
}

// Sum of a workgroup's values through LDS; the result is valid on thread 0.
__device__ Fr block_sum(Fr acc, Fr* sh) {
  const unsigned t = threadIdx.x;
  sh[t] = acc;
  __syncthreads();
  for (unsigned s = kSumThreads / 2; s; s >>= 1) {
    if (t < s) sh[t] = sh[t] + sh[t + s];
    __syncthreads();
  }
  return sh[0];
}

// part[j * slices + slice] = sum over the slice's proofs of rho_i x_ij (column 0: of rho_i); grid (n_public + 1, slices)
__global__ __launch_bounds__(kSumThreads) void aggregate_colsum_kernel(const Fr* inputs, size_t n_public, const Fr* rho,
                                                                        const Fr* rk, size_t n, Fr* part) {
  __shared__ Fr sh[kSumThreads];
  const size_t j = blockIdx.x;
  Fr acc = Fr::zero();
  for (size_t i = (size_t)blockIdx.y * kSumThreads + threadIdx.x; i < n; i += (size_t)gridDim.y * kSumThreads)
    acc = acc + (j ? rk[i] * inputs[i * n_public + (j - 1)] : rho[i]);
  acc = block_sum(acc, sh);
  if (threadIdx.x == 0) part[j * gridDim.y + blockIdx.y] = acc;
}
// s[j] = sum of column j's slices; grid (n_public + 1)
__global__ __launch_bounds__(kSumThreads) void aggregate_colsum_final_kernel(const Fr* part, unsigned slices, Fr* s) {
  __shared__ Fr sh[kSumThreads];
  const size_t j = blockIdx.x;
  Fr acc = Fr::zero();
  for (unsigned i = threadIdx.x; i < slices; i += kSumThreads) acc = acc + part[j * slices + i];
  acc = block_sum(acc, sh);
  if (threadIdx.x == 0) s[j] = acc;
}

// Product of a one-wave workgroup's 64 values through LDS (32 slots: the upper half of the live lanes parks its values,
// the lower half multiplies them in); the result is valid on thread 0.
__device__ Fq12 block_product(Fq12 f, Fq12* sh) {
  const unsigned t = threadIdx.x;
  for (unsigned s = kLanes / 2; s; s >>= 1) {
    if (t >= s && t < 2 * s) sh[t - s] = f;
    __syncthreads();
    if (t < s) {
      Fq12 g = sh[t];
      f = P::mul12(f, g);
    }
    __syncthreads();
  }
  return f;
}

struct AggKey {             // the key-side pairs: line tables (null = that G2 point is the identity) and -alpha
  const P::Line* gamma;
  const P::Line* delta;
  const P::Line* beta;
  const Affine<Fq>* neg_alpha;
};

// blocks 0 .. ceil(n / 64) - 1: the proofs; the last block: the three key-side pairs.  sums = {ACC, CS} (affine), s[0] = s_0.
__global__ __launch_bounds__(kLanes) void aggregate_miller_kernel(AggKey key, const P::Proof* proofs, size_t n,
                                                                   const Affine<Fq>* ra, const uint8_t* ok,
                                                                   const Affine<Fq>* sums, const Fr* s, Fq12* part) {
  __shared__ Fq12 sh[kLanes / 2];
  Fq12 f = P::one12();
  if (blockIdx.x + 1 < gridDim.x) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i < n && ok[i]) {
      Affine<Fq> a = ra[i];
      Affine<Fq2> b = proofs[i].b;
      f = P::miller(a, b);
    }
  } else if (threadIdx.x < 3) {
    const unsigned t = threadIdx.x;
    const P::Line* table = t == 0 ? key.gamma : t == 1 ? key.delta : key.beta;
    Affine<Fq> p;
    if (t < 2) {
      p = sums[t];
      if (!p.is_inf()) p.y = p.y.neg();
    } else {
      Fr s0 = s[0];
      p = scalar_mul<Fq, Fr::NL>(XYZZ<Fq>::from_affine(*key.neg_alpha), s0.l).to_affine();
    }
    f = P::miller3(Affine<Fq>::inf(), Affine<Fq2>::inf(), p, table, Affine<Fq>::inf(), nullptr);
  }
  f = block_product(f, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = f;
}

__global__ __launch_bounds__(kLanes) void aggregate_product_kernel(const Fq12* in, size_t m, Fq12* out) {
  __shared__ Fq12 sh[kLanes / 2];
  const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
  Fq12 f = P::one12();
  if (i < m) f = in[i];
  f = block_product(f, sh);
  if (threadIdx.x == 0) out[blockIdx.x] = f;
}

__global__ __launch_bounds__(kLanes) void aggregate_decide_kernel(const Fq12* f, const unsigned* bad, uint8_t* accepted) {
  if (threadIdx.x) return;
  uint8_t v = 0;
  if (!*bad) {
    Fq12 g = *f;
    v = P::is_one12(P::final_exp(g)) ? 1 : 0;
  }
  *accepted = v;
}

}  // namespace

template <>
void verify_aggregate_run<DG_CURVE>(Call& k, const VkData& vk, const void* inputs_dev, size_t n_public, bool mont,
                                    const void* proofs_dev, size_t n, const void* coeffs_dev, uint8_t* accepted_dev) {
  const size_t n_ic = n_public + 1;
  const unsigned blocks = (unsigned)((n + kLanes - 1) / kLanes);
  const unsigned slices = (unsigned)std::min<size_t>(kSumSlices, (n + kSumThreads - 1) / kSumThreads);
  // workspace (the MSM's own slots are 4-7, 9, 10, 15-17, 24, 25, 30; the C entry point stages through 0-3)
  uint8_t* small = (uint8_t*)ws(k.c, 8, 2 * sizeof(Affine<Fq>) + n_ic * sizeof(Fr) + 16);
  Affine<Fq>* sums = (Affine<Fq>*)small;
  Fr* s = (Fr*)(small + 2 * sizeof(Affine<Fq>));
  unsigned* bad = (unsigned*)(s + n_ic);
  Affine<Fq>* ra = (Affine<Fq>*)ws(k.c, 11, n * sizeof(Affine<Fq>));
  Affine<Fq>* cs = (Affine<Fq>*)ws(k.c, 12, n * sizeof(Affine<Fq>));
  Fr* rho = (Fr*)ws(k.c, 13, n * sizeof(Fr));
  Fr* rk = (Fr*)ws(k.c, 14, n * sizeof(Fr));
  uint8_t* ok = (uint8_t*)ws(k.c, 18, n);
  Fr* part = (Fr*)ws(k.c, 19, n_ic * slices * sizeof(Fr));
  Fq12* prod[2] = {(Fq12*)ws(k.c, 20, ((size_t)blocks + 1) * sizeof(Fq12)),
                   (Fq12*)ws(k.c, 21, ((size_t)blocks / kLanes + 1) * sizeof(Fq12))};
  const Fr* x = (const Fr*)inputs_dev;
  const P::Proof* proofs = (const P::Proof*)proofs_dev;

  DG_HIP(hipMemsetAsync(bad, 0, sizeof(unsigned), k.s()));
  hipLaunchKernelGGL(aggregate_check_kernel, dim3(blocks), dim3(kLanes), 0, k.s(), x, n_public, mont, proofs,
                     (const uint32_t*)coeffs_dev, n, ra, cs, rho, rk, ok, bad);
  DG_HIP(hipGetLastError());
  hipLaunchKernelGGL(aggregate_colsum_kernel, dim3((unsigned)n_ic, slices), dim3(kSumThreads), 0, k.s(), x, n_public,
                     (const Fr*)rho, (const Fr*)rk, n, part);
  DG_HIP(hipGetLastError());
  hipLaunchKernelGGL(aggregate_colsum_final_kernel, dim3((unsigned)n_ic), dim3(kSumThreads), 0, k.s(), (const Fr*)part,
                     slices, s);
  DG_HIP(hipGetLastError());
  // canonical scalars, bases known to be in the order-r subgroup (the key's were checked at dg16_vk_create, every C_i above)
  msm_launch(k, DG_CURVE, 1, vk.ic, s, n_ic, 2u, true, &sums[0]);
  msm_launch(k, DG_CURVE, 1, cs, rho, n, 2u, true, &sums[1]);
  AggKey key = {(const P::Line*)vk.gamma, (const P::Line*)vk.delta, (const P::Line*)vk.beta,
                (const Affine<Fq>*)vk.neg_alpha};
  hipLaunchKernelGGL(aggregate_miller_kernel, dim3(blocks + 1), dim3(kLanes), 0, k.s(), key, proofs, n,
                     (const Affine<Fq>*)ra, (const uint8_t*)ok, (const Affine<Fq>*)sums, (const Fr*)s, prod[0]);
  DG_HIP(hipGetLastError());
  size_t m = (size_t)blocks + 1;
  int cur = 0;
  while (m > 1) {
    const size_t out = (m + kLanes - 1) / kLanes;
    hipLaunchKernelGGL(aggregate_product_kernel, dim3((unsigned)out), dim3(kLanes), 0, k.s(), (const Fq12*)prod[cur], m,
                       prod[cur ^ 1]);
    DG_HIP(hipGetLastError());
    m = out;
    cur ^= 1;
  }
  hipLaunchKernelGGL(aggregate_decide_kernel, dim3(1), dim3(kLanes), 0, k.s(), (const Fq12*)prod[cur],
                     (const unsigned*)bad, accepted_dev);
  DG_HIP(hipGetLastError());
}

}  // namespace dg16
