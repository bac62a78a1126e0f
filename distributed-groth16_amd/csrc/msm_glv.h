// The plain MSM (dg16_msm): the endomorphisms of the six groups (GlvOf), the scalar splits as kernels, and msm_run, which
// follows msm_geom.h's msm_plain_plan.  Pipeline: msm_impl.h.
#pragma once
#include "glv.h"
#include "glv_endo.h"
#include "msm_finalize.h"

namespace dg16 {

template <class Fr, class GC>
__global__ void __launch_bounds__(256) glv_split_kernel(const Fr* __restrict__ scalars, size_t n, int mont,
                                                         Fr* __restrict__ halves /* [2 n]: |k1| .., then |k2| .. */) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fr s = scalars[i];
  if (mont) s = s.from_mont();
  Fr h1, h2;
  glv::split<GC>(s.l, h1.l, h2.l);
  halves[i] = h1;
  halves[n + i] = h2;
}
template <class Fr, class GC>
__global__ void __launch_bounds__(256) glv_split4_kernel(const Fr* __restrict__ scalars, size_t n, int mont,
                                                          Fr* __restrict__ quarters /* [4 n]: |k0| .., |k1| .., .. */) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fr s = scalars[i];
  if (mont) s = s.from_mont();
  Fr h0, h1, h2, h3;
  glv::split4<GC>(s.l, h0.l, h1.l, h2.l, h3.l);
  quarters[i] = h0;
  quarters[n + i] = h1;
  quarters[2 * n + i] = h2;
  quarters[3 * n + i] = h3;
}
// bases -> internal form, DIM times: P_i at i, its images under the endomorphism at n + i, 2n + i, .. (the identity maps to itself)
template <class F>
__global__ void __launch_bounds__(256) msm_to_internal_glv_kernel(const Affine<F>* __restrict__ in, size_t n,
                                                                   uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int PW = 2 * FieldOf<F>::WORDS;
  Affine<F> p = in[i];
  uint32_t w[PW];
  affine_to_internal(p, w);
  uint4* dst = reinterpret_cast<uint4*>(out + i * PW);
#pragma unroll
  for (int k = 0; k < PW / 4; k++) dst[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
#pragma unroll 1
  for (int img = 1; img < GlvOf<F>::DIM; img++) {
    GlvOf<F>::endo(p);
    affine_to_internal(p, w);
    dst = reinterpret_cast<uint4*>(out + ((size_t)img * n + i) * PW);
#pragma unroll
    for (int k = 0; k < PW / 4; k++) dst[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
  }
}

// mode: bit 0 = scalars in Montgomery form, bit 1 = every base is in the order-r subgroup (ctx.h: msm_mode)
template <class F, class Fr, int SCALAR_BITS>
void msm_run(Call& k, const void* bases, const void* scalars, size_t n, unsigned mode, bool out_affine,
             void* out_dev) {
  const bool scalars_mont = mode & 1u;
  if constexpr (GlvOf<F>::enabled) {
    // Split every scalar with the curve's endomorphism where msm_plain_plan (msm_geom.h) says so.  Same number of bucket
    // entries (2n points x half the windows), half the windows: half the dependent doublings of the Horner tail, half the
    // bucket sets to reduce, twice the entries per bucket (longer, better balanced accumulation segments).
    constexpr size_t DIM = GlvOf<F>::DIM;
    const PlainPlan plan = msm_plain_plan(RR<typename FieldOf<F>::Params>::N == 9, (unsigned)DIM, n,
                                          GlvCofactorOne<F>::value || (mode & 2u));
    if (plan.split) {
      using GC = typename GlvOf<F>::C;
      Fr* halves = (Fr*)ws(k.c, 30, DIM * n * sizeof(Fr));
      MsmSort st;
      if constexpr (DIM == 2) {
        hipLaunchKernelGGL((glv_split_kernel<Fr, GC>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, k.s(),
                           (const Fr*)scalars, n, (int)scalars_mont, halves);
        st = msm_sort<Fr, kGlvBits>(k, halves, 2 * n, 2u, false, plan.c_small);     // (= plan.scalar_bits)
      } else {
        hipLaunchKernelGGL((glv_split4_kernel<Fr, GC>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, k.s(),
                           (const Fr*)scalars, n, (int)scalars_mont, halves);
        st = msm_sort<Fr, kGlv4Bits>(k, halves, 4 * n, 2u, false);                  // (= plan.scalar_bits)
      }
      uint32_t* internal = (uint32_t*)ws(k.c, 24, DIM * n * sizeof(Affine<F>));
      hipLaunchKernelGGL(msm_to_internal_glv_kernel<F>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, k.s(),
                         (const Affine<F>*)bases, n, internal);
      msm_reduce<F>(k, st, internal, out_affine, out_dev);
      return;
    }
  }
  MsmSort st = msm_sort<Fr, SCALAR_BITS>(k, scalars, n, scalars_mont ? 1u : 0u, false);
  uint32_t* internal = (uint32_t*)ws(k.c, 24, (n ? n : 1) * sizeof(Affine<F>));
  if (n)
    hipLaunchKernelGGL(msm_to_internal_kernel<F>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, k.s(),
                       (const Affine<F>*)bases, n, internal);
  // (ONE accumulation launch, then the reduction chain: the two-launch pipeline that overlapped the upper windows' chain with
  // the lower windows' accumulation was slower -- CHANGELOG.md round 4, profiles/r4e_msm_pipeline_ab.md)
  msm_reduce<F>(k, st, internal, out_affine, out_dev);
}

}  // namespace dg16
