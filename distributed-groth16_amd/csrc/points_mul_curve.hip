// Per-curve object of the batched point multiplication (points_mul.h): points_mul_kernel for G1 and G2 of curve DG_CURVE,
// and -- for the curves that have a prepared verifying key (BN254, BLS12-381) -- the two kernels around the products of
// dg16_groth16_rerandomize.
//
//   rr_prepare_kernel   per proof: checks 1 <= r1, r2 < r, writes the four multipliers 1/r1 | r2 | r1 | r1 r2 as plain
//                       integers (one Fr inversion, one Fr product) and gathers A (twice) and B into point arrays
//   products            2n G1 products (r1^-1 A, r2 A) and n G2 products (r1 B) through points_mul_typed, split path (a
//                       proof's points are in the subgroups by the call's contract); the n multiples r1 r2 delta of the
//                       FIXED point delta_g2 through the fixed-base machinery (fixed_base_impl.h: no doublings)
//   rr_combine_kernel   per proof: B' = r1 B + r1 r2 delta, C' = C + r2 A (one mixed addition and one inversion each),
//                       or three identities where the check failed
#include "points_mul.h"
#include "setup.h"

#ifndef DG_CURVE
#error "compile with -DDG_CURVE=<curve id>"
#endif

namespace dg16 {
namespace {

using CT = CurveTypes<DG_CURVE>;
using Fr = CT::Fr;
using Fq = CT::Fq;
using Fq2 = CT::Fq2;

#if DG_CURVE < 2
using Proof = pmul::RrProof<Fq, Fq2>;

__global__ void __launch_bounds__(64) rr_prepare_kernel(const Proof* proofs, const Fr* __restrict__ r1_r2, size_t n,
                                                         int mont, Fr* __restrict__ mult, Affine<Fq>* __restrict__ g1,
                                                         Affine<Fq2>* __restrict__ g2, uint8_t* __restrict__ ok) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fr r1 = fb_load(r1_r2 + 2 * i), r2 = fb_load(r1_r2 + 2 * i + 1);
  const bool good = pmul::rr_scalar_ok(r1) && pmul::rr_scalar_ok(r2);
  Fr m[4] = {Fr::zero(), Fr::zero(), Fr::zero(), Fr::zero()};
  if (good) pmul::rr_scalars(r1, r2, mont != 0, &m[0], &m[1], &m[2], &m[3]);
#pragma unroll
  for (int j = 0; j < 4; j++) fb_store(mult + (size_t)j * n + i, m[j]);
  const Affine<Fq> a = fb_load(&proofs[i].a);
  fb_store(g1 + i, a);
  fb_store(g1 + n + i, a);
  fb_store(g2 + i, fb_load(&proofs[i].b));
  ok[i] = good ? 1 : 0;
}

__global__ void __launch_bounds__(64) rr_combine_kernel(const Proof* proofs, size_t n, const Affine<Fq>* __restrict__ g1,
                                                         const Affine<Fq2>* __restrict__ g2,
                                                         const Affine<Fq2>* __restrict__ dl,
                                                         const uint8_t* __restrict__ ok, Proof* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Affine<Fq> c = fb_load(&proofs[i].c);       // read before the write below: out may be proofs
  const Proof o = pmul::rr_combine<Fq, Fq2>(ok[i] != 0, fb_load(g1 + i), fb_load(g1 + n + i), c, fb_load(g2 + i),
                                            fb_load(dl + i));
  fb_store(out + i, o);
}
#endif

}  // namespace

template <>
void points_mul_run<DG_CURVE>(Call& k, int group, const void* points_dev, const void* scalars_dev, size_t n,
                              unsigned mode, void* out_dev) {
  if (group == 1) pmul::points_mul_typed<Fq, Fr>(k, points_dev, scalars_dev, n, mode, out_dev);
  else pmul::points_mul_typed<Fq2, Fr>(k, points_dev, scalars_dev, n, mode, out_dev);
}

#if DG_CURVE < 2
// Workspace slots of the channel: 4 (multipliers), 5 (G1 points / products), 6 (G2), 7 (delta's multiples), 8 (flags),
// besides those of points_mul_typed and fixed_base_typed.
template <>
void rerandomize_run<DG_CURVE>(Call& k, const VkData& vk, const void* proofs_dev, size_t n, const void* r1_r2_dev,
                               bool mont, void* out_dev) {
  if (!n) return;
  Fr* mult = (Fr*)ws(k.c, 4, 4 * n * sizeof(Fr));
  Affine<Fq>* g1 = (Affine<Fq>*)ws(k.c, 5, 2 * n * sizeof(Affine<Fq>));
  Affine<Fq2>* g2 = (Affine<Fq2>*)ws(k.c, 6, n * sizeof(Affine<Fq2>));
  Affine<Fq2>* dl = (Affine<Fq2>*)ws(k.c, 7, n * sizeof(Affine<Fq2>));
  uint8_t* ok = (uint8_t*)ws(k.c, 8, n);
  const dim3 grid((unsigned)((n + 63) / 64)), block(64);
  hipLaunchKernelGGL(rr_prepare_kernel, grid, block, 0, k.s(), (const Proof*)proofs_dev, (const Fr*)r1_r2_dev, n,
                     (int)mont, mult, g1, g2, ok);
  DG_HIP(hipGetLastError());
  pmul::points_mul_typed<Fq, Fr>(k, g1, mult, 2 * n, 2u, g1);                // r1^-1 A | r2 A
  pmul::points_mul_typed<Fq2, Fr>(k, g2, mult + 2 * n, n, 2u, g2);           // r1 B
  fixed_base_run<DG_CURVE>(k, 2, vk.delta_point, mult + 3 * n, n, false, dl); // r1 r2 delta
  hipLaunchKernelGGL(rr_combine_kernel, grid, block, 0, k.s(), (const Proof*)proofs_dev, n, (const Affine<Fq>*)g1,
                     (const Affine<Fq2>*)g2, (const Affine<Fq2>*)dl, (const uint8_t*)ok, (Proof*)out_dev);
  DG_HIP(hipGetLastError());
}
#endif

}  // namespace dg16
