// Resident bases: the table of window multiples (msm_table_kernel, msm_build_table) and the synthetic bases of the
// benchmarks and tests (gen_*, to_affine_kernel).  Pipeline: msm_impl.h.
#pragma once
#include "ctx.h"
#include "ec.h"
#include "ec29.h"
#include "msm_geom.h"
#include "types.h"

namespace dg16 {

// ---- table of window multiples for resident bases: T[r*n + i] = 2^(c_step*r) * P_i (affine), r < rows -----------
// (c_step = c * stride: a full table has stride 1 and one row per window; a thinned one keeps every stride-th row;
// kMaxTableWin and the stride under an HBM budget, table_stride_for: msm_geom.h)
template <class F>
__global__ void __launch_bounds__(64) msm_table_kernel(const Affine<F>* __restrict__ bases, size_t n, unsigned c,
                                                        unsigned nwin, Affine<F>* __restrict__ table) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Affine<F> p = bases[i];
  // rows are stored in the accumulation kernels' internal form (same size; see msm_to_internal_kernel)
  auto put = [&](size_t at, const Affine<F>& v) { affine_to_internal(v, reinterpret_cast<uint32_t*>(table + at)); };
  put(i, p);
  if (p.is_inf()) {
    for (unsigned w = 1; w < nwin; w++) put((size_t)w * n + i, p);
    return;
  }
  // rows 1..nwin-1 by repeated doubling; one shared inversion (Montgomery's trick over the rows)
  XYZZ<F> pts[kMaxTableWin];
  F pref[kMaxTableWin];
  XYZZ<F> cur = XYZZ<F>::from_affine(p);
  F run = F::one();
  for (unsigned w = 1; w < nwin; w++) {
    for (unsigned j = 0; j < c; j++) cur = cur.dbl();
    pts[w] = cur;
    pref[w] = run;
    // a point of odd prime order never doubles to the identity; tolerate small-order inputs anyway
    run = run * (cur.is_inf() ? F::one() : cur.zzz);
  }
  F inv = run.inv();
  for (unsigned w = nwin - 1; w >= 1; w--) {
    if (pts[w].is_inf()) { put((size_t)w * n + i, Affine<F>::inf()); continue; }
    F zi3 = inv * pref[w];
    inv = inv * pts[w].zzz;
    F zi2 = (zi3 * pts[w].zz).sqr();
    put((size_t)w * n + i, Affine<F>{pts[w].x * zi2, pts[w].y * zi3});
  }
}

// returns a device table of nwin*n affine points (caller owns it) for window size c
template <class F>
void* msm_build_table(hipStream_t s, const void* bases, size_t n, unsigned c, unsigned nwin) {
  DG_REQUIRE(nwin <= kMaxTableWin, DG16_ERR_BAD_ARG, "too many table windows");
  void* t = nullptr;
  DG_HIP(hipMalloc(&t, (size_t)nwin * (n ? n : 1) * sizeof(Affine<F>)));
  if (n)
    hipLaunchKernelGGL(msm_table_kernel<F>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, (const Affine<F>*)bases, n,
                       c, nwin, (Affine<F>*)t);
  DG_HIP(hipGetLastError());
  return t;
}

// ---- synthetic bases: P_i = (k0 + i*k1) * G -----------------------------------------------------------
constexpr unsigned kGenChunk = 64;

template <class F, class C>
__global__ void gen_setup_kernel(const uint32_t* k1_words, Affine<F>* d_out) {
  Affine<F> G = GenLoader<F, C>::get();
  XYZZ<F> d = scalar_mul<F, 4>(XYZZ<F>::from_affine(G), k1_words);
  *d_out = d.to_affine();
}

template <class F, class C>
__global__ void __launch_bounds__(64) gen_bases_kernel(const uint32_t* k0_words, const uint32_t* k1_words,
                                                        const Affine<F>* d_ptr, size_t n, Affine<F>* out) {
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t lo = t * kGenChunk;
  if (lo >= n) return;
  size_t hi = lo + kGenChunk < n ? lo + kGenChunk : n;
  // k = k0 + lo * k1  (128-bit * 64-bit + 128-bit  <  2^193)
  uint32_t kk[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  {
    uint32_t lo_w[2] = {(uint32_t)lo, (uint32_t)((uint64_t)lo >> 32)};
    uint64_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 2; j++) {
        uint64_t pr = (uint64_t)k1_words[i] * lo_w[j];
        acc[i + j] += (uint32_t)pr;
        acc[i + j + 1] += pr >> 32;
      }
    for (int i = 0; i < 4; i++) acc[i] += k0_words[i];
    uint64_t carry = 0;
    for (int i = 0; i < 8; i++) {
      uint64_t v = acc[i] + carry;
      kk[i] = (uint32_t)v;
      carry = v >> 32;
    }
  }
  Affine<F> G = GenLoader<F, C>::get();
  Affine<F> D = *d_ptr;
  XYZZ<F> cur = scalar_mul<F, 7>(XYZZ<F>::from_affine(G), kk);
  // walk the chunk; batch-invert zzz with Montgomery's trick (scratch arrays live in private memory)
  XYZZ<F> pts[kGenChunk];
  F pref[kGenChunk];
  F run = F::one();
  size_t cnt = hi - lo;
  for (size_t i = 0; i < cnt; i++) {
    pts[i] = cur;
    pref[i] = run;
    run = run * cur.zzz;
    cur = cur.madd(D, false);
  }
  F inv = run.inv();
  for (size_t i = cnt; i-- > 0;) {
    F zi3 = inv * pref[i];          // 1 / zzz_i
    inv = inv * pts[i].zzz;
    F zi2 = (zi3 * pts[i].zz).sqr();
    out[lo + i] = {pts[i].x * zi2, pts[i].y * zi3};
  }
}

template <class F, class C>
void gen_bases_run(Call& k, uint64_t seed, size_t n, void* out_dev);

template <class F>
__global__ void __launch_bounds__(64) to_affine_kernel(const Jacobian<F>* __restrict__ in, Affine<F>* __restrict__ out,
                                                        size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = XYZZ<F>::from_jacobian(in[i]).to_affine();
}

inline uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ULL;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
  return x ^ (x >> 31);
}

template <class F, class C>
void gen_bases_run(Call& k, uint64_t seed, size_t n, void* out_dev) {
  // same (k0, k1) derivation as the checker uses, so generated bases can be compared bit for bit
  uint64_t k0[2] = {splitmix64(seed ^ 0xA5A5), splitmix64(seed ^ 0x5A5A)};
  uint64_t k1[2] = {splitmix64(seed ^ 0x1234) | 1, splitmix64(seed ^ 0x4321)};
  uint32_t host_words[8] = {(uint32_t)k0[0], (uint32_t)(k0[0] >> 32), (uint32_t)k0[1], (uint32_t)(k0[1] >> 32),
                            (uint32_t)k1[0], (uint32_t)(k1[0] >> 32), (uint32_t)k1[1], (uint32_t)(k1[1] >> 32)};
  uint8_t* scratch = (uint8_t*)ws(k.c, 16, 64 + sizeof(Affine<F>));
  uint32_t* words = (uint32_t*)scratch;
  Affine<F>* d = (Affine<F>*)(scratch + 64);
  DG_HIP(hipMemcpyAsync(words, host_words, sizeof host_words, hipMemcpyHostToDevice, k.s()));
  DG_HIP(hipStreamSynchronize(k.s()));   // host_words is a stack buffer
  hipLaunchKernelGGL((gen_setup_kernel<F, C>), dim3(1), dim3(1), 0, k.s(), words + 4, d);
  size_t threads = (n + kGenChunk - 1) / kGenChunk;
  hipLaunchKernelGGL((gen_bases_kernel<F, C>), dim3((unsigned)((threads + 63) / 64)), dim3(64), 0, k.s(), words,
                     words + 4, d, n, (Affine<F>*)out_dev);
  DG_HIP(hipGetLastError());
}

template <class F>
void to_affine_run(Call& k, const void* jac, void* out, size_t n) {
  hipLaunchKernelGGL(to_affine_kernel<F>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, k.s(),
                     (const Jacobian<F>*)jac, (Affine<F>*)out, n);
  DG_HIP(hipGetLastError());
}

}  // namespace dg16
