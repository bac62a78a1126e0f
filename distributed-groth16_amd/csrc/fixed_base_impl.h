// Fixed-base batch scalar multiplication out[i] = k_i * B (dg16_fixed_base_mul) -- what FixedBase::get_window_table +
// FixedBase::msm do inside ark-groth16's generator (reached from circuit_specific_setup, groth16/examples/sha256.rs:137).
//
//   table    T[w][d - 1] = d * 2^(c w) * B, d = 1 .. 2^(c-1), w < nwin = ceil((bits + 1) / c), affine, built per call:
//            one lane per window doubles B up to 2^(c w) B (fb_window_bases_kernel), then one lane per run of
//            kFbChunk consecutive multiples walks them by mixed additions and converts the run to affine with ONE
//            inversion (fb_table_kernel; the walk and Montgomery's trick of gen_bases_kernel, msm_table.h).
//   multiply one lane per output point: the scalar is recoded into signed c-bit digits d_w in [-2^(c-1), 2^(c-1)]
//            (k = sum d_w 2^(c w); nwin c >= bits + 1 leaves room for the last carry), and the lane adds
//            T[w][|d_w| - 1] (negated for d_w < 0) into an XYZZ accumulator: nwin mixed additions, NO doublings.
//   affine   a second kernel converts a batch of accumulators: lane t owns the points t, t + T, t + 2 T, ... (coalesced
//            across the lanes), multiplies their ZZZ forward, inverts once, and walks back (Montgomery's trick).
//
// Completeness.  The table entries and the accumulator are multiples of the same point, so equal and opposite operands
// ARE reachable: k = 2^(c w) + 2^(c w') style digits cannot collide (different windows hold different multiples), but
// k = r - 1 with signed digits, a base outside the order-r subgroup, or the identity as base make the running sum meet
// T[w][d] or its negative, or pass through the identity.  The loop therefore uses the complete XYZZ::madd of ec.h
// (identity accumulator, identity addend, P + P -> doubling, P - P -> identity are all branches of it); nothing is
// proven away.  The table build guards its batched inversion against identity entries for the same reason.
#pragma once
#include "ctx.h"
#include "types.h"

namespace dg16 {

constexpr unsigned kFbMinC = 4, kFbMaxC = 16;
constexpr unsigned kFbChunk = 32;          // consecutive multiples per lane of the table build (one inversion each)
constexpr size_t kFbBatch = (size_t)1 << 18;   // points per multiply / affine launch pair (bounds the XYZZ workspace)

// Window width from the number of scalars.  Work per call ~ n * nwin additions for the points + ~3 * nwin * 2^(c-1)
// addition-equivalents for the table (walk + shared inversion), minimised near c = log2(n) - 3; capped at 16, where
// the table (2^15 entries x 16-17 windows: 32 MB for BN254 G1, 100 MB for BLS12 G2) still sits in the 256 MB
// last-level cache of the chip while 2^20 lanes gather from it.
inline unsigned fixed_base_window_bits(size_t n) {
  unsigned lg = 0;
  while (lg < 63 && ((size_t)2 << lg) <= n) lg++;      // floor(log2 n), 0 for n <= 1
  unsigned c = lg > 3 ? lg - 3 : 0;
  return c < kFbMinC ? kFbMinC : c > kFbMaxC ? kFbMaxC : c;
}

// 16-byte vector loads / stores of a point (Fp is alignas(16); entries are 64 .. 192 bytes)
template <class T>
__device__ __forceinline__ T fb_load(const T* p) {
  static_assert(sizeof(T) % 16 == 0, "point size");
  T v;
  const uint4* s = reinterpret_cast<const uint4*>(p);
  uint4* d = reinterpret_cast<uint4*>(&v);
#pragma unroll
  for (unsigned i = 0; i < sizeof(T) / 16; i++) d[i] = s[i];
  return v;
}
template <class T>
__device__ __forceinline__ void fb_store(T* p, const T& v) {
  const uint4* s = reinterpret_cast<const uint4*>(&v);
  uint4* d = reinterpret_cast<uint4*>(p);
#pragma unroll
  for (unsigned i = 0; i < sizeof(T) / 16; i++) d[i] = s[i];
}

// wb[w] = 2^(c w) * base (affine), one lane per window
template <class F, class C>
__global__ void __launch_bounds__(64) fb_window_bases_kernel(const Affine<F>* __restrict__ base, int use_generator,
                                                              unsigned c, unsigned nwin, Affine<F>* __restrict__ wb) {
  unsigned w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nwin) return;
  Affine<F> b = use_generator ? GenLoader<F, C>::get() : *base;
  XYZZ<F> cur = XYZZ<F>::from_affine(b);
#pragma unroll 1
  for (unsigned j = 0; j < c * w; j++) cur = cur.dbl();
  wb[w] = cur.to_affine();
}

// table[w * half + lo .. lo + kFbChunk) = (lo + 1 .. lo + kFbChunk) * wb[w], half = 2^(c-1)
template <class F>
__global__ void __launch_bounds__(64) fb_table_kernel(const Affine<F>* __restrict__ wb, unsigned c, unsigned nwin,
                                                       Affine<F>* __restrict__ table) {
  const size_t half = (size_t)1 << (c - 1);
  const size_t chunks = (half + kFbChunk - 1) / kFbChunk;
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= chunks * nwin) return;
  const unsigned w = (unsigned)(t / chunks);
  const size_t lo = (t % chunks) * kFbChunk;
  const size_t cnt = lo + kFbChunk <= half ? kFbChunk : half - lo;
  const Affine<F> B = wb[w];
  const uint32_t first = (uint32_t)(lo + 1);
  XYZZ<F> cur = lo == 0 ? XYZZ<F>::from_affine(B) : scalar_mul<F, 1>(XYZZ<F>::from_affine(B), &first);
  XYZZ<F> pts[kFbChunk];
  F pref[kFbChunk];
  F run = F::one();
#pragma unroll 1
  for (size_t i = 0; i < cnt; i++) {
    pts[i] = cur;
    pref[i] = run;
    if (!cur.is_inf()) run = run * cur.zzz;     // (a base of small order, or the identity, reaches the identity)
    cur = cur.madd(B, false);
  }
  F inv = run.inv();
  Affine<F>* dst = table + (size_t)w * half + lo;
#pragma unroll 1
  for (size_t i = cnt; i-- > 0;) {
    if (pts[i].is_inf()) { fb_store(dst + i, Affine<F>::inf()); continue; }
    F zi3 = inv * pref[i];          // 1 / zzz_i
    inv = inv * pts[i].zzz;
    F zi2 = (zi3 * pts[i].zz).sqr();
    fb_store(dst + i, Affine<F>{pts[i].x * zi2, pts[i].y * zi3});
  }
}

// acc[i] = scalars[i] * base, i < n (n <= kFbBatch per launch), as XYZZ
template <class F, class Fr>
__global__ void __launch_bounds__(64) fb_mul_kernel(const Affine<F>* __restrict__ table, const Fr* __restrict__ scalars,
                                                     size_t n, int mont, unsigned c, unsigned nwin,
                                                     XYZZ<F>* __restrict__ acc_out) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fr k = fb_load(scalars + i);
  if (mont) k = k.from_mont();
  const size_t half = (size_t)1 << (c - 1);
  const uint32_t mask = (1u << c) - 1;
  XYZZ<F> acc = XYZZ<F>::inf();
  uint32_t carry = 0;
#pragma unroll 1
  for (unsigned w = 0; w < nwin; w++) {
    // c <= 16 bits at bit position c * w of the little-endian 32-bit limbs (bits beyond the scalar read as zero)
    const unsigned bit = c * w, li = bit >> 5, sh = bit & 31;
    uint64_t two = li < (unsigned)Fr::NL ? k.l[li] : 0u;
    if (li + 1 < (unsigned)Fr::NL) two |= (uint64_t)k.l[li + 1] << 32;
    uint32_t d = ((uint32_t)(two >> sh) & mask) + carry;
    const bool negd = d > half;
    carry = negd ? 1u : 0u;
    if (negd) d = (1u << c) - d;       // digit d - 2^c < 0: add the negated |digit|-th multiple, carry one up
    if (d == 0) continue;              // d <= half: the index below stays inside the window's row
    const Affine<F> q = fb_load(table + (size_t)w * half + (d - 1));
    acc = acc.madd(q, negd);
  }
  fb_store(acc_out + i, acc);
}

// out[i] = affine(acc[i]); lane t owns i = t + j * lanes, j < per_lane
template <class F>
__global__ void __launch_bounds__(64) fb_affine_kernel(const XYZZ<F>* __restrict__ acc, F* __restrict__ pref, size_t n,
                                                        size_t lanes, unsigned per_lane, Affine<F>* __restrict__ out) {
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= lanes) return;
  F run = F::one();
#pragma unroll 1
  for (unsigned j = 0; j < per_lane; j++) {
    const size_t i = t + (size_t)j * lanes;
    if (i >= n) break;
    fb_store(pref + i, run);
    const F zzz = fb_load(&acc[i].zzz);
    if (!zzz.is_zero()) run = run * zzz;
  }
  F inv = run.inv();
#pragma unroll 1
  for (unsigned j = per_lane; j-- > 0;) {
    const size_t i = t + (size_t)j * lanes;
    if (i >= n) continue;
    const XYZZ<F> p = fb_load(acc + i);
    if (p.is_inf()) { fb_store(out + i, Affine<F>::inf()); continue; }
    F zi3 = inv * fb_load(pref + i);
    inv = inv * p.zzz;
    F zi2 = (zi3 * p.zz).sqr();
    fb_store(out + i, Affine<F>{p.x * zi2, p.y * zi3});
  }
}

// out[i] = affine(acc[i]), i < cnt, on the call's stream; pref: cnt elements of scratch.  One inversion per lane: 32
// points per lane once there are enough lanes (2^13) to fill the chip without it
template <class F>
void fb_to_affine(Call& k, const XYZZ<F>* acc, F* pref, size_t cnt, Affine<F>* out) {
  unsigned per_lane = (unsigned)(cnt >> 13);
  per_lane = per_lane < 1 ? 1 : per_lane > 32 ? 32 : per_lane;
  const size_t lanes = (cnt + per_lane - 1) / per_lane;
  hipLaunchKernelGGL(fb_affine_kernel<F>, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, k.s(), acc, pref, cnt, lanes,
                     per_lane, out);
  DG_HIP(hipGetLastError());
}

// scalars_dev, out_dev: device pointers; base_host: one affine point on the host or NULL for the standard generator.
// Workspace slots of the channel: 3 (base + window bases), 12 (table), 13 (accumulators), 14 (prefix products).
template <class F, class C, class Fr, int BITS>
void fixed_base_typed(Call& k, const void* base_host, const void* scalars_dev, size_t n, bool mont, void* out_dev) {
  if (!n) return;
  const unsigned c = fixed_base_window_bits(n);
  const unsigned nwin = (BITS + 1 + c - 1) / c;
  const size_t half = (size_t)1 << (c - 1);
  Affine<F>* wb = (Affine<F>*)ws(k.c, 3, (nwin + 1) * sizeof(Affine<F>));
  Affine<F>* base_dev = wb + nwin;
  if (base_host) {
    DG_HIP(hipMemcpyAsync(base_dev, base_host, sizeof(Affine<F>), hipMemcpyHostToDevice, k.s()));
    DG_HIP(hipStreamSynchronize(k.s()));    // the caller may free the base on return
  }
  Affine<F>* table = (Affine<F>*)ws(k.c, 12, (size_t)nwin * half * sizeof(Affine<F>));
  hipLaunchKernelGGL((fb_window_bases_kernel<F, C>), dim3((nwin + 63) / 64), dim3(64), 0, k.s(), base_dev,
                     base_host ? 0 : 1, c, nwin, wb);
  const size_t tthreads = ((half + kFbChunk - 1) / kFbChunk) * nwin;
  hipLaunchKernelGGL(fb_table_kernel<F>, dim3((unsigned)((tthreads + 63) / 64)), dim3(64), 0, k.s(), wb, c, nwin, table);
  const size_t batch = n < kFbBatch ? n : kFbBatch;
  XYZZ<F>* acc = (XYZZ<F>*)ws(k.c, 13, batch * sizeof(XYZZ<F>));
  F* pref = (F*)ws(k.c, 14, batch * sizeof(F));
  k.begin_dominant();
  for (size_t lo = 0; lo < n; lo += kFbBatch) {
    const size_t cnt = n - lo < kFbBatch ? n - lo : kFbBatch;
    hipLaunchKernelGGL((fb_mul_kernel<F, Fr>), dim3((unsigned)((cnt + 63) / 64)), dim3(64), 0, k.s(), table,
                       (const Fr*)scalars_dev + lo, cnt, (int)mont, c, nwin, acc);
    DG_HIP(hipGetLastError());
    fb_to_affine(k, acc, pref, cnt, (Affine<F>*)out_dev + lo);
  }
  k.end_dominant();
}

}  // namespace dg16
