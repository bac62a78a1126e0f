// MSM phase 4, the kernels: segment accumulation in registers with the in-workgroup bucket tree (msm_accumulate_kernel)
// and with the accumulator staged through LDS (msm_accumulate_lds_kernel); the step-loop form of the 14-limb G2 groups is
// in msm_accumulate_steps.h, the launch side in msm_accumulate_phase.h.  Pipeline: msm_impl.h.
#pragma once
#include "bounds.h"
#include "ec29.h"
#include "msm_geom.h"
#include "types.h"

namespace dg16 {

// The shader clock UNDER a kernel, measured by the kernel (round 6): s_memtime ticks once per shader cycle, s_memrealtime at
// a constant 100 MHz (MI355X_MICROARCH.md); lane 0 of every workgroup adds its two deltas to clk[0], clk[1] (two atomics per
// workgroup, outside every loop), so clk[0] / clk[1] x 100 MHz is the duration-weighted clock the chip held while the
// kernel ran.  bench.py prices the accumulations against 16 lanes x 4 SIMDs x CUs x THAT clock (dg16_last_kernel_ms,
// which = 2) next to the calibrated issue rate -- a cycle-based utilisation that does not move with DVFS.  clk may be null.
struct ClkProbe {
  unsigned long long c0 = 0, w0 = 0;
  __device__ __forceinline__ void begin(const unsigned long long* clk) {
    if (clk && threadIdx.x == 0) { c0 = __builtin_readcyclecounter(); w0 = wall_clock64(); }
  }
  __device__ __forceinline__ void end(unsigned long long* clk) const {
    if (clk && threadIdx.x == 0) {
      atomicAdd(&clk[0], (unsigned long long)__builtin_readcyclecounter() - c0);
      atomicAdd(&clk[1], (unsigned long long)wall_clock64() - w0);
    }
  }
};

// ---- 4: segment accumulation -------------------------------------------------------------------
// Bases arrive in the library's INTERNAL form (msm_to_internal_kernel / msm_table_kernel): x || y, each coordinate
// x R mod p of the reduced-radix representation (fp29.h) packed into the arkworks word count, identity = zeros.
// The mixed additions run on 29/28-bit limbs with lazy bounds (ec29.h: 162 v_mad_u64_u32 per Fq product and no
// carry or compare instructions, against 128 mad + 128 addc + ~70 others for the 32-bit product); segment sums stay
// in that representation for the bucket reduction below.
template <class F>
__device__ __forceinline__ Affine29<F> load_internal(const uint32_t* __restrict__ bases, unsigned idx) {
  constexpr int PW = 2 * FieldOf<F>::WORDS;               // words per point
  uint32_t w[PW];
  const uint4* src = reinterpret_cast<const uint4*>(bases + (size_t)idx * PW);
#pragma unroll
  for (int i = 0; i < PW / 4; i++) {
    const uint4 v = src[i];
    w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
  }
  return Affine29<F>::load(w);
}

// The same load in two halves -- the raw packed words now, the limbs when the addition needs them -- for a loop that
// keeps the NEXT point's words in registers while it adds the current one (msm_accumulate_lds_kernel).
template <class F>
struct RawPoint {
  uint4 v[2 * FieldOf<F>::WORDS / 4];
};
template <class F>
__device__ __forceinline__ RawPoint<F> load_raw(const uint32_t* __restrict__ bases, unsigned idx) {
  constexpr int PW = 2 * FieldOf<F>::WORDS;
  RawPoint<F> r;
  const uint4* src = reinterpret_cast<const uint4*>(bases + (size_t)idx * PW);
#pragma unroll
  for (int i = 0; i < PW / 4; i++) r.v[i] = src[i];
  return r;
}
template <class F>
__device__ __forceinline__ Affine29<F> unpack_raw(const RawPoint<F>& r) {
  constexpr int PW = 2 * FieldOf<F>::WORDS;
  uint32_t w[PW];
#pragma unroll
  for (int i = 0; i < PW / 4; i++) {
    w[4 * i] = r.v[i].x; w[4 * i + 1] = r.v[i].y; w[4 * i + 2] = r.v[i].z; w[4 * i + 3] = r.v[i].w;
  }
  return Affine29<F>::load(w);
}

// Segment t of bucket-window w -> its bucket and its range of the bucket's entries.  seg_off is the exclusive scan of
// the per-bucket segment counts k_b = ceil(cnt_b / 2^seg_log): the bucket is the LAST b with seg_off[b] <= t (empty
// buckets share their offset with their successor and are skipped by construction); segment j of k covers the ranks
// [j cnt / k, (j + 1) cnt / k).
struct SegRange {
  size_t bslot;        // (w << log_nb) + bucket
  unsigned first, cnt; // rank of the segment's first entry inside the bucket, entries in the segment
  unsigned j, k;       // this is segment j of the bucket's k
};
__device__ __forceinline__ SegRange msm_segment(const MsmGeom& g, unsigned w, unsigned t,
                                                const unsigned* __restrict__ counts,
                                                const unsigned* __restrict__ seg_off) {
  const unsigned* so = seg_off + ((size_t)w << g.log_nb);
  unsigned lo = 0, hi = 1u << g.log_nb;          // invariant: so[lo] <= t, (hi == nb or so[hi] > t)
  while (hi - lo > 1) {
    const unsigned mid = (lo + hi) >> 1;
    if (so[mid] <= t) lo = mid; else hi = mid;
  }
  SegRange r;
  r.bslot = DG_IDX(1, ((size_t)w << g.log_nb) + lo, (size_t)g.bw << g.log_nb);
  const unsigned c = counts[r.bslot];
  const unsigned k = (c + (1u << g.seg_log) - 1) >> g.seg_log;
  const unsigned j = t - so[lo];
  r.first = (unsigned)(((uint64_t)j * c) / k);
  r.cnt = (unsigned)(((uint64_t)(j + 1) * c) / k) - r.first;
  r.j = j;
  r.k = k;
  return r;
}

// ---- in-workgroup bucket tree ---------------------------------------------------------------------------------
// The lanes of an accumulation workgroup hold the partial sums of CONSECUTIVE segments, i.e. runs of lanes belong to
// one bucket (~15 lanes per bucket of a 2^20-point table MSM).  Instead of writing one partial per segment and
// summing them in a separate, latency-bound finalize launch (a million full additions per MSM, 3 ms for G2 inside a
// proof), the workgroup adds the partials of every run in a tree, in place, in LDS columns ([coordinate word][lane]).
// The additions of a round are COMPACTED onto the low lanes (ballot + prefix counts), so whole waves drop out:
// 128 + 64 + 32 + 16 additions of a 256-lane workgroup are 2 + 1 + 1 + 1 wave-level additions, ~12 % on top of the
// 4 x 16 mixed additions of the accumulation itself.  A run that covers its whole bucket writes the BUCKET; a bucket
// that crosses a workgroup boundary leaves one partial per workgroup in the segment-sum array, at the slot of the
// run's first lane -- the bucket's first segment slot, then the first slot of every further workgroup:
__device__ __forceinline__ unsigned msm_nparts(unsigned first_slot, unsigned k, unsigned wg_log) {
  return k ? ((first_slot + k - 1) >> wg_log) - (first_slot >> wg_log) + 1 : 0;
}
__device__ __forceinline__ unsigned msm_part_slot(unsigned first_slot, unsigned s, unsigned wg_log) {
  return s ? ((first_slot >> wg_log) + s) << wg_log : first_slot;
}
template <class F, int BLOCK>
struct ColAcc {       // one lane's XYZZ29 in the LDS columns
  using S = typename FieldOf<F>::Store;
  static constexpr int WORDS = sizeof(S) / 4;
  uint32_t (*sh)[BLOCK];
  unsigned lane;
  __device__ __forceinline__ S get(int coord) const {
    S v;
    uint32_t* w = reinterpret_cast<uint32_t*>(&v);
#pragma unroll
    for (int i = 0; i < WORDS; i++) w[i] = sh[coord * WORDS + i][lane];
    return v;
  }
  __device__ __forceinline__ void put(int coord, const S& v) const {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(&v);
#pragma unroll
    for (int i = 0; i < WORDS; i++) sh[coord * WORDS + i][lane] = w[i];
  }
};
template <class F, int BLOCK>
__device__ __forceinline__ void wg_tree_add(uint32_t (*sh)[BLOCK], unsigned a, unsigned b) {
  XYZZ29<F>::add_acc(ColAcc<F, BLOCK>{sh, a}, ColAcc<F, BLOCK>{sh, a}, ColAcc<F, BLOCK>{sh, b});
}
// q: my index inside my run, el: end (exclusive, a lane index) of my run; lanes outside every run pass q = 0, el = lane + 1
template <class F, int BLOCK>
__device__ __forceinline__ void wg_bucket_tree(uint32_t (*sh)[BLOCK], unsigned short* list, unsigned* wcnt,
                                                         unsigned lane, unsigned q, unsigned el) {
  constexpr unsigned NW = BLOCK / 64;
  if (lane == 0) wcnt[NW] = 0;
  __syncthreads();
  atomicMax(&wcnt[NW], el - (lane - q));
  __syncthreads();
  const unsigned maxlen = wcnt[NW];
#pragma unroll 1
  for (unsigned d = 1; d < maxlen; d <<= 1) {
    const bool act = (q & (2 * d - 1)) == 0 && lane + d < el;
    const unsigned long long m = __ballot(act);
    const unsigned wv = lane >> 6;
    if ((lane & 63) == 0) wcnt[wv] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned base = 0, total = 0;
#pragma unroll
    for (unsigned i = 0; i < NW; i++) {
      const unsigned c = wcnt[i];
      base += i < wv ? c : 0u;
      total += c;
    }
    if (act) list[base + (unsigned)__popcll(m & ((1ull << (lane & 63)) - 1))] = (unsigned short)lane;
    __syncthreads();
    if (lane < total) {
      const unsigned a = list[lane];
      wg_tree_add<F, BLOCK>(sh, a, (unsigned)DG_IDX(16, a + d, BLOCK));
    }
    __syncthreads();
  }
}

// Several MSMs over the SAME scalars (the A, B1 and L queries of a proof share one digit sort) run as INSTANCES of one
// launch: blockIdx.y = inst * bw + w; the sort's arrays are indexed by the bucket-window w, everything an instance
// owns (segment sums, buckets, rows, window sums) by wy = blockIdx.y.  One launch = one ramp-down at the end instead
// of three, and the bucket reduction behind it is ONE chain of launches for all instances.
constexpr unsigned kMaxInst = 4;
struct MsmBases {
  const uint32_t* p[kMaxInst];
};
template <class F>
constexpr bool msm_acc_tree();
// log2 of the accumulation workgroup of coordinate field F (msm_accumulate_phase)
template <class F>
constexpr unsigned msm_acc_block_log() {
  if constexpr (sizeof(F) > 48) return sizeof(typename FieldOf<F>::Store) * 4 * 256 <= 80 * 1024 ? 8u : 7u;
  else if constexpr (!msm_acc_tree<F>()) return 8u;
  else return sizeof(typename FieldOf<F>::Store) * 4 * 256 <= 40 * 1024 ? 8u : 7u;   // G1: four workgroups' trees per CU
}
// Does the accumulation kernel of F add the partials of a bucket inside the workgroup (wg_bucket_tree)?  Coordinate fields
// up to this size do: the G1 of BN254.  G2 (the tree's Fq2 addition next to a loop at its register limit) and the 48-byte
// G1 fields were measured with it and are slower (CHANGELOG.md: rounds 3-4, profiles/r4d_ab.md): there every lane writes its
// partial and a throughput finalize adds the ~15 of a bucket.
#ifndef DG16_TREE_MAX_BYTES
#define DG16_TREE_MAX_BYTES 32
#endif
template <class F>
constexpr bool msm_acc_tree() {
  return sizeof(F) <= DG16_TREE_MAX_BYTES;
}
// log2 of the span of segment slots that share ONE partial (msm_part_slot): the workgroup with the tree, one slot without
template <class F>
constexpr unsigned msm_acc_wg_log() { return msm_acc_tree<F>() ? msm_acc_block_log<F>() : 0u; }

// Waves per SIMD the accumulation of a 48-byte coordinate field is compiled for: 2 = up to 256 VGPRs (the loop with the
// fused Y3 takes 178, no scratch).  Three (168 VGPRs) needs the unfused Y3 and was 4 % slower (fp29.h: rr_fuse_mul_sub).
#ifndef DG16_ACC48_WAVES
#define DG16_ACC48_WAVES 2
#endif
// (waves per SIMD = 4 caps the kernel at 128 VGPRs: the loop needs 108; what the tree's full addition needs beyond
// that is spilled INSIDE the tree, which a workgroup runs five times, not inside the loop it runs 16 x 4 times)
template <class F, int BLOCK>
__global__ void __launch_bounds__(BLOCK, (sizeof(F) > 32 ? DG16_ACC48_WAVES : 4))
msm_accumulate_kernel(MsmBases bases, size_t n,
                                                              MsmGeom g, const unsigned* __restrict__ offsets,
                                                              const unsigned* __restrict__ counts,
                                                              const unsigned* __restrict__ seg_off,
                                                              const unsigned* __restrict__ seg_total,
                                                              const unsigned* __restrict__ entries,
                                                              XYZZ29<F>* __restrict__ seg_sum,
                                                              XYZZ29<F>* __restrict__ buckets,
                                                              unsigned long long* __restrict__ clk) {
  ClkProbe probe;
  probe.begin(clk);
  const unsigned w = blockIdx.y % g.bw;
  const uint32_t* __restrict__ base_tab = bases.p[blockIdx.y / g.bw];
  const unsigned lane = threadIdx.x;
  const unsigned t = blockIdx.x * BLOCK + lane;
  const bool live = t < seg_total[w];
  SegRange sr{};
  XYZZ29<F> acc = XYZZ29<F>::inf();
  if (live) {
    sr = msm_segment(g, w, t, counts, seg_off);
    const unsigned cnt = DG_OK(2, (size_t)offsets[sr.bslot] + sr.first + sr.cnt, g.region + 1) ? sr.cnt : 0u;
    const unsigned* e = entries + (size_t)w * g.region + offsets[sr.bslot] + sr.first;
    // Latency hiding: several waves per SIMD cover the dependent (entry -> point) gathers; only the 4-byte entry
    // index is fetched one iteration ahead (a second point in registers costs the whole 128-register budget of four
    // waves and six scratch accesses per iteration: measured equal, profiles/r4b_ab_variants.md -- removed).
    unsigned cur = e[0];
    for (unsigned j = 0; j < cnt; j++) {
      unsigned nxt = (j + 1 < cnt) ? e[j + 1] : 0u;
      const Affine29<F> p = load_internal<F>(base_tab, DG_IDX(3, cur & 0x7fffffffu, g.region));
      acc = acc.madd(p, cur >> 31);
      cur = nxt;
    }
  }
  const size_t bucket_slot = ((size_t)blockIdx.y << g.log_nb) + (sr.bslot & (((size_t)1 << g.log_nb) - 1));
  if constexpr (msm_acc_tree<F>()) {
    using CA = ColAcc<F, BLOCK>;
    __shared__ uint32_t sh[4 * CA::WORDS][BLOCK];           // the partials of the bucket tree: 36 KiB for a 254-bit field
    __shared__ unsigned short list[BLOCK];
    __shared__ unsigned wcnt[BLOCK / 64 + 1];
    const CA me{sh, lane};
    me.put(0, acc.x); me.put(1, acc.y); me.put(2, acc.zz); me.put(3, acc.zzz);
    // my run: the lanes of this workgroup that hold segments of my bucket
    const unsigned hl = live ? (lane > sr.j ? lane - sr.j : 0u) : lane;
    const unsigned el = live ? (lane - sr.j + sr.k < (unsigned)BLOCK ? lane + sr.k - sr.j : (unsigned)BLOCK) : lane + 1;
    wg_bucket_tree<F, BLOCK>(sh, list, wcnt, lane, lane - hl, el);
    if (live && lane == hl) {
      const XYZZ29<F> v{me.get(0), me.get(1), me.get(2), me.get(3)};
      if (sr.j == 0 && lane + sr.k <= (unsigned)BLOCK) buckets[DG_IDX(5, bucket_slot, (size_t)gridDim.y << g.log_nb)] = v;   // the whole bucket
      else seg_sum[(size_t)blockIdx.y * g.seg_cap + DG_IDX(4, t, g.seg_cap)] = v;      // one partial per (bucket, workgroup): msm_part_slot
    }
  } else if (live) {
    if (sr.k == 1) buckets[DG_IDX(5, bucket_slot, (size_t)gridDim.y << g.log_nb)] = acc;   // a one-segment bucket needs no finalize
    else seg_sum[(size_t)blockIdx.y * g.seg_cap + DG_IDX(4, t, g.seg_cap)] = acc;
  }
  probe.end(clk);
}

// ---- 4 (G2): the same segment accumulation with the accumulator staged through LDS -------------------------
// An Fq2 mixed addition with its four accumulator coordinates in registers needs more than 256 VGPRs (one wave per
// SIMD, AGPR spills); with the coordinates in LDS between uses (layout [coordinate word][lane]: consecutive lanes ->
// consecutive banks, conflict-free ds_read/write_b32) the live set is the loaded point and ~6 temporaries.
// 4 coordinates x 2 N words x BLOCK lanes = 72 KiB for BN254 Fq2 at BLOCK = 256 (two workgroups per CU, 160 KiB LDS).
// (9-limb Fq2 -- BN254 -- only: the 14-limb curves run msm_accumulate_steps_kernel below)
template <class F, int BLOCK, int TU = 0>
__global__ void __launch_bounds__(BLOCK, (BLOCK == 256 ? 2 : 1))
msm_accumulate_lds_kernel(MsmBases bases, size_t n, MsmGeom g,
                          const unsigned* __restrict__ offsets, const unsigned* __restrict__ counts,
                          const unsigned* __restrict__ seg_off, const unsigned* __restrict__ seg_total,
                          const unsigned* __restrict__ entries, XYZZ29<F>* __restrict__ seg_sum,
                          XYZZ29<F>* __restrict__ buckets, unsigned long long* __restrict__ clk) {
  using FO = FieldOf<F>;
  using S = typename FO::Store;
  constexpr int BS = FO::BS;
  constexpr int WORDS = sizeof(S) / 4;
  __shared__ uint32_t sh[4 * WORDS][BLOCK];
  ClkProbe probe;
  probe.begin(clk);
  const unsigned lane = threadIdx.x;
  auto ld = [&](int coord) {
    S v;
    uint32_t* w = reinterpret_cast<uint32_t*>(&v);
#pragma unroll
    for (int i = 0; i < WORDS; i++) w[i] = sh[coord * WORDS + i][lane];
    return v;
  };
  auto st = [&](int coord, const S& v) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(&v);
#pragma unroll
    for (int i = 0; i < WORDS; i++) sh[coord * WORDS + i][lane] = w[i];
  };
#define DG_STAGE() asm volatile("" ::: "memory")   /* keep LDS reloads where they are written */
  const unsigned w = blockIdx.y % g.bw;
  const uint32_t* __restrict__ base_tab = bases.p[blockIdx.y / g.bw];
  const unsigned t = blockIdx.x * BLOCK + threadIdx.x;
  const bool live = t < seg_total[w];
  SegRange sr{};
  if (live) sr = msm_segment(g, w, t, counts, seg_off);
  const unsigned cnt = live && DG_OK(2, (size_t)offsets[sr.bslot] + sr.first + sr.cnt, g.region + 1) ? sr.cnt : 0u;
  const unsigned* e = entries + (size_t)w * g.region + (live ? offsets[sr.bslot] + sr.first : 0u);
  bool inf = true;
  // Gather latency.  This kernel runs two waves per SIMD (LDS-bound) with registers to spare (175 of 256 for BN254), so
  // for 64-byte coordinates the NEXT point's 32 packed words are gathered while the current addition runs (its entry
  // index was fetched an iteration earlier, the index after it is fetched now): the dependent entry -> point load no
  // longer sits in front of every addition.  An index past the segment is 0 (a valid row).  48-byte-field Fq2 (252
  // registers, one wave) has no room for it and loads at the top of the iteration as before.
  // Measured against the plain loop in round 4 (profiles/r4a_ab_variants.md): 2.871-2.883 ms per launch against
  // 2.877-2.909, same box, same call -- inside the noise, ahead on both passes: kept, the build switch is gone.
  constexpr bool PREFETCH = sizeof(F) <= 64;
  unsigned cur = cnt ? e[0] : 0u;
  unsigned nxt = cnt > 1 ? e[1] : 0u;
  RawPoint<F> raw_cur{};
  if (PREFETCH && cnt) raw_cur = load_raw<F>(base_tab, DG_IDX(3, cur & 0x7fffffffu, g.region));
  for (unsigned j = 0; j < cnt; j++) {
    const unsigned nn = (j + 2 < cnt) ? e[j + 2] : 0u;
    RawPoint<F> raw_nxt{};
    if (PREFETCH) raw_nxt = load_raw<F>(base_tab, DG_IDX(3, nxt & 0x7fffffffu, g.region));
    else raw_cur = load_raw<F>(base_tab, DG_IDX(3, cur & 0x7fffffffu, g.region));
    const Affine29<F> q = unpack_raw<F>(raw_cur);
    const bool negate = cur >> 31;
    cur = nxt;
    nxt = nn;
    if (PREFETCH) raw_cur = raw_nxt;
    if (q.is_inf()) continue;
    const auto nqy = neg(q.y);
    const auto qy = select(negate, nqy, q.y.template as<decltype(nqy)::Bound, decltype(nqy)::Limb>());
    if (inf) {
      st(0, q.x.template as<BS, 1>()); st(1, fit<BS>(qy)); st(2, FO::one()); st(3, FO::one());
      inf = false;
      continue;
    }
    const auto p_ = norm(q.x * ld(2) - ld(0));          // U2 - X1
    DG_STAGE();
    const auto r_ = norm(qy * ld(3) - ld(1));           // S2 - Y1
    DG_STAGE();
    if (is_zero(p_)) {
      if (is_zero(r_)) {
        const XYZZ29<F> d = XYZZ29<F>::dbl_affine(q.x, qy);
        st(0, d.x); st(1, d.y); st(2, d.zz); st(3, d.zzz);
        if constexpr (HasOrderTwoPoint<F>::value) inf = d.is_inf();     // (ec29.h) twice the point of order two
      } else {
        inf = true;
      }
      continue;
    }
    const auto pp = sqr(p_);
    const auto ppp = p_ * pp;
    DG_STAGE();
    st(2, fit<BS>(ld(2) * pp));
    DG_STAGE();
    st(3, fit<BS>(ld(3) * ppp));
    DG_STAGE();
    const auto q_ = ld(0) * pp;
    DG_STAGE();
    const auto x3 = fit<BS>(sqr(r_) - (ppp + dbl(q_)));
    st(0, x3);
    DG_STAGE();
    const auto y3 = fit<BS>(mul_sub(r_, q_ - x3, ppp, ld(1)));
    st(1, y3);
    DG_STAGE();
  }
  if (live) {
    // (no in-workgroup tree here: msm_acc_tree) one partial per segment; a one-segment bucket is written directly
    XYZZ29<F> out = XYZZ29<F>::inf();
    if (!inf) out = XYZZ29<F>{ld(0), ld(1), ld(2), ld(3)};
    if (sr.k == 1) buckets[((size_t)blockIdx.y << g.log_nb) + (sr.bslot & (((size_t)1 << g.log_nb) - 1))] = out;
    else seg_sum[(size_t)blockIdx.y * g.seg_cap + DG_IDX(4, t, g.seg_cap)] = out;
  }
  probe.end(clk);
#undef DG_STAGE
}

// arkworks-form bases (C ABI) -> internal form for the accumulation kernels (plain dg16_msm: one pass per call,
// 2 field products per point against ~10 W in the accumulation; resident keys convert once, in the table builder)
template <class F>
__global__ void __launch_bounds__(256) msm_to_internal_kernel(const Affine<F>* __restrict__ in, size_t n,
                                                               uint32_t* __restrict__ out) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int PW = 2 * FieldOf<F>::WORDS;
  uint32_t w[PW];
  affine_to_internal(in[i], w);
  uint4* dst = reinterpret_cast<uint4*>(out + i * PW);
#pragma unroll
  for (int k = 0; k < PW / 4; k++) dst[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}

}  // namespace dg16
