// MSM phase 4b: bucket = sum of the partials the accumulation left (throughput, wave-per-bucket and LDS forms, the stitch
// behind the in-workgroup tree, empty buckets), the giant work list, and msm_reduce = accumulate + bucket phase.
// Pipeline: msm_impl.h.
#pragma once
#include "lane29.h"
#include "msm_accumulate_phase.h"

namespace dg16 {

// ---- 4b: bucket = sum of its segment partials, as a throughput kernel -------------------------------------------
// Giant buckets (a boolean witness puts half of ALL entries into bucket 0; the short top window of a c that does
// not divide the scalar width does the same) go on a device-side work list: stage 1 cuts the bucket's segment
// partials into <= kGiantSlices slices, one workgroup each; stage 2 adds the slice sums (msm_reduce_impl.h; the slices:
// giant_geometry, msm_geom.h).
// A giant bucket (np > kGiantSegs partials) goes on the device-side work list: giant[0] = giants, giant[1] = work items,
// giant_list[0 .. giant_cap) = bucket ids, giant_list[giant_cap .. 3 giant_cap) = (id slot << 6 | slice) items.  Both
// capacities hold by construction (msm_buffers asserts the arithmetic; MSM_INVARIANTS.md): the giants of a launch own
// disjoint sets of > kGiantSegs of its <= nseg_slots partials, so there are < nseg_slots / kGiantSegs + 1 = giant_cap of
// them, and their slices number sum ceil(np / per) <= sum (np / kGiantSliceSegs + 1) < nseg_slots / kGiantSliceSegs +
// giant_cap <= 2 giant_cap.  The guards below keep a violated invariant from writing outside the list anyway.
__device__ __forceinline__ void msm_register_giant(unsigned gid, unsigned np, unsigned* __restrict__ giant_count,
                                                   unsigned* __restrict__ giant_list, unsigned giant_cap) {
  const unsigned slot = atomicAdd(giant_count, 1u);
  if (!DG_OK(8, slot, giant_cap) || slot >= giant_cap) return;
  giant_list[slot] = gid;
  unsigned slices, per;
  giant_geometry(np, slices, per);
  const unsigned wb = atomicAdd(giant_count + 1, slices);   // work items: (giant, slice)
  if (!DG_OK(9, (size_t)wb + slices, 2 * (size_t)giant_cap + 1) || (size_t)wb + slices > 2 * (size_t)giant_cap) return;
  unsigned* work = giant_list + giant_cap;
  for (unsigned i = 0; i < slices; i++) work[wb + i] = (slot << 6) | i;
}


// What is left of the finalize after the in-workgroup bucket tree: one lane per bucket adds the partials of the
// buckets that CROSS an accumulation workgroup (one bucket in ~17 for a 2^20 table MSM: one addition; a bucket held
// by one workgroup was written by it, an empty one is set to the identity here).  (Round 2 / early round 3 summed
// ~15 per-segment partials per bucket here, a million full additions per MSM at 5-18x the issue time of an
// addition: profiles/r3_finalize_experiments.md.)
// TU: 0 = instantiated in msm_group.hip (products inline), 1 = in msm_reduce.hip (for G2 compiled with out-of-line
// products, DG29_OUTLINE_MUL: an inlined Fq2 addition + doubling is 123 KB of code for BN254 and 250 KB for BLS12-381,
// against the 64 KB instruction cache two CUs share -- a BLS12-381 2^20 proof took 38 ms instead of 26 with it).
// Distinct symbols, so that both variants can live in one library.
// `total` = (instances * bw) << log_nb buckets; the sort's arrays are indexed by the bucket-window w = wy % bw.
template <class F, int TU = 0>
__global__ void __launch_bounds__(256) msm_finalize_thr_kernel(MsmGeom g, size_t total, unsigned wg_log,
                                                                const unsigned* __restrict__ counts,
                                                                const unsigned* __restrict__ seg_off,
                                                                const XYZZ29<F>* __restrict__ seg_sum,
                                                                XYZZ29<F>* __restrict__ buckets,
                                                                unsigned* __restrict__ giant_count,
                                                                unsigned* __restrict__ giant_list, unsigned giant_cap) {
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= total) return;
  const unsigned wy = (unsigned)(gid >> g.log_nb);
  const size_t gs = ((size_t)(wy % g.bw) << g.log_nb) + (gid & (((size_t)1 << g.log_nb) - 1));   // the sort's bucket slot
  const unsigned k = (counts[gs] + (1u << g.seg_log) - 1) >> g.seg_log;
  const unsigned first = seg_off[gs];
  const unsigned np = msm_nparts(first, k, wg_log);     // partials the accumulation workgroups left for this bucket
  if (np == 0) {
    buckets[gid] = XYZZ29<F>::inf();
    return;
  }
  if (np == 1) return;                                  // one workgroup held the whole bucket and wrote it
  if (np > kGiantSegs) {
    msm_register_giant((unsigned)gid, np, giant_count, giant_list, giant_cap);
    return;
  }
  const XYZZ29<F>* sp = seg_sum + (size_t)wy * g.seg_cap;
  XYZZ29<F> acc = sp[DG_IDX(7, first, g.seg_cap)];
#pragma unroll 1
  for (unsigned s = 1; s < np; s++) acc = acc.add(sp[DG_IDX(7, msm_part_slot(first, s, wg_log), g.seg_cap)]);
  buckets[gid] = acc;
}
// The same sums with a WAVE per bucket in lane form (lane29.h), for the launches where the lone-lane form above is at its
// worst: a 14-limb G1 addition inlined is ~60 KB of code against the 64-KB instruction cache two CUs share, and the
// serial loop above ran at ~125 us per dependent addition -- 0.89 ms of a 1.5-ms plain MSM at 2^13 BLS12-377 points,
// 0.92 of 1.97 at 2^16 (profiles/r6kk_timeline_bls12_377_g1_2e13.md).  A wave per bucket costs ~8x the issue slots of a lane
// per bucket, so this form takes the launches with at most kLaneFinalizeMaxPartials partial sums in all.
constexpr size_t kLaneFinalizeMaxPartials = (size_t)1 << 18;
template <class F>
__global__ void __launch_bounds__(64) msm_finalize_lane_kernel(MsmGeom g, unsigned wg_log,
                                                                const unsigned* __restrict__ counts,
                                                                const unsigned* __restrict__ seg_off,
                                                                const XYZZ29<F>* __restrict__ seg_sum,
                                                                XYZZ29<F>* __restrict__ buckets,
                                                                unsigned* __restrict__ giant_count,
                                                                unsigned* __restrict__ giant_list, unsigned giant_cap) {
  if constexpr (lane29::enabled<F>()) {
    using FO = lane29::Ops<F>;
    using LPt = lane29::Pt<FO>;
    const size_t gid = blockIdx.x;                       // one wave per bucket: everything below is uniform across it
    const unsigned wy = (unsigned)(gid >> g.log_nb);
    const size_t gs = ((size_t)(wy % g.bw) << g.log_nb) + (gid & (((size_t)1 << g.log_nb) - 1));
    const unsigned k = (counts[gs] + (1u << g.seg_log) - 1) >> g.seg_log;
    const unsigned first = seg_off[gs];
    const unsigned np = msm_nparts(first, k, wg_log);
    if (np == 0) {
      if (threadIdx.x == 0) buckets[gid] = XYZZ29<F>::inf();
      return;
    }
    if (np == 1) return;
    if (np > kGiantSegs) {
      if (threadIdx.x == 0) msm_register_giant((unsigned)gid, np, giant_count, giant_list, giant_cap);
      return;
    }
    typename FO::KT kc;
    kc.init();
    const XYZZ29<F>* sp = seg_sum + (size_t)wy * g.seg_cap;
    LPt acc = lane29::load_pt<F>(kc, &sp[DG_IDX(7, first, g.seg_cap)]);
    LPt nx = lane29::load_pt_words<F>(kc, &sp[DG_IDX(7, msm_part_slot(first, 1, wg_log), g.seg_cap)]);
#pragma unroll 1
    for (unsigned s = 1; s < np; s++) {
      const LPt cur = lane29::with_inf_flag<FO>(nx);
      if (s + 1 < np) nx = lane29::load_pt_words<F>(kc, &sp[DG_IDX(7, msm_part_slot(first, s + 1, wg_log), g.seg_cap)]);
      acc = lane29::add_pt<FO>(kc, acc, cur);
    }
    lane29::store_pt<F>(kc, &buckets[gid], acc);
  }
}
// The same finalize as a THROUGHPUT kernel (G2): LPB lanes per bucket, each summing its share of the bucket's partials
// into an accumulator that lives in LDS columns between the products (the layout and register budget of
// msm_accumulate_lds_kernel: two workgroups per CU, ~175 VGPRs), then a log2(LPB)-step tree over neighbouring columns.
// A 2^20-point table MSM is one round of 2 waves per SIMD with 8 + 1 additions per lane; runs on the accumulation's own
// stream, right behind it (msm_accumulate_phase).  ONE addition site: the serial partials (global memory) and the tree
// partners (LDS columns) go through the same accessor, told apart at run time -- one site per operand kind was 227 KB of
// code against the 64-KB instruction cache (CHANGELOG.md, round 4).
template <class F, int BLOCK>
struct PartialAcc {      // an XYZZ29 behind the accessor interface of XYZZ29::add_into: memory if p, else LDS column
  using S = typename FieldOf<F>::Store;
  const XYZZ29<F>* p;
  ColAcc<F, BLOCK> col;
  __device__ __forceinline__ S get(int coord) const {
    if (p) return coord == 0 ? p->x : coord == 1 ? p->y : coord == 2 ? p->zz : p->zzz;
    return col.get(coord);
  }
  // the pointer as a value the compiler cannot trace (xyzz_add_into_steps: keeps address arithmetic inside the step)
  __device__ __forceinline__ void launder() { asm volatile("" : "+v"(p)); }
};
template <class F, int BLOCK>
__global__ void __launch_bounds__(BLOCK, (BLOCK == 256 ? 2 : 1))
msm_finalize_lds_kernel(MsmGeom g, size_t total, unsigned wg_log, unsigned lpb_log,
                        const unsigned* __restrict__ counts,
                        const unsigned* __restrict__ seg_off, const XYZZ29<F>* __restrict__ seg_sum,
                        XYZZ29<F>* __restrict__ buckets, unsigned* __restrict__ giant_count,
                        unsigned* __restrict__ giant_list, unsigned giant_cap) {
  using FO = FieldOf<F>;
  constexpr int WORDS = sizeof(typename FO::Store) / 4;
  __shared__ uint32_t sh[4 * WORDS][BLOCK];
  __shared__ unsigned max_serial;
  if constexpr (sizeof(F) > 64) asm volatile("" ::: DG_ACC_FILE_CLOBBERS);   // xyzz_add_into_steps' temporaries (acc_set / acc_get)
  const unsigned LPB = 1u << lpb_log;
  const unsigned lane = threadIdx.x, sub = lane & (LPB - 1);
  const size_t gid = ((size_t)blockIdx.x * BLOCK + lane) >> lpb_log;
  const ColAcc<F, BLOCK> me{sh, lane};
  unsigned np = 0, first = 0;
  unsigned wy = 0;
  if (lane == 0) max_serial = 0;
  if (gid < total) {
    wy = (unsigned)(gid >> g.log_nb);
    const size_t gs = DG_IDX(6, ((size_t)(wy % g.bw) << g.log_nb) + (gid & (((size_t)1 << g.log_nb) - 1)), (size_t)g.bw << g.log_nb);
    const unsigned k = (counts[gs] + (1u << g.seg_log) - 1) >> g.seg_log;
    first = seg_off[gs];
    np = msm_nparts(first, k, wg_log);
    if (sub == 0) {
      if (np == 0) buckets[gid] = XYZZ29<F>::inf();
      if (np > kGiantSegs) msm_register_giant((unsigned)gid, np, giant_count, giant_list, giant_cap);
    }
  }
  const bool work = np >= 2 && np <= kGiantSegs;      // np == 1: the accumulation wrote the bucket itself
  const XYZZ29<F>* sp = seg_sum + (size_t)wy * g.seg_cap;
  const unsigned lo = work ? (unsigned)(((uint64_t)sub * np) >> lpb_log) : 0u;
  const unsigned hi = work ? (unsigned)(((uint64_t)(sub + 1) * np) >> lpb_log) : 0u;
  if (lo < hi) {
    const XYZZ29<F>* q = &sp[DG_IDX(7, msm_part_slot(first, lo, wg_log), g.seg_cap)];
    me.put(0, q->x); me.put(1, q->y); me.put(2, q->zz); me.put(3, q->zzz);
  } else {
    me.put(2, FO::zero());                              // the identity for add_into: zz = 0
  }
  const unsigned nser = lo < hi ? hi - lo - 1 : 0u;     // this lane's serial additions
  __syncthreads();
  atomicMax(&max_serial, nser);
  __syncthreads();
  const unsigned ms = max_serial;
  // steps 0 .. ms - 1: my share of the bucket's partials, one after another; then lpb_log tree steps over
  // neighbouring columns (behind a barrier each)
#pragma unroll 1
  for (unsigned step = 0; step < ms + lpb_log; step++) {
    const bool tree = step >= ms;
    if (tree) __syncthreads();
    const unsigned d = tree ? 1u << (step - ms) : 0u;
    const bool on = tree ? (work && (sub & (2 * d - 1)) == 0) : step < nser;
    if (on) {
      const PartialAcc<F, BLOCK> b{tree ? nullptr : &sp[DG_IDX(7, msm_part_slot(first, lo + 1 + step, wg_log), g.seg_cap)],
                                   ColAcc<F, BLOCK>{sh, (unsigned)DG_IDX(10, lane + d, BLOCK)}};
      // 14-limb Fq2: the addition as a step loop over the accumulation's three product sites (35 900 -> 22 700
      // instructions; 21.8 -> 21.5 ms per BLS12-381 2^20 proof, same call, twice: profiles/r6b_finalize_steps_ab.txt).
      // Withdrawn in round 5 behind an HSA aperture violation, back in round 6 with its cause removed: hipcc had put
      // sixteen of its own spills into the temporaries' register file (kAccFileBase).
      if constexpr (sizeof(F) > 64) xyzz_add_into_steps<F>(me, b);
      else XYZZ29<F>::add_into(me, b);
    }
  }
  if (work && sub == 0) {
    XYZZ29<F> out = XYZZ29<F>::inf();
    if (!limbs_all_zero(me.get(2))) out = XYZZ29<F>{me.get(0), me.get(1), me.get(2), me.get(3)};
    buckets[gid] = out;
  }
}
// G2 finalize as a throughput kernel behind the accumulation, two lanes per bucket (measured in round 4 against one and
// four lanes and against the one-lane-per-bucket kernel on the reduction stream: profiles/r4r_finalize_lpb_ab.txt,
// r3b_finalize_lds_ab.txt -- the switches are gone)
inline int msm_finalize_lds_lpb() { return 2; }
template <class F>
void msm_finalize_lds_phase(hipStream_t s, const MsmSort& st, const MsmBuffers<F>& b) {
  constexpr int BLOCK = 1 << msm_acc_block_log<F>();
  const int lpb = msm_finalize_lds_lpb();
  const unsigned lpb_log = lpb == 4 ? 2u : lpb == 2 ? 1u : 0u;
  DG_HIP(hipMemsetAsync(b.giant, 0, 8, s));
  const unsigned blocks = (unsigned)((b.nbw * (size_t)lpb + BLOCK - 1) / BLOCK);
  hipLaunchKernelGGL((msm_finalize_lds_kernel<F, BLOCK>), dim3(blocks), dim3(BLOCK), 0, s, st.g, b.nbw,
                     msm_acc_wg_log<F>(), lpb_log, st.counts, st.seg_off, b.seg_sum, b.buckets, b.giant, b.giant + 2,
                     b.giant_cap);
}

// With the in-workgroup tree the finalize shrinks to a STITCH: one lane per accumulation-workgroup BOUNDARY (a few
// thousand lanes, not one per bucket) looks at the bucket that straddles it and, if this is the first boundary that
// bucket crosses, adds the partials its workgroups left.  Buckets held by one workgroup were written by it, empty ones
// are zeroed by msm_empty_buckets_kernel (all-zero limbs ARE the identity: zz = 0).  A 65 536-lane finalize with nothing
// to do still took 0.2-0.5 ms inside a proof, waiting for wave slots next to the accumulation.
template <class F, int TU = 0>
__global__ void __launch_bounds__(256) msm_stitch_kernel(MsmGeom g, unsigned wg_log, const unsigned* __restrict__ counts,
                                                          const unsigned* __restrict__ seg_off,
                                                          const unsigned* __restrict__ seg_total,
                                                          const XYZZ29<F>* __restrict__ seg_sum,
                                                          XYZZ29<F>* __restrict__ buckets,
                                                          unsigned* __restrict__ giant_count,
                                                          unsigned* __restrict__ giant_list, unsigned giant_cap) {
  const unsigned wy = blockIdx.y, w = wy % g.bw;
  const unsigned bd = blockIdx.x * blockDim.x + threadIdx.x + 1;      // boundary between workgroups bd - 1 and bd
  const unsigned slot = bd << wg_log;
  if (slot >= seg_total[w]) return;
  const unsigned* so = seg_off + ((size_t)w << g.log_nb);
  unsigned lo = 0, hi = 1u << g.log_nb;                                 // the bucket whose segments contain `slot`
  while (hi - lo > 1) {
    const unsigned mid = (lo + hi) >> 1;
    if (so[mid] <= slot) lo = mid; else hi = mid;
  }
  const unsigned first = so[lo];
  if (first == slot || (first >> wg_log) != bd - 1) return;             // starts here, or crossed an earlier boundary
  const size_t gs = ((size_t)w << g.log_nb) + lo;
  const size_t gid = ((size_t)wy << g.log_nb) + lo;
  const unsigned k = (counts[gs] + (1u << g.seg_log) - 1) >> g.seg_log;
  const unsigned np = msm_nparts(first, k, wg_log);
  if (np > kGiantSegs) {
    msm_register_giant((unsigned)gid, np, giant_count, giant_list, giant_cap);
    return;
  }
  const XYZZ29<F>* sp = seg_sum + (size_t)wy * g.seg_cap;
  XYZZ29<F> acc = sp[DG_IDX(7, first, g.seg_cap)];
#pragma unroll 1
  for (unsigned s = 1; s < np; s++) acc = acc.add(sp[DG_IDX(7, msm_part_slot(first, s, wg_log), g.seg_cap)]);
  buckets[gid] = acc;
}
// ... and the empty buckets are set to the identity by a kernel of a dozen registers per lane (it fits next to any
// accumulation wave; a memset on the main stream in front of the accumulation cost a launch boundary per MSM: +0.2 ms
// per proof, measured)
template <class F>
__global__ void __launch_bounds__(256) msm_empty_buckets_kernel(MsmGeom g, size_t total, const unsigned* __restrict__ counts,
                                                                 XYZZ29<F>* __restrict__ buckets) {
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= total) return;
  const unsigned wy = (unsigned)(gid >> g.log_nb);
  const size_t gs = ((size_t)(wy % g.bw) << g.log_nb) + (gid & (((size_t)1 << g.log_nb) - 1));
  if (counts[gs]) return;
  uint4* dst = reinterpret_cast<uint4*>(buckets + gid);
  static_assert(sizeof(XYZZ29<F>) % 16 == 0, "vector stores");
#pragma unroll
  for (unsigned i = 0; i < sizeof(XYZZ29<F>) / 16; i++) dst[i] = make_uint4(0u, 0u, 0u, 0u);   // zz = 0: the identity
}
template <class F>
void msm_finalize_phase(hipStream_t s, const MsmSort& st, const MsmBuffers<F>& b) {
  DG_BOUNDS_BIND();
  if constexpr (msm_acc_tree<F>()) {
    hipLaunchKernelGGL(msm_empty_buckets_kernel<F>, dim3((unsigned)((b.nbw + 255) / 256)), dim3(256), 0, s, st.g, b.nbw,
                       st.counts, b.buckets);
    const unsigned nbd = (st.g.seg_cap >> msm_acc_wg_log<F>()) + 1;
    hipLaunchKernelGGL(msm_stitch_kernel<F>, dim3((nbd + 255) / 256, st.g.bw * b.ninst), dim3(256), 0, s, st.g,
                       msm_acc_wg_log<F>(), st.counts, st.seg_off, st.seg_total, b.seg_sum, b.buckets, b.giant,
                       b.giant + 2, b.giant_cap);
  } else {
    bool lane = false;
    if constexpr (lane29::enabled<F>()) {
      static const bool off = [] { const char* e = getenv("DG16_NO_LANE_FINALIZE"); return e && atoi(e) != 0; }();
      const size_t partials = ((st.g.region * st.g.bw * b.ninst) >> st.g.seg_log) + b.nbw;      // (an upper bound)
      lane = !off && !b.busy_chip && partials <= kLaneFinalizeMaxPartials && b.nbw < ((size_t)1 << 31);
    }
    if (lane)
      hipLaunchKernelGGL(msm_finalize_lane_kernel<F>, dim3((unsigned)b.nbw), dim3(64), 0, s, st.g, msm_acc_wg_log<F>(),
                         st.counts, st.seg_off, b.seg_sum, b.buckets, b.giant, b.giant + 2, b.giant_cap);
    else
      hipLaunchKernelGGL(msm_finalize_thr_kernel<F>, dim3((unsigned)((b.nbw + 255) / 256)), dim3(256), 0, s, st.g, b.nbw,
                         msm_acc_wg_log<F>(), st.counts, st.seg_off, b.seg_sum, b.buckets, b.giant, b.giant + 2,
                         b.giant_cap);
  }
  DG_HIP(hipGetLastError());
}

// Phase B (latency-bound, few waves): finalize -> giants -> rows -> top -> tail.  May run on another stream than
// phase A so that it hides behind the next MSM's accumulation.  Defined in msm_reduce_impl.h and instantiated once per
// (curve, group) in msm_reduce.hip -- a translation unit of its own because its kernels are compiled with out-of-line
// field products (DG29_OUTLINE_MUL, fp29.h).
// out_dev: b.ninst results back to back (Jacobian x, y, z -- or affine x, y -- of instance 0, then instance 1, ..)
template <class F>
void msm_bucket_phase(hipStream_t s, const MsmSort& st, const MsmBuffers<F>& b, bool out_affine, void* out_dev);

// both phases on the call's own stream and workspace
template <class F>
void msm_reduce(Call& k, const MsmSort& st, const void* bases, bool out_affine, void* out_dev) {
  MsmBuffers<F> b = msm_buffers<F>(k.c, st.g);
  k.begin_dominant();
  b.acc_done = k.c.ev[3];                    // = end_dominant(), but in front of the G2 finalize
  if (k.ctx->kclk) b.clk = k.ctx->kclk + 2 * (&k.c - k.ctx->ch);
  msm_accumulate_phase<F>(k.s(), st, b, bases);
  k.c.ev_valid[1] = true;
  msm_bucket_phase<F>(k.s(), st, b, out_affine, out_dev);
}

}  // namespace dg16
