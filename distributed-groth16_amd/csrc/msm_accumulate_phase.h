// MSM phase 4, the launch side: the workspace of one MSM's bucket phases (MsmBuffers) and msm_accumulate_phase, which picks
// the accumulation kernel of the coordinate field.  Pipeline: msm_impl.h.
#pragma once
#include "ctx.h"
#include "lane29.h"
#include "msm_accumulate.h"
#include "msm_accumulate_steps.h"
#include "msm_sort.h"

namespace dg16 {

// Workspace of one MSM's bucket phases (lives in `wsch`'s slots 7, 17, 15, 10 until the reduction is done).
// Small bucket sets (a short shard, BASELINE config 4, a plain MSM of <= 2^15 points) are reduced by the radix-16 / radix-8
// lane-form kernel of msm_reduce_impl.h (msm_lane_reduce_kernel): one WAVE per bucket at the first level
// (kLaneReduceMaxBuckets: msm_geom.h)
template <class F>
inline bool lane_reduce_applies(size_t buckets_over_all_windows) {
  if constexpr (!lane29::enabled<F>()) return false;
  else {
    static const bool off = [] { const char* e = getenv("DG16_NO_LANE_REDUCE"); return e && atoi(e) != 0; }();
    return !off && buckets_over_all_windows <= kLaneReduceMaxBuckets;
  }
}
template <class F>
struct MsmBuffers {
  XYZZ29<F>* buckets;
  XYZZ29<F>* seg_sum;
  XYZZ29<F>* row_w;
  XYZZ29<F>* row_r;
  XYZZ29<F>* fold;
  XYZZ29<F>* window_sums;    // internal form: the tail's wave-cooperative chain runs on the reduced-radix types
  XYZZ29<F>* lane_tmp;       // (W, R) pairs between the levels of msm_lane_reduce_kernel, or null (msm_reduce_impl.h)
  XYZZ29<F>* top_tmp;        // the same for the lane-form levels that stand in for msm_top_kernel (msm_lane_top), or null
  hipStream_t finalize_stream = nullptr;   // G2: the throughput finalize goes to this stream (behind acc_done) instead of
                                           // following the accumulation on its own (the prover: B's reduction stream)
  bool busy_chip = false;    // the reduction runs beside saturating kernels of other streams (a proof's MSMs): small
                             // workgroups only (msm_lane_reduce_serial_kernel instead of the 16-wave form)
  unsigned* giant;
  unsigned giant_cap;
  size_t nbw, nrows;     // over all instances
  unsigned ninst;        // MSMs sharing the sort (msm_accumulate_kernel): bucket-window index wy = inst * bw + w
  RowGeom rg;
  unsigned long long* clk = nullptr;   // ClkProbe counters of the accumulation kernel (two device words), or null
  hipEvent_t acc_done = nullptr;   // recorded right behind the accumulation KERNEL (in front of the G2 finalize that
                                   // msm_accumulate_phase launches after it): the end of dg16_last_kernel_ms's bracket
};

template <class F>
MsmBuffers<F> msm_buffers(Channel& wsch, const MsmGeom& g, unsigned ninst = 1) {
  MsmBuffers<F> b;
  DG_REQUIRE(ninst >= 1 && ninst <= kMaxInst, DG16_ERR_BAD_ARG, "1..4 MSM instances per sort");
  b.ninst = ninst;
  const size_t bwi = (size_t)g.bw * ninst;
  b.nbw = bwi << g.log_nb;
  const size_t nseg_slots = bwi * g.seg_cap;
  b.giant_cap = (unsigned)(nseg_slots / kGiantSegs + 1);
  // capacities of the giant work list (msm_register_giant): ids < giant_cap, work items <= 2 giant_cap
  DG_REQUIRE(nseg_slots / kGiantSegs + 1 < ((size_t)1 << 26), DG16_ERR_BAD_ARG, "giant list: id slot must fit 26 bits");
  static_assert(kGiantSlices <= 64, "a work item keeps its slice in six bits");
  static_assert(kGiantSliceSegs >= kGiantSegs, "work items <= 2 giant_cap needs slices no shorter than kGiantSegs partials");
  DG_REQUIRE(nseg_slots / kGiantSliceSegs + 1 + b.giant_cap <= 2 * (size_t)b.giant_cap + 1, DG16_ERR_BAD_ARG,
             "giant list: work-item capacity");
  b.buckets = (XYZZ29<F>*)ws(wsch, 7, b.nbw * sizeof(XYZZ29<F>));
  b.seg_sum = (XYZZ29<F>*)ws(wsch, 17, nseg_slots * sizeof(XYZZ29<F>));
  b.rg = row_geometry(g);
  b.nrows = bwi << b.rg.rows_log;
  const size_t nfold = bwi * 3 * 256;
  const size_t nlane = lane_reduce_applies<F>(b.nbw) ? b.nbw / 2 + 4 : 0;
  const size_t ntop = lane29::enabled<F>() ? bwi * 96 + 8 : 0;      // <= 256 entries per bucket-window: 64 + 8 pairs' slots
  uint8_t* p15 = (uint8_t*)ws(wsch, 15, (2 * b.nrows + nfold + bwi + nlane + ntop) * sizeof(XYZZ29<F>));
  b.row_w = (XYZZ29<F>*)p15;
  b.row_r = b.row_w + b.nrows;
  b.fold = b.row_r + b.nrows;
  b.window_sums = b.fold + nfold;
  b.lane_tmp = nlane ? b.window_sums + bwi : nullptr;
  b.top_tmp = ntop ? b.window_sums + bwi + nlane : nullptr;
  // [0] giants, [1] work items, then giant_cap bucket ids, then <= 2 * giant_cap (giant, slice) work items
  b.giant = (unsigned*)ws(wsch, 10, ((size_t)b.giant_cap * 3 + 2) * 4);
  return b;
}

inline int msm_finalize_lds_lpb();
template <class F>
struct MsmBuffers;
template <class F>
void msm_finalize_lds_phase(hipStream_t s, const MsmSort& st, const MsmBuffers<F>& b);
// Phase A (saturates the GPU): segment accumulation.  `bases` is the array of n points or, in table mode, the
// table of W*n points -- in INTERNAL form (msm_to_internal_kernel / msm_table_kernel).
// bases: b.ninst tables (or plain base arrays), one per instance
template <class F>
void msm_accumulate_phase(hipStream_t s, const MsmSort& st, const MsmBuffers<F>& b, const void* const* bases) {
  const MsmGeom& g = st.g;
  DG_BOUNDS_BIND();
  MsmBases mb{};
  for (unsigned i = 0; i < b.ninst; i++) mb.p[i] = (const uint32_t*)bases[i];
  if (b.clk) DG_HIP(hipMemsetAsync(b.clk, 0, 16, s));
  if constexpr (sizeof(F) > 48) {
    // G2 (Fq2 coordinates): LDS-staged accumulator; two workgroups per CU must fit the 160 KiB of LDS
    constexpr int BLOCK = 1 << msm_acc_block_log<F>();
    const dim3 grid((g.seg_cap + BLOCK - 1) / BLOCK, g.bw * b.ninst);
    if constexpr (sizeof(F) > 64) {
      // 14-limb Fq2: ONE form -- three product sites visited by a step loop (msm_accumulate_steps_kernel: a loop that fits
      // the instruction cache).  Measured against round 4's straight-line loop, same call: 8.84-8.90 ms against 8.85-8.93
      // per 2^20-point launch on a fast box of the pool, 8.93-9.17 against 18.0-18.1 on a slow one
      // (profiles/r5b_*, r5c_*); both round-4 forms and the timing-based choice between them are gone.
      hipLaunchKernelGGL((msm_accumulate_steps_kernel<F, BLOCK>), grid, dim3(BLOCK), 0, s, mb, st.n, g, st.offsets,
                         st.counts, st.seg_off, st.seg_total, st.entries, b.seg_sum, b.buckets, b.clk);
    } else {
      hipLaunchKernelGGL((msm_accumulate_lds_kernel<F, BLOCK>), grid, dim3(BLOCK), 0, s, mb, st.n, g, st.offsets, st.counts,
                         st.seg_off, st.seg_total, st.entries, b.seg_sum, b.buckets, b.clk);
    }
    if (b.acc_done) DG_HIP(hipEventRecord(b.acc_done, s));
    if (b.finalize_stream && b.acc_done) {
      DG_HIP(hipStreamWaitEvent(b.finalize_stream, b.acc_done, 0));
      msm_finalize_lds_phase<F>(b.finalize_stream, st, b);
    } else {
      msm_finalize_lds_phase<F>(s, st, b);
    }
  } else {
    constexpr int BLOCK = 1 << msm_acc_block_log<F>();
    hipLaunchKernelGGL((msm_accumulate_kernel<F, BLOCK>), dim3((g.seg_cap + BLOCK - 1) / BLOCK, g.bw * b.ninst),
                       dim3(BLOCK), 0, s, mb, st.n, g, st.offsets, st.counts, st.seg_off, st.seg_total, st.entries,
                       b.seg_sum, b.buckets, b.clk);
    if (b.acc_done) DG_HIP(hipEventRecord(b.acc_done, s));
  }
  DG_HIP(hipGetLastError());
}
template <class F>
void msm_accumulate_phase(hipStream_t s, const MsmSort& st, const MsmBuffers<F>& b, const void* bases) {
  const void* one[1] = {bases};
  msm_accumulate_phase<F>(s, st, b, one);
}

}  // namespace dg16
