// The MSM's host planning arithmetic: window width, bucket-window and segment geometry, the sort's partition choice, the
// plain MSM's plan, the row stride of a budgeted table and the slices of a giant bucket.  Plain C++ -- no HIP include and no
// device type -- so that the host compiler builds it alone and tests/test_msm_geom_host.py checks the code that ships
// (tests/witness_shapes.py mirrors it).  The structs here travel to the kernels by value.  Pipeline: msm_impl.h.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#ifndef DG_HD      // fp.h's idiom, word for word; under hipcc the includer brings the HIP runtime header (fp.h does)
#if defined(__HIPCC__)
#define DG_HD __host__ __device__ __forceinline__
#else
#define DG_HD inline
#endif
#endif

namespace dg16 {

// Accumulation segments: a bucket of cnt entries is cut into k = ceil(cnt / 2^seg_log) segments of EQUAL length
// (floor / ceil of cnt / k), one lane each: the lanes of a wave run chains of nearly the same length (with fixed-length
// segments every bucket ended in a short one and its wave idled behind the long ones), and k -- the number of partials
// the finalize has to add per bucket -- is as small as the segment length allows.  seg_log follows the mean bucket
// occupancy, clamped by the lane count a launch needs.  The (segment -> bucket) map is not stored: a lane finds its
// bucket by binary search in the exclusive scan of the per-bucket segment counts.
constexpr unsigned kMinSegLog = 3, kMaxSegLog = 9;
constexpr unsigned kMinLanesLog = 18;    // want >= 2^18 segments (4 waves per SIMD) in an accumulation launch
constexpr unsigned kGiantSegs = 64;      // buckets with more segments are reduced by a whole workgroup
constexpr unsigned kGiantSlices = 64;    // ... in at most this many slices (one workgroup each) of about
constexpr unsigned kGiantSliceSegs = 512;   // ... this many partials (giant_geometry)

struct MsmGeom {
  unsigned c;        // window bits
  unsigned nwin;     // W: signed digits per scalar
  unsigned log_nb;   // log2 buckets per bucket-window = c - 1
  unsigned seg_log;  // log2 entries per accumulation segment
  unsigned seg_cap;  // segment slots per bucket-window
  unsigned bw;       // bucket-windows: W (plain), 1 (full table: all digits share one bucket set), or the row stride
                     // k of a table thinned to every k-th row (window w feeds bucket-window w % k through row w / k)
  unsigned table;    // 1: bases are a table T[r*n + i] = 2^(c*bw*r) * P_i (resident keys)
  unsigned rows;     // table rows R = ceil(W / bw) (1 in plain mode)
  size_t region;     // entries per bucket-window: rows * n
};

// window size: plain mode keeps ~32 points per bucket; table mode has a single bucket set of W*n entries:
// c = log2(n) - 3 keeps the bucket reduction at a few percent of the MSM (measured at 2^20: c = 17 beats
// both 16 and 20; again in round 4 with the last reduction off the critical path, profiles/r4w_table_window_sweep.txt:
// 17: 10.19 ms per proof, 18: 11.10, 19: 11.35, 20: 11.83; H alone at 19 / 20: 10.28 / 10.38)
inline unsigned msm_window_bits(size_t n, bool table, unsigned scalar_bits = 0) {
  unsigned lg = 0;
  while (((size_t)1 << (lg + 1)) <= n) lg++;
  if (n > ((size_t)3 << lg) / 2) lg++;     // nearest power of two (2^20 - 5 points are "2^20")
  int c = table ? (int)lg - 3 : (int)lg - 4;
  // short tables (the shards of a multi-GPU key): the bucket reduction's latency does not shrink with the bucket
  // count, the number of bucket entries W*n does shrink with c -- measured on a 2^17-point shard: c = 14: 8.2 ms
  // per proof, 15: 6.2, 16: 6.2, 17: 6.3.  Round 6 (lane-form reductions; profiles/r6tt_*, r6uu_*, r6vv_*): on BN254 what
  // decides between neighbouring widths is the TOP window -- a width that leaves it two or three bits puts a quarter of the
  // key into a handful of giant buckets (255 digit bits: c = 12 or 14 cost a 2^15-point proof 1.8 / 1.45 ms against 1.36 at
  // 15 = 255 / 17; 16 leaves 15 bits too and costs 1.56 with twice the buckets).  So where 15 and 16 leave the same top
  // window (BN254, BLS12-377) 15 up to 2^16 points and 16 beyond; BLS12-381 (256 digit bits: 16 | 256) measured flat to
  // within 4 % between 14, 15 and 16 at 2^14..2^16 points and 12 % better at 14 for 2^13 -- it keeps lg + 1.
  if (table && c < 16) {
    c = (int)lg + 1 < 16 ? (int)lg + 1 : 16;
    if (scalar_bits && lg >= 13) {   // below 2^13 points nothing was measured: lg + 1 as before
      auto top = [&](int w) { const int bits = (int)scalar_bits + 1; return bits - ((bits + w - 1) / w - 1) * w; };
      const int t15 = top(15), t16 = top(16);
      if (t15 >= t16) c = (t15 > t16 || lg <= 16) ? 15 : 16;
    }
  }
  if (const char* e = getenv(table ? "DG16_MSM_TABLE_C" : "DG16_MSM_C")) c = atoi(e);
  int hi = table ? 20 : 16;
  if (c < 4) c = 4;
  if (c > hi) c = hi;
  return (unsigned)c;
}

// stride (table mode): 1 = every window has its table row; k > 1 = the table keeps every k-th row (HBM budget) and the
// MSM has k bucket sets combined by a Horner tail of (k - 1) * c doublings:
//   sum_w d_w 2^(c w) P = sum_{j < k} 2^(c j) sum_r d_{k r + j} (2^(c k r) P)
inline MsmGeom msm_geometry(size_t n, unsigned scalar_bits, bool table = false, unsigned c_fixed = 0, unsigned stride = 1) {
  MsmGeom g;
  g.c = c_fixed ? c_fixed : msm_window_bits(n, table, table ? scalar_bits : 0);   // a table's own width (msm_window_bits)
  g.nwin = (scalar_bits + 1 + g.c - 1) / g.c;   // one spare bit absorbs the last carry
  g.log_nb = g.c - 1;
  g.table = table ? 1u : 0u;
  if (stride < 1) stride = 1;
  if (stride > g.nwin) stride = g.nwin;
  g.bw = table ? stride : g.nwin;
  g.rows = (g.nwin + g.bw - 1) / g.bw;
  g.region = (size_t)g.rows * n;
  {
    size_t mean = g.region >> g.log_nb;   // entries per bucket
    unsigned lm = 0;
    while (((size_t)2 << lm) <= mean) lm++;
    // Segment length: 16 entries while the launch has ~2^20 segments, 32 beyond -- short segments balance the last rounds of
    // a launch, long ones leave fewer partials per bucket for the tree / finalize, and which matters more is a matter of
    // how many rounds the launch runs.  Measured (profiles/r4seg_*, r5k_*, r5l_*, same call each): BN254 2^20 (2^23.9
    // entries) 16: 10.01-10.04 ms per proof, 32: 10.14-10.19; BLS12-381 2^20 (2^24 entries) 8: 22.4-23.1, **16: 21.2-21.6**,
    // 32: 22.3-22.4 (the rule before round 5 -- mean occupancy / 8 -- gave 32 there: 256 entries per bucket exactly),
    // 64: 24.2; BN254 2^22 (2^25.8) 16: 36.8-37.1, **32: 36.0-36.6**; BLS12-381 2^22 16: 83.5-83.8, 32: 82.0-82.1.
    unsigned le_all = 0;
    while (((size_t)2 << le_all) <= g.region * g.bw) le_all++;   // floor(log2(entries of the launch: all bucket-windows))
    int sl = (int)le_all - 20;
    if (sl < 4) sl = 4;
    if (sl > 5) sl = 5;
    if (sl > (int)lm - 2) sl = (int)lm - 2;                      // ... and at least four segments per mean bucket
    if (sl < 4) sl = 4;
    // ... but never so long that the launch runs out of lanes (a 2^17-point shard with 32-entry segments has
    // 1.2 waves per SIMD: measured 0.62 ms per G1 accumulation instead of 0.25)
    unsigned le = 0;
    while (((size_t)2 << le) <= (size_t)g.nwin * n) le++;
    int cap = (int)le - (int)kMinLanesLog;
    // ... except a PLAIN MSM of 2^20..2^21 entries (2^16 points after the GLV split): 8-entry segments are 1.25 rounds of the
    // 14-limb G1 accumulation's 2^17 resident lanes and ~4 partials per bucket for the wave-per-bucket finalize, 16-entry
    // ones are one round of the same length and half the partials -- BLS12-377 G1 2^16 1.51 -> 1.20 ms, BLS12-381 G1 1.26 ->
    // 1.13, BN254 G2 1.87 -> 1.64, BN254 G1 unchanged; a size down or up 16 is no better or worse
    // (profiles/r6xx_seg_log_small_plain_msm.txt: DG16_MSM_SEG_LOG sweep, same call)
    if (!table && le == 20 && cap < 4) cap = 4;
    if (sl > cap) sl = cap;
    g.seg_log = (unsigned)(sl < (int)kMinSegLog ? (int)kMinSegLog : sl > (int)kMaxSegLog ? (int)kMaxSegLog : sl);
    static const int seg_env = [] { const char* e = getenv("DG16_MSM_SEG_LOG"); return e ? atoi(e) : 0; }();   // (sweeps)
    if (seg_env >= (int)kMinSegLog && seg_env <= (int)kMaxSegLog) g.seg_log = (unsigned)seg_env;
  }
  g.seg_cap = (1u << g.log_nb) + (unsigned)((g.region + (1u << g.seg_log) - 1) >> g.seg_log);
  return g;
}

// ---- the digit sort (msm_sort.h) ------------------------------------------------------------------------------------
constexpr unsigned kScanBlock = 4096;   // buckets per workgroup of the bucket scans (1024 threads x 4)

// the partitioned sort: the slot index (bucket-window, bucket) = partition (high bits, <= kPartMax) | bin (low bits)
constexpr unsigned kPartScalars = 1024;   // scalars per workgroup in pass 1
constexpr unsigned kPartMax = 256;        // partitions
constexpr unsigned kPartMaxLowBits = 12;  // bins per partition <= 4096
constexpr unsigned kPartTileLog = 11;     // entries per tile in pass 2 (8 per lane)
constexpr unsigned kPartBlocks = 32;      // workgroups striding over one partition's tiles

struct PartGeom {
  unsigned low_bits, nparts, nblk1;
};
struct PartPlan {
  PartGeom pg;
  bool partitioned;    // the LDS-partitioned passes; false: the direct atomic path (pg is then unused)
};
// large sorts: LDS-partitioned passes; small ones: the direct atomic path (fewer launches)
inline PartPlan msm_partition_plan(const MsmGeom& g, size_t n) {
  const size_t nbw = (size_t)g.bw << g.log_nb;
  unsigned lg_nbw = 0;
  while (((size_t)1 << lg_nbw) < nbw) lg_nbw++;
  static const int force_path = [] { const char* e = getenv("DG16_MSM_SORT"); return e ? atoi(e) : 0; }();  // 1 atomic, 2 partitioned
  PartPlan p;
  p.pg.low_bits = lg_nbw > 8 ? lg_nbw - 8 : 0;
  p.partitioned = p.pg.low_bits <= kPartMaxLowBits &&
                  (force_path == 2 || (force_path != 1 && (size_t)g.nwin * n >= ((size_t)1 << 18)));
  p.pg.nparts = (unsigned)((nbw + ((size_t)1 << p.pg.low_bits) - 1) >> p.pg.low_bits);
  p.pg.nblk1 = (unsigned)((n + kPartScalars - 1) / kPartScalars);
  return p;
}

// ---- the bucket reduction (msm_reduce_impl.h) ------------------------------------------------------------------------
// rows of 2^kRowLog buckets
constexpr unsigned kRowLog = 8;
struct RowGeom {
  unsigned row_log;    // log2 buckets per row (<= kRowLog)
  unsigned rows_log;   // log2 rows per bucket-window
};
inline RowGeom row_geometry(const MsmGeom& g) {
  RowGeom r;
  r.row_log = g.log_nb < kRowLog ? g.log_nb : kRowLog;
  r.rows_log = g.log_nb - r.row_log;
  return r;
}
// bucket sets up to this size (over all windows) go to the lane-form reduction (msm_accumulate_phase.h: lane_reduce_applies)
constexpr size_t kLaneReduceMaxBuckets = 32768;

// Giant buckets go on a device-side work list: stage 1 cuts the bucket's segment partials into <= kGiantSlices slices, one
// workgroup each; stage 2 adds the slice sums (msm_finalize.h: msm_register_giant, msm_reduce_impl.h).
DG_HD void giant_geometry(unsigned nseg, unsigned& slices, unsigned& per) {
  slices = (nseg + kGiantSliceSegs - 1) / kGiantSliceSegs;
  if (slices > kGiantSlices) slices = kGiantSlices;
  per = (nseg + slices - 1) / slices;
  slices = (nseg + per - 1) / per;
}

// ---- the plain MSM (msm_glv.h: msm_run) -----------------------------------------------------------------------------
constexpr int kGlvBits = 127;      // |k1|, |k2| < 2^127 (measured bound: 0.81 x 2^127 over all 255-bit inputs; tests/test_host_arith.py)
constexpr int kGlv4Bits = 65;      // the quarters of split4: < 2^65 (BLS12-381: 0.52 x 2^64 for canonical scalars; one spare bit for non-canonical 255-bit inputs)

struct PlainPlan {
  bool split;             // the scalars are split by the endomorphism: the sort sees dim * n part scalars
  unsigned c_small;       // the sort's fixed window width, 0 = msm_window_bits' rule
  unsigned scalar_bits;   // the width the sort runs at: kGlvBits / kGlv4Bits when split, 0 = the curve's own
};
// nine_limbs: RR<..>::N == 9 (BN254's base field); dim: GlvOf<F>::DIM; split_applies: the group has an endomorphism and its
// bases are known to lie in the order-r subgroup (msm_run)
inline PlainPlan msm_plain_plan(bool nine_limbs, unsigned dim, size_t n, bool split_applies) {
  PlainPlan p{false, 0u, 0u};
  if (!split_applies || !n || !((size_t)dim * n * 40 < ((size_t)1 << 31))) return p;
  p.split = true;
  p.scalar_bits = dim == 2 ? (unsigned)kGlvBits : (unsigned)kGlv4Bits;
  if (dim == 2) {
    // Window width at SMALL sizes (round 6, profiles/r6b_msm_window_sweep.txt): the halves have 127 + 1 bits, and a
    // width of 7 or 9 (what log2(2 n) - 4 gives at n = 2^10 / 2^12) leaves a top window of two bits whose few buckets
    // turn giant -- 8 divides 128: BN254 G1 2^10 0.663 -> 0.606 ms, 2^12 0.685 -> 0.649; G2 1.68 -> 1.47, 1.92 -> 1.62
    // (same call).  The 14-limb G1 groups measured the other way (2^12: 1.33 -> 1.49 ms) and keep the rule.
    // ... and at LARGE sizes (end of round 6, profiles/r6zu_*, r6zt_*): 16 divides 128 as well -- eight windows instead of
    // the ten / nine of log2(2 n) - 4 = 14 / 15 (whose top windows are 2 / 8 bits), i.e. a fifth fewer additions per
    // point, and the bucket reductions are cheap enough since the lane forms to take 2^15 buckets per window: 2^17
    // points BN254 G1 1.24 -> 0.93 ms, BLS12-377 1.70 -> 1.60, BLS12-381 1.78 -> 1.59; 2^18 points 1.17 -> 1.15 / 2.33 ->
    // 2.06 / 2.64 -> 2.07 (same call, twice).  The G2 groups (four 64-bit quarters) measured mixed and keep the rule.
    const unsigned c0 = msm_window_bits(2 * n, false);
    if (nine_limbs && (c0 == 7 || c0 == 9) && !getenv("DG16_MSM_C")) p.c_small = 8;
    if ((c0 == 14 || c0 == 15) && !getenv("DG16_MSM_C")) p.c_small = 16;
  }
  return p;
}

// ---- resident tables (msm_table.h) ----------------------------------------------------------------------------------
constexpr unsigned kMaxTableWin = 64;
// Row stride of a table under an HBM budget: the smallest k such that ceil(nwin / k) rows fit (0 = no budget -> 1).
inline unsigned table_stride_for(size_t full_bytes, size_t budget, unsigned nwin) {
  if (!budget || full_bytes <= budget || nwin <= 1) return 1;
  const size_t row = full_bytes / nwin;
  size_t rows_fit = budget / (row ? row : 1);
  if (rows_fit < 1) rows_fit = 1;                         // (one row -- the bases themselves -- is the floor)
  unsigned k = (unsigned)((nwin + rows_fit - 1) / rows_fit);
  return k < 1 ? 1 : k > nwin ? nwin : k;
}

}  // namespace dg16
