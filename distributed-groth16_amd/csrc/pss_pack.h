// Packing a point vector into party shares (dg16_pss_pack_points) and, on top of it, a whole proving key
// (dg16_pk_pack): out[r][e] = sum_{c<l} M[r][c] * P[e * l + c], r < n = 4 l parties, e < chunks = ceil(n_points / l), P
// padded with identities, M the canonical pack matrix of the handle (dist_impl.h: dg16_pss::mats).
//
//   why not matvec_points_kernel   it multiplies each of the l terms of an output by a complete double-and-add and
//              inverts once per lane.  The multipliers are the n l constants of (curve, l): every lane of a launch that
//              works on party r walks the SAME digits, as in points_scale.h, and the l terms of one output can share ONE
//              doubling chain (Straus interleaving), which a single product cannot.
//   schedule   made on the host once per (handle, group, split) (make_schedule) and cached in the dg16_pss under its
//              mutex.  Every M[r][c] is split with the group's endomorphism where the rule of dg16_msm allows it
//              (pmul::may_split), every part recoded as a width-w non-adjacent form with its sign folded in
//              (wnaf.h: recode_wnaf).  Row r holds, per position, the signed bytes of its l DIM parts -- byte
//              c * DIM + j is part j of M[r][c], padded to whole 32-bit words -- from position 0 to the highest non-zero
//              position of any of its parts.
//   table      kernel 1, one lane per input point of the slice: the odd multiples P, 3P, .. (2^(w-1) - 1) P, one doubling
//              and 2^(w-2) - 1 additions (wnaf.h: build_odd_table), written ONCE per point and read by all n rows.  Word
//              t of entry j of point (e, c) lies at ((c * kTable + j - 1) * W + t) * stride + e: the lanes of a wave of
//              kernel 2 hold consecutive e and the same c, so they read consecutive words (pmul::GlobalTab with the base
//              moved by c).
//   combine    kernel 2, one lane per (e, r), r = blockIdx.y: the digit row is read at an address that depends on r and
//              the position alone, so every "digit is zero" branch is uniform.  Per position ONE doubling, then one
//              addition of psi^j(T_c[|d|]) (y negated for d < 0) per non-zero digit; a zero word of the row is skipped
//              whole.  The chain starts at the row's top position, so no identity is doubled.  One addition site in the
//              text: the parts are walked by a run-time loop (uniform over the wave).
//   width      w = 7, by the count.  Per output (density of a width-w NAF: one non-zero digit in w + 1 positions; the
//              table of an input point is shared by n = 4 l outputs, so an output pays l / n = 1/4 of one table):
//                 additions per output = (2^(w-2) - 1) / 4 + l * bits / (w + 1), bits = 254 (2 x 127; 255 plain, 264 DIM 4)
//                 w      table adds / 4    l = 1     l = 2     l = 4     l = 8     entries   table per chunk (BN254 G1)
//                 5      1.75              44.1      86.4      171.1     340.4     8         l x 1 KB
//                 6      3.75              40.0      76.3      148.9     294.0     16        l x 2 KB
//                 7      7.75              39.5      71.3      134.8     261.8     32        l x 4 KB
//                 8      15.75             44.0      72.2      128.6     241.5     64        l x 8 KB
//              w = 7 is the minimum at l = 1 and l = 2 and within 5 % / 8 % of w = 8 at l = 4 / 8, whose table is twice
//              as large.  At w = 7 a chunk's tables are 32 l XYZZ entries = 8 entries per output: exactly the bytes
//              dg16_points_mul's eight-entry tables take per product, so the same slice setting bounds the same workspace
//              (l x 4 KB per chunk for BN254 G1, l x 12 KB for a BLS12 G2).  Digits stay signed bytes (|d| <= 63).
//   budget     doublings per output: 1/4 (table) + the top position of the row: at most 256 / 128 / 68 on the plain /
//              DIM 2 / DIM 4 paths, whatever l is.  matvec_points_kernel: about 254 l doublings and 127 l additions.
//   affine     the accumulators of a slice go through fixed_base_impl.h's batched inversion (fb_to_affine).
//   slices     chunks per slice = the context's points_mul_slice (slices.h's default) / n rounded down to a multiple of
//              64 (at least 64): the slice's outputs do not exceed the setting.  Tables, accumulators and staging come
//              from channel 0's workspace.
//
// Exceptional cases of the addition law.  Every addition is XYZZ::add, which is complete.  Inside one chunk they all
// occur: the accumulator is the identity until the first non-zero digit of a non-identity point, an identity input (the
// padding) makes its table the identity, P and P or P and -P in one chunk make the terms of two columns meet, and on the
// plain path a point outside the subgroup can meet its own multiples anywhere.  Nothing is proven away.
//
// The schedule and the loops are host and device text: tests/host_arith/host_pss_pack.cpp runs them on a CPU against the
// oracle and counts the group operations through the Ops parameter.
#pragma once
#include <vector>

#include "points_scale.h"

namespace dg16 {
namespace ppack {

constexpr int kWidth = 7;
constexpr int kTable = 1 << (kWidth - 2);      // entries 1P, 3P, .. 63P
using wnaf::kMaxRows;                          // positions of a part: at most 256
constexpr unsigned kMaxL = 8;                  // dg16_pss_create's bound

// The schedule of one (pack matrix, split).  words: 32-bit words per position = ceil(l * dim / 4); row r occupies
// rows[r * stride * words ..), position-major; len[r] positions are in use (0 for an all-zero row of M).
struct Schedule {
  int dim = 1;             // 1 (plain), 2 or 4
  unsigned l = 0, n = 0;
  int words = 0;
  int stride = 0;          // positions allotted per row: the longest row
  std::vector<int> len;
  std::vector<uint32_t> rows;
  // the device image: n lengths, then the rows
  std::vector<uint32_t> image() const {
    std::vector<uint32_t> v(len.begin(), len.end());
    v.insert(v.end(), rows.begin(), rows.end());
    return v;
  }
};

// M: [n][l] canonical scalars of 8 words (below r < 2^255).  split: use the group's endomorphism (the caller applied
// pmul::may_split)
template <class F>
inline void make_schedule(const uint32_t* M, unsigned l, bool split, Schedule& s) {
  s.l = l;
  s.n = 4 * l;
  s.dim = 1;
  if constexpr (GlvOf<F>::enabled) {
    if (split) s.dim = GlvOf<F>::DIM;
  }
  const int parts = (int)l * s.dim;
  s.words = (parts + 3) / 4;
  std::vector<int8_t> dig((size_t)s.n * parts * kMaxRows);
  s.len.assign(s.n, 0);
  s.stride = 0;
  for (unsigned r = 0; r < s.n; r++) {
    for (unsigned c = 0; c < l; c++) {
      const uint32_t* k = M + ((size_t)r * l + c) * 8;
      int8_t* d = &dig[((size_t)r * parts + (size_t)c * s.dim) * kMaxRows];
      int len = 0;
      bool done = false;
      if constexpr (GlvOf<F>::enabled) {
        if (split) {
          pmul::SplitScalar<F> sp;
          pmul::split_scalar<F>(k, sp);
          for (int j = 0; j < GlvOf<F>::DIM; j++) {
            const int lj = wnaf::recode_wnaf<kWidth>(sp.mag[j], sp.neg[j], d + (size_t)j * kMaxRows);
            len = lj > len ? lj : len;
          }
          done = true;
        }
      }
      if (!done) len = wnaf::recode_wnaf<kWidth>(k, false, d);
      s.len[r] = len > s.len[r] ? len : s.len[r];
    }
    s.stride = s.len[r] > s.stride ? s.len[r] : s.stride;
  }
  s.rows.assign((size_t)s.n * s.stride * s.words, 0u);
  for (unsigned r = 0; r < s.n; r++)
    for (int p = 0; p < parts; p++)
      for (int i = 0; i < s.len[r]; i++) {
        const uint32_t b = (uint8_t)dig[((size_t)r * parts + p) * kMaxRows + i];
        s.rows[((size_t)r * s.stride + i) * s.words + p / 4] |= b << (8 * (p % 4));
      }
}

// the table of one input point at this header's width
template <class F, class Ops, class Tab>
DG_HD void build_odd_table(const Affine<F>& p, Ops& ops, Tab& tab) {
  wnaf::build_odd_table<kTable>(p, ops, tab);
}

// sum_c M[r][c] P_c under row r's schedule: rows = the row's words, len its positions; tabs.get(c, j) = entry j of the
// table of the chunk's c-th point.  DIM = 1 for ANY points of the curve, DIM = 2 / 4 for points of the order-r subgroup.
template <int DIM, class F, class Ops, class Tabs>
DG_HD XYZZ<F> combine(const uint32_t* rows, int len, int words, Ops& ops, const Tabs& tabs) {
  XYZZ<F> acc = XYZZ<F>::inf();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int i = len - 1; i >= 0; i--) {
    if (i != len - 1) acc = ops.dbl(acc);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int w = 0; w < words; w++) {
      const uint32_t row = rows[(size_t)i * words + w];
      if (!row) continue;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
      for (int b = 0; b < 4; b++) {
        const int d = wnaf::row_digit(row, b);
        if (!d) continue;
        const int part = 4 * w + b;
        const int m = d < 0 ? -d : d;
        XYZZ<F> e = tabs.get(part / DIM, (m >> 1) + 1);
        if constexpr (DIM > 1) {
          const int j = part % DIM;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
          for (int t = 0; t < j; t++) GlvOf<F>::endo_xyzz(e);
        }
        if (d < 0) e.y = e.y.neg();
        acc = ops.add(acc, e);
      }
    }
  }
  return acc;
}

// chunks of a vector of n_points points
inline size_t chunks_of(size_t n_points, unsigned l) { return (n_points + l - 1) / l; }
// chunks per slice under a points_mul_slice setting of `slice` outputs
inline size_t slice_chunks(size_t slice, unsigned n) {
  const size_t c = slice / n / 64 * 64;
  return c < 64 ? 64 : c;
}

}  // namespace ppack
}  // namespace dg16

#if defined(__HIPCC__)
// ---- device side ----------------------------------------------------------------------------------------------------------
#include "dist_impl.h"

namespace dg16 {
namespace ppack {

// the tables of one chunk in the slice's buffer (see the header comment); base is offset by the chunk
template <class F>
struct ChunkTabs {
  static constexpr size_t W = sizeof(XYZZ<F>) / 4;
  uint32_t* base;
  size_t stride;       // chunks of the slice, a multiple of 64
  __device__ __forceinline__ pmul::GlobalTab<F> of(int c) const {
    return pmul::GlobalTab<F>{base + (size_t)c * kTable * W * stride, stride};
  }
  __device__ __forceinline__ XYZZ<F> get(int c, int j) const { return of(c).get(j); }
};

// One lane per (e, c): c = blockIdx.y, e < cnt <= stride.  points: the slice's points, point (e, c) at e * l + c; an
// index from npts on is the identity padding.
template <class F>
__global__ void __launch_bounds__(64) pss_pack_table_kernel(const Affine<F>* __restrict__ points, size_t npts, unsigned l,
                                                             size_t cnt, uint32_t* __restrict__ table, size_t stride) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= cnt) return;
  const unsigned c = blockIdx.y;
  const size_t idx = e * l + c;
  const Affine<F> p = idx < npts ? fb_load(points + idx) : Affine<F>::inf();
  ChunkTabs<F> tabs{table + e, stride};
  pmul::GlobalTab<F> tab = tabs.of((int)c);
  pmul::PlainOps<F> ops;
  build_odd_table(p, ops, tab);
}

// One lane per (e, r): r = blockIdx.y.  sched: n lengths, then the rows (Schedule::image).  acc_out: [n][cnt].
template <class F, int DIM>
__global__ void __launch_bounds__(64) pss_pack_combine_kernel(const uint32_t* __restrict__ sched, unsigned n, int words,
                                                               int sstride, size_t cnt, uint32_t* __restrict__ table,
                                                               size_t stride, XYZZ<F>* __restrict__ acc_out) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= cnt) return;
  const unsigned r = blockIdx.y;
  const int len = (int)sched[r];
  const uint32_t* rows = sched + n + (size_t)r * sstride * words;
  ChunkTabs<F> tabs{table + e, stride};
  pmul::PlainOps<F> ops;
  fb_store(acc_out + (size_t)r * cnt + e, combine<DIM, F>(rows, len, words, ops, tabs));
}

// the handle's schedule of (group, split); made on first use.  The mutex is held across the copy-back and the stream
// synchronisation: every user of a pp is on pp's context, and the first of them pays once.  The reference returned
// outlives the lock: a slot is written once and never reset or replaced while the handle lives (dg16_pss_destroy
// frees it with the handle), so the Schedule it points to stays where it is.
template <class F>
const Schedule& schedule_of(Call& k, const dg16_pss* pp, int group, bool split) {
  std::lock_guard<std::mutex> g(pp->sched_mu);
  std::shared_ptr<const void>& slot = pp->sched[group - 1][split ? 1 : 0];
  if (!slot) {
    const size_t cnt = (size_t)pp->n * pp->l;
    std::vector<uint32_t> M(cnt * 8);
    // the canonical copy of block 0 (pack [n][l]) follows the three Montgomery matrices
    DG_HIP(hipMemcpyAsync(M.data(), (const char*)pp->mats + 3 * cnt * 32, cnt * 32, hipMemcpyDeviceToHost, k.s()));
    DG_HIP(hipStreamSynchronize(k.s()));
    auto s = std::make_shared<Schedule>();
    make_schedule<F>(M.data(), pp->l, split, *s);
    slot = s;
  }
  return *static_cast<const Schedule*>(slot.get());
}

// shares_host[r][e] (party-major, [n][chunks] affine) from points_host[0 .. n_points); synchronous.
// Workspace slots of channel 0: 0 (the slice's points), 1 (schedule), 2 (the slice's shares), and those of
// pmul::points_mul_typed with the same sizes per output: 20 (tables), 21 (accumulators), 22 (prefix products).
template <class F>
void pack_points_typed(Call& k, const dg16_pss* pp, int group, const void* points_host, size_t n_points,
                       void* shares_host, bool in_subgroup) {
  if (!n_points) return;
  const unsigned l = pp->l, n = pp->n;
  const Schedule& s = schedule_of<F>(k, pp, group, pmul::may_split<F>(in_subgroup));
  const std::vector<uint32_t> img = s.image();
  const size_t chunks = chunks_of(n_points, l);
  const size_t per = slice_chunks(k.ctx->points_mul_slice ? k.ctx->points_mul_slice : kSliceDefault, n);
  const size_t stride = launch_stride(chunks, per);
  constexpr size_t W = sizeof(XYZZ<F>) / 4;
  Affine<F>* p = (Affine<F>*)ws(k.c, 0, stride * l * sizeof(Affine<F>));
  uint32_t* sched = (uint32_t*)ws(k.c, 1, img.size() * 4);
  Affine<F>* out = (Affine<F>*)ws(k.c, 2, (size_t)n * stride * sizeof(Affine<F>));
  uint32_t* table = (uint32_t*)ws(k.c, 20, (size_t)l * kTable * W * stride * 4);
  XYZZ<F>* acc = (XYZZ<F>*)ws(k.c, 21, (size_t)n * stride * sizeof(XYZZ<F>));
  F* pref = (F*)ws(k.c, 22, (size_t)n * stride * sizeof(F));
  DG_HIP(hipMemcpyAsync(sched, img.data(), img.size() * 4, hipMemcpyHostToDevice, k.s()));
  k.begin_dominant();
  for (size_t lo = 0; lo < chunks; lo += per) {
    const size_t cnt = chunks - lo < per ? chunks - lo : per;
    const size_t first = lo * l;
    const size_t npts = n_points - first < cnt * l ? n_points - first : cnt * l;
    // (the copy is ordered behind the previous slice's kernels on the stream)
    DG_HIP(hipMemcpyAsync(p, (const Affine<F>*)points_host + first, npts * sizeof(Affine<F>), hipMemcpyHostToDevice,
                          k.s()));
    const dim3 block(64);
    hipLaunchKernelGGL(pss_pack_table_kernel<F>, dim3((unsigned)((cnt + 63) / 64), l), block, 0, k.s(), p, npts, l, cnt,
                       table, stride);
    DG_HIP(hipGetLastError());
    const dim3 grid((unsigned)((cnt + 63) / 64), n);
    if (s.dim == 1)
      hipLaunchKernelGGL((pss_pack_combine_kernel<F, 1>), grid, block, 0, k.s(), sched, n, s.words, s.stride, cnt, table,
                         stride, acc);
    else
      hipLaunchKernelGGL((pss_pack_combine_kernel<F, GlvOf<F>::DIM>), grid, block, 0, k.s(), sched, n, s.words, s.stride,
                         cnt, table, stride, acc);
    DG_HIP(hipGetLastError());
    fb_to_affine(k, acc, pref, cnt * n, out);
    // [n][cnt] -> columns lo .. lo + cnt of [n][chunks]
    DG_HIP(hipMemcpy2DAsync((Affine<F>*)shares_host + lo, chunks * sizeof(Affine<F>), out, cnt * sizeof(Affine<F>),
                            cnt * sizeof(Affine<F>), n, hipMemcpyDeviceToHost, k.s()));
  }
  k.end_dominant();
  DG_HIP(hipStreamSynchronize(k.s()));
}

}  // namespace ppack

// host pointers
template <int CURVE>
void pss_pack_run(Call& k, const dg16_pss* pp, int group, const void* points_host, size_t n_points, void* shares_host,
                  bool in_subgroup);
// (defined in the per-curve objects pss_pack_<curve>.o)
template <> void pss_pack_run<0>(Call&, const dg16_pss*, int, const void*, size_t, void*, bool);
template <> void pss_pack_run<1>(Call&, const dg16_pss*, int, const void*, size_t, void*, bool);
template <> void pss_pack_run<2>(Call&, const dg16_pss*, int, const void*, size_t, void*, bool);

}  // namespace dg16
#endif
