// Planning of dg16_groth16_setup_srs (setup_srs_curve.hip): which of the three summation paths a wire's segment takes and
// how the segments of one output are cut into term slices.  Plain C++ -- no HIP include and no device type -- so that the
// host compiler builds it alone (tests/test_setup_srs_plan.py) and the kernels use the same rule.
//
//   segment   the terms v * P[i] of ONE wire of ONE output: the wire's columns of the contributing matrices one after the
//             other (A for a_query; B for the two b queries; A, B, C -- each with its own point table -- for K) and, for
//             an instance wire of an output that A enters, one more term with coefficient 1 (the row nc + k)
//   path      by the segment's length: 0 entries = the identity; below kWaveFrom one lane adds them up; from kWaveFrom
//             a wave does (each lane a strided share, then a tree over the lanes); from kMsmFrom the segment is an MSM in
//             its own right and goes to the library's Pippenger path over the gathered bases
//   slice     the term buffer holds at most `slice` terms: the entries of the lane and wave segments are cut into runs of
//             that many CONSECUTIVE entries (a run never contains an MSM segment; it may start or end inside a segment,
//             whose partial sums then meet in the wire's accumulator)
//
// Thresholds (reasoned, not measured: DESIGN.md).  A lane-path segment costs its lane len - 1 serial additions while
// the other lanes of the wave wait for the longest, so the lane path ends where a wave's 64 lanes + 6 tree steps are no
// more additions than the serial chain: 32 is half a wave.  A wave-path segment of len entries is len / 64 + 6 serial
// additions; at 4096 that is 70, about one point multiplication, and from there on a segment with full-width
// coefficients is cheaper as a bucket MSM (no doubling chain per term) and a segment of +-1 terms is long enough to
// fill the chip on its own.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#ifndef DG_HD      // fp.h's idiom, word for word; under hipcc the includer brings the HIP runtime header (fp.h does)
#if defined(__HIPCC__)
#define DG_HD __host__ __device__ __forceinline__
#else
#define DG_HD inline
#endif
#endif

namespace dg16 {
namespace srs {

constexpr unsigned kWaveFrom = 32;
constexpr unsigned kMsmFrom = 4096;
constexpr unsigned kWave = 64;             // lanes of a wave: the wave path's stride

enum Path : unsigned { kPathEmpty = 0, kPathLane = 1, kPathWave = 2, kPathMsm = 3 };

DG_HD Path path_of(size_t len) {
  return len == 0 ? kPathEmpty : len < kWaveFrom ? kPathLane : len < kMsmFrom ? kPathWave : kPathMsm;
}

// entries of wire k's segment: its column in up to three matrices and the instance term
DG_HD size_t segment_len(unsigned col_a, unsigned col_b, unsigned col_c, bool instance_term) {
  return (size_t)col_a + col_b + col_c + (instance_term ? 1u : 0u);
}

struct Slice {       // entries [lo, hi) of the output's entry numbering; they belong to the wires k0 .. k1 (inclusive)
  uint32_t lo, hi, k0, k1;
  uint32_t w0, w1;   // the wave-path wires among them: wave[w0 .. w1)
};

struct Plan {
  std::vector<Slice> slices;
  std::vector<uint32_t> wave, msm;       // wires on the wave path / the MSM path, ascending
  size_t columns[4] = {0, 0, 0, 0};      // wires per path (indexed by Path)
  size_t terms[4] = {0, 0, 0, 0};        // entries per path
};

// seg_ptr[k] .. seg_ptr[k + 1]: the entries of wire k, k < nv (the exclusive scan of the segment lengths); slice >= 1
inline Plan make_plan(const uint32_t* seg_ptr, size_t nv, size_t slice) {
  Plan p;
  if (slice < 1) slice = 1;
  size_t k = 0;
  while (k < nv) {
    // a run of consecutive wires without an MSM segment
    size_t e = k;
    while (e < nv && path_of(seg_ptr[e + 1] - seg_ptr[e]) != kPathMsm) e++;
    for (size_t j = k; j < e; j++) {
      const size_t len = seg_ptr[j + 1] - seg_ptr[j];
      const Path path = path_of(len);
      p.columns[path]++;
      p.terms[path] += len;
      if (path == kPathWave) p.wave.push_back((uint32_t)j);
    }
    if (e < nv) {
      p.columns[kPathMsm]++;
      p.terms[kPathMsm] += seg_ptr[e + 1] - seg_ptr[e];
      p.msm.push_back((uint32_t)e);
    }
    // cut the run's entries [seg_ptr[k], seg_ptr[e]) into slices; kf, wf walk along with the cuts
    size_t kf = k, wf = p.wave.size();
    while (wf > 0 && p.wave[wf - 1] >= k) wf--;
    for (size_t lo = seg_ptr[k]; lo < seg_ptr[e];) {
      const size_t hi = seg_ptr[e] - lo < slice ? seg_ptr[e] : lo + slice;
      while (seg_ptr[kf + 1] <= lo) kf++;                   // the wire that holds entry lo (empty wires are passed)
      size_t kl = kf;
      while (seg_ptr[kl + 1] < hi) kl++;                    // the wire that holds entry hi - 1
      while (wf < p.wave.size() && p.wave[wf] < kf) wf++;
      size_t wl = wf;
      while (wl < p.wave.size() && p.wave[wl] <= kl) wl++;
      p.slices.push_back(Slice{(uint32_t)lo, (uint32_t)hi, (uint32_t)kf, (uint32_t)kl, (uint32_t)wf, (uint32_t)wl});
      lo = hi;
    }
    k = e < nv ? e + 1 : e;
  }
  return p;
}

}  // namespace srs
}  // namespace dg16
