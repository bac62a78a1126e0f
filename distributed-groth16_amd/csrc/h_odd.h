// The index rule of dg16_ext_wit_h with DG16_F_H_ODD: which of the king's gathered packed elements, and which row of
// the unpack matrix, give the evaluation that position i of output chunk c needs.  Host and device text, no field
// arithmetic: tests/host_arith/host_h_odd.cpp compiles it into a stand-alone program.
//
// After the six transform rounds every party holds 2m/l shares per vector (p, q, w); packed element e shares the l
// natural-order evaluations e*l .. e*l + l - 1 of the 2m-point domain, and row r of the unpack matrix recovers
// evaluation e*l + r.  The witness map keeps the odd evaluations: h_k = p[2k+1] q[2k+1] - w[2k+1], k < m.  The output
// is pack_vec's (utils/pack.rs:4-16): chunk c < m/l holds h_k for k = c*l + i, i < l.  So position i of chunk c reads
// evaluation 2(c*l + i) + 1 = (2c)*l + (2i + 1):
//
//   l >= 2   2i + 1 < 2l: element 2c + (2i+1)/l, row (2i+1) mod l.  A chunk reads exactly its two elements 2c and
//            2c + 1, and of each only the odd rows 1, 3, .., l-1: the even rows are never formed.
//   l == 1   one evaluation per element and one row: element 2c + 1, row 0.  Element 2c is not read at all.
//
// The reference's `s1.swap(i, i*l + t)`, t = l - 1 (ext_wit.rs:74-76), is this rule at l = 2 alone: there
// i*l + t = 2i + 1.  At l = 1 it keeps evaluation i, at l = 4, 8 it reads evaluation i*l + l - 1 up to l*m - 1 >= 2m.
#pragma once
#include <stddef.h>

#ifndef DG_HD      // fp.h's idiom, word for word; under hipcc the includer brings the HIP runtime header (fp.h does)
#if defined(__HIPCC__)
#define DG_HD __host__ __device__ __forceinline__
#else
#define DG_HD inline
#endif
#endif

namespace dg16 {
namespace hodd {

struct Source {
  size_t elem;    // packed element of the 2m/l a party holds per vector
  unsigned row;   // row of the unpack matrix ([l][n])
};

DG_HD Source source(unsigned l, size_t c, unsigned i) {
  if (l == 1) return Source{2 * c + 1, 0u};
  const unsigned pos = 2 * i + 1;   // among the 2l evaluations of elements 2c and 2c + 1
  return Source{2 * c + pos / l, pos % l};
}

// the evaluation (of 2m) that (elem, row) is: what the rule must make 2(c*l + i) + 1
DG_HD size_t evaluation(unsigned l, const Source& s) { return s.elem * l + s.row; }

}  // namespace hodd
}  // namespace dg16
