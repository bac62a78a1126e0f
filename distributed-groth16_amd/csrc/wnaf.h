// The sliding-window pieces shared by the calls whose lanes all walk the SAME digits: points_scale.h (one scalar, w = 5)
// and pss_pack.h (the constants of a pack matrix, w = 7).  The width-w non-adjacent form of an integer has digits odd or
// zero, |d| < 2^(w-1), and two non-zero digits at least w positions apart; its table holds the odd multiples only.
// The loops that walk the digits stay with their callers (pscale::product, ppack::combine).  Host and device text.
#pragma once
#include "ec.h"

namespace dg16 {
namespace wnaf {

constexpr int kMaxRows = 260;                  // positions of an integer below 2^255: at most 256

// the width-W NAF of the 8-word integer m, negated where neg, into digits[0 .. kMaxRows), one signed digit per
// position; returns its length (the highest non-zero position + 1; 0 for m = 0)
template <int W>
inline int recode_wnaf(const uint32_t* m, bool neg, int8_t* digits) {
  static_assert(W >= 2 && W <= 8, "a digit is a signed byte");
  uint32_t k[9] = {m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], 0};
  int len = 0;
  for (int pos = 0; pos < kMaxRows; pos++) {
    digits[pos] = 0;
    uint32_t any = 0;
    for (int j = 0; j < 9; j++) any |= k[j];
    if (!any) continue;
    if (k[0] & 1u) {
      int d = (int)(k[0] & ((1u << W) - 1u));
      if (d >= (1 << (W - 1))) d -= 1 << W;
      if (d > 0) {
        k[0] -= (uint32_t)d;                          // the low w bits are d: no borrow
      } else {
        uint64_t c = (uint64_t)(-d);
        for (int j = 0; j < 9 && c; j++) {
          c += k[j];
          k[j] = (uint32_t)c;
          c >>= 32;
        }
      }
      digits[pos] = (int8_t)(neg ? -d : d);
      len = pos + 1;
    }
    for (int j = 0; j < 9; j++) k[j] = (k[j] >> 1) | (j + 1 < 9 ? k[j + 1] << 31 : 0u);
  }
  return len;
}

// byte `part` of a 32-bit word of a schedule: the signed digit of that part
DG_HD int row_digit(uint32_t row, int part) { return (int)(int8_t)(row >> (8 * part)); }

// T[j] = (2 j - 1) p, j = 1 .. TABLE: one doubling, TABLE - 1 additions
template <int TABLE, class F, class Ops, class Tab>
DG_HD void build_odd_table(const Affine<F>& p, Ops& ops, Tab& tab) {
  XYZZ<F> t = XYZZ<F>::from_affine(p);
  tab.put(1, t);
  const XYZZ<F> two = ops.dbl(t);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int j = 2; j <= TABLE; j++) {
    t = ops.add(t, two);
    tab.put(j, t);
  }
}

}  // namespace wnaf
}  // namespace dg16
