// Test-only: the schedule, the table build and the combine loop of distributed-groth16_amd/csrc/pss_pack.h compiled with
// the HOST compiler, so that the CPU tests (tests/test_pss_pack_host.py) run exactly the text the kernels run and count
// its group operations.  Never part of the product.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../distributed-groth16_amd/csrc/pss_pack.h"

using namespace dg16;

namespace {

// the tables of one chunk: l x kTable entries
template <class F>
struct LocalTabs {
  std::vector<XYZZ<F>> t;
  explicit LocalTabs(unsigned l) : t((size_t)l * ppack::kTable) {}
  struct One {
    XYZZ<F>* p;
    void put(int j, const XYZZ<F>& e) { p[j - 1] = e; }
  };
  One of(int c) { return One{&t[(size_t)c * ppack::kTable]}; }
  XYZZ<F> get(int c, int j) const { return t[(size_t)c * ppack::kTable + j - 1]; }
};

template <class F>
struct CountOps {
  uint32_t n[2] = {0, 0};   // doublings, additions
  XYZZ<F> dbl(const XYZZ<F>& a) { n[0]++; return a.dbl(); }
  XYZZ<F> add(const XYZZ<F>& a, const XYZZ<F>& b) { n[1]++; return a.add(b); }
};

template <class F>
int schedule(int split, unsigned l, const uint32_t* M, int8_t* digits, int* lens) {
  ppack::Schedule s;
  ppack::make_schedule<F>(M, l, split != 0, s);
  const int parts = (int)l * s.dim;
  for (unsigned r = 0; r < s.n; r++) {
    lens[r] = s.len[r];
    for (int p = 0; p < parts; p++)
      for (int i = 0; i < ppack::kMaxRows; i++) {
        int d = 0;
        if (i < s.len[r]) d = pscale::row_digit(s.rows[((size_t)r * s.stride + i) * s.words + p / 4], p % 4);
        digits[((size_t)r * parts + p) * ppack::kMaxRows + i] = (int8_t)d;
      }
  }
  return s.dim;
}

// shares [n][chunks]; tcounts [chunks * l][2], ccounts [n][chunks][2]
template <class F>
void pack(int split, unsigned l, const uint32_t* M, const void* points, size_t n_points, void* shares, uint32_t* tcounts,
          uint32_t* ccounts) {
  const Affine<F>* p = (const Affine<F>*)points;
  Affine<F>* o = (Affine<F>*)shares;
  ppack::Schedule s;
  ppack::make_schedule<F>(M, l, split != 0, s);
  const size_t chunks = ppack::chunks_of(n_points, l);
  for (size_t e = 0; e < chunks; e++) {
    LocalTabs<F> tabs(l);
    for (unsigned c = 0; c < l; c++) {
      const size_t idx = e * l + c;
      CountOps<F> ops;
      auto tab = tabs.of((int)c);
      ppack::build_odd_table(idx < n_points ? p[idx] : Affine<F>::inf(), ops, tab);
      memcpy(tcounts + 2 * idx, ops.n, sizeof ops.n);
    }
    for (unsigned r = 0; r < s.n; r++) {
      CountOps<F> ops;
      const uint32_t* rows = s.rows.data() + (size_t)r * s.stride * s.words;
      XYZZ<F> acc;
      if (s.dim == 1) acc = ppack::combine<1, F>(rows, s.len[r], s.words, ops, tabs);
      else acc = ppack::combine<GlvOf<F>::DIM, F>(rows, s.len[r], s.words, ops, tabs);
      o[(size_t)r * chunks + e] = acc.to_affine();
      memcpy(ccounts + 2 * ((size_t)r * chunks + e), ops.n, sizeof ops.n);
    }
  }
}

template <class F>
struct ScaleTab {
  XYZZ<F> t[pscale::kTable];
  void put(int j, const XYZZ<F>& e) { t[j - 1] = e; }
  XYZZ<F> get(int j) const { return t[j - 1]; }
};

// the operations of ONE pscale::product for the constant k (table included)
template <class F>
void one_product(int split, const void* point, const uint32_t* k, uint32_t* counts) {
  pscale::Schedule s;
  pscale::make_schedule<F>(k, split != 0, s);
  ScaleTab<F> tab;
  CountOps<F> ops;
  const Affine<F> p = *(const Affine<F>*)point;
  if (s.dim == 1) pscale::product<1, F>(p, s.rows, s.len, ops, tab);
  else pscale::product<GlvOf<F>::DIM, F>(p, s.rows, s.len, ops, tab);
  memcpy(counts, ops.n, sizeof ops.n);
}

}  // namespace

#define BY_GROUP(gid, CALL)                                           \
  switch (gid) {                                                      \
    case 0: { using F = CurveTypes<0>::Fq; CALL; break; }             \
    case 1: { using F = CurveTypes<0>::Fq2; CALL; break; }            \
    case 2: { using F = CurveTypes<1>::Fq; CALL; break; }             \
    case 3: { using F = CurveTypes<1>::Fq2; CALL; break; }            \
    case 4: { using F = CurveTypes<2>::Fq; CALL; break; }             \
    case 5: { using F = CurveTypes<2>::Fq2; CALL; break; }            \
    default: return -1;                                               \
  }

extern "C" {

// width, table entries, positions of a part
void hp_params(int* out) { out[0] = ppack::kWidth; out[1] = ppack::kTable; out[2] = ppack::kMaxRows; }
// gid = 2 * curve + group - 1; M: [4 l][l] canonical scalars of 8 words.  Returns the parts per scalar (1, 2, 4);
// digits: [4 l][l * parts][kMaxRows] signed digits (the parts' signs folded in), lens: [4 l] positions in use
int hp_schedule(int gid, int split, unsigned l, const uint32_t* M, int8_t* digits, int* lens) {
  BY_GROUP(gid, return schedule<F>(split, l, M, digits, lens));
  return -1;
}
// LAMBDA of the group's split (8 words): k = sum_j part_j LAMBDA^j mod r
int hp_lambda(int gid, uint32_t* out) {
  BY_GROUP(gid, memcpy(out, GlvOf<F>::C::LAMBDA, 32));
  return 0;
}
int hp_pack(int gid, int split, unsigned l, const uint32_t* M, const void* points, size_t n_points, void* shares,
            uint32_t* tcounts, uint32_t* ccounts) {
  BY_GROUP(gid, pack<F>(split, l, M, points, n_points, shares, tcounts, ccounts));
  return 0;
}
int hp_one_product(int gid, int split, const void* point, const uint32_t* k, uint32_t* counts) {
  BY_GROUP(gid, one_product<F>(split, point, k, counts));
  return 0;
}
size_t hp_slice_chunks(size_t slice, unsigned n) { return ppack::slice_chunks(slice, n); }

}  // extern "C"
