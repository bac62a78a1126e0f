// Test-only: the stage schedule and the butterfly of distributed-groth16_amd/csrc/group_ntt.h compiled with the HOST
// compiler into a stand-alone program, so that the CPU tests (tests/test_group_ntt_plan.py) run the text the kernels
// run -- on field elements and on points -- and count its multiplications.  Never part of the product.
//
//   host_group_ntt plan                  checks the lane maps and the slices; prints "plan <slice> <log_n> <products>
//                                        <launches>" per case, exit status 1 with a message on the first violation
//   host_group_ntt run <in> <out>        transforms the cases of <in>, writes results and counts to <out>
//
// <in>:  u32 cases; per case u32 kind (0 = Fr elements, 1 = points), u32 id (kind 0: curve; kind 1: 2 * curve + group
//        - 1), u32 log_n, u32 inverse, u64 slice (the context's setting, 0 = default), the forward root w_n (32 bytes,
//        Montgomery), then 2^log_n elements (Montgomery Fr / affine points, identity = zeros).
// <out>: per case the 2^log_n results, then u64 x 4: products, additions, lanes of a multiplying launch with w = 1,
//        lanes of an add/sub launch with w != 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../distributed-groth16_amd/csrc/group_ntt.h"

using namespace dg16;

namespace {

struct Counts {
  uint64_t products = 0, additions = 0, trivial_in_mul = 0, twiddled_in_addsub = 0;
};

// the additive group of Fr: the transform of dg16_ntt itself
template <class Fr>
struct FieldOps {
  using In = Fr;
  using Out = Fr;
  using Scalar = gntt::Words8;
  Counts& c;
  Out lift(const In& a) { return a; }
  Out mul(const In& b, const Scalar& k) {
    c.products++;
    Fr w;
    memcpy(w.l, k.l, 32);
    return b * w.to_mont();
  }
  Out add(const Out& a, const Out& b) {
    c.additions++;
    return a + b;
  }
  Out neg(const Out& a) { return a.neg(); }
  In finish(const Out& a) { return a; }
};

template <class F>
struct CountTab {          // a product is counted where its table starts
  XYZZ<F> t[pmul::kTable];
  Counts& c;
  void put(int j, const XYZZ<F>& e) {
    if (j == 1) c.products++;
    t[j - 1] = e;
  }
  XYZZ<F> get(int j) const { return t[j - 1]; }
};
template <class F>
struct CountInner {
  Counts& c;
  XYZZ<F> dbl(const XYZZ<F>& a) { return a.dbl(); }
  XYZZ<F> add(const XYZZ<F>& a, const XYZZ<F>& b) { return a.add(b); }
};
template <class F>
struct GroupOps : gntt::PointOps<F, CountInner<F>, CountTab<F>> {
  using Base = gntt::PointOps<F, CountInner<F>, CountTab<F>>;
  Counts& c;
  GroupOps(CountInner<F>& i, CountTab<F>& t, Counts& c_) : Base{i, t}, c(c_) {}
  XYZZ<F> add(const XYZZ<F>& a, const XYZZ<F>& b) {       // the butterfly's own two additions
    c.additions++;
    return Base::add(a, b);
  }
  Affine<F> finish(const XYZZ<F>& a) { return a.to_affine(); }
};

// what group_ntt_curve.hip's transform() launches, lane by lane
template <class Ops, class Fr>
void transform(Ops& ops, std::vector<typename Ops::In>& x, unsigned log_n, int inverse, size_t ctx_slice, Fr root,
               Counts& c) {
  if (!log_n) return;
  const size_t n = (size_t)1 << log_n, slice = gntt::slice_lanes(ctx_slice);
  if (inverse) root = root.inv();
  const unsigned lb = log_n < 11 ? log_n : 11;       // the split of ctx.h's TwiddleSet
  std::vector<Fr> lo((size_t)1 << lb), hi((size_t)1 << (log_n - lb));
  lo[0] = Fr::one();
  for (size_t j = 1; j < lo.size(); j++) lo[j] = lo[j - 1] * root;
  Fr step = lo.back() * root;
  hi[0] = Fr::one();
  for (size_t j = 1; j < hi.size(); j++) hi[j] = hi[j - 1] * step;
  std::vector<typename Ops::In> y(n);
  for (unsigned s = 1; s <= log_n; s++) {
    for (const gntt::Slice& sl : gntt::stage_slices(log_n, s, slice)) {
      for (size_t l = 0; l < sl.cnt; l++) {
        const gntt::Pair p = gntt::pair_of(log_n, s, sl.lo + l);
        typename Ops::Out sum, diff;
        if (sl.kind == gntt::kMul) {
          if (p.tw == 0) c.trivial_in_mul++;
          const Fr w = gntt::twiddle<Fr>(lo.data(), hi.data(), lb, p.tw, (const Fr*)nullptr);
          gntt::Words8 k;
          memcpy(k.l, w.l, 32);
          gntt::butterfly(ops, x[p.a], x[p.b], k, &sum, &diff);
        } else {
          if (p.tw != 0) c.twiddled_in_addsub++;
          gntt::butterfly_trivial(ops, x[p.a], x[p.b], &sum, &diff);
        }
        y[p.lo] = ops.finish(sum);
        y[p.hi] = ops.finish(diff);
      }
    }
    x.swap(y);
  }
  if (inverse) {
    Fr nn = Fr::one();
    for (unsigned i = 0; i < log_n; i++) nn = nn + nn;
    const Fr n_inv = nn.inv();
    for (const gntt::Slice& sl : gntt::scale_slices(n, slice)) {
      for (size_t l = 0; l < sl.cnt; l++) {
        const Fr w = gntt::twiddle<Fr>(lo.data(), hi.data(), lb, 0, &n_inv);
        gntt::Words8 k;
        memcpy(k.l, w.l, 32);
        y[sl.lo + l] = ops.finish(ops.mul(x[sl.lo + l], k));
      }
    }
    x.swap(y);
  }
}

bool read_exact(FILE* f, void* p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

template <class Fr>
bool run_field(FILE* in, FILE* out, unsigned log_n, int inverse, size_t slice) {
  Fr root;
  std::vector<Fr> x((size_t)1 << log_n);
  if (!read_exact(in, &root, sizeof root) || !read_exact(in, x.data(), x.size() * sizeof(Fr))) return false;
  Counts c;
  FieldOps<Fr> ops{c};
  transform(ops, x, log_n, inverse, slice, root, c);
  fwrite(x.data(), sizeof(Fr), x.size(), out);
  fwrite(&c, sizeof c, 1, out);
  return true;
}
template <class F, class Fr>
bool run_points(FILE* in, FILE* out, unsigned log_n, int inverse, size_t slice) {
  Fr root;
  std::vector<Affine<F>> x((size_t)1 << log_n);
  if (!read_exact(in, &root, sizeof root) || !read_exact(in, x.data(), x.size() * sizeof(Affine<F>))) return false;
  Counts c;
  CountInner<F> inner{c};
  CountTab<F> tab{{}, c};
  GroupOps<F> ops(inner, tab, c);
  transform(ops, x, log_n, inverse, slice, root, c);
  fwrite(x.data(), sizeof(Affine<F>), x.size(), out);
  fwrite(&c, sizeof c, 1, out);
  return true;
}

int run(const char* in_path, const char* out_path) {
  FILE* in = fopen(in_path, "rb");
  FILE* out = fopen(out_path, "wb");
  if (!in || !out) return 2;
  uint32_t cases = 0;
  if (!read_exact(in, &cases, 4)) return 2;
  for (uint32_t i = 0; i < cases; i++) {
    uint32_t h[4];
    uint64_t slice;
    if (!read_exact(in, h, sizeof h) || !read_exact(in, &slice, 8) || h[2] > 16) return 2;
    bool ok = false;
    if (h[0] == 0) {
      if (h[1] == 0) ok = run_field<CurveTypes<0>::Fr>(in, out, h[2], (int)h[3], slice);
      else if (h[1] == 1) ok = run_field<CurveTypes<1>::Fr>(in, out, h[2], (int)h[3], slice);
      else if (h[1] == 2) ok = run_field<CurveTypes<2>::Fr>(in, out, h[2], (int)h[3], slice);
    } else {
      switch (h[1]) {
        case 0: ok = run_points<CurveTypes<0>::Fq, CurveTypes<0>::Fr>(in, out, h[2], (int)h[3], slice); break;
        case 1: ok = run_points<CurveTypes<0>::Fq2, CurveTypes<0>::Fr>(in, out, h[2], (int)h[3], slice); break;
        case 2: ok = run_points<CurveTypes<1>::Fq, CurveTypes<1>::Fr>(in, out, h[2], (int)h[3], slice); break;
        case 3: ok = run_points<CurveTypes<1>::Fq2, CurveTypes<1>::Fr>(in, out, h[2], (int)h[3], slice); break;
        case 4: ok = run_points<CurveTypes<2>::Fq, CurveTypes<2>::Fr>(in, out, h[2], (int)h[3], slice); break;
        case 5: ok = run_points<CurveTypes<2>::Fq2, CurveTypes<2>::Fr>(in, out, h[2], (int)h[3], slice); break;
        default: break;
      }
    }
    if (!ok) return 2;
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 2;
}

#define PLAN_CHECK(cond, what)                                                                          \
  do {                                                                                                  \
    if (!(cond)) {                                                                                      \
      printf("plan violation: %s (slice %zu, log_n %u, stage %u, lane %zu)\n", what, ctx_slice, log_n, s, j); \
      return 1;                                                                                         \
    }                                                                                                   \
  } while (0)

// every lane of every stage exactly once, all of one kind per launch, reading every source position once and
// writing every destination position once
int plan_case(size_t ctx_slice, unsigned log_n) {
  const size_t n = (size_t)1 << log_n, half = n >> 1, slice = gntt::slice_lanes(ctx_slice);
  size_t products = 0, launches = 0;
  for (unsigned s = 1; s <= log_n; s++) {
    std::vector<uint8_t> lane(half, 0), rd(n, 0), wr(n, 0);
    for (const gntt::Slice& sl : gntt::stage_slices(log_n, s, slice)) {
      size_t j = sl.lo;
      launches++;
      PLAN_CHECK(sl.cnt >= 1 && sl.cnt <= slice && sl.cnt <= gntt::launch_stride(half, slice), "slice size");
      PLAN_CHECK(sl.lo + sl.cnt <= half, "slice range");
      for (; j < sl.lo + sl.cnt; j++) {
        const gntt::Pair p = gntt::pair_of(log_n, s, j);
        PLAN_CHECK(!lane[j], "lane twice");
        lane[j] = 1;
        PLAN_CHECK(gntt::launch_of(log_n, s, j) == sl.kind, "lane in a launch of the other kind");
        PLAN_CHECK((p.tw == 0) == (sl.kind == gntt::kAddSub), "twiddle 1 in a multiplying launch or the reverse");
        PLAN_CHECK(p.tw < half, "twiddle index");
        PLAN_CHECK(p.a < n && p.b < n && p.lo < n && p.hi < n, "position out of range");
        PLAN_CHECK(p.a != p.b && p.lo != p.hi, "pair not distinct");
        PLAN_CHECK(!rd[p.a] && !rd[p.b] && !wr[p.lo] && !wr[p.hi], "position twice");
        rd[p.a] = rd[p.b] = wr[p.lo] = wr[p.hi] = 1;
        if (sl.kind == gntt::kMul) products++;
      }
    }
    for (size_t j = 0; j < half; j++) PLAN_CHECK(lane[j], "lane missing");
  }
  size_t covered = 0;
  for (const gntt::Slice& sl : gntt::scale_slices(n, slice)) {
    if (sl.lo != covered || sl.cnt < 1 || sl.cnt > slice || sl.cnt > gntt::launch_stride(n, slice)) {
      printf("plan violation: scale slices (slice %zu, log_n %u)\n", ctx_slice, log_n);
      return 1;
    }
    covered += sl.cnt;
  }
  if (covered != n || products != gntt::forward_products(log_n)) {
    printf("plan violation: totals (slice %zu, log_n %u)\n", ctx_slice, log_n);
    return 1;
  }
  printf("plan %zu %u %zu %zu\n", ctx_slice, log_n, products, launches);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "plan")) {
    const size_t slices[3] = {64, 192, 0};
    for (size_t sl : slices)
      for (unsigned log_n = 0; log_n <= (sl ? 12u : 18u); log_n++)
        if (plan_case(sl, log_n)) return 1;
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
  fprintf(stderr, "usage: host_group_ntt plan | run <in> <out>\n");
  return 2;
}
