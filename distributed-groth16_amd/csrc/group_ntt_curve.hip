// Per-curve object of the group transform (group_ntt.h): the two butterfly kernels for G1 and G2 of curve DG_CURVE, the
// stage loop, and the two G1 passes dg16_srs_prepare puts in front of a transform.
//
//   gntt_addsub_kernel   the lanes whose twiddle is 1: two additions, no table
//   gntt_mul_kernel      the other lanes, multiplication and additions fused: the table of b in the channel's workspace
//                        (pmul::GlobalTab), pmul::product_split, then a is loaded and both sums are formed and stored as
//                        XYZZ.  The same kernel with butterfly = 0 is a pass of products w^(e_step j) * scale * src[j]
//                        (the n^-1 of an inverse; the twisted half of a size-2m inverse).
//   fb_affine_kernel     (fixed_base_impl.h) brings the results back to affine, into the destination
//
// The tables are per slice (workspace slot 20 of the channel, as for points_mul_typed).  The XYZZ results of a WHOLE
// stage are kept -- lane j's sum at j, its difference at n / 2 + j, the layout of the destination -- and ONE batched
// inversion converts them: a conversion per slice is a launch whose time is the latency of one field inversion, and
// with two result runs per slice those launches cost a transform of 2^20 BLS12-381 points a sixth of its time.  The
// result and prefix buffers (4 + 1 field elements per point) are allocated per call and freed with it.
#include "group_ntt.h"

#ifndef DG_CURVE
#error "compile with -DDG_CURVE=<curve id>"
#endif

namespace dg16 {

const TwiddleSet& get_twiddles_any(Call& k, int curve, unsigned log_n, int inverse);     // ntt.hip

namespace {

using CT = CurveTypes<DG_CURVE>;
using Fr = CT::Fr;
using Fq = CT::Fq;
using Fq2 = CT::Fq2;

// acc[l] = a + b, acc[acc_hi + l] = a - b for the lane lane0 + l of stage `stage`.  stage = 0: a = src[j + a_off],
// b = src[j + b_off] and only the difference is stored, at acc[l].
template <class F>
__global__ void __launch_bounds__(64) gntt_addsub_kernel(const Affine<F>* __restrict__ src, unsigned log_n, unsigned stage,
                                                          size_t lane0, size_t cnt, size_t a_off, size_t b_off,
                                                          size_t acc_hi, XYZZ<F>* __restrict__ acc) {
  const size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= cnt) return;
  const size_t j = lane0 + l;
  size_t ia = j + a_off, ib = j + b_off;
  if (stage) {
    const gntt::Pair p = gntt::pair_of(log_n, stage, j);
    ia = p.a;
    ib = p.b;
  }
  pmul::PlainOps<F> inner;
  struct NoTab {} tab;
  gntt::PointOps<F, pmul::PlainOps<F>, NoTab> ops{inner, tab};
  XYZZ<F> sum, diff;
  gntt::butterfly_trivial(ops, fb_load(src + ia), fb_load(src + ib), &sum, &diff);
  if (stage) {
    fb_store(acc + l, sum);
    fb_store(acc + acc_hi + l, diff);
  } else {
    fb_store(acc + l, diff);
  }
}

// butterfly != 0: the lane lane0 + l of stage `stage`, w = w_n^tw from the split table.  butterfly == 0: acc[l] =
// w^(e_step * j) * scale * src[j], j = lane0 + l.  table: kTable * W * stride words; the difference goes to acc[acc_hi + l].
template <class F>
__global__ void __launch_bounds__(64) gntt_mul_kernel(const Affine<F>* __restrict__ src, unsigned log_n, unsigned stage,
                                                       int butterfly, size_t lane0, size_t cnt,
                                                       const Fr* __restrict__ tw_lo, const Fr* __restrict__ tw_hi,
                                                       unsigned lb, size_t e_step, const Fr* __restrict__ scale,
                                                       uint32_t* __restrict__ table, size_t stride, size_t acc_hi,
                                                       XYZZ<F>* __restrict__ acc) {
  const size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= cnt) return;
  const size_t j = lane0 + l;
  gntt::Pair p{j, j, 0, 0, e_step * j};
  if (butterfly) p = gntt::pair_of(log_n, stage, j);
  const Fr w = gntt::twiddle<Fr>(tw_lo, tw_hi, lb, p.tw, scale);
  gntt::Words8 k;
#pragma unroll
  for (int i = 0; i < 8; i++) k.l[i] = w.l[i];
  pmul::GlobalTab<F> tab{table + l, stride};
  pmul::PlainOps<F> inner;
  gntt::PointOps<F, pmul::PlainOps<F>, pmul::GlobalTab<F>> ops{inner, tab};
  const XYZZ<F> t = ops.mul(fb_load(src + p.b), k);
  if (!butterfly) {
    fb_store(acc + l, t);
    return;
  }
  XYZZ<F> sum, diff;
  gntt::combine(ops, fb_load(src + p.a), t, &sum, &diff);     // a is loaded after the product: it does not live through the loop
  fb_store(acc + l, sum);
  fb_store(acc + acc_hi + l, diff);
}

// the buffers of one call: the tables of a slice (workspace), the results and prefix products of `points` points (owned)
template <class F>
struct Work {
  uint32_t* table = nullptr;
  XYZZ<F>* acc = nullptr;
  F* pref = nullptr;
  size_t stride = 0, slice = 0;
  Work(Call& k, size_t lanes, size_t points, bool tables) {
    slice = slice_lanes(k.ctx->points_mul_slice);
    stride = launch_stride(lanes, slice);
    constexpr size_t W = sizeof(XYZZ<F>) / 4;
    if (tables) table = (uint32_t*)ws(k.c, 20, (size_t)pmul::kTable * W * stride * 4);
    DG_HIP(hipMalloc((void**)&acc, points * sizeof(XYZZ<F>)));
    DG_HIP(hipMalloc((void**)&pref, points * sizeof(F)));
  }
  ~Work() {      // (hipFree waits for the kernels that still use the buffers)
    if (acc) (void)hipFree(acc);
    if (pref) (void)hipFree(pref);
  }
  Work(const Work&) = delete;
  Work& operator=(const Work&) = delete;
};

// one pass of products: out[j] = w^(e_step j) * scale * src[j], j < n
template <class F>
void scale_pass(Call& k, const Work<F>& w, const Affine<F>* src, size_t n, const TwiddleSet& ts, size_t e_step,
                Affine<F>* out) {
  for (const gntt::Slice& sl : gntt::scale_slices(n, w.slice)) {
    hipLaunchKernelGGL(gntt_mul_kernel<F>, dim3((unsigned)((sl.cnt + 63) / 64)), dim3(64), 0, k.s(), src, 0u, 0u, 0,
                       sl.lo, sl.cnt, (const Fr*)ts.lo, (const Fr*)ts.hi, ts.lb, e_step, (const Fr*)ts.n_inv, w.table,
                       w.stride, (size_t)0, w.acc + sl.lo);
    DG_HIP(hipGetLastError());
  }
  fb_to_affine(k, w.acc, w.pref, n, out);
}

template <class F>
void* transform(Call& k, void* xv, void* yv, unsigned log_n, int inverse, bool scale) {
  if (!log_n) return xv;
  const size_t n = (size_t)1 << log_n, half = n >> 1;
  const bool scaled = inverse && scale;
  const TwiddleSet& ts = get_twiddles_any(k, DG_CURVE, log_n, inverse);
  const Work<F> w(k, scaled ? n : half, n, log_n > 1 || scaled);
  Affine<F>*src = (Affine<F>*)xv, *dst = (Affine<F>*)yv;
  k.begin_dominant();
  for (unsigned s = 1; s <= log_n; s++) {
    for (const gntt::Slice& sl : gntt::stage_slices(log_n, s, w.slice)) {
      const dim3 grid((unsigned)((sl.cnt + 63) / 64)), block(64);
      if (sl.kind == gntt::kAddSub)
        hipLaunchKernelGGL(gntt_addsub_kernel<F>, grid, block, 0, k.s(), (const Affine<F>*)src, log_n, s, sl.lo, sl.cnt,
                           (size_t)0, (size_t)0, half, w.acc + sl.lo);
      else
        hipLaunchKernelGGL(gntt_mul_kernel<F>, grid, block, 0, k.s(), (const Affine<F>*)src, log_n, s, 1, sl.lo, sl.cnt,
                           (const Fr*)ts.lo, (const Fr*)ts.hi, ts.lb, (size_t)0, (const Fr*)nullptr, w.table, w.stride,
                           half, w.acc + sl.lo);
      DG_HIP(hipGetLastError());
    }
    fb_to_affine(k, w.acc, w.pref, n, dst);       // results j and n / 2 + j are the destination's positions
    Affine<F>* t = src;
    src = dst;
    dst = t;
  }
  if (scaled) {
    scale_pass<F>(k, w, src, n, ts, 0, dst);
    src = dst;
  }
  k.end_dominant();
  return src;
}

}  // namespace

template <>
void* group_ntt_run<DG_CURVE>(Call& k, int group, void* x, void* y, unsigned log_n, int inverse, bool scale) {
  if (group == 1) return transform<Fq>(k, x, y, log_n, inverse, scale);
  return transform<Fq2>(k, x, y, log_n, inverse, scale);
}

template <>
void group_diff_run<DG_CURVE>(Call& k, const void* src, size_t a_off, size_t b_off, size_t n, void* out) {
  const Work<Fq> w(k, n, n, false);
  for (const gntt::Slice& sl : gntt::scale_slices(n, w.slice)) {
    hipLaunchKernelGGL(gntt_addsub_kernel<Fq>, dim3((unsigned)((sl.cnt + 63) / 64)), dim3(64), 0, k.s(),
                       (const Affine<Fq>*)src, 0u, 0u, sl.lo, sl.cnt, a_off, b_off, (size_t)0, w.acc + sl.lo);
    DG_HIP(hipGetLastError());
  }
  fb_to_affine(k, w.acc, w.pref, n, (Affine<Fq>*)out);
}

template <>
void group_twist_run<DG_CURVE>(Call& k, const void* src, unsigned log_m, void* out) {
  const size_t m = (size_t)1 << log_m;
  const TwiddleSet& ts = get_twiddles_any(k, DG_CURVE, log_m + 1, 1);
  const Work<Fq> w(k, m, m, true);
  scale_pass<Fq>(k, w, (const Affine<Fq>*)src, m, ts, 1, (Affine<Fq>*)out);
}

}  // namespace dg16
