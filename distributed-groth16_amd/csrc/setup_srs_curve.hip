// Per-curve object of dg16_groth16_setup_srs: the Groth16 key "in the exponent", from the Lagrange-basis points of a
// powers-of-tau ceremony instead of the trapdoor.  Every query is a sparse TRANSPOSED matrix times a vector of points,
//
//   out[k] = sum over the entries (i, k, v) of M of v * P[i]            (setup_wire_kernel's sum, over a group)
//
// for the matrices and point tables of the output (a_query: A x lag_g1; b_g1_query: B x lag_g1; b_g2_query: B x lag_g2;
// K = A x beta_lag_g1 + B x alpha_lag_g1 + C x lag_g1, split into gamma_abc_g1 | l_query; an output that A enters has
// one more term P[nc + k] for the instance wires k < ni).
//
//   transposes   setup_transpose.h, shared with the trapdoor generator: the three matrices by wire
//   segments     the entries of wire k of one output are numbered consecutively: seg_ptr = scan of the segment lengths
//                (srs_seg_len_kernel + setup_scan_kernel).  Nothing per entry is stored: a lane finds the wire of its
//                entry by binary search in seg_ptr and the (matrix, position) by walking the wire's <= 3 columns.
//   plan         setup_srs_plan.h on the host copy of seg_ptr: the path of every wire and the term slices
//   terms        srs_term_kernel, one lane per entry of a slice: gathers P[t_row] and the coefficient; v = 0 (or the
//                identity) gives the identity, v = 1 the point, v = r - 1 its negative -- no multiplication; any other
//                entry is appended to the slice's multiplication list.  srs_mul_kernel, one lane per list entry, runs
//                points_mul.h's loops (regular signed windows, the endomorphism split where it is allowed, the
//                word-major table) and writes the product into the entry's term slot.  The list keeps the lanes that
//                multiply together: a wave of +-1 terms never waits for a multiplication.
//   sums         srs_lane_sum_kernel (one lane per wire of the slice, segments below kWaveFrom) and srs_wave_sum_kernel
//                (one wave per wire of the slice's share of the wave list: strided partial sums, then a tree over the
//                lanes through LDS) add the slice's part of a segment into the wire's XYZZ accumulator.  All additions
//                are the complete XYZZ::add: duplicate entries (a doubling) and cancelling coefficients do occur.
//   affine       fb_affine_kernel's batched inversion over the accumulators
//   MSM wires    a segment of kMsmFrom entries or more (the constant-one wire of a real circuit) is gathered into a
//                base and a scalar array and handed to msm_launch; its affine result overwrites out[k]
#include <string.h>

#include <vector>

#include "points_mul.h"
#include "setup.h"
#include "setup_srs_plan.h"
#include "setup_transpose.h"

#ifndef DG_CURVE
#error "compile with -DDG_CURVE=<curve id>"
#endif

namespace dg16 {
namespace {

using CT = CurveTypes<DG_CURVE>;
using Fr = CT::Fr;
using TCsr = TCsrT<Fr>;

constexpr size_t kSrsSliceDefault = (size_t)1 << 17;     // terms per launch group (bounds the term buffer and the table)

template <class F>
struct SrsOutput {          // one output: its matrices by wire, each with the point table its rows index
  TCsr m[3];
  const Affine<F>* tab[3];
  int nm;
  const Affine<F>* inst;    // the table of the instance term (entry nc + k, coefficient 1, k < ni), or null
  unsigned nc, ni;
};

template <class F>
__global__ void __launch_bounds__(256) srs_seg_len_kernel(SrsOutput<F> o, size_t nv, unsigned* __restrict__ len) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nv) return;
  unsigned c[3] = {0, 0, 0};
  for (int j = 0; j < o.nm; j++) c[j] = o.m[j].ptr[k + 1] - o.m[j].ptr[k];
  len[k] = (unsigned)srs::segment_len(c[0], c[1], c[2], o.inst && k < o.ni);
}

// the wire k0 <= k <= k1 whose segment holds entry e (seg_ptr[k0] <= e < seg_ptr[k1 + 1]): the largest k with
// seg_ptr[k] <= e -- empty wires behind the holder start beyond e
__device__ __forceinline__ unsigned srs_wire_of(const unsigned* __restrict__ seg_ptr, unsigned k0, unsigned k1,
                                                unsigned e) {
  unsigned lo = k0, hi = k1;
  while (lo < hi) {
    const unsigned mid = lo + (hi - lo + 1) / 2;
    if (seg_ptr[mid] <= e) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// entry number off of wire k's segment: the point and the coefficient (Montgomery form).  off < the segment's length.
template <class F>
__device__ __forceinline__ void srs_entry(const SrsOutput<F>& o, unsigned k, unsigned off, Affine<F>& P, Fr& v) {
  for (int j = 0; j < o.nm; j++) {
    const unsigned b = o.m[j].ptr[k], cnt = o.m[j].ptr[k + 1] - b;
    if (off < cnt) {
      P = fb_load(o.tab[j] + o.m[j].t_row[b + off]);       // t_row < nc <= m: inside the table
      v = fb_load(o.m[j].coeff + o.m[j].t_src[b + off]);
      return;
    }
    off -= cnt;
  }
  P = fb_load(o.inst + (size_t)o.nc + k);                   // k < ni, nc + ni <= m
  v = Fr::one();
}

// term[i] for the entries lo + i < hi of one slice, or an entry of the multiplication list
template <class F>
__global__ void __launch_bounds__(64) srs_term_kernel(SrsOutput<F> o, const unsigned* __restrict__ seg_ptr,
                                                       srs::Slice sl, XYZZ<F>* __restrict__ term,
                                                       unsigned* __restrict__ mul_count, unsigned* __restrict__ mul_dst,
                                                       Affine<F>* __restrict__ mul_pt, Fr* __restrict__ mul_k) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= sl.hi - sl.lo) return;
  const unsigned e = sl.lo + i;
  const unsigned k = srs_wire_of(seg_ptr, sl.k0, sl.k1, e);
  Affine<F> P;
  Fr v;
  srs_entry(o, k, e - seg_ptr[k], P, v);
  const Fr one = Fr::one();
  if (v.is_zero() || P.is_inf()) {
    fb_store(term + i, XYZZ<F>::inf());
  } else if (v == one) {
    fb_store(term + i, XYZZ<F>::from_affine(P));
  } else if (v == one.neg()) {
    fb_store(term + i, XYZZ<F>::from_affine(P).neg());
  } else {
    const unsigned pos = atomicAdd(mul_count, 1u);          // < hi - lo: one slot per entry at most
    mul_dst[pos] = i;
    fb_store(mul_pt + pos, P);
    fb_store(mul_k + pos, v.from_mont());
  }
}

// term[mul_dst[i]] = mul_k[i] * mul_pt[i], i < *mul_count <= stride; table: kTable * W * stride words
template <class F, bool SPLIT>
__global__ void __launch_bounds__(64) srs_mul_kernel(const unsigned* __restrict__ mul_count,
                                                      const unsigned* __restrict__ mul_dst,
                                                      const Affine<F>* __restrict__ mul_pt, const Fr* __restrict__ mul_k,
                                                      uint32_t* __restrict__ table, size_t stride,
                                                      XYZZ<F>* __restrict__ term) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= *mul_count) return;
  const Fr s = fb_load(mul_k + i);
  const Affine<F> p = fb_load(mul_pt + i);
  pmul::GlobalTab<F> tab{table + i, stride};
  pmul::PlainOps<F> ops;
  XYZZ<F> acc;
  if constexpr (SPLIT) acc = pmul::product_split<F>(p, s.l, ops, tab);
  else acc = pmul::product_plain<F>(p, s.l, ops, tab);
  fb_store(term + mul_dst[i], acc);
}

// acc[k] += the slice's terms of wire k, k0 <= k <= k1, for the wires on the lane path
template <class F>
__global__ void __launch_bounds__(64) srs_lane_sum_kernel(const unsigned* __restrict__ seg_ptr, srs::Slice sl,
                                                           const XYZZ<F>* __restrict__ term, XYZZ<F>* __restrict__ acc) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g > sl.k1 - sl.k0) return;
  const unsigned k = sl.k0 + (unsigned)g;
  unsigned s = seg_ptr[k], e = seg_ptr[k + 1];
  if (srs::path_of(e - s) != srs::kPathLane) return;
  s = s < sl.lo ? sl.lo : s;
  e = e > sl.hi ? sl.hi : e;
  if (s >= e) return;
  XYZZ<F> a = fb_load(acc + k);
#pragma unroll 1
  for (unsigned p = s; p < e; p++) a = a.add(fb_load(term + (p - sl.lo)));
  fb_store(acc + k, a);
}

// acc[k] += the slice's terms of wire k = wave[blockIdx.x]: one wave per wire
template <class F>
__global__ void __launch_bounds__(64) srs_wave_sum_kernel(const unsigned* __restrict__ seg_ptr,
                                                           const unsigned* __restrict__ wave, srs::Slice sl,
                                                           const XYZZ<F>* __restrict__ term, XYZZ<F>* __restrict__ acc) {
  constexpr unsigned Q = sizeof(XYZZ<F>) / 16;
  __shared__ uint4 sh[(srs::kWave / 2) * Q];
  XYZZ<F>* shp = reinterpret_cast<XYZZ<F>*>(sh);
  const unsigned lane = threadIdx.x;
  const unsigned k = wave[blockIdx.x];
  unsigned s = seg_ptr[k], e = seg_ptr[k + 1];
  s = s < sl.lo ? sl.lo : s;
  e = e > sl.hi ? sl.hi : e;                  // (uniform over the block: every lane reaches every barrier)
  XYZZ<F> a = XYZZ<F>::inf();
#pragma unroll 1
  for (unsigned p = s + lane; p < e; p += srs::kWave) a = a.add(fb_load(term + (p - sl.lo)));
#pragma unroll 1
  for (unsigned off = srs::kWave / 2; off >= 1; off >>= 1) {
    if (lane >= off && lane < 2 * off) fb_store(shp + (lane - off), a);
    __syncthreads();
    if (lane < off) a = a.add(fb_load(shp + lane));
    __syncthreads();
  }
  if (lane == 0) fb_store(acc + k, fb_load(acc + k).add(a));
}

// the segment of an MSM wire as the two operands of msm_launch
template <class F>
__global__ void __launch_bounds__(256) srs_gather_kernel(SrsOutput<F> o, unsigned k, unsigned len,
                                                          Affine<F>* __restrict__ bases, Fr* __restrict__ scalars) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= len) return;
  Affine<F> P;
  Fr v;
  srs_entry(o, k, i, P, v);
  fb_store(bases + i, P);
  fb_store(scalars + i, v);
}

// out[k] = the sum of wire k's segment, k < nv (affine)
template <class F>
void srs_output(Call& k, const SrsOutput<F>& o, size_t nv, int group, bool in_subgroup, Affine<F>* out) {
  if (!nv) return;
  // ---- segments and the plan --------------------------------------------------------------------------------------
  DevBuf len(nv * sizeof(unsigned)), scratch(nv * sizeof(unsigned)), seg(((size_t)nv + 1) * sizeof(unsigned));
  hipLaunchKernelGGL(srs_seg_len_kernel<F>, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, k.s(), o, nv,
                     len.as<unsigned>());
  hipLaunchKernelGGL(setup_scan_kernel, dim3(1), dim3(1024), 0, k.s(), len.as<unsigned>(), nv, seg.as<unsigned>(),
                     scratch.as<unsigned>());
  DG_HIP(hipGetLastError());
  std::vector<uint32_t> seg_host(nv + 1);
  DG_HIP(hipMemcpyAsync(seg_host.data(), seg.p, (nv + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, k.s()));
  DG_HIP(hipStreamSynchronize(k.s()));
  const size_t slice = k.ctx->points_mul_slice ? k.ctx->points_mul_slice : kSrsSliceDefault;
  const srs::Plan plan = srs::make_plan(seg_host.data(), nv, slice);
  const unsigned* seg_ptr = seg.as<unsigned>();

  // ---- lane and wave wires: terms per slice, partial sums into the accumulators ----------------------------------
  size_t cap = 0;
  for (const srs::Slice& sl : plan.slices) cap = cap < (size_t)(sl.hi - sl.lo) ? sl.hi - sl.lo : cap;
  cap = (cap + 63) / 64 * 64;
  constexpr size_t W = sizeof(XYZZ<F>) / 4;
  DevBuf acc(nv * sizeof(XYZZ<F>));
  DG_HIP(hipMemsetAsync(acc.p, 0, nv * sizeof(XYZZ<F>), k.s()));       // zz = 0: the identity
  if (!plan.slices.empty()) {
    DevBuf term(cap * sizeof(XYZZ<F>)), table((size_t)pmul::kTable * W * cap * 4), mul_dst(cap * sizeof(unsigned)),
        mul_pt(cap * sizeof(Affine<F>)), mul_k(cap * sizeof(Fr)), counts(plan.slices.size() * sizeof(unsigned)),
        wave(plan.wave.size() * sizeof(unsigned));
    DG_HIP(hipMemsetAsync(counts.p, 0, plan.slices.size() * sizeof(unsigned), k.s()));
    if (!plan.wave.empty())
      DG_HIP(hipMemcpyAsync(wave.p, plan.wave.data(), plan.wave.size() * sizeof(unsigned), hipMemcpyHostToDevice, k.s()));
    const bool split = pmul::may_split<F>(in_subgroup);
    k.begin_dominant();
    for (size_t j = 0; j < plan.slices.size(); j++) {
      const srs::Slice& sl = plan.slices[j];
      const dim3 grid((sl.hi - sl.lo + 63) / 64), block(64);
      unsigned* cnt = counts.as<unsigned>() + j;
      hipLaunchKernelGGL(srs_term_kernel<F>, grid, block, 0, k.s(), o, seg_ptr, sl, term.as<XYZZ<F>>(), cnt,
                         mul_dst.as<unsigned>(), mul_pt.as<Affine<F>>(), mul_k.as<Fr>());
      if (split)
        hipLaunchKernelGGL((srs_mul_kernel<F, true>), grid, block, 0, k.s(), cnt, mul_dst.as<unsigned>(),
                           mul_pt.as<Affine<F>>(), mul_k.as<Fr>(), table.as<uint32_t>(), cap, term.as<XYZZ<F>>());
      else
        hipLaunchKernelGGL((srs_mul_kernel<F, false>), grid, block, 0, k.s(), cnt, mul_dst.as<unsigned>(),
                           mul_pt.as<Affine<F>>(), mul_k.as<Fr>(), table.as<uint32_t>(), cap, term.as<XYZZ<F>>());
      hipLaunchKernelGGL(srs_lane_sum_kernel<F>, dim3((sl.k1 - sl.k0) / 64 + 1), block, 0, k.s(), seg_ptr, sl,
                         term.as<XYZZ<F>>(), acc.as<XYZZ<F>>());
      if (sl.w1 > sl.w0)
        hipLaunchKernelGGL(srs_wave_sum_kernel<F>, dim3(sl.w1 - sl.w0), block, 0, k.s(), seg_ptr,
                           wave.as<unsigned>() + sl.w0, sl, term.as<XYZZ<F>>(), acc.as<XYZZ<F>>());
      DG_HIP(hipGetLastError());
    }
    k.end_dominant();
    DG_HIP(hipStreamSynchronize(k.s()));      // the plan's host vector and the slice buffers end here
  }
  // ---- affine ---------------------------------------------------------------------------------------------------
  {
    const size_t batch = nv < kFbBatch ? nv : kFbBatch;
    DevBuf pref(batch * sizeof(F));
    for (size_t lo = 0; lo < nv; lo += kFbBatch) {
      const size_t cnt = nv - lo < kFbBatch ? nv - lo : kFbBatch;
      fb_to_affine(k, acc.as<XYZZ<F>>() + lo, pref.as<F>(), cnt, out + lo);
    }
    DG_HIP(hipStreamSynchronize(k.s()));
  }
  // ---- MSM wires ------------------------------------------------------------------------------------------------
  if (!plan.msm.empty()) {
    size_t longest = 0;
    for (uint32_t w : plan.msm) longest = longest < (size_t)(seg_host[w + 1] - seg_host[w]) ? seg_host[w + 1] - seg_host[w] : longest;
    DevBuf bases(longest * sizeof(Affine<F>)), scalars(longest * sizeof(Fr));
    for (uint32_t w : plan.msm) {
      const unsigned n = seg_host[w + 1] - seg_host[w];
      hipLaunchKernelGGL(srs_gather_kernel<F>, dim3((n + 255) / 256), dim3(256), 0, k.s(), o, w, n,
                         bases.as<Affine<F>>(), scalars.as<Fr>());
      DG_HIP(hipGetLastError());
      msm_launch(k, DG_CURVE, group, bases.p, scalars.p, n, 1u | (in_subgroup ? 2u : 0u), true, out + w);
    }
    DG_HIP(hipStreamSynchronize(k.s()));
  }
}

}  // namespace

template <>
void groth16_setup_srs_run<DG_CURVE>(Call& k, const SrsSetupArgs& s) {
  using Fq = CT::Fq;
  using Fq2 = CT::Fq2;
  const size_t nc = s.nc, ni = s.ni, nv = s.nv;
  DevBuf flagb(16);
  unsigned* flag = flagb.as<unsigned>();
  DG_HIP(hipMemsetAsync(flag, 0, 16, k.s()));
  Transposes<Fr> tr(k, s.row_ptr, s.col, s.coeff, s.nnz, nc, nv, flag);
  DG_HIP(hipGetLastError());
  DG_HIP(hipStreamSynchronize(k.s()));
  unsigned bad = 0;
  DG_HIP(hipMemcpy(&bad, flag, sizeof bad, hipMemcpyDeviceToHost));
  DG_REQUIRE(!bad, DG16_ERR_BAD_ARG,
             "dg16_groth16_setup_srs: matrix entry out of range (column >= num_vars or bad row_ptr)");
  const TCsr* t = tr.t;
  const Affine<Fq>* lag1 = (const Affine<Fq>*)s.lag_g1;
  const Affine<Fq>* alag = (const Affine<Fq>*)s.alpha_lag_g1;
  const Affine<Fq>* blag = (const Affine<Fq>*)s.beta_lag_g1;
  const Affine<Fq2>* lag2 = (const Affine<Fq2>*)s.lag_g2;

  SrsOutput<Fq> a{};
  a.m[0] = t[0]; a.tab[0] = lag1; a.nm = 1; a.inst = lag1; a.nc = (unsigned)nc; a.ni = (unsigned)ni;
  srs_output<Fq>(k, a, nv, 1, s.in_subgroup, (Affine<Fq>*)s.a_query);

  SrsOutput<Fq> b1{};
  b1.m[0] = t[1]; b1.tab[0] = lag1; b1.nm = 1; b1.inst = nullptr; b1.nc = (unsigned)nc; b1.ni = (unsigned)ni;
  srs_output<Fq>(k, b1, nv, 1, s.in_subgroup, (Affine<Fq>*)s.b_g1_query);

  SrsOutput<Fq2> b2{};
  b2.m[0] = t[1]; b2.tab[0] = lag2; b2.nm = 1; b2.inst = nullptr; b2.nc = (unsigned)nc; b2.ni = (unsigned)ni;
  srs_output<Fq2>(k, b2, nv, 2, s.in_subgroup, (Affine<Fq2>*)s.b_g2_query);

  // K_k = beta a_k + alpha b_k + c_k in the exponent: A over the beta table (instance term included), B over the
  // alpha table, C over the plain one; gamma = delta = 1, so K is gamma_abc_g1 | l_query as it stands
  SrsOutput<Fq> kk{};
  kk.m[0] = t[0]; kk.tab[0] = blag;
  kk.m[1] = t[1]; kk.tab[1] = alag;
  kk.m[2] = t[2]; kk.tab[2] = lag1;
  kk.nm = 3; kk.inst = blag; kk.nc = (unsigned)nc; kk.ni = (unsigned)ni;
  DevBuf kbuf(nv * sizeof(Affine<Fq>));
  srs_output<Fq>(k, kk, nv, 1, s.in_subgroup, kbuf.as<Affine<Fq>>());
  DG_HIP(hipMemcpyAsync(s.gamma_abc_g1, kbuf.p, ni * sizeof(Affine<Fq>), hipMemcpyDeviceToDevice, k.s()));
  if (nv > ni)
    DG_HIP(hipMemcpyAsync(s.l_query, kbuf.as<Affine<Fq>>() + ni, (nv - ni) * sizeof(Affine<Fq>),
                          hipMemcpyDeviceToDevice, k.s()));
  DG_HIP(hipStreamSynchronize(k.s()));
}

}  // namespace dg16
