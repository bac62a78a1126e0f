// The Libsnark QAP reduction (DG16_F_QAP_LIBSNARK) next to the circom one: the witness map every arkworks circuit
// that is not a circom circuit is proved with (`Groth16::<E>` defaults to LibsnarkReduction; the reference uses it at
// ark-circom/src/zkey.rs:921 and describes the two maps at ark-circom/src/circom/qap.rs:11-15).
//
//   dg16_qap_r1cs   a = A w, b = B w, c = C w on the constraint rows (dg16_qap sets c = a o b and never reads C), and the
//                   R1CS check a_i b_i == c_i fused into the same pass: count of violated rows, smallest violated row
//   h               the m coefficients of (A B - C) / Z, Z = X^m - 1:
//                     iNTT(a, b, c) | coset NTT at offset g (x g^i fused into the first pass's load) |
//                     (a o b - c) / Z(g) | coset iNTT (x g^-i fused into the last pass's store)
//                   seven transforms through the launches dg16_ntt uses (ntt.hip: ntt_batch_launch); the circom pipeline's
//                   kernels are not touched.  g = F::GENERATOR (5 / 7 / 22): any coset off the domain gives the same h.
#include "ctx.h"
#include "types.h"

namespace dg16 {

// ---- R1CS x witness with C, and the witness check ------------------------------------------------------------------
// One lane per domain slot, as qap_kernel (field_ops.hip) assigns them; the same rules for untrusted indices.
template <class Fr>
__device__ __forceinline__ Fr r1cs_row(const unsigned* __restrict__ ptr, const unsigned* __restrict__ col,
                                       const Fr* __restrict__ val, const Fr* __restrict__ w, int w_mont, size_t i,
                                       size_t nv, bool& bad) {
  Fr acc = Fr::zero();
  const unsigned lo = ptr[i], hi = ptr[i + 1];
  if (hi < lo || hi - lo > nv) { bad = true; return acc; }
  for (unsigned j = lo; j < hi; j++) {
    const unsigned cl = col[j];
    if (cl >= nv) { bad = true; break; }
    Fr x = w[cl];
    if (!w_mont) x = x.to_mont();
    acc = acc + val[j] * x;
  }
  return acc;
}

struct R1csMatrices {
  const unsigned *ptr[3], *col[3];
  const void* val[3];
};

// viol: null, or two words -- [0] += violated rows of this launch, [1] = min(violated domain row) -- preset to
// (0, UINT64_MAX) by the host.  One pair of global atomics per workgroup that saw a violation.
template <class Fr>
__global__ void __launch_bounds__(256) qap_r1cs_kernel(R1csMatrices M, const Fr* __restrict__ w, int w_mont, size_t nc,
                                                        size_t ni, size_t nv, size_t m, size_t row_start,
                                                        size_t row_stride, Fr* __restrict__ a, Fr* __restrict__ b,
                                                        Fr* __restrict__ c, unsigned long long* __restrict__ viol,
                                                        unsigned* __restrict__ err_flag) {
  __shared__ unsigned s_count;
  __shared__ unsigned long long s_first;
  if (threadIdx.x == 0) {
    s_count = 0u;
    s_first = ~0ull;
  }
  __syncthreads();
  const size_t slot = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i = row_start + row_stride * slot;
  if (i < m) {
    Fr av = Fr::zero(), bv = Fr::zero(), cv = Fr::zero();
    if (i < nc) {
      bool bad = false;
      av = r1cs_row<Fr>(M.ptr[0], M.col[0], (const Fr*)M.val[0], w, w_mont, i, nv, bad);
      bv = r1cs_row<Fr>(M.ptr[1], M.col[1], (const Fr*)M.val[1], w, w_mont, i, nv, bad);
      cv = r1cs_row<Fr>(M.ptr[2], M.col[2], (const Fr*)M.val[2], w, w_mont, i, nv, bad);
      if (bad) {
        *(volatile unsigned*)err_flag = 1u;   // plain store: the word lives in pinned host memory
        av = bv = cv = Fr::zero();
      }
      if (viol && av * bv != cv) {
        atomicAdd(&s_count, 1u);
        atomicMin(&s_first, (unsigned long long)i);
      }
    } else if (i < nc + ni) {
      av = w[i - nc];
      if (!w_mont) av = av.to_mont();
    }
    a[slot] = av;
    b[slot] = bv;
    c[slot] = cv;
  }
  if (!viol) return;
  __syncthreads();
  if (threadIdx.x == 0 && s_count) {
    atomicAdd(&viol[0], (unsigned long long)s_count);
    atomicMin(&viol[1], s_first);
  }
}

void qap_r1cs_launch(Call& k, int curve, const unsigned* const* row_ptr, const unsigned* const* col, const void* const* val,
                     const void* w, bool w_mont, size_t nc, size_t ni, size_t nv, size_t m, size_t row_start,
                     size_t row_stride, void* a, void* b, void* c, unsigned long long* violations) {
  R1csMatrices M;
  for (int j = 0; j < 3; j++) { M.ptr[j] = row_ptr[j]; M.col[j] = col[j]; M.val[j] = val[j]; }
  if (violations) {
    DG_HIP(hipMemsetAsync(violations, 0, 8, k.s()));
    DG_HIP(hipMemsetAsync(violations + 1, 0xff, 8, k.s()));
  }
  const unsigned blocks = (unsigned)((m / row_stride + 255) / 256);
#define QAP3(F)                                                                                                      \
  hipLaunchKernelGGL(qap_r1cs_kernel<F>, dim3(blocks), dim3(256), 0, k.s(), M, (const F*)w, (int)w_mont, nc, ni, nv, m, \
                     row_start, row_stride, (F*)a, (F*)b, (F*)c, violations, k.ctx->dev_flag)
  switch (curve) {
    case 0: QAP3(bn254_fr); break;
    case 1: QAP3(bls12_381_fr); break;
    default: QAP3(bls12_377_fr); break;
  }
#undef QAP3
  DG_HIP(hipGetLastError());
}

// ---- h = (A B - C) / Z ----------------------------------------------------------------------------------------------
// t = (a o b - c) / Z(g) over the three coset-evaluated vectors, in place on a
template <class F>
__global__ void __launch_bounds__(256) coset_quotient_kernel(F* __restrict__ a, const F* __restrict__ b,
                                                              const F* __restrict__ c, const F* __restrict__ zg_inv,
                                                              size_t n) {
  const F zi = *zg_inv;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) a[i] = (a[i] * b[i] - c[i]) * zi;
}

constexpr unsigned kCosetLoBits = 11;     // split of the g^i tables (the NTT passes take any split: StepArgs::plb)

template <class F>
static const CosetSet& get_coset(Call& k, int curve, unsigned log_m) {
  std::lock_guard<std::mutex> g(k.ctx->mu);
  const auto key = std::make_pair(curve, log_m);
  auto it = k.ctx->cosets.find(key);
  if (it != k.ctx->cosets.end()) return it->second;
  static const uint32_t generator[3] = {5, 7, 22};          // ark-ff GENERATOR of the three scalar fields
  const F gen = F::from_u32(generator[curve]);
  F zg = gen;
  for (unsigned i = 0; i < log_m; i++) zg = zg.sqr();
  zg = zg - F::one();                                        // Z(g) = g^m - 1 != 0: g generates the whole group
  const F host[3] = {gen, gen.inv(), zg.inv()};
  CosetSet cs;
  cs.lb = log_m < kCosetLoBits ? log_m : kCosetLoBits;
  const size_t nlo = (size_t)1 << cs.lb, nhi = (size_t)1 << (log_m - cs.lb);
  DG_HIP(hipMalloc(&cs.zg_inv, 3 * sizeof(F)));              // 1 / Z(g) | g | 1 / g
  F* consts = (F*)cs.zg_inv;
  DG_HIP(hipMalloc(&cs.g_lo, nlo * sizeof(F)));
  DG_HIP(hipMalloc(&cs.g_hi, nhi * sizeof(F)));
  DG_HIP(hipMalloc(&cs.gi_lo, nlo * sizeof(F)));
  DG_HIP(hipMalloc(&cs.gi_hi, nhi * sizeof(F)));
  DG_HIP(hipMemcpyAsync(consts, &host[2], sizeof(F), hipMemcpyHostToDevice, k.s()));
  DG_HIP(hipMemcpyAsync(consts + 1, &host[0], 2 * sizeof(F), hipMemcpyHostToDevice, k.s()));
  power_tables_launch(k, curve, consts + 1, log_m, cs.g_lo, cs.g_hi, cs.lb);
  power_tables_launch(k, curve, consts + 2, log_m, cs.gi_lo, cs.gi_hi, cs.lb);
  DG_HIP(hipStreamSynchronize(k.s()));   // `host` is a stack buffer; the tables are shared by all channels from here on
  return k.ctx->cosets.emplace(key, cs).first->second;
}

// Workspace: the slots of the circom h-polynomial (ntt.hip: h_poly_typed) -- 12, 13, 14 for the three vectors, 8 for the
// passes' ping-pong -- all touched on the call's stream only, so a queue of proofs (prover_impl.h) orders them as it
// orders the circom path's.  a, b, c are read by the first pass only; out may alias a.
template <class F>
static void h_poly_libsnark_typed(Call& k, int curve, const void* a, const void* b, const void* c, unsigned log_m,
                                  void* out) {
  const size_t n = (size_t)1 << log_m, bytes = sizeof(F) << log_m;
  const CosetSet& cs = get_coset<F>(k, curve, log_m);
  void* v[3] = {ws(k.c, 12, bytes), ws(k.c, 13, bytes), ws(k.c, 14, bytes)};
  uint8_t* t0 = (uint8_t*)ws(k.c, 8, 3 * bytes);
  void* tmp[3] = {t0, t0 + bytes, t0 + 2 * bytes};
  const void* in[3] = {a, b, c};
  k.begin_dominant();
  ntt_batch_launch(k, curve, 3, in, v, tmp, log_m, 1, nullptr, nullptr, nullptr, nullptr, 0);
  ntt_batch_launch(k, curve, 3, v, v, tmp, log_m, 0, cs.g_lo, cs.g_hi, nullptr, nullptr, cs.lb);
  size_t blocks = (n + 255) / 256;
  const size_t cap = (size_t)k.ctx->compute_units * 8;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(coset_quotient_kernel<F>, dim3((unsigned)blocks), dim3(256), 0, k.s(), (F*)v[0], (const F*)v[1],
                     (const F*)v[2], (const F*)cs.zg_inv, n);
  DG_HIP(hipGetLastError());
  ntt_batch_launch(k, curve, 1, v, &out, tmp, log_m, 1, nullptr, nullptr, cs.gi_lo, cs.gi_hi, cs.lb);
  k.end_dominant();
}

void h_poly_libsnark_launch(Call& k, int curve, const void* a, const void* b, const void* c, unsigned log_m, void* out) {
  switch (curve) {
    case 0: h_poly_libsnark_typed<bn254_fr>(k, curve, a, b, c, log_m, out); break;
    case 1: h_poly_libsnark_typed<bls12_381_fr>(k, curve, a, b, c, log_m, out); break;
    default: h_poly_libsnark_typed<bls12_377_fr>(k, curve, a, b, c, log_m, out); break;
  }
}

}  // namespace dg16
