// The three CSR matrices of an R1CS by wire: what both key generators (setup_curve.hip from a trapdoor,
// setup_srs_curve.hip from a structured reference string) gather from.  A counting sort over the columns -- count, scan,
// fill -- per matrix; there is no atomic add in Fr or in a group, so the sums over a column are gathers.
#pragma once
#include "ctx.h"

namespace dg16 {
namespace {

struct DevBuf {     // temporary device memory of one setup call (hipFree waits for the kernels that use it)
  void* p = nullptr;
  explicit DevBuf(size_t bytes) { DG_HIP(hipMalloc(&p, bytes ? bytes : 16)); }
  ~DevBuf() { if (p) (void)hipFree(p); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  template <class T> T* as() const { return (T*)p; }
};

// A row whose pointers are not ordered or reach beyond nnz, and an entry whose column is not a wire, are skipped and
// reported (flag): nothing is read or written out of range.  The same rule in the count and the fill pass.
__device__ __forceinline__ bool setup_row(const unsigned* row_ptr, size_t i, size_t nnz, unsigned& lo, unsigned& hi,
                                          unsigned* flag) {
  lo = row_ptr[i];
  hi = row_ptr[i + 1];
  if (hi < lo || hi > nnz) {
    *flag = 1u;
    return false;
  }
  return true;
}
__global__ void __launch_bounds__(256) setup_count_kernel(const unsigned* __restrict__ row_ptr,
                                                           const unsigned* __restrict__ col, size_t nc, size_t nv,
                                                           size_t nnz, unsigned* __restrict__ counts, unsigned* flag) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nc) return;
  unsigned lo, hi;
  if (!setup_row(row_ptr, i, nnz, lo, hi, flag)) return;
  for (unsigned j = lo; j < hi; j++) {
    const unsigned cl = col[j];
    if (cl >= nv) { *flag = 1u; continue; }
    atomicAdd(&counts[cl], 1u);
  }
}
// ptr[k] = cursor[k] = sum of counts[0..k), ptr[n] = total; one workgroup
__global__ void __launch_bounds__(1024) setup_scan_kernel(const unsigned* __restrict__ counts, size_t n,
                                                           unsigned* __restrict__ ptr, unsigned* __restrict__ cursor) {
  __shared__ unsigned sums[1024];
  const unsigned tid = threadIdx.x;
  const size_t per = (n + 1023) / 1024;
  const size_t lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
  unsigned s = 0;
  for (size_t i = lo; i < hi; i++) s += counts[i];
  sums[tid] = s;
  __syncthreads();
  for (unsigned off = 1; off < 1024; off <<= 1) {
    const unsigned v = tid >= off ? sums[tid - off] : 0u;
    __syncthreads();
    sums[tid] += v;
    __syncthreads();
  }
  unsigned run = tid ? sums[tid - 1] : 0u;
  for (size_t i = lo; i < hi; i++) {
    ptr[i] = run;
    cursor[i] = run;
    run += counts[i];
  }
  if (tid == 1023) ptr[n] = sums[1023];
}
__global__ void __launch_bounds__(256) setup_fill_kernel(const unsigned* __restrict__ row_ptr,
                                                          const unsigned* __restrict__ col, size_t nc, size_t nv,
                                                          size_t nnz, unsigned* __restrict__ cursor,
                                                          unsigned* __restrict__ t_row, unsigned* __restrict__ t_src,
                                                          unsigned* flag) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nc) return;
  unsigned lo, hi;
  if (!setup_row(row_ptr, i, nnz, lo, hi, flag)) return;
  for (unsigned j = lo; j < hi; j++) {
    const unsigned cl = col[j];
    if (cl >= nv) continue;
    const unsigned pos = atomicAdd(&cursor[cl], 1u);    // < ptr[cl + 1] <= nnz: the count pass saw the same entries
    t_row[pos] = (unsigned)i;
    t_src[pos] = j;
  }
}

template <class Fr>
struct TCsrT {     // a matrix by wire: entries ptr[k] .. ptr[k + 1) of wire k are (constraint t_row, coeff[t_src])
  const unsigned *ptr, *t_row, *t_src;
  const Fr* coeff;
};

// The transposes of A, B, C on the call's stream.  Per matrix ptr[nv + 1], cursor / counts [nv], t_row, t_src [nnz];
// *flag is set where setup_row or a column refuses an entry (the caller reads it after the stream has drained).
template <class Fr>
struct Transposes {
  DevBuf counts, cursor, ptr, trow, tsrc;
  TCsrT<Fr> t[3];
  Transposes(Call& k, const unsigned* const* row_ptr, const unsigned* const* col, const void* const* coeff,
             const size_t* nnz, size_t nc, size_t nv, unsigned* flag)
      : counts(3 * nv * sizeof(unsigned)), cursor(3 * nv * sizeof(unsigned)), ptr(3 * (nv + 1) * sizeof(unsigned)),
        trow((nnz[0] + nnz[1] + nnz[2]) * sizeof(unsigned)), tsrc((nnz[0] + nnz[1] + nnz[2]) * sizeof(unsigned)) {
    DG_HIP(hipMemsetAsync(counts.p, 0, 3 * nv * sizeof(unsigned), k.s()));
    size_t off = 0;
    for (int j = 0; j < 3; j++) {
      unsigned* cnt = counts.as<unsigned>() + j * nv;
      unsigned* cur = cursor.as<unsigned>() + j * nv;
      unsigned* p = ptr.as<unsigned>() + j * (nv + 1);
      unsigned* tr = trow.as<unsigned>() + off;
      unsigned* tsr = tsrc.as<unsigned>() + off;
      off += nnz[j];
      const unsigned blocks = (unsigned)((nc + 255) / 256);
      if (nc)
        hipLaunchKernelGGL(setup_count_kernel, dim3(blocks), dim3(256), 0, k.s(), row_ptr[j], col[j], nc, nv, nnz[j], cnt,
                           flag);
      hipLaunchKernelGGL(setup_scan_kernel, dim3(1), dim3(1024), 0, k.s(), cnt, nv, p, cur);
      if (nc)
        hipLaunchKernelGGL(setup_fill_kernel, dim3(blocks), dim3(256), 0, k.s(), row_ptr[j], col[j], nc, nv, nnz[j], cur,
                           tr, tsr, flag);
      t[j] = TCsrT<Fr>{p, tr, tsr, (const Fr*)coeff[j]};
    }
  }
};

}  // namespace
}  // namespace dg16
