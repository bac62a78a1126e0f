// MSM phases 1-3: signed digits, per-bucket counts, scans and placement -- the direct atomic path for small inputs and
// the two-level LDS-partitioned counting sort for large ones (msm_geom.h: msm_partition_plan chooses).  Pipeline: msm_impl.h.
#pragma once
#include "bounds.h"
#include "ctx.h"
#include "msm_geom.h"
#include "types.h"

namespace dg16 {

// atomicAdd(&ctr[idx], 1) for every active lane, returning the old value -- robust to heavy hitters.  Random
// digits almost never collide inside a wave, but the top window of any c (2 bits at c = 18: ALL scalars land
// in 3 buckets) and real witnesses (bits: half of all entries hit bucket 0 of window 0) serialise a million
// atomics on one address (measured: 23 -> 57 ms per proof at c = 18).  Cheap test first (does my neighbour
// lane hit the same counter?); only skewed waves pay the leader loop: one atomic per distinct counter.
__device__ __forceinline__ unsigned wave_atomic_inc(unsigned* __restrict__ ctr, unsigned idx, bool active) {
  const unsigned lane = __lane_id();
  const unsigned nb = __shfl_down(idx, 1);
  const bool nb_active = __shfl_down((int)active, 1);
  const unsigned long long like = __ballot(active && nb_active && nb == idx && lane < 63);
  unsigned old = 0;
  if (__popcll(like) < 8) {
    if (active) old = atomicAdd(&ctr[idx], 1u);
    return old;
  }
  unsigned long long todo = __ballot(active);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned lidx = __shfl(idx, leader);
    const unsigned long long grp = __ballot(active && idx == lidx) & todo;
    unsigned base = 0;
    if ((int)lane == leader) base = atomicAdd(&ctr[lidx], (unsigned)__popcll(grp));
    base = __shfl(base, leader);
    if ((grp >> lane) & 1) old = base + (unsigned)__popcll(grp & ((1ull << lane) - 1));
    todo &= ~grp;
  }
  return old;
}

// digit w of scalar s in signed c-bit windows: |d| <= 2^(c - 1), the carry goes on to window w + 1
template <class Fr>
__device__ __forceinline__ int msm_digit(const Fr& s, unsigned w, unsigned c, unsigned& carry) {
  const unsigned half = 1u << (c - 1);
  unsigned bit = w * c;
  unsigned limb = bit >> 5, off = bit & 31;
  uint64_t v = 0;
  if (limb < (unsigned)Fr::NL) {
    v = s.l[limb];
    if (limb + 1 < (unsigned)Fr::NL) v |= (uint64_t)s.l[limb + 1] << 32;
    v >>= off;
  }
  int d = (int)((unsigned)v & ((1u << c) - 1)) + (int)carry;
  if ((unsigned)d > half) { d -= (int)(1u << c); carry = 1; } else { carry = 0; }
  return d;
}

// ---- 1: digits + histogram -------------------------------------------------------------------
template <class Fr>
__global__ void __launch_bounds__(256) msm_digits_kernel(const Fr* __restrict__ scalars, size_t n, int mont,
                                                          MsmGeom g, int* __restrict__ digits,
                                                          unsigned* __restrict__ counts) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < n;          // no early exit: the wave-aggregated histogram needs every lane
  Fr s = Fr::zero();
  if (live) {
    s = scalars[i];
    if (mont & 1) s = s.from_mont();
  }
  const bool flip = (mont & 2) && (s.l[Fr::NL - 1] >> 31);   // bit 255 = "negate this scalar": ONLY for the halves glv.h makes
  unsigned carry = 0;
  for (unsigned w = 0; w < g.nwin; w++) {
    int d = msm_digit(s, w, g.c, carry);
    if (flip) d = -d;
    if (live) digits[(size_t)w * n + i] = d;
    unsigned b = d ? (unsigned)(d < 0 ? -d : d) - 1 : 0u;
    unsigned slot = ((w % g.bw) << g.log_nb) + b;
    wave_atomic_inc(counts, slot, live && d != 0);
  }
}

// ---- 2: per-bucket-window exclusive scans (entry offsets and segment offsets), three small launches ---
// (kernels are templated on a dummy so that every translation unit carries its own copy; kScanBlock: msm_geom.h)
template <int TU>
__global__ void __launch_bounds__(1024) msm_scan_local_kernel(const unsigned* __restrict__ counts,
                                                               unsigned* __restrict__ offsets,
                                                               unsigned* __restrict__ seg_off,
                                                               unsigned* __restrict__ block_tot, unsigned log_nb,
                                                               unsigned seg_log) {
  __shared__ unsigned sh[1024];
  __shared__ unsigned sh2[1024];
  const unsigned nb = 1u << log_nb;
  const unsigned seg_round = (1u << seg_log) - 1;
  const size_t base = (size_t)blockIdx.y << log_nb;
  const unsigned lo = blockIdx.x * kScanBlock + threadIdx.x * 4;
  unsigned cn[4], sum = 0, ssum = 0;
#pragma unroll
  for (unsigned j = 0; j < 4; j++) {
    cn[j] = (lo + j < nb) ? counts[base + lo + j] : 0;
    sum += cn[j];
    ssum += (cn[j] + seg_round) >> seg_log;
  }
  sh[threadIdx.x] = sum;
  sh2[threadIdx.x] = ssum;
  __syncthreads();
  for (unsigned d = 1; d < 1024; d <<= 1) {
    unsigned v = threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
    unsigned v2 = threadIdx.x >= d ? sh2[threadIdx.x - d] : 0;
    __syncthreads();
    sh[threadIdx.x] += v;
    sh2[threadIdx.x] += v2;
    __syncthreads();
  }
  unsigned run = sh[threadIdx.x] - sum, srun = sh2[threadIdx.x] - ssum;
#pragma unroll
  for (unsigned j = 0; j < 4; j++)
    if (lo + j < nb) {
      offsets[base + lo + j] = run;
      seg_off[base + lo + j] = srun;
      run += cn[j];
      srun += (cn[j] + seg_round) >> seg_log;
    }
  if (threadIdx.x == 1023) {
    size_t t = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
    block_tot[t] = sh[1023];
    block_tot[t + 1] = sh2[1023];
  }
}
// one workgroup per bucket-window: exclusive scan of the (<= 1024) block totals
template <int TU>
__global__ void __launch_bounds__(1024) msm_scan_tops_kernel(unsigned* __restrict__ block_tot, unsigned nblocks,
                                                              unsigned* __restrict__ seg_total) {
  __shared__ unsigned sh[1024];
  __shared__ unsigned sh2[1024];
  unsigned* t = block_tot + (size_t)blockIdx.x * nblocks * 2;
  unsigned a = threadIdx.x < nblocks ? t[threadIdx.x * 2] : 0;
  unsigned b = threadIdx.x < nblocks ? t[threadIdx.x * 2 + 1] : 0;
  sh[threadIdx.x] = a;
  sh2[threadIdx.x] = b;
  __syncthreads();
  for (unsigned d = 1; d < 1024; d <<= 1) {
    unsigned v = threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
    unsigned v2 = threadIdx.x >= d ? sh2[threadIdx.x - d] : 0;
    __syncthreads();
    sh[threadIdx.x] += v;
    sh2[threadIdx.x] += v2;
    __syncthreads();
  }
  if (threadIdx.x < nblocks) {
    t[threadIdx.x * 2] = sh[threadIdx.x] - a;
    t[threadIdx.x * 2 + 1] = sh2[threadIdx.x] - b;
  }
  if (threadIdx.x == 1023) seg_total[blockIdx.x] = sh2[1023];
}
template <int TU>
__global__ void __launch_bounds__(1024) msm_scan_fix_kernel(unsigned* __restrict__ offsets,
                                                             unsigned* __restrict__ seg_off,
                                                             unsigned* __restrict__ cursor,
                                                             const unsigned* __restrict__ block_tot, unsigned log_nb) {
  const unsigned nb = 1u << log_nb;
  const size_t base = (size_t)blockIdx.y << log_nb;
  const size_t t = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
  const unsigned add = block_tot[t], sadd = block_tot[t + 1];
  const unsigned lo = blockIdx.x * kScanBlock + threadIdx.x * 4;
#pragma unroll
  for (unsigned j = 0; j < 4; j++)
    if (lo + j < nb) {
      offsets[base + lo + j] += add;
      seg_off[base + lo + j] += sadd;
      cursor[base + lo + j] = 0;
    }
}

// ---- 3: scatter ---------------------------------------------------------------------------------
template <int TU>
__global__ void __launch_bounds__(256) msm_scatter_kernel(const int* __restrict__ digits, size_t n, MsmGeom g,
                                                           const unsigned* __restrict__ offsets,
                                                           const unsigned* __restrict__ seg_off,
                                                           unsigned* __restrict__ cursor,
                                                           unsigned* __restrict__ entries) {
  // one thread per (scalar, window) -- blockIdx.y = window: the rank comes back from an atomic, and a thread that walked
  // its scalar's windows paid W dependent round trips: 34 -> 4 us of a 0.55-ms MSM at 2^10 points (at 2^13 the 2^17.6
  // returning atomics are the bound either way: 45 -> 38 us; the digits kernel's atomics return nothing and gain nothing
  // from the same split: profiles/r6zv)
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < n;
  const unsigned w = blockIdx.y;
  int d = live ? digits[(size_t)w * n + i] : 0;
  const bool act = d != 0;
  unsigned b = act ? (unsigned)(d < 0 ? -d : d) - 1 : 0u;
  const unsigned bwin = w % g.bw;
  unsigned slot = (bwin << g.log_nb) + b;
  unsigned rank = wave_atomic_inc(cursor, slot, act);
  if (!act) return;
  unsigned ref = (unsigned)((size_t)(w / g.bw) * n + i);   // table row w / bw = 2^(c*bw*(w/bw)) * P_i (plain: row 0)
  entries[DG_IDX(15, (size_t)bwin * g.region + offsets[slot] + rank, (size_t)g.bw * g.region)] = ref | (d < 0 ? 0x80000000u : 0u);
}

// ---- 1'-3': partitioned digit sort (large MSMs) ------------------------------------------------------
// The atomic path above issues one device-scope atomic per entry twice (histogram, rank) and scatters 4-byte
// entries at random: ~31 G atomics/s and a 64-byte memory transaction per entry, 1.5 ms per 2^20-scalar sort.
// Here the slot index (bucket-window, bucket) is split into a partition (high bits, <= 256 of them) and a bin
// (low bits, <= 4096).  Pass 1 recomputes the digits twice instead of storing them: (a) per-workgroup LDS
// histogram over partitions, (b) after a scan, (ref, slot) pairs go to their partition at LDS-ranked
// positions.  Pass 2 walks each partition in tiles: (a) LDS histogram over bins -> bucket counts (one global
// atomic per non-empty bin and workgroup instead of one per entry), (b) after the usual bucket scans, LDS ranks
// inside the tile + one returning atomic per bin and tile give every entry its final position.  (kPart*, PartGeom: msm_geom.h)
template <class Fr>
__global__ void __launch_bounds__(256) msm_part_hist_kernel(const Fr* __restrict__ scalars, size_t n, int mont,
                                                             MsmGeom g, PartGeom pg,
                                                             unsigned* __restrict__ blockhist) {
  __shared__ unsigned hist[kPartMax];
  hist[threadIdx.x] = 0;
  __syncthreads();
  for (unsigned k = 0; k < kPartScalars / 256; k++) {
    size_t i = (size_t)blockIdx.x * kPartScalars + k * 256 + threadIdx.x;
    if (i >= n) continue;
    Fr s = scalars[i];
    if (mont & 1) s = s.from_mont();
    unsigned carry = 0;
    for (unsigned w = 0; w < g.nwin; w++) {
      int d = msm_digit(s, w, g.c, carry);
      if (d == 0) continue;
      unsigned slot = ((w % g.bw) << g.log_nb) + (unsigned)(d < 0 ? -d : d) - 1;
      atomicAdd(&hist[slot >> pg.low_bits], 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x < pg.nparts) blockhist[(size_t)threadIdx.x * pg.nblk1 + blockIdx.x] = hist[threadIdx.x];
}

template <class Fr>
__global__ void __launch_bounds__(256) msm_part_scatter_kernel(const Fr* __restrict__ scalars, size_t n, int mont,
                                                                MsmGeom g, PartGeom pg,
                                                                const unsigned* __restrict__ blockoff,
                                                                uint2* __restrict__ part) {
  __shared__ unsigned cur[kPartMax];
  if (threadIdx.x < pg.nparts) cur[threadIdx.x] = blockoff[(size_t)threadIdx.x * pg.nblk1 + blockIdx.x];
  __syncthreads();
  for (unsigned k = 0; k < kPartScalars / 256; k++) {
    size_t i = (size_t)blockIdx.x * kPartScalars + k * 256 + threadIdx.x;
    if (i >= n) continue;
    Fr s = scalars[i];
    if (mont & 1) s = s.from_mont();
    const bool flip = (mont & 2) && (s.l[Fr::NL - 1] >> 31);   // bit 255 = "negate this scalar": ONLY for the halves glv.h makes
    unsigned carry = 0;
    for (unsigned w = 0; w < g.nwin; w++) {
      int d = msm_digit(s, w, g.c, carry);
      if (d == 0) continue;
      unsigned slot = ((w % g.bw) << g.log_nb) + (unsigned)(d < 0 ? -d : d) - 1;
      unsigned ref = (unsigned)((size_t)(w / g.bw) * n + i);   // table row w / bw (plain mode: bw = W, row 0)
      unsigned pos = atomicAdd(&cur[slot >> pg.low_bits], 1u);
      part[DG_IDX(14, pos, (size_t)g.nwin * n)] = make_uint2(ref | (((d < 0) != flip) ? 0x80000000u : 0u), slot);
    }
  }
}

// generic in-place exclusive scan of a[0..len): chunk scan -> scan of chunk totals -> add back
template <int TU>
__global__ void __launch_bounds__(1024) scan_chunk_kernel(unsigned* __restrict__ a, size_t len,
                                                           unsigned* __restrict__ tot) {
  __shared__ unsigned sh[1024];
  const size_t lo = (size_t)blockIdx.x * 4096 + threadIdx.x * 4;
  unsigned v[4], sum = 0;
#pragma unroll
  for (unsigned j = 0; j < 4; j++) {
    v[j] = lo + j < len ? a[lo + j] : 0;
    sum += v[j];
  }
  sh[threadIdx.x] = sum;
  __syncthreads();
  for (unsigned d = 1; d < 1024; d <<= 1) {
    unsigned t = threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
    __syncthreads();
    sh[threadIdx.x] += t;
    __syncthreads();
  }
  unsigned run = sh[threadIdx.x] - sum;
#pragma unroll
  for (unsigned j = 0; j < 4; j++)
    if (lo + j < len) {
      a[lo + j] = run;
      run += v[j];
    }
  if (threadIdx.x == 1023) tot[blockIdx.x] = sh[1023];
}
template <int TU>
__global__ void __launch_bounds__(1024) scan_tops_kernel(unsigned* __restrict__ tot, unsigned nchunks) {
  __shared__ unsigned sh[1024];
  const unsigned per = (nchunks + 1023) / 1024;
  const unsigned lo = threadIdx.x * per;
  unsigned sum = 0;
  for (unsigned j = 0; j < per; j++)
    if (lo + j < nchunks) sum += tot[lo + j];
  sh[threadIdx.x] = sum;
  __syncthreads();
  for (unsigned d = 1; d < 1024; d <<= 1) {
    unsigned t = threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
    __syncthreads();
    sh[threadIdx.x] += t;
    __syncthreads();
  }
  unsigned run = sh[threadIdx.x] - sum;
  for (unsigned j = 0; j < per; j++)
    if (lo + j < nchunks) {
      unsigned t = tot[lo + j];
      tot[lo + j] = run;
      run += t;
    }
}
template <int TU>
__global__ void __launch_bounds__(1024) scan_add_kernel(unsigned* __restrict__ a, size_t len,
                                                         const unsigned* __restrict__ tot) {
  const size_t lo = (size_t)blockIdx.x * 4096 + threadIdx.x * 4;
  const unsigned add = tot[blockIdx.x];
#pragma unroll
  for (unsigned j = 0; j < 4; j++)
    if (lo + j < len) a[lo + j] += add;
}

template <int TU>
__global__ void __launch_bounds__(256) msm_part_count_kernel(const uint2* __restrict__ part,
                                                              const unsigned* __restrict__ blockoff, PartGeom pg,
                                                              unsigned* __restrict__ counts) {
  __shared__ unsigned hist[1u << kPartMaxLowBits];
  const unsigned p = blockIdx.y;
  const unsigned lo = blockoff[(size_t)p * pg.nblk1];
  const unsigned size = blockoff[(size_t)(p + 1) * pg.nblk1] - lo;
  if (((size_t)blockIdx.x << kPartTileLog) >= size) return;
  const unsigned nlow = 1u << pg.low_bits;
  for (unsigned b = threadIdx.x; b < nlow; b += 256) hist[b] = 0;
  __syncthreads();
  for (size_t t = (size_t)blockIdx.x << kPartTileLog; t < size; t += (size_t)gridDim.x << kPartTileLog)
    for (unsigned j = 0; j < (1u << kPartTileLog) / 256; j++) {
      size_t idx = t + j * 256 + threadIdx.x;
      if (idx < size) atomicAdd(&hist[part[lo + idx].y & (nlow - 1)], 1u);
    }
  __syncthreads();
  for (unsigned b = threadIdx.x; b < nlow; b += 256)
    if (hist[b]) atomicAdd(&counts[((size_t)p << pg.low_bits) + b], hist[b]);
}

template <int TU>
__global__ void __launch_bounds__(256) msm_part_place_kernel(const uint2* __restrict__ part,
                                                              const unsigned* __restrict__ blockoff, PartGeom pg,
                                                              MsmGeom g, const unsigned* __restrict__ offsets,
                                                              const unsigned* __restrict__ seg_off,
                                                              unsigned* __restrict__ cursor,
                                                              unsigned* __restrict__ entries) {
  __shared__ unsigned cnt[1u << kPartMaxLowBits];    // entries of this tile per bin
  __shared__ unsigned rank0[1u << kPartMaxLowBits];  // rank of the tile's first entry inside its bucket
  __shared__ unsigned dst0[1u << kPartMaxLowBits];   // position of the bucket's first entry
  const unsigned p = blockIdx.y;
  const unsigned lo = blockoff[(size_t)p * pg.nblk1];
  const unsigned size = blockoff[(size_t)(p + 1) * pg.nblk1] - lo;
  if (((size_t)blockIdx.x << kPartTileLog) >= size) return;
  const unsigned nlow = 1u << pg.low_bits;
  constexpr unsigned PER = (1u << kPartTileLog) / 256;
  for (size_t t = (size_t)blockIdx.x << kPartTileLog; t < size; t += (size_t)gridDim.x << kPartTileLog) {
    for (unsigned b = threadIdx.x; b < nlow; b += 256) cnt[b] = 0;
    __syncthreads();
    uint2 e[PER];
    unsigned lr[PER];
#pragma unroll
    for (unsigned j = 0; j < PER; j++) {
      size_t idx = t + j * 256 + threadIdx.x;
      e[j] = make_uint2(0u, 0xFFFFFFFFu);
      if (idx < size) {
        e[j] = part[lo + idx];
        lr[j] = atomicAdd(&cnt[e[j].y & (nlow - 1)], 1u);
      }
    }
    __syncthreads();
    for (unsigned b = threadIdx.x; b < nlow; b += 256)
      if (cnt[b]) {
        const size_t slot = ((size_t)p << pg.low_bits) + b;
        rank0[b] = atomicAdd(&cursor[slot], cnt[b]);
        dst0[b] = (unsigned)((slot >> g.log_nb) * g.region) + offsets[slot];
      }
    __syncthreads();
#pragma unroll
    for (unsigned j = 0; j < PER; j++) {
      if (e[j].y == 0xFFFFFFFFu) continue;
      const unsigned slot = e[j].y, b = slot & (nlow - 1);
      const unsigned rank = rank0[b] + lr[j];
      entries[DG_IDX(13, dst0[b] + rank, (size_t)g.bw * g.region)] = e[j].x;
    }
    __syncthreads();
  }
}

// Result of the scalar-side passes (digits, scan, scatter): shared by every MSM over the same scalars.
struct MsmSort {
  MsmGeom g;
  size_t n = 0;
  int* digits = nullptr;
  unsigned *entries = nullptr, *counts = nullptr, *offsets = nullptr, *seg_off = nullptr, *cursor = nullptr;
  unsigned* seg_total = nullptr;
};

// scalars_mont: bit 0 = Montgomery form, bit 1 = bit 255 of a scalar is a sign flag (the halves of glv.h)
template <class Fr, int SCALAR_BITS>
MsmSort msm_sort_on(hipStream_t s, Channel& wsch, const void* scalars, size_t n, unsigned scalars_mont, bool table,
                    unsigned c_fixed, unsigned stride);
template <class Fr, int SCALAR_BITS>
MsmSort msm_sort(Call& k, const void* scalars, size_t n, unsigned scalars_mont, bool table, unsigned c_fixed = 0,
                 unsigned stride = 1) {
  return msm_sort_on<Fr, SCALAR_BITS>(k.s(), k.c, scalars, n, scalars_mont, table, c_fixed, stride);
}
// sort on stream `s` with the buffers of channel `wsch`
template <class Fr, int SCALAR_BITS>
MsmSort msm_sort_on(hipStream_t s, Channel& wsch, const void* scalars, size_t n, unsigned scalars_mont, bool table,
                    unsigned c_fixed, unsigned stride) {
  MsmSort r;
  DG_BOUNDS_BIND();
  r.n = n;
  r.g = msm_geometry(n ? n : 1, SCALAR_BITS, table, c_fixed, stride);
  const MsmGeom& g = r.g;
  const size_t nbw = (size_t)g.bw << g.log_nb;
  DG_REQUIRE((size_t)g.nwin * n < ((size_t)1 << 31), DG16_ERR_BAD_ARG, "W * n must be < 2^31");
  const PartPlan plan = msm_partition_plan(g, n);
  const PartGeom& pg = plan.pg;
  const bool partitioned = plan.partitioned;
  r.digits = (int*)ws(wsch, 4, (size_t)g.nwin * n * (partitioned ? 8 : 4));
  r.entries = (unsigned*)ws(wsch, 5, (size_t)g.nwin * n * 4);
  unsigned* tabs = (unsigned*)ws(wsch, 6, (nbw * 4 + g.bw) * 4);
  r.counts = tabs;
  r.offsets = r.counts + nbw;
  r.seg_off = r.offsets + nbw;
  r.cursor = r.seg_off + nbw;
  r.seg_total = r.cursor + nbw;
  unsigned* blockoff = nullptr;
  if (n && partitioned) {
    const size_t len = (size_t)pg.nparts * pg.nblk1 + 1;
    blockoff = (unsigned*)ws(wsch, 25, (len + (unsigned)((len + 4095) / 4096)) * 4);
  }
  const unsigned scan_nblocks = ((1u << g.log_nb) + kScanBlock - 1) / kScanBlock;
  unsigned* block_tot = (unsigned*)ws(wsch, 9, (size_t)g.bw * scan_nblocks * 2 * 4);
  DG_HIP(hipMemsetAsync(r.counts, 0, nbw * 4, s));
  uint2* part = (uint2*)r.digits;
  if (n && partitioned) {
    const size_t len = (size_t)pg.nparts * pg.nblk1 + 1;      // + sentinel = total entries
    const unsigned nchunks = (unsigned)((len + 4095) / 4096);
    unsigned* tot = blockoff + len;
    DG_HIP(hipMemsetAsync(blockoff + len - 1, 0, 4, s));
    hipLaunchKernelGGL(msm_part_hist_kernel<Fr>, dim3(pg.nblk1), dim3(256), 0, s, (const Fr*)scalars, n,
                       (int)scalars_mont, g, pg, blockoff);
    hipLaunchKernelGGL(scan_chunk_kernel<0>, dim3(nchunks), dim3(1024), 0, s, blockoff, len, tot);
    hipLaunchKernelGGL(scan_tops_kernel<0>, dim3(1), dim3(1024), 0, s, tot, nchunks);
    hipLaunchKernelGGL(scan_add_kernel<0>, dim3(nchunks), dim3(1024), 0, s, blockoff, len, tot);
    hipLaunchKernelGGL(msm_part_scatter_kernel<Fr>, dim3(pg.nblk1), dim3(256), 0, s, (const Fr*)scalars, n,
                       (int)scalars_mont, g, pg, blockoff, part);
    hipLaunchKernelGGL(msm_part_count_kernel<0>, dim3(kPartBlocks, pg.nparts), dim3(256), 0, s, part, blockoff, pg,
                       r.counts);
  } else if (n) {
    hipLaunchKernelGGL(msm_digits_kernel<Fr>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const Fr*)scalars,
                       n, (int)scalars_mont, g, r.digits, r.counts);
  }
  {
    const unsigned nblocks = ((1u << g.log_nb) + kScanBlock - 1) / kScanBlock;   // <= 512 for c <= 22
    hipLaunchKernelGGL(msm_scan_local_kernel<0>, dim3(nblocks, g.bw), dim3(1024), 0, s, r.counts, r.offsets,
                       r.seg_off, block_tot, g.log_nb, g.seg_log);
    hipLaunchKernelGGL(msm_scan_tops_kernel<0>, dim3(g.bw), dim3(1024), 0, s, block_tot, nblocks, r.seg_total);
    hipLaunchKernelGGL(msm_scan_fix_kernel<0>, dim3(nblocks, g.bw), dim3(1024), 0, s, r.offsets, r.seg_off, r.cursor,
                       block_tot, g.log_nb);
  }
  if (n && partitioned)
    hipLaunchKernelGGL(msm_part_place_kernel<0>, dim3(kPartBlocks, pg.nparts), dim3(256), 0, s, part, blockoff, pg, g,
                       r.offsets, r.seg_off, r.cursor, r.entries);
  else if (n)
    hipLaunchKernelGGL(msm_scatter_kernel<0>, dim3((unsigned)((n + 255) / 256), g.nwin), dim3(256), 0, s, r.digits, n, g,
                       r.offsets, r.seg_off, r.cursor, r.entries);
  DG_HIP(hipGetLastError());
  return r;
}

}  // namespace dg16
