// Packing scalar vectors into party shares, with or without blinds (dg16_pss_pack_scalars, dg16_request_pack), and the
// expansion of a 32-byte seed into field elements (dg16_fr_expand).
//
//   what       share r of chunk e = sum_{c<l} P[r][c] * secret(e, c) + sum_{k<l} P[r][l + k] * blind(e, k), r < n = 4 l, with
//              P = FFT_share o iFFT_secret restricted to its first 2 l columns: the secret domain has l + t + 1 = 2 l
//              points, pack_from_public (secret-sharing/src/pss.rs:86-92) leaves the upper l at zero and
//              pack_from_public_rand (pss.rs:72-82) fills them with randomness.  Columns 0 .. l are the handle's pack
//              matrix (dist_impl.h: dg16_pss::mats, block 0), so without blinds the result is dg16_pss_apply's, byte for
//              byte: field elements have one representation and the sums are exact.  Columns l .. 2 l are appended to
//              `mats` behind the existing blocks (pack_entry below, the text the host test runs).
//   hiding     any t = l - 1 parties see shares whose t x (t + 1) block of blind columns has rank t (tested on the host
//              for every subset), so for any other secrets a blind vector with the same shares exists.
//   layouts    CHUNKS: secret (e, c) = values[e l + c], zero past the end (pack_from_witness,
//              groth16/examples/sha256.rs:97-121).  DFFT: n_values = m = 2^k >= l and secret (e, c) = x[e + c m / l] with
//              x the bit-reversed vector (QAP::pss, groth16/src/qap.rs:151-165).  rev_k(e + c m / l) =
//              rev_(k - log l)(e) * l + rev_(log l)(c): the l sources of a chunk are one contiguous run of l elements
//              (source_index), read by ONE lane, and the n shares of a chunk are written by that lane at stride `chunks`
//              -- consecutive lanes write consecutive addresses of every party's row, the 4x larger side of the traffic.
//   expansion  element i of stream s of a seed: the two SHA-256 digests of
//              "dg16fe" || seed[32] || le64(s) || le64(i) || byte(j), j = 0, 1, read as one 512-bit little-endian
//              integer and reduced mod r (bias below 2^-250).  The message is 55 bytes: with the padding exactly ONE
//              compression block, whose 16 words are a per-(seed, stream) template plus the index.  The reduction is two
//              Montgomery products per half: x * R^2 * R^-1 = x R mod r is exact for ANY x < 2^256 (the product of a
//              value below 2^256 and one below r, divided by R, stays below 2 r), and 2^256 in Montgomery form is R^2.
//   request    dg16_request_pack makes its blinds inside the packing kernel (blind (e, k) of output v = element e l + k of
//              stream v): they are never uploaded and never reach HBM.
//   slices     the shares of a slice of chunks are computed into channel 0's workspace and copied out as n rows; the
//              explicit blinds and, for CHUNKS, the values of a slice are uploaded per slice.  A DFFT input is resident
//              in full for the call: a slice of consecutive chunks reads runs spread over the whole vector, and the
//              input is a fifth of what moves.
//
// The hash, the reduction, the index plan and the matrix entries are host and device text:
// tests/host_arith/host_request_pack.cpp runs them on a CPU against hashlib, Python's % and the oracle.  The field
// product beneath them is NOT one text (fp.h: product scanning on the device, CIOS on the host): the edge words of the
// reduction are tested on the host's; for the device's the bound above is the argument -- (a b + m p) / R < 2 p for
// any a < 2^256 and b < p, which reduce_once finishes -- and the GPU expansion test feeds it unreduced digests.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fp.h"
#include "slices.h"
#include "types.h"

namespace dg16 {
namespace pscal {

constexpr unsigned kMaxL = 8;                          // dg16_pss_create's bound
constexpr int kLayoutChunks = 0, kLayoutDfft = 1;      // DG16_PACK_CHUNKS, DG16_PACK_DFFT
constexpr size_t kSliceOutputsDefault = (size_t)1 << 21;   // share elements of a slice (64 MB) where the context sets none

// ---- SHA-256, one block ---------------------------------------------------------------------------------------------------
DG_HD uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// the compression of ONE block from the initial state (FIPS 180-4, 6.2.2): w = the block as 16 big-endian words,
// out = the digest as 8 big-endian words
DG_HD void sha256_block(const uint32_t w16[16], uint32_t out[8]) {
  constexpr uint32_t K[64] = {
      0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
      0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
      0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
      0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
      0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
      0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
      0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
      0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
  constexpr uint32_t H0[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                              0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = w16[i];
  uint32_t a = H0[0], b = H0[1], c = H0[2], d = H0[3], e = H0[4], f = H0[5], g = H0[6], h = H0[7];
#pragma unroll
  for (int i = 0; i < 64; i++) {
    if (i >= 16) {   // the schedule in a ring of 16 words
      const uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
      const uint32_t s0 = rotr(w15, 7) ^ rotr(w15, 18) ^ (w15 >> 3);
      const uint32_t s1 = rotr(w2, 17) ^ rotr(w2, 19) ^ (w2 >> 10);
      w[i & 15] = w[i & 15] + s0 + w[(i + 9) & 15] + s1;
    }
    const uint32_t S1 = rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25);
    const uint32_t ch = (e & f) ^ (~e & g);
    const uint32_t t1 = h + S1 + ch + K[i] + w[i & 15];
    const uint32_t S0 = rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22);
    const uint32_t mj = (a & b) ^ (a & c) ^ (b & c);
    const uint32_t t2 = S0 + mj;
    h = g; g = f; f = e; e = d + t1;
    d = c; c = b; b = a; a = t1 + t2;
  }
  out[0] = H0[0] + a; out[1] = H0[1] + b; out[2] = H0[2] + c; out[3] = H0[3] + d;
  out[4] = H0[4] + e; out[5] = H0[5] + f; out[6] = H0[6] + g; out[7] = H0[7] + h;
}

// ---- the message of one element ---------------------------------------------------------------------------------------------
// The padded block of "dg16fe" || seed || le64(stream) || le64(index) || byte(j) with index = 0 and j = 0: byte p of the
// block is bits 24 - 8 (p % 4) .. of word p / 4.  Bytes 46 .. 53 hold the index, byte 54 j, byte 55 the 0x80 of the
// padding, bytes 56 .. 63 the length in bits (440), big-endian.
struct Block {
  uint32_t w[16];
};
DG_HD void put_byte(uint32_t* w, int pos, uint32_t b) { w[pos >> 2] |= (b & 0xffu) << (24 - 8 * (pos & 3)); }
DG_HD Block block_template(const uint8_t seed[32], uint64_t stream) {
  Block t;
  for (int i = 0; i < 16; i++) t.w[i] = 0;
  const char tag[6] = {'d', 'g', '1', '6', 'f', 'e'};
  for (int i = 0; i < 6; i++) put_byte(t.w, i, (uint8_t)tag[i]);
  for (int i = 0; i < 32; i++) put_byte(t.w, 6 + i, seed[i]);
  for (int i = 0; i < 8; i++) put_byte(t.w, 38 + i, (uint32_t)(stream >> (8 * i)));
  put_byte(t.w, 55, 0x80u);
  t.w[15] = 55 * 8;
  return t;
}
DG_HD uint32_t bswap32(uint32_t x) { return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24); }
// the block of (index, j): the index's bytes 0, 1 end word 11, bytes 2 .. 5 are word 12, bytes 6, 7 begin word 13
DG_HD void block_of(const Block& t, uint64_t index, uint32_t j, uint32_t w[16]) {
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = t.w[i];
  const uint32_t lo = (uint32_t)index, hi = (uint32_t)(index >> 32);
  w[11] |= ((lo & 0xffu) << 8) | ((lo >> 8) & 0xffu);
  w[12] = bswap32((lo >> 16) | (hi << 16));
  w[13] |= (((hi >> 16) & 0xffu) << 24) | (((hi >> 24) & 0xffu) << 16) | ((j & 0xffu) << 8);
}

// ---- 512 bits mod r -----------------------------------------------------------------------------------------------------------
// (lo + 2^256 hi) mod r in Montgomery form, for ANY 8-word lo and hi (see the header comment)
template <class Fr>
DG_HD Fr reduce512_mont(const uint32_t lo[8], const uint32_t hi[8]) {
  static_assert(Fr::NL == 8, "scalar fields of 8 words");
  Fr a, b;
#pragma unroll
  for (int i = 0; i < 8; i++) { a.l[i] = lo[i]; b.l[i] = hi[i]; }
  const Fr r2 = Fr::r2();
  return a * r2 + (b * r2) * r2;
}

// element `index` of the stream whose template is t; Montgomery form if mont, else canonical
template <class Fr>
DG_HD Fr expand_element(const Block& t, uint64_t index, bool mont) {
  uint32_t w[16], d0[8], d1[8];
  block_of(t, index, 0, w);
  sha256_block(w, d0);
  block_of(t, index, 1, w);
  sha256_block(w, d1);
  // digest bytes 4 k .. 4 k + 3 are digest word k big-endian: as a little-endian limb, the word byte-swapped
#pragma unroll
  for (int i = 0; i < 8; i++) { d0[i] = bswap32(d0[i]); d1[i] = bswap32(d1[i]); }
  const Fr v = reduce512_mont<Fr>(d0, d1);
  return mont ? v : v.from_mont();
}

// ---- the index plan ---------------------------------------------------------------------------------------------------------------
DG_HD unsigned log2_exact(size_t v) {
  unsigned k = 0;
  while (((size_t)1 << k) < v) k++;
  return k;
}
DG_HD size_t bitrev(size_t v, unsigned bits) {
  size_t r = 0;
  for (unsigned i = 0; i < bits; i++) r |= ((v >> i) & 1) << (bits - 1 - i);
  return r;
}
// chunks of a vector of n_values under a layout (DFFT: n_values = m, a multiple of l)
DG_HD size_t chunks_of(int layout, size_t n_values, unsigned l) {
  return layout == kLayoutDfft ? n_values / l : (n_values + l - 1) / l;
}
// what a DFFT call accepts
DG_HD bool dfft_size_ok(size_t m, unsigned l) { return m >= l && !(m & (m - 1)); }
// the index in `values` of secret c of chunk e; an index >= n_values is the zero padding (CHUNKS only)
DG_HD size_t source_index(int layout, unsigned l, size_t n_values, size_t e, unsigned c) {
  if (layout != kLayoutDfft) return e * l + c;
  const unsigned log_l = log2_exact(l), log_c = log2_exact(n_values) - log_l;   // chunks = 2^log_c
  return bitrev(e, log_c) * l + bitrev(c, log_l);
}
// chunks per slice under a setting of `outputs` share elements per slice: a multiple of 64, at least 64
DG_HD size_t slice_chunks(size_t outputs, unsigned n) {
  const size_t c = outputs / n / 64 * 64;
  return c < 64 ? 64 : c;
}

// ---- the pack matrix, all 2 l columns ----------------------------------------------------------------------------------------------
template <class Fr>
DG_HD Fr root_of_unity(unsigned log_n) {
  Fr w;
  for (int i = 0; i < Fr::NL; i++) w.l[i] = Fr::Params::TWO_ADIC_ROOT[i];
  for (unsigned i = log_n; i < (unsigned)Fr::Params::TWO_ADICITY; i++) w = w.sqr();
  return w;
}
// P[j][i], j < n = 4 l, i < s = 2 l, Montgomery form: sum_{k<s} wn^(j k) * s^-1 * g^-k * ws^(-i k) (pss.rs:72-92: the
// inverse transform on the coset g <ws> of size s, then the forward transform on <wn>).  For i < l this is
// pss_setup_kernel's pack[j][i], sum for sum.
template <class Fr>
DG_HD Fr pack_entry(unsigned l, unsigned j, unsigned i) {
  const unsigned n = 4 * l, s = 2 * l;
  const Fr wn = root_of_unity<Fr>(log2_exact(n)), ws = root_of_unity<Fr>(log2_exact(s));
  Fr g;
  for (int q = 0; q < Fr::NL; q++) g.l[q] = Fr::Params::GEN[q];
  const Fr ws_inv = ws.inv(), g_inv = g.inv(), s_inv = Fr::from_u32(s).inv();
  Fr acc = Fr::zero();
  for (unsigned k = 0; k < s; k++)
    acc = acc + wn.pow_u64((uint64_t)j * k) * g_inv.pow_u64(k) * ws_inv.pow_u64((uint64_t)i * k);
  return acc * s_inv;
}

}  // namespace pscal
}  // namespace dg16

#if defined(__HIPCC__)
// ---- device side --------------------------------------------------------------------------------------------------------------------
#include "dist_impl.h"

namespace dg16 {
namespace pscal {

// the blind columns of a handle: blind[j][k] = P[j][l + k], one lane per entry (n l <= 256)
template <class Fr>
__global__ void pss_blind_cols_kernel(unsigned l, Fr* __restrict__ blind) {
  const unsigned tid = threadIdx.x;
  if (tid < 4 * l * l) blind[tid] = pack_entry<Fr>(l, tid / l, l + tid % l);
}

// out of line: the two compressions are about 4 000 instructions, and a lane of the packing kernel needs l of them
template <class Fr>
__device__ __noinline__ void expand_call(const Block* t, uint64_t index, bool mont, Fr* out) {
  *out = expand_element<Fr>(*t, index, mont);
}

template <class Fr>
__global__ void __launch_bounds__(256) fr_expand_kernel(Block t, uint64_t first, size_t n, bool mont,
                                                         Fr* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = expand_element<Fr>(t, first + (uint64_t)i, mont);
}

enum { kBlindNone = 0, kBlindGiven = 1, kBlindSeed = 2 };

// One lane per chunk of the slice: chunk lo + i, i < cnt.  values[0] is element src_off of the caller's vector of
// n_values (CHUNKS uploads a slice, DFFT the whole vector).  blinds: the slice's [cnt][L] (kBlindGiven).  out: [n][cnt].
template <class Fr, unsigned L, int BLIND>
__global__ void __launch_bounds__(256) pack_scalars_kernel(const Fr* __restrict__ M, const Fr* __restrict__ MB, int layout,
                                                            const Fr* __restrict__ values, size_t n_values,
                                                            size_t src_off, const Fr* __restrict__ blinds, Block t,
                                                            bool mont, size_t lo, size_t cnt, Fr* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cnt) return;
  const size_t e = lo + i;
  constexpr unsigned N = 4 * L, COLS = BLIND == kBlindNone ? L : 2 * L;
  Fr v[COLS];
#pragma unroll
  for (unsigned c = 0; c < L; c++) {
    const size_t idx = source_index(layout, L, n_values, e, c);
    v[c] = idx < n_values ? values[idx - src_off] : Fr::zero();
  }
  if constexpr (BLIND == kBlindGiven) {
#pragma unroll
    for (unsigned k = 0; k < L; k++) v[L + k] = blinds[i * L + k];
  }
  if constexpr (BLIND == kBlindSeed) {
#pragma unroll
    for (unsigned k = 0; k < L; k++) expand_call<Fr>(&t, (uint64_t)e * L + k, mont, &v[L + k]);
  }
#pragma unroll 1
  for (unsigned r = 0; r < N; r++) {
    Fr acc = Fr::zero();
#pragma unroll
    for (unsigned c = 0; c < L; c++) acc = acc + M[r * L + c] * v[c];
    if constexpr (BLIND != kBlindNone) {
#pragma unroll
      for (unsigned k = 0; k < L; k++) acc = acc + MB[r * L + k] * v[L + k];
    }
    out[(size_t)r * cnt + i] = acc;
  }
}

// the blind columns of a handle, Montgomery form, [n][l] (behind every block pss_setup_kernel writes)
template <class Fr>
inline const Fr* blind_cols(const dg16_pss* pp) {
  return (const Fr*)pp->mats + 6 * (size_t)pp->n * pp->l + pp->n;
}

// One vector: shares_host[r][e] (party-major, [n][chunks]) from values_host[0 .. n_values).  blind: kBlindNone, kBlindGiven
// (blinds_host [chunks][l]) or kBlindSeed (template t, form mont).  The caller holds channel 0 and checked the arguments.
// Workspace slots of channel 0: 0 values, 1 the slice's blinds, 2 the slice's shares.
template <class Fr>
void pack_scalars_typed(Call& k, const dg16_pss* pp, int layout, const void* values_host, size_t n_values, int blind,
                        const void* blinds_host, const Block& t, bool mont, void* shares_host) {
  if (!n_values) return;
  const unsigned l = pp->l, n = pp->n;
  const size_t chunks = chunks_of(layout, n_values, l);
  const size_t per = slice_chunks(k.ctx->points_mul_slice ? k.ctx->points_mul_slice : kSliceOutputsDefault, n);
  const size_t stride = launch_stride(chunks, per);
  const bool whole = layout == kLayoutDfft;
  Fr* vals = (Fr*)ws(k.c, 0, (whole ? n_values : stride * l) * sizeof(Fr));
  Fr* bl = blind == kBlindGiven ? (Fr*)ws(k.c, 1, stride * l * sizeof(Fr)) : nullptr;
  Fr* out = (Fr*)ws(k.c, 2, (size_t)n * stride * sizeof(Fr));
  const Fr* M = (const Fr*)pp->mats;
  const Fr* MB = blind_cols<Fr>(pp);
  if (whole) DG_HIP(hipMemcpyAsync(vals, values_host, n_values * sizeof(Fr), hipMemcpyHostToDevice, k.s()));
  for (size_t lo = 0; lo < chunks; lo += per) {
    const size_t cnt = chunks - lo < per ? chunks - lo : per;
    size_t src_off = 0;
    if (!whole) {
      src_off = lo * l;
      const size_t have = n_values - src_off < cnt * l ? n_values - src_off : cnt * l;
      // (the copy is ordered behind the previous slice's kernel on the stream)
      DG_HIP(hipMemcpyAsync(vals, (const Fr*)values_host + src_off, have * sizeof(Fr), hipMemcpyHostToDevice, k.s()));
    }
    if (bl)
      DG_HIP(hipMemcpyAsync(bl, (const Fr*)blinds_host + lo * l, cnt * l * sizeof(Fr), hipMemcpyHostToDevice, k.s()));
    const dim3 grid(nblk(cnt)), block(256);
    k.begin_dominant();      // the kernel of the call's last slice is what dg16_last_kernel_ms(which = 1) reports
#define DG_PACK_LAUNCH(LL, BB)                                                                                          \
  hipLaunchKernelGGL((pack_scalars_kernel<Fr, LL, BB>), grid, block, 0, k.s(), M, MB, layout, (const Fr*)vals, n_values, \
                     src_off, (const Fr*)bl, t, mont, lo, cnt, out)
#define DG_PACK_BLIND(LL)                                         \
  switch (blind) {                                                \
    case kBlindNone: DG_PACK_LAUNCH(LL, kBlindNone); break;       \
    case kBlindGiven: DG_PACK_LAUNCH(LL, kBlindGiven); break;     \
    default: DG_PACK_LAUNCH(LL, kBlindSeed); break;               \
  }
    switch (l) {
      case 1: DG_PACK_BLIND(1) break;
      case 2: DG_PACK_BLIND(2) break;
      case 4: DG_PACK_BLIND(4) break;
      default: DG_PACK_BLIND(8) break;
    }
#undef DG_PACK_BLIND
#undef DG_PACK_LAUNCH
    DG_HIP(hipGetLastError());
    k.end_dominant();
    // [n][cnt] -> columns lo .. lo + cnt of [n][chunks]
    DG_HIP(hipMemcpy2DAsync((Fr*)shares_host + lo, chunks * sizeof(Fr), out, cnt * sizeof(Fr), cnt * sizeof(Fr), n,
                            hipMemcpyDeviceToHost, k.s()));
  }
  DG_HIP(hipStreamSynchronize(k.s()));
}

}  // namespace pscal
}  // namespace dg16
#endif
