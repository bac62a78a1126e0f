// Test-only: the SHA-256 block, the 512-bit reduction, the seed expansion, the index plan and the pack-matrix entries of
// distributed-groth16_amd/csrc/pss_scalars.h compiled with the HOST compiler, so that the CPU tests
// (tests/test_request_pack_host.py) run the text the kernels run -- with ONE exception: Fp::operator* (fp.h) has a device
// body (product scanning) and a host body (CIOS), so the edge words of reduce512 are checked here on the host's
// multiplier only; the device's is held to the same bound by the argument in pss_scalars.h and runs on unreduced
// digests in tests/test_gpu_request_pack.py.  Never part of the product.
#include <stdint.h>
#include <string.h>
#include "../../distributed-groth16_amd/csrc/pss_scalars.h"

using namespace dg16;

namespace {

template <class Fr>
void reduce(const uint32_t* lo, const uint32_t* hi, uint32_t* out) {
  const Fr v = pscal::reduce512_mont<Fr>(lo, hi).from_mont();
  memcpy(out, &v, 32);
}

template <class Fr>
void expand(const uint8_t* seed, uint64_t stream, uint64_t first, size_t n, bool mont, uint32_t* out) {
  const pscal::Block t = pscal::block_template(seed, stream);
  for (size_t i = 0; i < n; i++) {
    const Fr v = pscal::expand_element<Fr>(t, first + i, mont);
    memcpy(out + 8 * i, &v, 32);
  }
}

template <class Fr>
void matrix(unsigned l, uint32_t* out) {
  for (unsigned j = 0; j < 4 * l; j++)
    for (unsigned i = 0; i < 2 * l; i++) {
      const Fr v = pscal::pack_entry<Fr>(l, j, i).from_mont();
      memcpy(out + ((size_t)j * 2 * l + i) * 8, &v, 32);
    }
}

}  // namespace

#define BY_CURVE(curve, call)                  \
  do {                                         \
    if ((curve) == 0) { using Fr = bn254_fr; call; }           \
    else if ((curve) == 1) { using Fr = bls12_381_fr; call; }  \
    else { using Fr = bls12_377_fr; call; }                    \
  } while (0)

extern "C" {

// the 64-byte block of (seed, stream, index, j) as bytes, and its digest as bytes
void hrp_block(const uint8_t* seed, uint64_t stream, uint64_t index, uint32_t j, uint8_t* block64, uint8_t* digest32) {
  const pscal::Block t = pscal::block_template(seed, stream);
  uint32_t w[16], d[8];
  pscal::block_of(t, index, j, w);
  for (int i = 0; i < 64; i++) block64[i] = (uint8_t)(w[i / 4] >> (24 - 8 * (i % 4)));
  pscal::sha256_block(w, d);
  for (int i = 0; i < 32; i++) digest32[i] = (uint8_t)(d[i / 4] >> (24 - 8 * (i % 4)));
}
// (lo + 2^256 hi) mod r, canonical
void hrp_reduce512(int curve, const uint32_t* lo, const uint32_t* hi, uint32_t* out) { BY_CURVE(curve, reduce<Fr>(lo, hi, out)); }
// elements first .. first + n of a stream
void hrp_expand(int curve, const uint8_t* seed, uint64_t stream, uint64_t first, size_t n, int mont, uint32_t* out) {
  BY_CURVE(curve, expand<Fr>(seed, stream, first, n, mont != 0, out));
}
size_t hrp_chunks(int layout, size_t n_values, unsigned l) { return pscal::chunks_of(layout, n_values, l); }
int hrp_dfft_size_ok(size_t m, unsigned l) { return pscal::dfft_size_ok(m, l) ? 1 : 0; }
size_t hrp_source_index(int layout, unsigned l, size_t n_values, size_t e, unsigned c) {
  return pscal::source_index(layout, l, n_values, e, c);
}
size_t hrp_slice_chunks(size_t outputs, unsigned n) { return pscal::slice_chunks(outputs, n); }
// P[j][i], j < 4 l, i < 2 l, canonical, 8 words each
void hrp_matrix(int curve, unsigned l, uint32_t* out) { BY_CURVE(curve, matrix<Fr>(l, out)); }

}  // extern "C"
