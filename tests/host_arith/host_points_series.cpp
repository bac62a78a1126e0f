// Test-only: the term function, the chunk loop and the slice plan of distributed-groth16_amd/csrc/points_series.h and
// the decision function of dg16_srs_verify_contribution (points_check.h) compiled with the HOST compiler, so that the
// CPU tests (tests/test_points_series_host.py) run exactly the text the kernel and the verifier run.  Never part of the
// product.
#include <stdint.h>
#include <string.h>
#include "../../distributed-groth16_amd/csrc/points_series.h"
#include "../../distributed-groth16_amd/csrc/points_check.h"

using namespace dg16;

namespace {

// what series_kernel does for one slice, one "lane" per chunk: out[i], i < p.cnt, as canonical integers
template <class Fr>
void slice_terms(const pseries::SlicePlan& p, const Fr& first_m, const Fr& ratio_m, Fr* out) {
  for (size_t c = 0; c < p.chunks; c++) {
    const size_t i0 = pseries::chunk_begin(c);
    pseries::fill_chunk(first_m, ratio_m, p.exp0 + (uint64_t)i0, pseries::chunk_len(p, c), out + i0);
  }
  for (size_t i = 0; i < p.cnt; i++) out[i] = out[i].from_mont();
}

// the whole call: every slice of the plan, written where the slice says
template <class Fr>
int series(const uint32_t* first8, const uint32_t* ratio8, uint64_t start, size_t n, size_t slice, uint32_t* out) {
  Fr first, ratio;
  memcpy(&first, first8, 32);
  memcpy(&ratio, ratio8, 32);
  if (!pseries::below_modulus(first) || !pseries::below_modulus(ratio)) return -1;
  const Fr first_m = first.to_mont(), ratio_m = ratio.to_mont();
  slice = pseries::round_slice(slice);
  for (size_t s = 0, ns = pseries::slice_count(n, slice); s < ns; s++) {
    const pseries::SlicePlan p = pseries::plan_slice(n, slice, start, s);
    slice_terms(p, first_m, ratio_m, (Fr*)out + p.lo);
  }
  return 0;
}

// one term by the term function alone
template <class Fr>
void one_term(const uint32_t* first8, const uint32_t* ratio8, uint64_t e, uint32_t* out) {
  Fr first, ratio;
  memcpy(&first, first8, 32);
  memcpy(&ratio, ratio8, 32);
  const Fr t = pseries::term(first.to_mont(), ratio.to_mont(), e).from_mont();
  memcpy(out, &t, 32);
}

}  // namespace

extern "C" {

// the chunk length
unsigned hps_chunk(void) { return pseries::kChunk; }
// the plan of a call: slices (return value) and, per slice, lo | cnt | exp0 | chunks, then per chunk of every slice its
// begin and length in `chunks` (pairs, slice after slice); max_* bound the two arrays
size_t hps_plan(size_t n, size_t slice, uint64_t start, uint64_t* slices, size_t max_slices, uint64_t* chunks,
                size_t max_chunks) {
  slice = pseries::round_slice(slice);
  const size_t ns = pseries::slice_count(n, slice);
  size_t nc = 0;
  for (size_t s = 0; s < ns && s < max_slices; s++) {
    const pseries::SlicePlan p = pseries::plan_slice(n, slice, start, s);
    slices[4 * s] = p.lo;
    slices[4 * s + 1] = p.cnt;
    slices[4 * s + 2] = p.exp0;
    slices[4 * s + 3] = p.chunks;
    for (size_t c = 0; c < p.chunks && nc < max_chunks; c++, nc++) {
      chunks[2 * nc] = p.lo + pseries::chunk_begin(c);
      chunks[2 * nc + 1] = pseries::chunk_len(p, c);
    }
  }
  return ns;
}
// out[i] = first * ratio^(start + i) mod r, i < n (8 words each, canonical), through the plan and the chunk loop;
// -1 where first or ratio is not below r
int hps_series(int curve, const uint32_t* first8, const uint32_t* ratio8, uint64_t start, size_t n, size_t slice,
               uint32_t* out) {
  if (curve == 0) return series<bn254_fr>(first8, ratio8, start, n, slice, out);
  if (curve == 1) return series<bls12_381_fr>(first8, ratio8, start, n, slice, out);
  return series<bls12_377_fr>(first8, ratio8, start, n, slice, out);
}
// first * ratio^e mod r by the term function
void hps_term(int curve, const uint32_t* first8, const uint32_t* ratio8, uint64_t e, uint32_t* out) {
  if (curve == 0) one_term<bn254_fr>(first8, ratio8, e, out);
  else if (curve == 1) one_term<bls12_381_fr>(first8, ratio8, e, out);
  else one_term<bls12_377_fr>(first8, ratio8, e, out);
}
// the word of dg16_srs_verify_contribution from the outcomes of its checks; relations: 8 flags (1 = the equality fails)
uint32_t hps_decide(uint32_t after_failed, int bad_point, int identity, int base_differs, const uint8_t* relations) {
  pchk::P1Outcomes o = {};
  o.after_failed = after_failed;
  o.bad_point = bad_point != 0;
  o.identity = identity != 0;
  o.base_differs = base_differs != 0;
  for (int j = 0; j < pchk::kP1Relations; j++) o.relation_fails[j] = relations[j] != 0;
  return pchk::p1_decide(o);
}
int hps_skipped(uint32_t after_failed, int bad_point, int identity) {
  return pchk::p1_relations_skipped(after_failed, bad_point != 0, identity != 0) ? 1 : 0;
}

}  // extern "C"
