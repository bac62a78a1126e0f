// Test-only: the planning of dg16_groth16_setup_srs (distributed-groth16_amd/csrc/setup_srs_plan.h) built with the HOST
// compiler, so that tests/test_setup_srs_plan.py checks the code that ships without a GPU (-m "not gpu").  Thin C wrappers,
// nothing else.  Never part of the product.
#include "../../distributed-groth16_amd/csrc/setup_srs_plan.h"

using namespace dg16;

extern "C" {

void sp_limits(unsigned* out) { out[0] = srs::kWaveFrom; out[1] = srs::kMsmFrom; }

unsigned sp_path(size_t len) { return (unsigned)srs::path_of(len); }

size_t sp_segment_len(unsigned a, unsigned b, unsigned c, int instance_term) {
  return srs::segment_len(a, b, c, instance_term != 0);
}

// summary: columns[4] | terms[4] | slices | wave wires | msm wires.  slices: 6 words each (lo, hi, k0, k1, w0, w1), at most
// cap of them; wave, msm: at most nv words each.  Returns the number of slices.
size_t sp_plan(const uint32_t* seg_ptr, size_t nv, size_t slice, uint64_t* summary, uint32_t* slices, size_t cap,
               uint32_t* wave, uint32_t* msm) {
  const srs::Plan p = srs::make_plan(seg_ptr, nv, slice);
  for (int i = 0; i < 4; i++) { summary[i] = p.columns[i]; summary[4 + i] = p.terms[i]; }
  summary[8] = p.slices.size(); summary[9] = p.wave.size(); summary[10] = p.msm.size();
  for (size_t i = 0; i < p.slices.size() && i < cap; i++) {
    const srs::Slice& s = p.slices[i];
    uint32_t* o = slices + 6 * i;
    o[0] = s.lo; o[1] = s.hi; o[2] = s.k0; o[3] = s.k1; o[4] = s.w0; o[5] = s.w1;
  }
  for (size_t i = 0; i < p.wave.size(); i++) wave[i] = p.wave[i];
  for (size_t i = 0; i < p.msm.size(); i++) msm[i] = p.msm[i];
  return p.slices.size();
}

}
