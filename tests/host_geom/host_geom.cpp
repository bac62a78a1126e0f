// Test-only: the MSM's planning arithmetic (distributed-groth16_amd/csrc/msm_geom.h) built with the HOST compiler, so that
// tests/test_msm_geom_host.py checks the code that ships against the Python mirror (tests/witness_shapes.py) without a GPU
// (-m "not gpu").  Thin C wrappers, nothing else.  Never part of the product.
#include "../../distributed-groth16_amd/csrc/msm_geom.h"

using namespace dg16;

extern "C" {

unsigned hg_window_bits(size_t n, int table, unsigned scalar_bits) { return msm_window_bits(n, table != 0, scalar_bits); }

// out: c, nwin, log_nb, seg_log, seg_cap, bw, table, rows, region
void hg_geometry(size_t n, unsigned scalar_bits, int table, unsigned c_fixed, unsigned stride, uint64_t* out) {
  const MsmGeom g = msm_geometry(n, scalar_bits, table != 0, c_fixed, stride);
  out[0] = g.c; out[1] = g.nwin; out[2] = g.log_nb; out[3] = g.seg_log; out[4] = g.seg_cap;
  out[5] = g.bw; out[6] = g.table; out[7] = g.rows; out[8] = g.region;
}

// out: row_log, rows_log
void hg_row_geometry(unsigned log_nb, unsigned* out) {
  MsmGeom g{};
  g.log_nb = log_nb;
  const RowGeom r = row_geometry(g);
  out[0] = r.row_log; out[1] = r.rows_log;
}

// out: slices, per
void hg_giant_geometry(unsigned nseg, unsigned* out) { giant_geometry(nseg, out[0], out[1]); }

unsigned hg_table_stride_for(size_t full_bytes, size_t budget, unsigned nwin) {
  return table_stride_for(full_bytes, budget, nwin);
}

// the partition choice for a geometry given by (nwin, bw, log_nb); out: partitioned, low_bits, nparts, nblk1
void hg_partition_plan(unsigned nwin, unsigned bw, unsigned log_nb, size_t n, unsigned* out) {
  MsmGeom g{};
  g.nwin = nwin; g.bw = bw; g.log_nb = log_nb;
  const PartPlan p = msm_partition_plan(g, n);
  out[0] = p.partitioned; out[1] = p.pg.low_bits; out[2] = p.pg.nparts; out[3] = p.pg.nblk1;
}

// out: split, c_small, scalar_bits
void hg_plain_plan(int nine_limbs, unsigned dim, size_t n, int split_applies, unsigned* out) {
  const PlainPlan p = msm_plain_plan(nine_limbs != 0, dim, n, split_applies != 0);
  out[0] = p.split; out[1] = p.c_small; out[2] = p.scalar_bits;
}

// the constants the mirror copies: kMinSegLog, kMaxSegLog, kMinLanesLog, kGiantSegs, kGiantSlices, kGiantSliceSegs,
// kPartScalars, kPartMaxLowBits, kGlvBits, kGlv4Bits
void hg_constants(unsigned* out) {
  out[0] = kMinSegLog; out[1] = kMaxSegLog; out[2] = kMinLanesLog; out[3] = kGiantSegs; out[4] = kGiantSlices;
  out[5] = kGiantSliceSegs; out[6] = kPartScalars; out[7] = kPartMaxLowBits; out[8] = kGlvBits; out[9] = kGlv4Bits;
}

}
