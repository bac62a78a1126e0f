// Test-only: the decision function of distributed-groth16_amd/csrc/points_check.h (reduced coordinates, curve equation,
// r P by the fixed chain on the 29-bit-limb arithmetic) compiled with the HOST compiler into a stand-alone program, so
// that the CPU test (tests/test_points_check_host.py) runs exactly the text the kernel runs, under the address and
// undefined-behaviour sanitizers, and counts its group operations.  Never part of the product.
//
//   host_points_check chain              prints "chain <gid> <doublings> <additions>" per group: the fixed budget
//   host_points_check run <in> <out>     in:  u32 cases, then per case u32 gid, u32 subgroup, u64 n, n affine points
//                                        out: per point i32 verdict (pchk::Verdict), u32 doublings, u32 additions
//   gid = 2 * curve + group - 1
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../distributed-groth16_amd/csrc/points_check.h"

using namespace dg16;

namespace {

template <class F>
struct CountOps {
  uint32_t n[2] = {0, 0};
  XYZZ29<F> dbl(const XYZZ29<F>& a) { n[0]++; return a.dbl_pt(); }
  XYZZ29<F> madd(const XYZZ29<F>& a, const Affine29<F>& q, bool negate) { n[1]++; return a.madd(q, negate); }
};

template <int CURVE, int GROUP>
void run_case(bool subgroup, size_t n, const uint8_t* in, std::vector<uint8_t>& out) {
  using F = typename pchk::GroupOf<CURVE, GROUP>::F;
  for (size_t i = 0; i < n; i++) {
    Affine<F> p;
    memcpy(&p, in + i * sizeof p, sizeof p);
    CountOps<F> ops;
    const int32_t v = pchk::classify<CURVE, GROUP>(p, subgroup, ops);
    const uint32_t rec[3] = {(uint32_t)v, ops.n[0], ops.n[1]};
    out.insert(out.end(), (const uint8_t*)rec, (const uint8_t*)rec + sizeof rec);
  }
}

template <int CURVE, int GROUP>
size_t point_bytes() { return sizeof(Affine<typename pchk::GroupOf<CURVE, GROUP>::F>); }

#define BY_GROUP(gid, CALL)                                       \
  switch (gid) {                                                  \
    case 0: { constexpr int C = 0, G = 1; CALL; break; }          \
    case 1: { constexpr int C = 0, G = 2; CALL; break; }          \
    case 2: { constexpr int C = 1, G = 1; CALL; break; }          \
    case 3: { constexpr int C = 1, G = 2; CALL; break; }          \
    case 4: { constexpr int C = 2, G = 1; CALL; break; }          \
    case 5: { constexpr int C = 2, G = 2; CALL; break; }          \
    default: return 2;                                            \
  }

template <int CURVE, int GROUP>
void print_chain(int gid) {
  using N = pchk::NafOf<typename pchk::GroupOf<CURVE, GROUP>::RP>;
  printf("chain %d %d %d\n", gid, N::v.top, N::v.adds);
}

int chain() {
  for (int gid = 0; gid < 6; gid++) {
    BY_GROUP(gid, (print_chain<C, G>(gid)));
  }
  return 0;
}

int run(const char* fin, const char* fout) {
  FILE* f = fopen(fin, "rb");
  if (!f) return 2;
  std::vector<uint8_t> in;
  uint8_t chunk[1 << 16];
  size_t got;
  while ((got = fread(chunk, 1, sizeof chunk, f)) > 0) in.insert(in.end(), chunk, chunk + got);
  fclose(f);
  std::vector<uint8_t> out;
  size_t pos = 0;
  uint32_t cases;
  if (in.size() < 4) return 2;
  memcpy(&cases, in.data(), 4);
  pos = 4;
  for (uint32_t c = 0; c < cases; c++) {
    uint32_t gid, subgroup;
    uint64_t n;
    if (in.size() - pos < 16) return 2;
    memcpy(&gid, in.data() + pos, 4);
    memcpy(&subgroup, in.data() + pos + 4, 4);
    memcpy(&n, in.data() + pos + 8, 8);
    pos += 16;
    size_t pb = 0;
    BY_GROUP(gid, pb = (point_bytes<C, G>()));
    if ((in.size() - pos) / pb < n) return 2;
    BY_GROUP(gid, (run_case<C, G>(subgroup != 0, (size_t)n, in.data() + pos, out)));
    pos += n * pb;
  }
  if (pos != in.size()) return 2;
  f = fopen(fout, "wb");
  if (!f) return 2;
  fwrite(out.data(), 1, out.size(), f);
  fclose(f);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "chain")) return chain();
  if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
  fprintf(stderr, "usage: host_points_check chain | run <cases> <results>\n");
  return 2;
}
