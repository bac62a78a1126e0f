// Test-only: the index rule of distributed-groth16_amd/csrc/h_odd.h compiled with the HOST compiler into a stand-alone
// program, so that tests/test_h_odd_host.py compares the text the kernel runs with the Python rule and runs it under the
// address and undefined-behaviour sanitizers.  Never part of the product.
//
//   host_h_odd            prints "l chunks c i elem row evaluation" for l in 1, 2, 4, 8, chunks (= m/l) in 1 .. 8, every
//                         c < chunks and i < l
//
// It also walks the rule the way h_king_kernel does -- over a gathered buffer [n][3][2 chunks] and a send buffer
// [n][chunks] of exactly the sizes dg16_ext_wit_h allocates -- touching every address the kernel touches, so an index
// out of range is a sanitizer report, and returns 1 if an address repeats within a chunk or lies outside.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../distributed-groth16_amd/csrc/h_odd.h"

using namespace dg16;

int main() {
  int bad = 0;
  for (unsigned l = 1; l <= 8; l *= 2) {
    const unsigned n = 4 * l;
    for (size_t chunks = 1; chunks <= 8; chunks++) {
      const size_t vec = 2 * chunks, rec = 3 * vec;
      std::vector<uint32_t> gathered(n * rec, 0), send(n * chunks, 0);
      std::vector<uint8_t> unpack(l * n, 1);
      for (size_t c = 0; c < chunks; c++) {
        for (unsigned i = 0; i < l; i++) {
          const hodd::Source s = hodd::source(l, c, i);
          printf("%u %zu %zu %u %zu %u %zu\n", l, chunks, c, i, s.elem, s.row, hodd::evaluation(l, s));
          if (s.elem >= vec || s.row >= l) bad = 1;
          for (unsigned j = 0; j < n; j++) {
            if (!unpack[(size_t)s.row * n + j]) bad = 1;
            for (unsigned v = 0; v < 3; v++) gathered[j * rec + v * vec + s.elem] += 1;
          }
        }
        for (unsigned j = 0; j < n; j++) send[j * chunks + c] += 1;
      }
      // every share of an element is read once per odd row it has: l / 2 times (once at l = 1, and element 2c not at all)
      for (unsigned j = 0; j < n; j++)
        for (unsigned v = 0; v < 3; v++)
          for (size_t e = 0; e < vec; e++) {
            const uint32_t want = l == 1 ? (uint32_t)(e & 1) : l / 2;
            if (gathered[j * rec + v * vec + e] != want) bad = 1;
          }
      for (uint32_t w : send)
        if (w != 1) bad = 1;
    }
  }
  return bad;
}
