// Mutation driver for the host parsers of libdg16 (csrc/formats.hip: dg16_r1cs_parse, dg16_zkey_parse,
// dg16_arkkey_layout; csrc/serialize.hip: dg16_proof_decompress), meant to be built with the host compiler and
// -fsanitize=address,undefined together with those two sources (tests/test_parser_mutation.py does) -- a stand-alone
// program: nothing here touches a GPU.
//
//   mutate_parsers <format> <seed file> <count>
//   format: r1cs | zkey | arkkey | arkkey_vk | proof | proof_validate
//
// Every mutant is parsed from a heap block of exactly its length, so a read one byte past the input is a sanitizer
// report.  On acceptance everything the handle exposes is walked -- every matrix, the first and last byte of every
// point array, the wire map -- and the handle is freed.  Mutants, from a fixed-seed generator (the run is reproducible):
//   fields      every u32 / u64 count, size or length field of the seed overwritten in turn with
//               0, 1, v - 1, v + 1, 2^31, 2^32 - 1, 2^63, 2^64 - 1 (the values that fit the field);
//   flips       1-4 bytes xor-ed or overwritten, three times out of four within the first 2 KB;
//   truncation  the seed cut at a random length (not for proof.bin: dg16_proof_decompress takes exactly 128 bytes).
// <count> random mutants follow the field mutants, one in six of them a truncation.
// Output: `rc <code> <mutants>` per return code, `accepted` / `refused` totals, and `field_violations <n>`: the number of
// field mutants that were ACCEPTED although the field governs how many bytes the parser reads and the value exceeds the
// length of the file.  Such a mutant is listed on its own line, and the exit status is 1.  (Four header fields of an
// .r1cs -- the three public / private input counts and the label count -- describe no bytes of the file and are not
// read back by the parser: they are overwritten too, and may be accepted.)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/dg16.h"

namespace {

struct Rng {   // xorshift64*
  uint64_t s;
  uint64_t next() {
    s ^= s >> 12;
    s ^= s << 25;
    s ^= s >> 27;
    return s * 0x2545F4914F6CDD1Dull;
  }
  size_t below(size_t n) { return n ? (size_t)(next() % n) : 0; }
};

struct Field {
  size_t off;
  int width;       // 4 or 8 bytes
  bool sized;      // governs how many bytes the parser reads
  std::string name;
};

volatile uint64_t g_sink;

uint64_t rd(const std::vector<uint8_t>& b, size_t off, int width) {
  uint64_t v = 0;
  memcpy(&v, b.data() + off, width);
  return v;
}

void touch(const void* p, size_t bytes) {   // first and last byte
  if (!bytes) return;
  const volatile uint8_t* q = (const volatile uint8_t*)p;
  g_sink += q[0];
  g_sink += q[bytes - 1];
}

void walk(const dg16_csr& m) {
  uint64_t acc = 0;
  if (m.row_ptr)
    for (uint64_t i = 0; i <= m.n_rows; i++) acc += m.row_ptr[i];
  for (uint64_t j = 0; j < m.nnz; j++) acc += m.col[j];
  for (uint64_t j = 0; j < m.nnz; j++) acc += ((const uint8_t*)m.coeff)[32 * j] + ((const uint8_t*)m.coeff)[32 * j + 31];
  g_sink += acc;
}

// ---- where the seed keeps its counts, sizes and lengths ----------------------------------------------------------------
// iden3 container: "magic" | version u32 | sections u32 | { id u32 | size u64 | payload }
std::map<uint32_t, size_t> container_fields(const std::vector<uint8_t>& b, std::vector<Field>& out) {
  std::map<uint32_t, size_t> payload;
  out.push_back({8, 4, true, "section count"});
  const uint32_t count = (uint32_t)rd(b, 8, 4);
  size_t off = 12;
  for (uint32_t i = 0; i < count; i++) {
    const uint32_t id = (uint32_t)rd(b, off, 4);
    out.push_back({off + 4, 8, true, "size of section " + std::to_string(id)});
    payload.emplace(id, off + 12);
    off += 12 + rd(b, off + 4, 8);
  }
  return payload;
}

std::vector<Field> fields_of(const std::string& format, const std::vector<uint8_t>& b) {
  std::vector<Field> out;
  if (format == "r1cs") {
    auto sec = container_fields(b, out);
    const size_t h = sec.at(1);
    out.push_back({h, 4, true, "field size"});
    out.push_back({h + 36, 4, true, "n_wires"});
    out.push_back({h + 40, 4, false, "n_pub_out"});
    out.push_back({h + 44, 4, false, "n_pub_in"});
    out.push_back({h + 48, 4, false, "n_prv_in"});
    out.push_back({h + 52, 8, false, "n_labels"});
    out.push_back({h + 60, 4, true, "n_constraints"});
    const uint32_t nc = (uint32_t)rd(b, h + 60, 4);
    size_t p = sec.at(2);
    for (uint32_t c = 0; c < 3 * nc; c++) {
      out.push_back({p, 4, true, "terms of linear combination " + std::to_string(c)});
      p += 4 + 36 * (size_t)rd(b, p, 4);
    }
  } else if (format == "zkey") {
    auto sec = container_fields(b, out);
    const size_t h = sec.at(2);
    out.push_back({h, 4, true, "n8q"});
    out.push_back({h + 36, 4, true, "n8r"});
    out.push_back({h + 72, 4, true, "n_vars"});
    out.push_back({h + 76, 4, true, "n_public"});
    out.push_back({h + 80, 4, true, "domain_size"});
    out.push_back({sec.at(4), 4, true, "n_coeffs"});
  } else if (format == "arkkey" || format == "arkkey_vk") {
    dg16_arkkey_layout_t lay;
    if (dg16_arkkey_layout(b.data(), b.size(), format == "arkkey_vk", &lay) != DG16_OK) {
      fprintf(stderr, "the seed is not a valid key file: %s\n", dg16_codec_error());
      exit(2);
    }
    out.push_back({(size_t)lay.off_ic - 8, 8, true, "len gamma_abc_g1"});
    if (format == "arkkey") {
      out.push_back({(size_t)lay.off_a - 8, 8, true, "len a_query"});
      out.push_back({(size_t)lay.off_b1 - 8, 8, true, "len b_g1_query"});
      out.push_back({(size_t)lay.off_b2 - 8, 8, true, "len b_g2_query"});
      out.push_back({(size_t)lay.off_h - 8, 8, true, "len h_query"});
      out.push_back({(size_t)lay.off_l - 8, 8, true, "len l_query"});
    }
  }
  return out;
}

// ---- one mutant through the parser ---------------------------------------------------------------------------------------
int parse(const std::string& format, const uint8_t* data, size_t len) {
  if (format == "r1cs") {
    dg16_r1cs* f = nullptr;
    const int rc = dg16_r1cs_parse(data, len, &f);
    if (rc) {
      if (f) { fprintf(stderr, "a handle came back with status %d\n", rc); exit(3); }
      return rc;
    }
    dg16_r1cs_header h;
    dg16_r1cs_header_get(f, &h);
    for (int k = 0; k < 3; k++) {
      dg16_csr m;
      dg16_r1cs_matrix(f, k, &m);
      if (m.n_rows != h.n_constraints) { fprintf(stderr, "matrix %d has %llu rows\n", k, (unsigned long long)m.n_rows); exit(3); }
      walk(m);
    }
    const uint64_t* map = nullptr;
    dg16_r1cs_wire_map(f, &map);
    if (map)
      for (uint32_t i = 0; i < h.n_wires; i++) g_sink += map[i];
    dg16_r1cs_free(f);
    return rc;
  }
  if (format == "zkey") {
    dg16_zkey* z = nullptr;
    const int rc = dg16_zkey_parse(data, len, &z);
    if (rc) {
      if (z) { fprintf(stderr, "a handle came back with status %d\n", rc); exit(3); }
      return rc;
    }
    dg16_zkey_header h;
    dg16_zkey_header_get(z, &h);
    g_sink += h.n_vars + h.domain_size;
    for (int which = 0; which <= DG16_ZKEY_H; which++) {
      const void* p = nullptr;
      size_t count = 0;
      dg16_zkey_points(z, which, &p, &count);
      const bool g2 = which == DG16_ZKEY_BETA_G2 || which == DG16_ZKEY_GAMMA_G2 || which == DG16_ZKEY_DELTA_G2 || which == DG16_ZKEY_B2;
      touch(p, count * (g2 ? 128 : 64));
    }
    for (int k = 0; k < 2; k++) {
      dg16_csr m;
      dg16_zkey_matrix(z, k, &m);
      if (m.n_rows != h.num_constraints) { fprintf(stderr, "matrix %d has %llu rows\n", k, (unsigned long long)m.n_rows); exit(3); }
      walk(m);
    }
    dg16_zkey_free(z);
    return rc;
  }
  if (format == "arkkey" || format == "arkkey_vk") {
    dg16_arkkey_layout_t lay;
    const int rc = dg16_arkkey_layout(data, len, format == "arkkey_vk", &lay);
    if (rc) return rc;
    if (lay.bytes != len) { fprintf(stderr, "layout of %llu bytes for a file of %zu\n", (unsigned long long)lay.bytes, len); exit(3); }
    touch(data + lay.off_alpha_g1, 32);
    touch(data + lay.off_beta_g2, 64);
    touch(data + lay.off_gamma_g2, 64);
    touch(data + lay.off_delta_g2, 64);
    touch(data + lay.off_ic, lay.n_ic * 32);
    if (format == "arkkey") {
      touch(data + lay.off_beta_g1, 32);
      touch(data + lay.off_delta_g1, 32);
      touch(data + lay.off_a, lay.n_a * 32);
      touch(data + lay.off_b1, lay.n_b1 * 32);
      touch(data + lay.off_b2, lay.n_b2 * 64);
      touch(data + lay.off_h, lay.n_h * 32);
      touch(data + lay.off_l, lay.n_l * 32);
    }
    return rc;
  }
  // proof.bin: exactly 128 bytes in, A | B | C affine Montgomery limbs out (64 + 128 + 64 bytes)
  uint8_t* out = (uint8_t*)malloc(256);
  memset(out, 0xAB, 256);
  const int rc = dg16_proof_decompress(DG16_BN254, data, format == "proof_validate", out);
  if (!rc) touch(out, 256);
  free(out);
  return rc;
}

int run(const std::string& format, const std::vector<uint8_t>& bytes) {
  uint8_t* block = (uint8_t*)malloc(bytes.size() ? bytes.size() : 1);   // exactly the mutant (one spare byte for an empty one)
  if (!bytes.empty()) memcpy(block, bytes.data(), bytes.size());
  const int rc = parse(format, block, bytes.size());
  free(block);
  return rc;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    fprintf(stderr, "usage: %s r1cs|zkey|arkkey|arkkey_vk|proof|proof_validate <seed file> <count>\n", argv[0]);
    return 2;
  }
  const std::string format = argv[1];
  const bool proof = format == "proof" || format == "proof_validate";
  if (!proof && format != "r1cs" && format != "zkey" && format != "arkkey" && format != "arkkey_vk") {
    fprintf(stderr, "unknown format %s\n", argv[1]);
    return 2;
  }
  FILE* fp = fopen(argv[2], "rb");
  if (!fp) { perror(argv[2]); return 2; }
  std::vector<uint8_t> seed;
  uint8_t buf[4096];
  for (size_t k; (k = fread(buf, 1, sizeof buf, fp)) > 0;) seed.insert(seed.end(), buf, buf + k);
  fclose(fp);
  const long count = atol(argv[3]);
  if (proof && seed.size() != 128) { fprintf(stderr, "a proof.bin has 128 bytes\n"); return 2; }
  if (run(format, seed) != DG16_OK) { fprintf(stderr, "the seed itself is refused\n"); return 2; }

  std::map<int, long> by_rc;
  long violations = 0, n_fields = 0, n_large = 0;
  // ---- every count / size / length field in turn ----
  const std::vector<Field> fields = fields_of(format, seed);
  for (const Field& f : fields) {
    const uint64_t v = rd(seed, f.off, f.width);
    const uint64_t values[8] = {0, 1, v - 1, v + 1, 1ull << 31, 0xFFFFFFFFull, 1ull << 63, ~0ull};
    for (uint64_t nv : values) {
      if (f.width == 4 && (nv >> 32)) {
        if (nv != v - 1 && nv != v + 1) continue;      // does not fit the field
        nv &= 0xFFFFFFFFull;                             // 0 - 1 and (2^32 - 1) + 1 wrap like the field does
      }
      if (nv == v) continue;
      std::vector<uint8_t> m = seed;
      memcpy(m.data() + f.off, &nv, f.width);
      const int rc = run(format, m);
      by_rc[rc]++;
      n_fields++;
      if (f.sized && nv > seed.size()) {
        n_large++;
        if (rc == DG16_OK) {
          printf("accepted: %s (offset %zu) = %llu in a file of %zu bytes\n", f.name.c_str(), f.off, (unsigned long long)nv, seed.size());
          violations++;
        }
      }
    }
  }
  // ---- random flips and truncations ----
  Rng rng{0x9E3779B97F4A7C15ull ^ (uint64_t)seed.size()};
  for (long i = 0; i < count; i++) {
    std::vector<uint8_t> m = seed;
    if (!proof && rng.below(6) == 0) {
      m.resize(rng.below(m.size()));
    } else {
      const int k = 1 + (int)rng.below(4);
      for (int j = 0; j < k; j++) {
        const size_t head = m.size() < 2048 ? m.size() : 2048;
        const size_t at = rng.below(4) ? rng.below(head) : rng.below(m.size());
        const uint64_t r = rng.next();
        if (r & 1) m[at] ^= (uint8_t)(1u << ((r >> 1) & 7));         // one bit
        else m[at] = (uint8_t)(r >> 8);                               // any byte (0x00 and 0xFF one time in eight each)
        if ((r & 0x70000) == 0) m[at] = (r & 0x80000) ? 0xFF : 0x00;
      }
    }
    by_rc[run(format, m)]++;
  }
  long accepted = 0, refused = 0;
  for (const auto& kv : by_rc) {
    printf("rc %d %ld\n", kv.first, kv.second);
    (kv.first == DG16_OK ? accepted : refused) += kv.second;
  }
  printf("fields %zu field_mutants %ld larger_than_file %ld\n", fields.size(), n_fields, n_large);
  printf("accepted %ld\nrefused %ld\nfield_violations %ld\n", accepted, refused, violations);
  return violations ? 1 : 0;
}
