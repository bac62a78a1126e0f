// C ABI of the share packing of point vectors and of a whole proving key (include/dg16.h): dg16_pss_pack_points,
// dg16_pss_pack_chunks, dg16_pk_pack.  Argument checks and the dispatch on the curve; the schedule, the two kernels and
// the slices live in pss_pack.h and the per-curve objects (pss_pack_curve.hip).  Both calls take host pointers only, run
// on channel 0 and are synchronous.
#include "pss_pack.h"

using namespace dg16;

namespace {

void pack(Call& k, const dg16_pss* pp, int group, const void* points, size_t n_points, void* shares, bool sub) {
  switch (pp->curve) {
    case 0: pss_pack_run<0>(k, pp, group, points, n_points, shares, sub); break;
    case 1: pss_pack_run<1>(k, pp, group, points, n_points, shares, sub); break;
    default: pss_pack_run<2>(k, pp, group, points, n_points, shares, sub); break;
  }
}

}  // namespace

extern "C" {

size_t dg16_pss_pack_chunks(const dg16_pss* pp, size_t n_points) { return pp ? ppack::chunks_of(n_points, pp->l) : 0; }

int dg16_pss_pack_points(dg16_ctx* ctx, const dg16_pss* pp, int group, const void* points_affine, size_t n_points,
                         void* shares, int in_subgroup) {
  if (!ctx) return DG16_ERR_BAD_ARG;
  return guarded(ctx, [&] {
    DG_REQUIRE(pp && pp->ctx == ctx, DG16_ERR_BAD_ARG, "pp is null or belongs to another context");
    DG_REQUIRE(group == 1 || group == 2, DG16_ERR_BAD_ARG, "group must be 1 (G1) or 2 (G2)");
    DG_REQUIRE(n_points == 0 || (points_affine && shares), DG16_ERR_BAD_ARG, "null operand");
    DG_REQUIRE(n_points < ((size_t)1 << 30), DG16_ERR_BAD_ARG, "n_points must be < 2^30");
    if (!n_points) return;
    Call k(ctx, 0);
    pack(k, pp, group, points_affine, n_points, shares, in_subgroup != 0);
    k.finish();
  });
}

int dg16_pk_pack(dg16_ctx* ctx, const dg16_pss* pp, size_t num_vars, size_t num_inputs, size_t domain_size,
                 const void* a_query, const void* b_g1_query, const void* b_g2_query, const void* h_query,
                 const void* l_query, const dg16_pk_shares* out, int in_subgroup) {
  if (!ctx) return DG16_ERR_BAD_ARG;
  return guarded(ctx, [&] {
    DG_REQUIRE(pp && pp->ctx == ctx, DG16_ERR_BAD_ARG, "pp is null or belongs to another context");
    DG_REQUIRE(out, DG16_ERR_BAD_ARG, "null out");
    DG_REQUIRE(num_vars >= 1 && num_inputs >= 1 && num_inputs <= num_vars, DG16_ERR_BAD_ARG,
               "need 1 <= num_inputs <= num_vars");
    DG_REQUIRE(num_vars < ((size_t)1 << 30) && domain_size < ((size_t)1 << 30), DG16_ERR_BAD_ARG,
               "num_vars and domain_size must be < 2^30");
    const size_t n_q = num_vars - 1, n_l = num_vars - num_inputs;
    DG_REQUIRE(n_q == 0 || (a_query && b_g1_query && b_g2_query && out->s && out->h && out->v), DG16_ERR_BAD_ARG,
               "null a_query / b_g1_query / b_g2_query or output");
    DG_REQUIRE(domain_size == 0 || (h_query && out->u), DG16_ERR_BAD_ARG, "null h_query or output");
    DG_REQUIRE(n_l == 0 || (l_query && out->w), DG16_ERR_BAD_ARG, "null l_query or output");
    const bool sub = in_subgroup != 0;
    const size_t g1b = affine_bytes(pp->curve, 1), g2b = affine_bytes(pp->curve, 2);
    Call k(ctx, 0);
    // the three [1..] queries drop element 0 (proving_key.rs:48-65)
    if (n_q) pack(k, pp, 1, (const char*)a_query + g1b, n_q, out->s, sub);
    if (domain_size) pack(k, pp, 1, h_query, domain_size, out->u, sub);
    if (n_l) pack(k, pp, 1, l_query, n_l, out->w, sub);
    if (n_q) pack(k, pp, 1, (const char*)b_g1_query + g1b, n_q, out->h, sub);
    if (n_q) pack(k, pp, 2, (const char*)b_g2_query + g2b, n_q, out->v, sub);
    k.finish();
  });
}

}  // extern "C"
