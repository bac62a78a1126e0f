// C ABI of the seed expansion and of the share packing of scalar vectors and of a whole proof request (include/dg16.h):
// dg16_fr_expand, dg16_pss_scalar_chunks, dg16_pss_pack_scalars, dg16_request_pack.  Argument checks and the dispatch on
// the scalar field; the hash, the index plan, the kernels and the slices live in pss_scalars.h.  All calls take host
// pointers only, run on channel 0 and are synchronous.
#include "pss_scalars.h"

using namespace dg16;

namespace {

#define FR_SWITCH(curve, ...)                                   \
  switch (curve) {                                              \
    case 0: { using Fr = bn254_fr; __VA_ARGS__ } break;         \
    case 1: { using Fr = bls12_381_fr; __VA_ARGS__ } break;     \
    default: { using Fr = bls12_377_fr; __VA_ARGS__ } break;    \
  }

constexpr size_t kMaxCount = (size_t)1 << 30;

void pack(Call& k, const dg16_pss* pp, int layout, const void* values, size_t n_values, int blind, const void* blinds,
          const pscal::Block& t, bool mont, void* shares) {
  FR_SWITCH(pp->curve, pscal::pack_scalars_typed<Fr>(k, pp, layout, values, n_values, blind, blinds, t, mont, shares);)
}

template <class Fr>
void expand_typed(Call& k, const pscal::Block& t, uint64_t first, size_t n, bool mont, void* out_host) {
  const size_t per = pscal::kSliceOutputsDefault;
  Fr* d = (Fr*)ws(k.c, 2, (n < per ? n : per) * sizeof(Fr));
  k.begin_dominant();
  for (size_t lo = 0; lo < n; lo += per) {
    const size_t cnt = n - lo < per ? n - lo : per;
    hipLaunchKernelGGL(pscal::fr_expand_kernel<Fr>, dim3(nblk(cnt)), dim3(256), 0, k.s(), t, first + (uint64_t)lo, cnt,
                       mont, d);
    DG_HIP(hipGetLastError());
    DG_HIP(hipMemcpyAsync((Fr*)out_host + lo, d, cnt * sizeof(Fr), hipMemcpyDeviceToHost, k.s()));
  }
  k.end_dominant();
  DG_HIP(hipStreamSynchronize(k.s()));
}

}  // namespace

extern "C" {

int dg16_fr_expand(dg16_ctx* ctx, int curve, const void* seed32, uint64_t stream, uint64_t first, size_t n, int mont,
                   void* out) {
  if (!ctx) return DG16_ERR_BAD_ARG;
  return guarded(ctx, [&] {
    DG_REQUIRE(curve >= 0 && curve <= 2, DG16_ERR_BAD_CURVE, "unknown curve id");
    DG_REQUIRE(seed32, DG16_ERR_BAD_ARG, "null seed");
    DG_REQUIRE(n == 0 || out, DG16_ERR_BAD_ARG, "null out");
    DG_REQUIRE(n < kMaxCount, DG16_ERR_BAD_ARG, "n must be < 2^30");
    DG_REQUIRE(first <= UINT64_MAX - (uint64_t)n, DG16_ERR_BAD_ARG, "first + n must not exceed 2^64 - 1");
    if (!n) return;
    const pscal::Block t = pscal::block_template((const uint8_t*)seed32, stream);
    Call k(ctx, 0);
    FR_SWITCH(curve, expand_typed<Fr>(k, t, first, n, mont != 0, out);)
    k.finish();
  });
}

size_t dg16_pss_scalar_chunks(const dg16_pss* pp, int layout, size_t n_values) {
  if (!pp || (layout != DG16_PACK_CHUNKS && layout != DG16_PACK_DFFT)) return 0;
  if (layout == DG16_PACK_DFFT && !pscal::dfft_size_ok(n_values, pp->l)) return 0;
  return pscal::chunks_of(layout, n_values, pp->l);
}

int dg16_pss_pack_scalars(dg16_ctx* ctx, const dg16_pss* pp, int layout, const void* values, size_t n_values,
                          const void* blinds, void* shares) {
  if (!ctx) return DG16_ERR_BAD_ARG;
  return guarded(ctx, [&] {
    DG_REQUIRE(pp && pp->ctx == ctx, DG16_ERR_BAD_ARG, "pp is null or belongs to another context");
    DG_REQUIRE(layout == DG16_PACK_CHUNKS || layout == DG16_PACK_DFFT, DG16_ERR_BAD_ARG,
               "layout must be DG16_PACK_CHUNKS or DG16_PACK_DFFT");
    DG_REQUIRE(n_values < kMaxCount, DG16_ERR_BAD_ARG, "n_values must be < 2^30");
    if (!n_values) return;
    DG_REQUIRE(values && shares, DG16_ERR_BAD_ARG, "null operand");
    DG_REQUIRE(layout != DG16_PACK_DFFT || pscal::dfft_size_ok(n_values, pp->l), DG16_ERR_BAD_ARG,
               "DG16_PACK_DFFT takes a power of two of at least l values");
    Call k(ctx, 0);
    pack(k, pp, layout, values, n_values, blinds ? pscal::kBlindGiven : pscal::kBlindNone, blinds, pscal::Block{}, false,
         shares);
    k.finish();
  });
}

int dg16_request_pack(dg16_ctx* ctx, const dg16_pss* pp, unsigned log_m, const void* a, const void* b, const void* c,
                      const void* full_assignment, size_t num_vars, size_t num_inputs, const void* seed32, int mont,
                      const dg16_request_shares* out) {
  if (!ctx) return DG16_ERR_BAD_ARG;
  return guarded(ctx, [&] {
    DG_REQUIRE(pp && pp->ctx == ctx, DG16_ERR_BAD_ARG, "pp is null or belongs to another context");
    DG_REQUIRE(out, DG16_ERR_BAD_ARG, "null out");
    DG_REQUIRE(log_m < 30 && ((size_t)1 << log_m) >= pp->l, DG16_ERR_BAD_ARG, "need l <= 2^log_m < 2^30");
    DG_REQUIRE(num_vars >= 1 && num_inputs >= 1 && num_inputs <= num_vars, DG16_ERR_BAD_ARG,
               "need 1 <= num_inputs <= num_vars");
    DG_REQUIRE(num_vars < kMaxCount, DG16_ERR_BAD_ARG, "num_vars must be < 2^30");
    const size_t m = (size_t)1 << log_m, n_a = num_vars - 1, n_ax = num_vars - num_inputs;
    DG_REQUIRE(a && b && c && out->a && out->b && out->c, DG16_ERR_BAD_ARG, "null a / b / c or output");
    DG_REQUIRE(full_assignment, DG16_ERR_BAD_ARG, "null full_assignment");
    DG_REQUIRE(n_a == 0 || out->a_share, DG16_ERR_BAD_ARG, "null a_share");
    DG_REQUIRE(n_ax == 0 || out->ax_share, DG16_ERR_BAD_ARG, "null ax_share");
    const int blind = seed32 ? pscal::kBlindSeed : pscal::kBlindNone;
    const char* w = (const char*)full_assignment;
    struct Job { int layout; const void* values; size_t n; void* shares; } jobs[5] = {
        {DG16_PACK_DFFT, a, m, out->a},
        {DG16_PACK_DFFT, b, m, out->b},
        {DG16_PACK_DFFT, c, m, out->c},
        {DG16_PACK_CHUNKS, w + 32, n_a, out->a_share},                     // full_assignment[1..]  (sha256.rs:102)
        {DG16_PACK_CHUNKS, w + 32 * num_inputs, n_ax, out->ax_share}};     // full_assignment[num_inputs..]
    Call k(ctx, 0);
    // blind (e, k) of output v is element e l + k of stream v: equal inputs get unrelated shares
    for (unsigned v = 0; v < 5; v++) {
      const pscal::Block t = seed32 ? pscal::block_template((const uint8_t*)seed32, v) : pscal::Block{};
      pack(k, pp, jobs[v].layout, jobs[v].values, jobs[v].n, blind, nullptr, t, mont != 0, jobs[v].shares);
    }
    k.finish();
  });
}

}  // extern "C"
