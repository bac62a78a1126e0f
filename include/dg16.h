/* dg16 -- C ABI of the MI355X (gfx950) Groth16 hot path: MSM, NTT, h-polynomial, prover glue.
 *
 * This is the drop-in boundary for zkHubHQ/distributed-groth16.  The reference has no FFI; the
 * seams a maintainer re-points at this library are Rust call sites (INTEGRATION.md shows the
 * `extern "C"` block and the feature-gated replacements):
 *
 *   dg16_msm            <- `G::msm(bases, scalars)`            dist-primitives/src/dmsm/mod.rs:82
 *                          (also examples/msm_bench.rs:20, groth16/examples/local_groth_bench.rs:139-147)
 *   dg16_ntt            <- `EvaluationDomain::{fft,ifft}_in_place` ark-circom/src/circom/qap.rs:64-85
 *                          and the butterfly loops fft1/fft2_in_place  dist-primitives/src/dfft/mod.rs:98-182
 *   dg16_h_poly         <- `CircomReduction::witness_map_from_matrices` (NTT part)
 *                                                              ark-circom/src/circom/qap.rs:64-91
 *   dg16_qap            <- `qap::qap` (R1CS x witness)          groth16/src/qap.rs:44-91
 *   dg16_field_op       <- element-wise ark-ff ops (parity probe for the Montgomery kernels)
 *   dg16_gen_bases      <- `PackedProvingKeyShare::rand`       groth16/src/proving_key.rs:112-155
 *   dg16_groth16_setup  <- `circuit_specific_setup`             groth16/examples/sha256.rs:137
 *                          (dg16_fixed_base_mul <- FixedBase::msm inside it)
 *   dg16_groth16_prove  <- `create_proof_with_reduction_and_matrices`  groth16/examples/sha256.rs:159
 *                          and the A/B/C assembly of groth16/src/prove.rs:21-136
 *
 * Conventions
 *   - Field elements: little-endian limbs, 32 bytes (Fr of all curves, BN254 Fq) or 48 bytes
 *     (BLS12-381 / BLS12-377 Fq), Montgomery form with R = 2^256 / 2^384 -- the arkworks in-memory
 *     representation (pinned by ark-circom/src/zkey.rs:417-427).
 *   - G1 affine point: x || y (64 / 96 bytes).  G2 affine: x.c0 || x.c1 || y.c0 || y.c1 (128 / 192
 *     bytes).  Identity = all-zero bytes (ark-circom/src/zkey.rs:353-361).  No `infinity` flag
 *     byte: the Rust shim repacks `Affine<P>`.
 *   - Results of group operations are Jacobian (x, y, z) in Montgomery form (== ark-ec
 *     `Projective` for short-Weierstrass curves); z = 0 encodes the identity.
 *   - Scalars: 32 bytes each, canonical integers unless DG16_F_SCALARS_MONT is set.
 *   - Pointers are host pointers unless DG16_F_DEVICE_PTRS is set (then ALL data pointers of the
 *     call, inputs and outputs, are device pointers on the context's GPU).
 *   - `channel` (0..2) mirrors `MultiplexedStreamID::{Zero,One,Two}` (mpc-net/src/lib.rs:29-33):
 *     each channel owns a HIP stream and a workspace; calls on different channels may run
 *     concurrently from different host threads, calls on one channel are serialised.
 *   - Every function returns a dg16_status; nothing throws or aborts across this boundary.  The
 *     Rust side maps non-zero to `MpcNetError::Generic` (mpc-net/src/lib.rs:15-27).
 *   - The library owns device memory; the caller owns every buffer it passes and may free it on
 *     return (host-pointer calls are synchronous; device-pointer calls are stream-ordered on the
 *     channel's stream -- use dg16_sync or the stream you installed with dg16_set_stream).
 *   - The one-time calls WITHOUT a `channel` argument that take device pointers -- dg16_pk_create, dg16_pk_create_shard,
 *     dg16_vk_create, dg16_groth16_setup, dg16_groth16_setup_srs -- are synchronous; ordered behind the work enqueued on
 *     channel 0's stream (the library's own, or the one installed with dg16_set_stream(ctx, 0, ..)); outputs complete on
 *     return.  An input that another stream is still producing must be joined to channel 0's stream by the caller.
 */
#ifndef DG16_H
#define DG16_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dg16_ctx dg16_ctx;

enum dg16_curve { DG16_BN254 = 0, DG16_BLS12_381 = 1, DG16_BLS12_377 = 2 };

enum dg16_status {
  DG16_OK = 0,
  DG16_ERR_LENGTH_MISMATCH = 1, /* mirrors Err(usize) of VariableBaseMSM::msm */
  DG16_ERR_BAD_CURVE = 2,
  DG16_ERR_BAD_ARG = 3,
  DG16_ERR_OOM = 4,
  DG16_ERR_HIP = 5,
  DG16_ERR_NET = 6,
  DG16_ERR_UNSUPPORTED = 7
};

enum dg16_flags {
  DG16_F_SCALARS_MONT = 1u, /* scalars are in Montgomery form (arkworks memory) */
  DG16_F_DEVICE_PTRS = 2u,  /* all data pointers are device pointers */
  DG16_F_OUT_AFFINE = 4u,   /* group result as affine x || y (one inversion on the device) */
  DG16_F_H_CYCLIC = 8u,     /* dg16_pk_create_shard: this shard's h_query bases are h_query[shard + n_shards * j]
                               (the output layout of the sharded h-polynomial) instead of a contiguous slice */
  DG16_F_SERIAL_CHANNELS = 16u, /* dg16_prove_c: run the three d_msm one after another (channel 0, 1, 2 in that order
                               on every party) instead of joined from three host threads -- for a dg16_net whose
                               channels are not independent (one ordered pipe); the result is the same */
  DG16_F_OVERLAP_TAIL = 32u, /* dg16_groth16_prove and dg16_groth16_prove_dist with DG16_F_DEVICE_PTRS, for a queue of proofs on
                               one context (prove_dist: also the all-gather of the records, on channel 2's stream): the last
                               MSM's bucket reduction, the assembly and the copy to proof_out are ordered on CHANNEL 2's
                               stream instead of channel 0's, so the work enqueued next on channel 0 (the next proof's
                               dg16_qap and h-polynomial) starts under that latency-bound tail.  proof_out is complete
                               after dg16_sync(ctx, 2) (or stream-ordered work on channel 2); every other call on the
                               context orders itself behind the tail.  Ignored with host pointers.
                               What is ordered where (dg16_groth16_prove, the whole h-polynomial): channel 0's stream carries
                               the h-polynomial and the five accumulations and is NOT joined with the library's other streams
                               when the call returns -- work enqueued on it afterwards is ordered behind this proof's last
                               accumulation and behind its read of full_assignment, nothing else; channel 2's stream is
                               ordered behind ALL of the proof (every reduction, the assembly, the copy to proof_out).  The
                               next proof with this flag fences each workspace buffer at its first reuse.  DG16_QUEUE_JOIN=1 in the environment restores the join of
                               channel 0 with the other streams at the end of the call (dg16_groth16_prove_dist keeps it). */
  DG16_F_BASES_IN_SUBGROUP = 64u, /* dg16_msm, dg16_d_msm, dg16_prove_a / _b / _c: the caller guarantees that every base is
                               in the order-r subgroup (true of any arkworks G1Affine / G2Affine obtained through
                               Validate::Yes or from CRS generation).  The library may then split the scalars with the
                               curve's endomorphism (GLV: phi(P) = lambda P holds only in that subgroup), which is what
                               its headline MSM rates are measured with.  Without the flag only cofactor-one groups
                               (BN254 G1) take that path and every other group runs plain Pippenger, which -- like
                               VariableBaseMSM::msm -- is correct for ANY point of the curve.  Resident keys / tables
                               (dg16_pk_create*, dg16_bases_upload) never split and ignore the flag. */
  DG16_F_QAP_LIBSNARK = 128u, /* dg16_h_poly, dg16_groth16_setup, dg16_groth16_prove: the Libsnark QAP reduction instead of the
                               circom one (see "The two QAP reductions" below).  Without the flag every call is unchanged.
                               The sharded entry points (dg16_groth16_msms, dg16_groth16_msms_h, dg16_groth16_prove_dist,
                               dg16_h_poly_dist, dg16_h_poly_dist_stage) return DG16_ERR_UNSUPPORTED with it. */
  DG16_F_H_ODD = 256u /* dg16_ext_wit_h only: the king keeps the ODD positions of the 2m unpacked evaluations, whatever l is
                         -- CircomReduction's witness map at l = 1, 2, 4, 8 -- instead of mirroring the reference's swap,
                         which does that at l = 2 alone (see dg16_ext_wit_h).  Without the flag the call is unchanged. */
};

/* field ids for dg16_field_op: curve for the base field Fq, 16 + curve for the scalar field Fr */
enum dg16_field_opcode {
  DG16_OP_ADD = 0, DG16_OP_SUB = 1, DG16_OP_MUL = 2, DG16_OP_SQR = 3, DG16_OP_INV = 4,
  DG16_OP_TO_MONT = 5, DG16_OP_FROM_MONT = 6, DG16_OP_NEG = 7
};

/* ---- context ------------------------------------------------------------------------------- */
int dg16_ctx_create(int device, dg16_ctx **out);
void dg16_ctx_destroy(dg16_ctx *ctx);
const char *dg16_last_error(dg16_ctx *ctx);
/* Run `channel` on a caller-owned hipStream_t (e.g. torch's current stream). NULL restores the
 * context's own stream. */
int dg16_set_stream(dg16_ctx *ctx, int channel, void *hip_stream);
int dg16_sync(dg16_ctx *ctx, int channel);
/* Device name, CU count (for reports). */
int dg16_device_info(dg16_ctx *ctx, char *name, size_t name_len, int *compute_units);

/* ---- element-wise field arithmetic (parity probe) -------------------------------------------- */
int dg16_field_op(dg16_ctx *ctx, int field_id, int op, const void *a, const void *b, void *out,
                  size_t n, unsigned flags, int channel);

/* ---- NTT ---------------------------------------------------------------------------------------
 * In-place Radix2EvaluationDomain transform of 2^log_n Montgomery-form Fr elements, natural order
 * in and out.  inverse != 0 scales by n^-1.  coset_offset: NULL, or a HOST pointer to the domain
 * offset g (Montgomery form): forward multiplies coefficient i by g^i first, inverse multiplies
 * output i by g^-i.  Every element (and g) must be reduced, i.e. below r; a non-reduced element
 * gives an undefined result (the kernel's lazy-reduction bounds start from it). */
int dg16_ntt(dg16_ctx *ctx, int curve, void *data, unsigned log_n, int inverse,
             const void *coset_offset, unsigned flags, int channel);

/* h = NTT(shift(iNTT a)) * NTT(shift(iNTT b)) - NTT(shift(iNTT c)) on the size-2^log_m domain,
 * shift = multiply coefficient i by w_{2m}^i.  a, b, c are not modified; out may alias a.
 * Every element of a, b, c must be reduced (below r); a non-reduced element gives an undefined result.
 * With DG16_F_QAP_LIBSNARK: the coefficients of (A B - C) / Z instead ("The two QAP reductions" below). */
int dg16_h_poly(dg16_ctx *ctx, int curve, const void *a, const void *b, const void *c,
                unsigned log_m, void *out, unsigned flags, int channel);

/* ---- QAP evaluation vectors (sparse R1CS x witness) ------------------------------------------------
 * Replaces `qap::qap` (groth16/src/qap.rs:44-91; the same loops open ark-circom/src/circom/qap.rs:34-62):
 * a[i] = <A_i, w>, b[i] = <B_i, w> for the num_constraints CSR rows (coefficients in Montgomery form),
 * a[num_constraints + j] = w[j] for j < num_inputs, c = a o b on the constraint rows, zero padding up to
 * 2^log_m = D::new(num_constraints + num_inputs).size().  full_assignment: num_vars Fr elements
 * (Montgomery iff DG16_F_SCALARS_MONT); outputs: 2^log_m Montgomery elements each. */
int dg16_qap(dg16_ctx *ctx, int curve, size_t num_constraints, size_t num_inputs, size_t num_vars,
             unsigned log_m, const uint32_t *a_row_ptr, const uint32_t *a_col, const void *a_coeff,
             const uint32_t *b_row_ptr, const uint32_t *b_col, const void *b_coeff,
             const void *full_assignment, void *a_out, void *b_out, void *c_out, unsigned flags,
             int channel);

/* The same for the rows i = row_start + row_stride * j, j < 2^log_m / row_stride, written densely (a_out[j] is row
 * i): rank `row_start` of `row_stride` ranks computes exactly the cyclic rows the sharded h-polynomial consumes. */
int dg16_qap_rows(dg16_ctx *ctx, int curve, size_t num_constraints, size_t num_inputs, size_t num_vars,
                  unsigned log_m, const uint32_t *a_row_ptr, const uint32_t *a_col, const void *a_coeff,
                  const uint32_t *b_row_ptr, const uint32_t *b_col, const void *b_coeff,
                  const void *full_assignment, size_t row_start, size_t row_stride, void *a_out, void *b_out,
                  void *c_out, unsigned flags, int channel);

/* ---- The two QAP reductions ------------------------------------------------------------------------
 * The reference's own words (ark-circom/src/circom/qap.rs:11-15): the circom / snarkjs witness map differs from the
 * default LibsnarkReduction of ark-groth16 -- it takes c = a o b and evaluates on the odd coset of the doubled domain --
 * so a key and a prover must agree on the reduction.  `Groth16::<E>` defaults to LibsnarkReduction (the reference uses
 * it at ark-circom/src/zkey.rs:921); every arkworks circuit that is not a circom circuit, and any libsnark- or
 * bellman-shaped key, is of that kind.  DG16_F_QAP_LIBSNARK selects it:
 *   a, b, c   the evaluation vectors of dg16_qap, except that c[i] = <C_i, w> on the constraint rows (dg16_qap_r1cs)
 *   h         the unique polynomial of degree <= m - 2 with h Z = A B - C, Z = X^m - 1, A, B, C the interpolants of
 *             a, b, c on the size-m domain: dg16_h_poly returns its m coefficients (the top one zero), Montgomery form.
 *             (Computed on the coset g H, g = F::GENERATOR; any coset off the domain gives the same h.  For a witness
 *             that does not satisfy the R1CS the division is not exact and h is whatever the pipeline returns: ask
 *             dg16_qap_r1cs for the violations first.)
 *   key       h_query[i] = (tau^i Z(tau) / delta) G1 for i < m - 1, the identity at i = m - 1 (h_query keeps its 2^log_m
 *             length: dg16_pk_create and the key layout are the same); every other element of the key is the same in
 *             both reductions (LibsnarkReduction::instance_map_with_evaluation serves both).
 *   proof     prove.rs:21-136 unchanged.  dg16_groth16_prove supports the flag with and without DG16_F_OVERLAP_TAIL (the
 *             quotient's workspace is the circom h-polynomial's, touched on channel 0's stream only).
 *
 * dg16_qap_r1cs: dg16_qap_rows with a third CSR triple -- a = A w, b = B w, c = C w, same layout, padding, row_start /
 * row_stride form and flags.  violations: NULL, or (device pointer iff DG16_F_DEVICE_PTRS) two uint64_t the same pass
 * writes: [0] the number of constraint rows among those this call evaluates with a_i b_i != c_i, [1] the smallest such
 * row index (the row of the constraint system, not the output slot), UINT64_MAX if none.  Instance and padding rows never
 * count.  Stream-ordered on `channel` like dg16_qap; violations is valid after dg16_sync. */
int dg16_qap_r1cs(dg16_ctx *ctx, int curve, size_t num_constraints, size_t num_inputs, size_t num_vars,
                  unsigned log_m, const uint32_t *a_row_ptr, const uint32_t *a_col, const void *a_coeff,
                  const uint32_t *b_row_ptr, const uint32_t *b_col, const void *b_coeff,
                  const uint32_t *c_row_ptr, const uint32_t *c_col, const void *c_coeff,
                  const void *full_assignment, size_t row_start, size_t row_stride, void *a_out, void *b_out,
                  void *c_out, uint64_t *violations, unsigned flags, int channel);

/* ---- MSM ----------------------------------------------------------------------------------------
 * out = sum_i scalars[i] * bases[i] in G1 (group = 1) or G2 (group = 2).
 * n_bases != n_scalars returns DG16_ERR_LENGTH_MISMATCH.  out: Jacobian (3 field elements of the
 * group's coordinate field) or affine with DG16_F_OUT_AFFINE.  Scalars are integers below 2^255 (canonical field
 * elements are; a set bit 255 is not part of the contract).  DG16_F_BASES_IN_SUBGROUP: see enum dg16_flags. */
int dg16_msm(dg16_ctx *ctx, int curve, int group, const void *bases, const void *scalars,
             size_t n_bases, size_t n_scalars, unsigned flags, int channel, void *out);

/* Resident bases (bases_upload -> handle, msm_resident): a CRS is fixed, so its bases go to HBM once,
 * as the table of window multiples T[w][i] = 2^(c w) P_i (288 GB of HBM: 15 rows x 64 B x 2^20 = 1 GB per G1
 * vector) -- an MSM over them then has ONE bucket set and no Horner tail (2^20 points: ~2 ms G1 / ~6 ms G2 against
 * ~4.7 / ~14 for dg16_msm).  This is what `PackedProvingKeyShare` (groth16/src/proving_key.rs:26-46) holds per party:
 * dg16_d_msm_resident is d_msm (dist-primitives/src/dmsm/mod.rs:70-98) over such a handle.
 * n_scalars != n returns DG16_ERR_LENGTH_MISMATCH like dg16_msm. */
typedef struct dg16_bases dg16_bases;
int dg16_bases_upload(dg16_ctx *ctx, int curve, int group, const void *bases, size_t n, unsigned flags,
                      dg16_bases **out);
void dg16_bases_free(dg16_bases *h);
int dg16_bases_info(const dg16_bases *h, size_t *n, unsigned *window_bits, uint64_t *table_bytes);
int dg16_msm_resident(dg16_ctx *ctx, const dg16_bases *h, const void *scalars, size_t n_scalars, unsigned flags,
                      int channel, void *out);

/* Synthetic bases P_i = (k0 + i*k1) * G (distinct, prime-order subgroup), written as affine points
 * to `out` (device or host per flags). */
int dg16_gen_bases(dg16_ctx *ctx, int curve, int group, uint64_t seed, size_t n, void *out,
                   unsigned flags, int channel);

/* Jacobian -> affine for n points (n inversions on the device, one thread each). */
int dg16_to_affine(dg16_ctx *ctx, int curve, int group, const void *jac, void *out, size_t n,
                   unsigned flags, int channel);

/* ---- key generation: fixed-base batch multiplication and the Groth16 generator --------------------------------
 * out[i] = scalars[i] * base as affine points (identity = all-zero bytes).  base: one affine point of `group` (HOST
 * pointer even with DG16_F_DEVICE_PTRS; NULL = the curve's standard generator).  Replaces FixedBase::get_window_table +
 * FixedBase::msm of ark-groth16's generator (generate_parameters_with_qap, reached from circuit_specific_setup:
 * groth16/examples/sha256.rs:137, million.rs:137, mpc-api/src/main.rs:151).  Scalars: canonical integers below r, or
 * Montgomery form with DG16_F_SCALARS_MONT.  A table of signed window multiples of the base is built on the device per
 * call; its window width depends on n alone (dg16_fixed_base_window_bits: floor(log2 n) - 3 clamped to 4..16), and a
 * point costs ceil((scalar bits + 1) / width) mixed additions and no doublings.  n = 0 is a no-op. */
int dg16_fixed_base_mul(dg16_ctx *ctx, int curve, int group, const void *base, const void *scalars, size_t n,
                        void *out_affine, unsigned flags, int channel);
unsigned dg16_fixed_base_window_bits(size_t n);

/* Groth16 parameters for an R1CS, CircomReduction flavour: replaces generate_parameters_with_qap as reached from
 * `Groth16::<Bn254, CircomReduction>::circuit_specific_setup` (groth16/examples/sha256.rs:137, d_sha256.rs:138,
 * test.rs:147,160, groth16/src/qap.rs:234, proving_key.rs:186) -- LibsnarkReduction::instance_map_with_evaluation
 * (through ark-circom/src/circom/qap.rs:20-25) and CircomReduction::h_query_scalars (qap.rs:94-110) -- all on the device.
 * A, B, C: CSR by constraint, coefficients in Montgomery form (the layout dg16_qap takes; C as well here).  trapdoor:
 * HOST pointer to alpha | beta | gamma | delta | tau (5 x 32 bytes, canonical, all non-zero and below r; tau^m != 1,
 * m = 2^log_m = D::new(num_constraints + num_inputs).size()), else DG16_ERR_BAD_ARG: the caller owns the randomness.
 * generators: HOST pointer to g1 affine | g2 affine, or NULL for the standard generators.  Outputs (device pointers
 * iff DG16_F_DEVICE_PTRS, like the matrices), affine, identity = zero bytes:
 *   a_query, b_g1_query [num_vars] G1 | b_g2_query [num_vars] G2 | h_query [2^log_m] G1 |
 *   l_query [num_vars - num_inputs] G1 | fixed_points = alpha_g1 | beta_g1 | delta_g1 | beta_g2 | delta_g2 (the
 *   dg16_pk_create layout) | gamma_g2 (one G2) | gamma_abc_g1 [num_inputs] G1.
 * Synchronous in both forms (it owns temporary device memory); runs on channel 0.  With DG16_F_DEVICE_PTRS: synchronous;
 * ordered behind the work enqueued on channel 0's stream; outputs complete on return.  A matrix entry whose column is
 * not a wire, or a row_ptr that is not ordered, is DG16_ERR_BAD_ARG.
 * flags | DG16_F_QAP_LIBSNARK: the LibsnarkReduction key -- h_query[i] = (tau^i Z(tau) / delta) G1 for i < m - 1 and zero
 * bytes at i = m - 1; every other output is byte-equal to the call without the flag. */
int dg16_groth16_setup(dg16_ctx *ctx, int curve, size_t num_constraints, size_t num_inputs, size_t num_vars,
                       unsigned log_m, const uint32_t *a_row_ptr, const uint32_t *a_col, const void *a_coeff,
                       const uint32_t *b_row_ptr, const uint32_t *b_col, const void *b_coeff,
                       const uint32_t *c_row_ptr, const uint32_t *c_col, const void *c_coeff,
                       const void *trapdoor, const void *generators, void *a_query, void *b_g1_query,
                       void *b_g2_query, void *h_query, void *l_query, void *fixed_points, void *gamma_g2,
                       void *gamma_abc_g1, unsigned flags);

/* The same key computed IN THE EXPONENT from a structured reference string: the Lagrange-basis points of a
 * powers-of-tau ceremony for the domain of size m = 2^log_m.  Nobody holds the trapdoor; the key has gamma = delta = 1
 * (what a snarkjs `zkey new` writes before any phase-2 contribution).  Where the arrays come from:
 *   lag_g1, lag_g2, alpha_lag_g1, beta_lag_g1   sections 12, 13, 14, 15 of a PREPARED phase-2 .ptau file (snarkjs
 *       `powersoftau prepare phase2`: tauG1, tauG2, alphaTauG1, betaTauG1 in Lagrange form), the block of the power
 *       log_m in each -- decoded to this library's affine Montgomery layout.  In arkworks terms: the group inverse FFT
 *       over Radix2EvaluationDomain::new(m) of [tau^j G], [tau^j G2], [alpha tau^j G], [beta tau^j G], j < m.
 *   h_g1   the h basis of the QAP reduction the key will be proved with, for delta = 1.  CircomReduction: the points
 *       L'_{2i+1}(tau) G of the size-2m Lagrange basis with odd index (snarkjs reads them from the block of the power
 *       log_m + 1 of section 12), i < m.  LibsnarkReduction: tau^i Z(tau) G = (tau^(i+m) - tau^i) G for i < m - 1
 *       and the identity at i = m - 1.  It is copied to h_query as it stands; dg16_srs_prepare derives it, and the
 *       four arrays above, from the tau powers a ceremony publishes.
 *   fixed  alpha G1, beta G1, G1, beta G2, G2: the first elements of sections 4 (alphaTauG1), 5 (betaTauG1) and 2
 *       (tauG1), section 6 (betaG2) and the first element of section 3 (tauG2).
 * THE CALLER GUARANTEES that every point of the reference string is on its curve and in the subgroup of order r --
 * the call does not check either (a ceremony verifier does).  With that guarantee DG16_F_BASES_IN_SUBGROUP may be
 * passed and allows the endomorphism split of the coefficients, exactly as for dg16_points_mul; without the flag the
 * plain loops run, which are correct for any point of the curve. */
typedef struct dg16_srs {          /* affine points, identity = zero bytes; device pointers iff DG16_F_DEVICE_PTRS */
  const void *lag_g1;              /* [m]  L_i(tau) G1, the Lagrange basis of the size-m domain */
  const void *lag_g2;              /* [m]  L_i(tau) G2 */
  const void *alpha_lag_g1;        /* [m]  alpha L_i(tau) G1 */
  const void *beta_lag_g1;         /* [m]  beta  L_i(tau) G1 */
  const void *h_g1;                /* [m]  the h basis of the chosen reduction with delta = 1, copied to h_query */
  const void *fixed;               /* HOST: alpha_g1 | beta_g1 | g1 (G1 affine) | beta_g2 | g2 (G2 affine) */
} dg16_srs;

/* A, B, C, the sizes and the eight outputs with their layouts are those of dg16_groth16_setup.  With u_i = L_i(tau):
 *   a_query[k]    = sum over the entries (i, k, v) of A of v * lag_g1[i], + lag_g1[nc + k] for k < num_inputs
 *   b_g1_query[k] = sum_B v * lag_g1[i];  b_g2_query[k] = sum_B v * lag_g2[i]
 *   K_k = sum_A v * beta_lag_g1[i] (+ beta_lag_g1[nc + k] for k < num_inputs) + sum_B v * alpha_lag_g1[i]
 *         + sum_C v * lag_g1[i];  gamma_abc_g1[k] = K_k for k < num_inputs, l_query[k - num_inputs] = K_k otherwise
 *   h_query = h_g1;  fixed_points = alpha_g1 | beta_g1 | g1 | beta_g2 | g2;  gamma_g2 = g2.
 * Coefficients 0, 1 and r - 1 cost no multiplication; the others go through dg16_points_mul's loops, in slices of the
 * size dg16_ctx_set_points_mul_slice sets (0: 2^17 terms).  A wire's terms are added by one lane, by a wave (from
 * wave_from terms) or, from msm_from terms on, by the library's MSM (dg16_setup_srs_limits reports the two thresholds).
 * Synchronous in both pointer forms; runs on channel 0.  With DG16_F_DEVICE_PTRS: synchronous; ordered behind the work
 * enqueued on channel 0's stream; outputs complete on return.  A matrix entry whose column is not a wire, or a row_ptr that
 * is not ordered, is DG16_ERR_BAD_ARG, as is a NULL srs or a NULL array in it; nothing is read out of range. */
int dg16_groth16_setup_srs(dg16_ctx *ctx, int curve, size_t num_constraints, size_t num_inputs, size_t num_vars,
                           unsigned log_m, const uint32_t *a_row_ptr, const uint32_t *a_col, const void *a_coeff,
                           const uint32_t *b_row_ptr, const uint32_t *b_col, const void *b_coeff,
                           const uint32_t *c_row_ptr, const uint32_t *c_col, const void *c_coeff,
                           const dg16_srs *srs, void *a_query, void *b_g1_query, void *b_g2_query, void *h_query,
                           void *l_query, void *fixed_points, void *gamma_g2, void *gamma_abc_g1, unsigned flags);
void dg16_setup_srs_limits(unsigned *wave_from, unsigned *msm_from);

/* ---- group transform and reference-string preparation ------------------------------------------------------------
 * The radix-2 transform of dg16_ntt over GROUP elements, in place on 2^log_n affine points of `group` (1 = G1, 2 = G2;
 * identity = zero bytes), natural order in and out -- Radix2EvaluationDomain::{fft, ifft} on a Vec<G>:
 *   forward  out[i] = sum_j w^(i j) P_j          inverse  out[i] = n^-1 sum_j w^(-i j) P_j
 * with w the root dg16_ntt uses for the same curve and size: for P_j = s_j G the result is dg16_ntt(s)_i G.
 * THE CALLER GUARANTEES that every point is in the subgroup of order r (a ceremony verifier checks that; this call
 * does not) (`dg16_srs_verify` checks it).  The scalar field does not act on other points: for them the result is
 * unspecified, but nothing is read or written out of range.
 * Every stage is n / 2 butterflies (a, b) -> (a + w b, a - w b), one lane each, cut into slices
 * of the size dg16_ctx_set_points_mul_slice sets; the butterflies with w = 1 (all of the first stage, n / 2^s of stage
 * s) add and subtract only, so a forward transform costs (n / 2) log_n - (n - 1) point multiplications and an inverse
 * n more.  points_affine: host pointers only.  Synchronous; runs on channel 0; the device copies are temporary
 * (DG16_ERR_OOM leaves the context usable).  log_n <= min(two-adicity of r, 27), else DG16_ERR_BAD_ARG; log_n = 0 is a
 * no-op. */
int dg16_group_ntt(dg16_ctx *ctx, int curve, int group, void *points_affine, unsigned log_n, int inverse);

/* The monomial powers a powers-of-tau ceremony publishes (the sections of a .ptau file, decoded to this library's affine
 * Montgomery layout), m = 2^log_m.  All five are host pointers. */
typedef struct dg16_srs_powers {
  const void *tau_g1;              /* [2m - 1] tau^j G1          (section 2) */
  const void *tau_g2;              /* [m]      tau^j G2          (section 3) */
  const void *alpha_tau_g1;        /* [m]      alpha tau^j G1    (section 4) */
  const void *beta_tau_g1;         /* [m]      beta tau^j G1     (section 5) */
  const void *beta_g2;             /* one G2 point: beta G2      (section 6) */
} dg16_srs_powers;
/* What dg16_srs_prepare writes: caller-allocated host buffers, laid out as the arrays of dg16_srs. */
typedef struct dg16_srs_prepared {
  void *lag_g1;                    /* [m] G1 */
  void *lag_g2;                    /* [m] G2 */
  void *alpha_lag_g1;              /* [m] G1 */
  void *beta_lag_g1;               /* [m] G1 */
  void *h_g1;                      /* [m] G1 */
  void *fixed;                     /* alpha_g1 | beta_g1 | g1 (G1 affine) | beta_g2 | g2 (G2 affine) */
} dg16_srs_prepared;

/* From ceremony output to the reference string dg16_groth16_setup_srs takes (snarkjs `powersoftau prepare phase2`):
 *   lag_g1, lag_g2, alpha_lag_g1, beta_lag_g1   the inverse dg16_group_ntt of size m of the first m powers
 *   h_g1, reduction 0 (CircomReduction)    the odd-indexed outputs of the inverse transform of size 2m of
 *                                          tau_g1[0 .. 2m - 1) | identity
 *   h_g1, reduction 1 (LibsnarkReduction)  tau_g1[i + m] - tau_g1[i] for i < m - 1, the identity at m - 1
 *   fixed   alpha_tau_g1[0] | beta_tau_g1[0] | tau_g1[0] | beta_g2 | tau_g2[0]
 * The caller's guarantee is dg16_group_ntt's: every point has order r (`dg16_srs_verify` checks it).
 * powers, out and every array in them: host pointers only.  Synchronous; runs on channel 0.  log_m + 1 <= two-adicity of r and log_m <= 26, else
 * DG16_ERR_BAD_ARG, as are a NULL pointer and another reduction; an unknown curve is DG16_ERR_BAD_CURVE. */
int dg16_srs_prepare(dg16_ctx *ctx, int curve, unsigned log_m, int reduction, const dg16_srs_powers *powers,
                     dg16_srs_prepared *out);

/* ---- Membership of points and verification of a powers-of-tau transcript ---------------------------------------------
 * dg16_points_check: are n affine points (the layout of dg16_points_mul: x || y Montgomery limbs, identity = all-zero
 * bytes) points of `group` (1 = G1, 2 = G2) of `curve`?  All three curves.  A point is BAD when a coordinate is not
 * reduced (>= q), when it is off the equation of the curve or of its twist, or -- with subgroup = 1 -- when r P != O.
 * The identity is a good point.  subgroup = 0 stops after the curve equation; BN254 G1 has cofactor one, so subgroup
 * changes nothing there.  Bad points are a RESULT, not an error: the call returns DG16_OK with *n_bad their count and
 * *first_bad the smallest bad index (n when there is none).  n = 0 is DG16_OK with *n_bad = 0.  One point per lane: the
 * two cheap tests, then r P by a fixed chain over the non-adjacent form of the public constant r -- no table per point,
 * no recoding, mixed additions.  points_affine, n_bad, first_bad: host pointers only.  Synchronous;
 * runs on channel 0.  A large n runs in slices of the size dg16_ctx_set_points_mul_slice sets (default 2^16 points), and
 * the device copy of a slice is temporary (DG16_ERR_OOM leaves the context usable).  A null pointer with n > 0, a NULL
 * n_bad or first_bad, n >= 2^30 or a group other than 1 or 2 is DG16_ERR_BAD_ARG, an unknown curve DG16_ERR_BAD_CURVE. */
int dg16_points_check(dg16_ctx *ctx, int curve, int group, const void *points_affine, size_t n,
                      int subgroup /* 0: reduced coordinates and curve equation; 1: also order r */,
                      size_t *n_bad, size_t *first_bad /* n when none */);

/* Bits of dg16_srs_report::failed. */
#define DG16_SRS_BAD_POINT 1u  /* a point with an unreduced coordinate, off its curve or outside the subgroup */
#define DG16_SRS_IDENTITY 2u   /* tau_g1[0], tau_g1[1], tau_g2[0], tau_g2[1], alpha_tau_g1[0], beta_tau_g1[0] or beta_g2 is O */
#define DG16_SRS_TAU_G1 4u     /* tau_g1 is not a geometric progression in the tau of tau_g2[1] */
#define DG16_SRS_TAU_G2 8u     /* tau_g2 is not a geometric progression in the tau of tau_g1[1] */
#define DG16_SRS_ALPHA 16u     /* alpha_tau_g1 is not one */
#define DG16_SRS_BETA 32u      /* beta_tau_g1 is not one */
#define DG16_SRS_BETA_G2 64u   /* beta_g2 and beta_tau_g1[0] hold different beta */
typedef struct dg16_srs_report {
  uint32_t failed;        /* 0 = accepted; bits above */
  uint32_t bad_array;     /* with DG16_SRS_BAD_POINT: 0 tau_g1, 1 tau_g2, 2 alpha_tau_g1, 3 beta_tau_g1, 4 beta_g2 */
  uint64_t bad_index;     /* the smallest bad index in that array (the first array that has one) */
  uint64_t n_bad_points;  /* over all five arrays */
} dg16_srs_report;
/* Is this a powers-of-tau transcript (snarkjs `powersoftau verify`, without the contribution chain)?  BN254 and
 * BLS12-381.  powers: dg16_srs_powers above, m = 2^log_m.  With T = tau_g1, U = tau_g2, A = alpha_tau_g1,
 * B = beta_tau_g1 and coefficients rho_j, a bit of report->failed is CLEAR when:
 *   DG16_SRS_BAD_POINT  dg16_points_check(subgroup = 1) finds nothing in any of the five arrays
 *   DG16_SRS_IDENTITY   none of T_0, T_1, U_0, U_1, A_0, B_0, beta_g2 is the identity
 *   DG16_SRS_TAU_G1     e(sum_{j < 2m-2} rho_j T_j, U_1) = e(sum_{j < 2m-2} rho_j T_(j+1), U_0)
 *   DG16_SRS_TAU_G2     e(T_1, sum_{j < m-1} rho_j U_j) = e(T_0, sum_{j < m-1} rho_j U_(j+1))
 *   DG16_SRS_ALPHA      e(sum_{j < m-1} rho_j A_j, U_1) = e(sum_{j < m-1} rho_j A_(j+1), U_0)
 *   DG16_SRS_BETA       the same with B
 *   DG16_SRS_BETA_G2    e(B_0, U_0) = e(T_0, beta_g2)
 * Membership runs first: with DG16_SRS_BAD_POINT or DG16_SRS_IDENTITY set the five pairing checks are skipped and
 * their bits stay clear (the sums use the endomorphism split and the pairing assumes subgroup points).  The eight sums
 * (six in G1, two in G2) are the library's MSM on the device, the second of a pair on the same array shifted by one point; the five
 * equalities are two Miller loops and one final exponentiation each, on the host.  The base points are whatever T_0
 * and U_0 are: comparing them with the standard generators is a byte comparison for the caller.
 * report->failed != 0 comes with DG16_OK: a bad transcript is a result, not an error.
 * THE COEFFICIENTS ARE THE CALLER'S, as in dg16_groth16_verify_aggregate: coeffs = (2m - 2) x 16 bytes, each a
 * little-endian unsigned 128-bit integer; the sums of m - 1 terms use the first m - 1.  The contract: the rho_j are
 * independent and uniform in [1, 2^128), and they are chosen AFTER the transcript is fixed.  A transcript that fails an
 * equation is then accepted with probability about 2^-128 per equation.  A zero coefficient is DG16_ERR_BAD_ARG,
 * checked before any work.
 * powers, coeffs, report and every array: host pointers only.  Synchronous; runs on channel 0; the device copies are
 * temporary (DG16_ERR_OOM leaves the context usable).  log_m = 0, log_m > 26, log_m + 1 above the two-adicity of r or
 * a NULL pointer: DG16_ERR_BAD_ARG.  DG16_BLS12_377 (no pairing here): DG16_ERR_UNSUPPORTED.  An unknown curve:
 * DG16_ERR_BAD_CURVE. */
int dg16_srs_verify(dg16_ctx *ctx, int curve, unsigned log_m, const dg16_srs_powers *powers,
                    const void *coeffs /* (2m - 2) x 16 bytes */, dg16_srs_report *report);

/* ---- Groth16 prover (single prover; the value the n-party run must equal) ------------------------
 * Replaces `Groth16::<E, CircomReduction>::create_proof_with_reduction_and_matrices` (third-party
 * fork; call sites groth16/examples/sha256.rs:159, mpc-api/src/main.rs:393) from the point where
 * the QAP evaluation vectors exist (groth16/src/qap.rs:44-91 produces a, b, c).
 *
 * dg16_pk_create makes the proving key resident in HBM.  Queries are the arkworks `ProvingKey`
 * vectors, element 0 included: a_query, b_g1_query, b_g2_query have num_vars entries, l_query has
 * num_vars - num_inputs, h_query has domain_size entries (CircomReduction::h_query_scalars,
 * ark-circom/src/circom/qap.rs:94-110).  fixed_points = alpha_g1 | beta_g1 | delta_g1 (G1 affine)
 * | beta_g2 | delta_g2 (G2 affine), contiguous.  The base-vector mapping follows
 * groth16/src/proving_key.rs:48-65.  flags: DG16_F_DEVICE_PTRS if every pointer is a device pointer.
 * dg16_pk_create and dg16_pk_create_shard with DG16_F_DEVICE_PTRS: synchronous; ordered behind the work enqueued on
 * channel 0's stream; outputs complete on return (the key is resident and the queries may be freed or overwritten).
 * curve: DG16_BN254, DG16_BLS12_381 or DG16_BLS12_377 -- the prover, its flags and its sharded forms are the same on all
 * three (BLS12-377 proofs cannot be VERIFIED here: dg16_vk_create).  Any other id: DG16_ERR_BAD_CURVE, *out = NULL. */
/* HBM budget, in bytes, of the window tables of ONE resident key (dg16_pk_create*: the five tables together) or ONE
 * base set (dg16_bases_upload) built on this context from now on; 0 (the default) = unlimited.  A full table has one
 * row T[w] = 2^(c w) P per c-bit window (BN254, 2^20 wires, c = 17: 6.0 GB per key; BLS12-381 at 2^24: 126 GB).  Under a
 * budget the tables keep every k-th row, the smallest k that fits: the MSMs then run k bucket sets joined by a
 * Horner tail of (k - 1) c doublings -- same results, more bucket reductions.  k = W degenerates to the plain bases. */
int dg16_ctx_set_table_budget(dg16_ctx *ctx, uint64_t bytes);
typedef struct dg16_pk dg16_pk;
int dg16_pk_create(dg16_ctx *ctx, int curve, size_t num_vars, size_t num_inputs, size_t domain_size,
                   const void *a_query, const void *b_g1_query, const void *b_g2_query,
                   const void *h_query, const void *l_query, const void *fixed_points, unsigned flags,
                   dg16_pk **out);
void dg16_pk_destroy(dg16_pk *pk);

/* What a resident key holds (for reports: bench.py prints it next to every timing, because the proof time depends
 * on the window tables built here, once per key).  n_*: points per MSM launch of this shard (slice + delta slots);
 * c_*: window bits of the tables; table_bytes: HBM held by the five tables.  (Facts of the key only: measured
 * rates and instruction counts of the kernels live with the benchmarks -- profiles/, bench.py -- not in the ABI.) */
typedef struct dg16_pk_info {
  uint64_t n_ab, n_l, n_h;
  uint32_t c_ab, c_l, c_h;
  uint32_t shard, n_shards;
  uint64_t table_bytes;
  uint32_t table_stride; /* 1: one table row per window; k > 1: every k-th row kept (dg16_ctx_set_table_budget) */
} dg16_pk_info;
int dg16_pk_info_get(const dg16_pk *pk, dg16_pk_info *out);

/* Multi-GPU form: the key holds slice `shard` of `n_shards` of every MSM range (contiguous slices of
 * a_query[1..], b_g1_query[1..], b_g2_query[1..]; the l_query elements of the same wires -- L shares the digit sort
 * of A / B1 / B; a contiguous slice of h_query, or with DG16_F_H_CYCLIC the elements shard + n_shards * j); the
 * delta pairs ride on the last shard.  Pass the FULL queries; only the slice is copied to the device. */
int dg16_pk_create_shard(dg16_ctx *ctx, int curve, size_t num_vars, size_t num_inputs,
                         size_t domain_size, const void *a_query, const void *b_g1_query,
                         const void *b_g2_query, const void *h_query, const void *l_query,
                         const void *fixed_points, unsigned shard, unsigned n_shards, unsigned flags,
                         dg16_pk **out);

/* a, b, c: QAP evaluation vectors (domain_size Montgomery Fr elements each); full_assignment:
 * num_vars Fr elements [1, public.., witness..] (Montgomery iff DG16_F_SCALARS_MONT); r_s: HOST
 * pointer to r || s (2 x 32 bytes, same form as the assignment).  proof_out: A (G1 Jacobian) |
 * B (G2 Jacobian) | C (G1 Jacobian).  Uses all three channels.  flags | DG16_F_QAP_LIBSNARK: for a LibsnarkReduction
 * key -- h is the quotient (A B - C) / Z of the a, b, c given (c from dg16_qap_r1cs); everything after h is the same. */
int dg16_groth16_prove(dg16_ctx *ctx, const dg16_pk *pk, const void *a, const void *b, const void *c,
                       const void *full_assignment, const void *r_s, unsigned flags, void *proof_out);

/* The two halves of dg16_groth16_prove, for one-process-per-GPU runs:
 *   dg16_groth16_msms      h-polynomial + this shard's five MSMs -> results record
 *                          (A, B1, L, H as G1 Jacobian, then B as G2 Jacobian; dg16_groth16_results_bytes)
 *   <all-gather of the records over RCCL, done by the caller>
 *   dg16_groth16_assemble  per-MSM sum of the n_shards records + the A/B/C assembly of prove.rs:21-136
 * This is d_msm's "gather to king, sum, broadcast" (dist-primitives/src/dmsm/mod.rs:88-97) with the
 * sum done on every rank.  dg16_groth16_results_bytes: bytes of one record (six G1 and one G2 Jacobian points: 768 for
 * BN254, 1152 for BLS12-381 and BLS12-377), 0 for an unknown curve id. */
size_t dg16_groth16_results_bytes(int curve);
int dg16_groth16_msms(dg16_ctx *ctx, const dg16_pk *pk, const void *a, const void *b, const void *c,
                      const void *full_assignment, const void *r_s, unsigned flags, void *results_out);
int dg16_groth16_assemble(dg16_ctx *ctx, const dg16_pk *pk, const void *gathered_results,
                          size_t n_shards, const void *r_s, unsigned flags, void *proof_out);

/* ---- one process per GPU: collectives, sharded h-polynomial, distributed prove ----------------------------------
 * The king / client exchange of the reference (mpc-net/src/lib.rs:61-140 under dist-primitives/src/channel/mod.rs:8-57)
 * re-mapped to the GPUs of one node: `dg16_comm` is what the prover needs from a transport, dg16_rccl_* is the
 * native implementation (RCCL grouped send / recv on device buffers over xGMI, stream-ordered: no host
 * synchronisation on the data path).  A comm may also be implemented by the caller (tests drive these entry points
 * with a torch.distributed / gloo-backed comm).
 *
 *   all_gather   every rank contributes `bytes`; recv_dev gets n_ranks * bytes ordered by rank
 *                (d_msm's "gather to king, sum, send back" with the sum on every rank, dmsm/mod.rs:88-97)
 *   all_to_all   bytes_per_peer bytes at send_dev + p * bytes_per_peer go to rank p and land at
 *                recv_dev + me * bytes_per_peer there (the butterfly exchange of the sharded NTT; the reference
 *                does gather -> fft2_in_place -> scatter through the king, dfft/mod.rs:185-256)
 * Both are ordered on `hip_stream`: the payload was produced on it, the result may be consumed on it. */
typedef struct dg16_comm {
  void *self;
  unsigned (*n_ranks)(void *self);
  unsigned (*rank)(void *self);
  int (*all_gather)(void *self, const void *send_dev, size_t bytes, void *recv_dev, void *hip_stream);
  int (*all_to_all)(void *self, const void *send_dev, void *recv_dev, size_t bytes_per_peer, void *hip_stream);
} dg16_comm;

/* ONE 2^log_n-point transform over n_ranks GPUs (2, 4 or 8; 2^log_n >= n_ranks^2) with ONE all-to-all -- the "all-to-all
 * of NTT butterflies": what d_fft / d_ifft (dist-primitives/src/dfft/mod.rs:17-95) do through the king (local levels,
 * gather, remaining levels, scatter), as a four-step transform without a king.  in: this rank's CYCLIC elements
 * x[n_ranks * j + rank], j < M = 2^log_n / n_ranks.  out (M elements, may not alias in): the transposed layout of a
 * four-step FFT, out[k1 * S + j] = X[M * k1 + rank * S + j], S = M / n_ranks, k1 < n_ranks (rank sigma ends with slice
 * sigma of every length-M block of the natural-order output).  inverse != 0: inverse root and the 1 / 2^log_n scale.
 * dg16_ntt_dist_stage: the two local stages for callers that run the exchange themselves (stage 0: in -> send buffer,
 * natural order = n_ranks pieces of S; stage 1: receive buffer -> out). */
int dg16_ntt_dist(dg16_ctx *ctx, int curve, const dg16_comm *comm, const void *in, void *out, unsigned log_n,
                  int inverse, unsigned flags, int channel);
int dg16_ntt_dist_stage(dg16_ctx *ctx, int curve, unsigned log_n, unsigned rank, unsigned n_ranks, int inverse,
                        int stage, const void *in, void *out, unsigned flags, int channel);

/* h-polynomial over n_ranks GPUs (2, 4 or 8; 2^log_m >= n_ranks^2).  a, b, c: this rank's CYCLIC rows of the QAP
 * evaluation vectors, a[n_ranks * j + rank], j < 2^log_m / n_ranks (dg16_qap_rows); out: h[rank + n_ranks * j] --
 * the scalars of a DG16_F_H_CYCLIC key shard.  Two all-to-alls of 3 * 32 * 2^log_m / n_ranks bytes per rank.
 * Device pointers only (DG16_F_DEVICE_PTRS must be set). */
int dg16_h_poly_dist(dg16_ctx *ctx, int curve, const dg16_comm *comm, const void *a_rows, const void *b_rows,
                     const void *c_rows, unsigned log_m, void *out, unsigned flags, int channel);
/* The three local stages of dg16_h_poly_dist, for callers that run the exchanges themselves:
 *   stage 0  in = {a_rows, b_rows, c_rows}         out = send buffer 1  [peer][vector][S], S = 2^log_m / n_ranks^2
 *   stage 1  in = {receive buffer 1}               out = send buffer 2  [peer][vector][S]
 *   stage 2  in = {receive buffer 2}               out = h[rank + n_ranks * j]
 * Buffers hold 3 * 2^log_m / n_ranks elements. */
int dg16_h_poly_dist_stage(dg16_ctx *ctx, int curve, unsigned log_m, unsigned rank, unsigned n_ranks, int stage,
                           const void *const *in, void *out, unsigned flags, int channel);

/* dg16_groth16_msms with the h-polynomial already made (h_shard: the n_h scalars of this key's h slice, Montgomery
 * form, device pointer or host per flags) -- the half of a distributed proof after the sharded h-polynomial. */
int dg16_groth16_msms_h(dg16_ctx *ctx, const dg16_pk *pk, const void *h_shard, const void *full_assignment,
                        const void *r_s, unsigned flags, void *results_out);

/* The whole distributed proof on this rank, stream-ordered: sharded h-polynomial (two all-to-alls), this shard's
 * five MSMs, one all-gather of the results records, assembly.  pk: a DG16_F_H_CYCLIC shard (rank = shard,
 * n_ranks = n_shards); a_rows, b_rows, c_rows as for dg16_h_poly_dist.  With comm == NULL (or one rank) and an
 * unsharded key this is dg16_groth16_prove.  Every rank receives the same proof. */
int dg16_groth16_prove_dist(dg16_ctx *ctx, const dg16_pk *pk, const dg16_comm *comm, const void *a_rows,
                            const void *b_rows, const void *c_rows, const void *full_assignment, const void *r_s,
                            unsigned flags, void *proof_out);

/* Native RCCL transport.  Rank 0 makes the 128-byte id (dg16_rccl_unique_id) and hands it to the other ranks out
 * of band (the launcher's rendezvous); every rank then calls dg16_rccl_create on its own context (blocking until all
 * ranks have joined).  dg16_rccl_comm serves dg16_h_poly_dist / dg16_groth16_prove_dist; dg16_rccl_net is the MpcNet
 * vtable below (king = rank 0), so that d_fft / d_msm / d_pp / ext_wit::h / prove::A,B,C run one party per GPU.
 * The handle holds THREE communicators, one per MultiplexedStreamID (mpc-net/src/lib.rs:29-33): channel c of the
 * vtable only ever touches communicator c, under that communicator's mutex, so the three d_msm that prove::C joins
 * (groth16/src/prove.rs:113-125; dg16_prove_c drives them from three host threads) cannot meet each other's
 * payloads whatever order the threads run in on each party.  Communicator 0 also carries the dg16_comm collectives.
 * Channels 1 and 2 are ncclCommSplit duplicates of the first communicator (dg16_rccl_channels_split() == 1) or, on a
 * librccl without that entry point, joined through two fresh ids broadcast over it.  librccl is bound at run time
 * (dlopen): without it these return DG16_ERR_UNSUPPORTED and the rest of the library is unaffected. */
typedef struct dg16_rccl dg16_rccl;
struct dg16_net;
int dg16_rccl_unique_id(void *out128);
int dg16_rccl_create(dg16_ctx *ctx, const void *unique_id128, unsigned n_ranks, unsigned rank, dg16_rccl **out);
/* rank count and this rank's index as the communicator itself reports them (ncclCommCount / ncclCommUserRank) */
int dg16_rccl_ranks(dg16_rccl *h, unsigned *n_ranks, unsigned *rank);
int dg16_rccl_channels_split(dg16_rccl *h);
const dg16_comm *dg16_rccl_comm(dg16_rccl *h);
const struct dg16_net *dg16_rccl_net(dg16_rccl *h);
void dg16_rccl_destroy(dg16_rccl *h);
const char *dg16_rccl_error(void);

/* ---- dist-primitives, literally (packed secret sharing over an MpcNet) -----------------------------
 * These mirror the reference's functions one to one; "party" = one caller (a host thread with its own
 * dg16_ctx for the in-process LocalNet, or one process per GPU with RCCL-backed callbacks).  All
 * payloads are device buffers.
 *
 *   dg16_pss_create        PackedSharingParams::new(l)                 secret-sharing/src/pss.rs:34-62
 *   dg16_pss_apply         pack_from_public / unpack / unpack2 (batched) pss.rs:86-148
 *   dg16_pss_apply_exp     packexp_from_public / unpackexp             dist-primitives/src/dmsm/mod.rs:7-68
 *   dg16_d_fft             d_fft (inverse = 0) / d_ifft (inverse = 1)  dist-primitives/src/dfft/mod.rs:17-95
 *                          incl. fft1_in_place :98-140, fft2_in_place :142-182,
 *                          fft2_with_rearrange_pad :185-256, fft_in_place_rearrange :258-271,
 *                          pack_vec / transpose utils/pack.rs:4-33
 *   dg16_d_msm             d_msm                                        dist-primitives/src/dmsm/mod.rs:70-98
 *   dg16_deg_red           deg_red                                      dist-primitives/src/utils/deg_red.rs:10-28
 *   dg16_d_pp              d_pp                                         dist-primitives/src/dpp/mod.rs:17-88
 *   dg16_ext_wit_h         ext_wit::h                                   groth16/src/ext_wit.rs:16-101
 *   dg16_prove_a / _b / _c prove::A / B / C::compute                    groth16/src/prove.rs:21-46, 62-85, 106-136
 *   dg16_net               MpcNet's provided gather / scatter           mpc-net/src/lib.rs:61-140
 *   dg16_localnet_*        LocalTestNet                                 mpc-net/src/multi.rs:227-329
 */
typedef struct dg16_pss dg16_pss;
typedef struct dg16_localnet dg16_localnet;

/* Transport vtable (MpcNet): both collectives are blocking and ordered per channel.  send/recv are
 * device pointers; `hip_stream` is the stream the payload was produced on (the callee synchronises or
 * orders on it).  gather: every party contributes `bytes`; on the king (party 0) `recv_dev` receives
 * n_parties * bytes ordered by party id (client_send_or_king_receive, lib.rs:61-99).  scatter: the king
 * provides n_parties * bytes in `send_dev`, every party receives its `bytes` (lib.rs:102-140; equal
 * lengths are enforced by the single `bytes`, as lib.rs:116-124 checks). */
typedef struct dg16_net {
  void *self;
  unsigned (*n_parties)(void *self);
  unsigned (*party_id)(void *self);
  int (*gather_to_king)(void *self, int channel, const void *send_dev, size_t bytes, void *recv_dev,
                        void *hip_stream);
  int (*scatter_from_king)(void *self, int channel, const void *send_dev, size_t bytes, void *recv_dev,
                           void *hip_stream);
  /* MpcNet's required methods (mpc-net/src/lib.rs:46-58): is_init, and the point-to-point pair the two provided
   * collectives above are written in terms of.  A send_to(peer) completes against the peer's recv_from(me) with
   * the same channel and the same `bytes` (a length mismatch is DG16_ERR_NET on both sides, like the reference's
   * framing error); both are ordered on `hip_stream`. */
  int (*is_init)(void *self);
  int (*send_to)(void *self, unsigned peer, int channel, const void *send_dev, size_t bytes, void *hip_stream);
  int (*recv_from)(void *self, unsigned peer, int channel, void *recv_dev, size_t bytes, void *hip_stream);
} dg16_net;

int dg16_localnet_create(unsigned n_parties, dg16_localnet **out);
const dg16_net *dg16_localnet_party(dg16_localnet *net, unsigned id);
void dg16_localnet_destroy(dg16_localnet *net);
/* A party that fails outside a collective aborts the net: pending and future collectives return
 * DG16_ERR_NET on every party ("Stream died", mpc-net/src/multi.rs:393) instead of waiting; a
 * collective that is not joined by all parties within the timeout aborts by itself. */
void dg16_localnet_abort(dg16_localnet *net);
void dg16_localnet_reset(dg16_localnet *net, unsigned timeout_s);

/* l: the packing factor, 1, 2, 4 or 8 (n = 4 l = 4, 8, 16 or 32 parties, t = l - 1); anything else is
 * DG16_ERR_BAD_ARG.  Every primitive below takes every accepted l; dg16_ext_wit_h does with
 * DG16_F_H_ODD (see there). */
int dg16_pss_create(dg16_ctx *ctx, int curve, unsigned l, dg16_pss **out);
void dg16_pss_destroy(dg16_pss *pp);
/* which: 0 pack ([count][l] -> [count][n]), 1 unpack ([count][n] -> [count][l]), 2 unpack2 */
int dg16_pss_apply(dg16_ctx *ctx, const dg16_pss *pp, int which, const void *in, size_t count,
                   void *out, unsigned flags, int channel);
/* same on affine group elements ("in the exponent"); group 1 or 2 */
int dg16_pss_apply_exp(dg16_ctx *ctx, const dg16_pss *pp, int group, int which, const void *in,
                       size_t count, void *out, unsigned flags, int channel);

/* packexp_from_public over l-chunks of a point vector, all parties at once (dist-primitives/src/dmsm/mod.rs:50-68 under
 * groth16/src/proving_key.rs:67-81).  shares: party-major, [pp->n][chunks] affine points, chunks = ceil(n_points / l) =
 * dg16_pss_pack_chunks(pp, n_points); share r of chunk e is sum_{c<l} M[r][c] * points[e * l + c] with M the pack matrix
 * of pp and the last chunk padded with identities (arkworks' resize before the transform).
 * THE CONTRACT: the result equals dg16_pss_apply_exp(which = 0) on the identity-padded chunks, transposed to party-major,
 * BYTE FOR BYTE -- affine Montgomery coordinates are unique and the identity is zero bytes.  The path differs: the n * l
 * multipliers are constants of (curve, l), so they are recoded once per handle (cached in pp; safe for concurrent host
 * threads), an input point's odd multiples are tabulated once for all n parties, the l terms of a share run on one
 * doubling chain, and the slice's results are converted with a batched inversion.
 * points_affine and shares are HOST pointers, as for dg16_points_scale.  in_subgroup != 0 is the caller's word that
 * every point has order r, which allows the endomorphism split for groups with a cofactor.  With in_subgroup = 0 the call
 * is correct for ANY point of the curve and only BN254 G1 is split (dg16_points_mul's rule).
 * Synchronous: the call runs on channel 0, is ordered behind the work enqueued on channel 0's stream, and the shares are
 * complete on return.  A large input runs in slices whose outputs do not exceed what dg16_ctx_set_points_mul_slice sets
 * (default 2^16), rounded to a multiple of 64 chunks; the device copy of a slice, its tables and its accumulators are
 * channel 0's workspace, and DG16_ERR_OOM leaves the context usable.
 * n_points = 0 is DG16_OK and writes nothing.  A NULL pointer with n_points > 0, a group other than 1 or 2,
 * n_points >= 2^30, or a pp of another context: DG16_ERR_BAD_ARG, and nothing is written.  A partial overlap of input
 * and output is the caller's error. */
int dg16_pss_pack_points(dg16_ctx *ctx, const dg16_pss *pp, int group, const void *points_affine, size_t n_points,
                         void *shares, int in_subgroup);
size_t dg16_pss_pack_chunks(const dg16_pss *pp, size_t n_points);

/* PackedProvingKeyShare::pack_from_arkworks_proving_key (proving_key.rs:35-110): s <- a_query[1..], u <- h_query,
 * w <- l_query, h <- b_g1_query[1..], v <- b_g2_query[1..] (G2); each output party-major as above, five
 * dg16_pss_pack_points under one call.  The arrays have the sizes of dg16_pk_create: a_query, b_g1_query, b_g2_query
 * num_vars points, h_query domain_size, l_query num_vars - num_inputs.  num_vars = 1 makes the three [1..] queries
 * empty, which is legal, and l_query (and out->w) may be NULL when num_vars == num_inputs; an empty query writes
 * nothing.  Host pointers, in_subgroup, synchronisation and errors are those of dg16_pss_pack_points; num_inputs = 0,
 * num_inputs > num_vars and sizes of 2^30 or more are DG16_ERR_BAD_ARG.  "Nothing is written" holds for these argument
 * errors, which are all checked before any work.  The five queries are packed one after another in the order s, u, w, h,
 * v, each complete before the next begins: a run-time failure in one of them (DG16_ERR_OOM, DG16_ERR_HIP) leaves the
 * outputs of the earlier ones written and the later ones untouched. */
typedef struct dg16_pk_shares { void *s, *u, *v, *w, *h; } dg16_pk_shares;
int dg16_pk_pack(dg16_ctx *ctx, const dg16_pss *pp, size_t num_vars, size_t num_inputs, size_t domain_size,
                 const void *a_query, const void *b_g1_query, const void *b_g2_query, const void *h_query,
                 const void *l_query, const dg16_pk_shares *out, int in_subgroup);

/* Element first + i of stream `stream` of a 32-byte seed, i < n: the caller's randomness stretched on the device, so that
 * only the seed crosses the bus.  With msg(j) = "dg16fe" || seed32[32] || le64(stream) || le64(first + i) || byte(j) (55
 * bytes: one SHA-256 compression each), the element is int_le(SHA-256(msg(0)) || SHA-256(msg(1))) mod r: a 512-bit
 * integer reduced, so the bias is below 2^-250.  out: n x 32 bytes, Montgomery form if mont != 0, else canonical.
 * Streams are independent; a (seed, stream, index) is one element whatever first and n a call uses.
 * seed32 and out are HOST pointers.  Synchronous: the call runs on channel 0 and out is complete on return.  n = 0 is
 * DG16_OK and writes nothing.  A NULL seed, a NULL out with n > 0, n >= 2^30 or first + n above 2^64 - 1:
 * DG16_ERR_BAD_ARG, and nothing is written; an unknown curve is DG16_ERR_BAD_CURVE. */
int dg16_fr_expand(dg16_ctx *ctx, int curve, const void *seed32, uint64_t stream, uint64_t first, size_t n, int mont,
                   void *out);

/* Packed shares of a scalar vector, all parties at once, plain (pack_from_public, secret-sharing/src/pss.rs:86-92) or
 * hiding (pack_from_public_rand, pss.rs:72-82, tested at :209-240).  shares: party-major, [pp->n][chunks] field elements,
 * chunks = dg16_pss_scalar_chunks(pp, layout, n_values).
 * layout: DG16_PACK_CHUNKS -- chunk e holds values[e l .. e l + l), the last one padded with zeros (pack_from_witness,
 * groth16/examples/sha256.rs:97-121), chunks = ceil(n_values / l).  DG16_PACK_DFFT -- n_values = m, a power of two with
 * m >= l; chunk e holds (x[e], x[e + m / l], ..) with x the bit-reversed vector (QAP::pss, groth16/src/qap.rs:151-165),
 * chunks = m / l.
 * blinds: NULL, or [chunks][l] field elements in the form of `values` (the map is linear, so Montgomery in gives
 * Montgomery out and canonical canonical).  Slot k of chunk e goes to position l + k of the secret domain, whose upper
 * l = t + 1 positions pack_from_public leaves at zero.  With blinds drawn uniformly by the caller any t parties' shares
 * are independent of the values; dg16_pss_apply(which = 1) and the protocols built on it drop the blind slots.
 * THE CONTRACT: with blinds == NULL the result equals dg16_pss_apply(which = 0) on the same chunks, transposed to
 * party-major, BYTE FOR BYTE.
 * values, blinds and shares are HOST pointers.  Synchronous: the call runs on channel 0, is ordered behind the work
 * enqueued on channel 0's stream, and the shares are complete on return.  A large input runs in slices of chunks whose
 * shares do not exceed what dg16_ctx_set_points_mul_slice sets, rounded down to a multiple of 64 chunks and never below
 * 64 chunks (a setting under 64 n is therefore exceeded: a slice is 64 chunks = 64 n shares).  Where the context sets
 * nothing the default here is 2^21 share elements (64 MB), not the 2^16 of the point calls that share the setting: a
 * share is 32 bytes and has no table.  The slices come from channel 0's workspace, a DG16_PACK_DFFT input is resident in full for the call, and DG16_ERR_OOM leaves the
 * context usable.
 * n_values = 0 is DG16_OK and writes nothing.  A NULL values or shares with n_values > 0, another layout, an m that is
 * not a power of two or is below l, n_values >= 2^30, or a pp of another context: DG16_ERR_BAD_ARG, and nothing is
 * written.  dg16_pss_scalar_chunks returns 0 for such arguments. */
enum { DG16_PACK_CHUNKS = 0, DG16_PACK_DFFT = 1 };
size_t dg16_pss_scalar_chunks(const dg16_pss *pp, int layout, size_t n_values);
int dg16_pss_pack_scalars(dg16_ctx *ctx, const dg16_pss *pp, int layout, const void *values, size_t n_values,
                          const void *blinds, void *shares);

/* What a client sends for one proof, packed for all parties in one call: a, b, c (m = 2^log_m evaluations each) with
 * DG16_PACK_DFFT (QAP::pss, qap.rs:151-165), full_assignment[1..] into a_share and full_assignment[num_inputs..] into
 * ax_share with DG16_PACK_CHUNKS (sha256.rs:97-121).  Outputs party-major as above: a, b, c [n][m / l], a_share
 * [n][ceil((num_vars - 1) / l)], ax_share [n][ceil((num_vars - num_inputs) / l)]; an empty vector writes nothing and its
 * output may be NULL.
 * seed32 == NULL packs plainly.  Otherwise every chunk is blinded as by dg16_pss_pack_scalars, and blind (e, k) of output
 * v (0 .. 4 in the struct's order) is element e l + k of stream v of dg16_fr_expand, in the form `mont` names -- the form
 * the inputs are in.  The blinds are made inside the packing kernel: they are never uploaded and never stored.  The seed
 * is the CALLER's randomness: 32 uniform bytes, used for one request.
 * Host pointers only.  Synchronous; runs on channel 0; slices and DG16_ERR_OOM as for dg16_pss_pack_scalars.  The five
 * vectors are packed in the struct's order, each complete before the next begins.  2^log_m < l, log_m >= 30,
 * num_inputs = 0, num_inputs > num_vars, num_vars >= 2^30, a NULL pointer or a pp of another context: DG16_ERR_BAD_ARG,
 * checked before any work, and nothing is written. */
typedef struct dg16_request_shares { void *a, *b, *c, *a_share, *ax_share; } dg16_request_shares;
int dg16_request_pack(dg16_ctx *ctx, const dg16_pss *pp, unsigned log_m, const void *a, const void *b, const void *c,
                      const void *full_assignment, size_t num_vars, size_t num_inputs, const void *seed32, int mont,
                      const dg16_request_shares *out);

/* share: this party's share_len packed shares; share_len * l must equal 2^log_m (the reference's
 * debug assertion, dfft/mod.rs:31-37) else DG16_ERR_BAD_ARG; out: pad * share_len elements. */
int dg16_d_fft(dg16_ctx *ctx, const dg16_pss *pp, const dg16_net *net, const void *share,
               size_t share_len, unsigned log_m, int rearrange, unsigned pad, int degree2, int inverse,
               void *out, unsigned flags, int channel);
/* bases / scalars: this party's share vectors; out: Jacobian point, identical on all parties. */
int dg16_d_msm(dg16_ctx *ctx, const dg16_pss *pp, const dg16_net *net, int group, const void *bases,
               const void *scalars, size_t n_bases, size_t n_scalars, unsigned flags, int channel,
               void *out);
/* d_msm with this party's base shares resident (dg16_bases_upload of the share vector). */
int dg16_d_msm_resident(dg16_ctx *ctx, const dg16_pss *pp, const struct dg16_net *net, const dg16_bases *bases,
                        const void *scalars, size_t n_scalars, unsigned flags, int channel, void *out);
int dg16_deg_red(dg16_ctx *ctx, const dg16_pss *pp, const dg16_net *net, const void *px, size_t count,
                 void *out, unsigned flags, int channel);
int dg16_d_pp(dg16_ctx *ctx, const dg16_pss *pp, const dg16_net *net, const void *num, const void *den,
              size_t count, void *out, unsigned flags, int channel);
/* a/b/c_share: this party's PackedQAPShare vectors (m/l each); out: m/l packed shares of h.
 * Uses channel 0 (the reference multiplexes channels 0..2 for the three transforms).  Six transform rounds (d_ifft
 * padded to 2m, d_fft on 2m, for each of a, b, c), then one gather of 3 * 2m/l shares and one scatter of m/l.
 * 2^log_m < l, log_m >= 48 and net.n_parties() != pp.n are DG16_ERR_BAD_ARG with and without the flag below.  Every
 * refusal is decided from pp, log_m and flags alone, before any collective: every party gets the same code and nobody
 * waits.
 *
 * Without DG16_F_H_ODD: the reference's ext_wit::h, share for share, its defect included.  The king's selection there
 * is `s1.swap(i, i * pp.l + pp.t)` for i < m on the 2m unpacked evaluations (ext_wit.rs:74-76).
 *   l = 2     keeps the odd positions: the packed sharing of CircomReduction's witness map.
 *   l = 4, 8  indexes past the vector and panics; here DG16_ERR_UNSUPPORTED.
 *   l = 1     (t = 0) the swap is the identity, so the FIRST m evaluations are kept, not the odd ones: the call mirrors
 *             that output, and it is NOT the witness map.
 *
 * With DG16_F_H_ODD: what the reference meant.  Same rounds, same channel, same message sizes; the king computes
 * h_i = p[2i+1] q[2i+1] - w[2i+1], i < m, over the natural-order unpacked evaluations, packs consecutive l-chunks
 * (pack_vec, utils/pack.rs:4-16) and scatters m/l shares per party.  The output is the packed sharing of
 * CircomReduction's witness map for l = 1, 2, 4, 8, and at l = 2 it is byte-equal to the unflagged call.  A Rust party
 * whose selection reads `s1[i] = s1[2 * i + 1]` interoperates.  The king forms only the odd-position secrets, in one
 * kernel (csrc/h_odd.h). */
int dg16_ext_wit_h(dg16_ctx *ctx, const dg16_pss *pp, const dg16_net *net, const void *a_share,
                   const void *b_share, const void *c_share, unsigned log_m, void *out, unsigned flags);
/* prove::A::compute (groth16/src/prove.rs:21-46): out = L + N * r + d_msm(S, a) on `channel` (the reference's `sid`).
 * L, N: G1 affine, in the clear (the identity (0, 0) is arkworks' default, as groth16/examples/sha256.rs:46-48 passes
 * it); r: one scalar (Montgomery iff DG16_F_SCALARS_MONT, like a); S, a: this party's packed shares; out: G1
 * Jacobian (E::G1), identical on all parties.  n_S != n_a is DG16_ERR_LENGTH_MISMATCH (the Err of G::msm). */
int dg16_prove_a(dg16_ctx *ctx, const dg16_pss *pp, const dg16_net *net, const void *L, const void *N,
                 const void *r, const void *S, const void *a, size_t n_S, size_t n_a, unsigned flags, int channel,
                 void *out);
/* prove::B::compute (prove.rs:62-85): out = Z + K * s + d_msm(V, a) in G2 (Z, K: G2 affine; out: G2 Jacobian). */
int dg16_prove_b(dg16_ctx *ctx, const dg16_pss *pp, const dg16_net *net, const void *Z, const void *K,
                 const void *s, const void *V, const void *a, size_t n_V, size_t n_a, unsigned flags, int channel,
                 void *out);
/* prove::C::compute (prove.rs:106-136): out = w + u + A * s + M * r + h * r with w = d_msm(W, ax), u = d_msm(U, h),
 * h = d_msm(H, a) JOINED on channels 0 / 1 / 2 like the reference's tokio::try_join! (:113-125): the call drives the
 * three channels of `ctx` from three host threads at once (every party must do the same, so the three collectives
 * of a channel meet their peers).  A: G1 Jacobian (E::G1, the value A::compute returned); M: G1 affine. */
int dg16_prove_c(dg16_ctx *ctx, const dg16_pss *pp, const dg16_net *net, const void *A, const void *M,
                 const void *s, const void *r, const void *W, const void *ax, size_t n_W, size_t n_ax,
                 const void *U, const void *h, size_t n_U, size_t n_h, const void *H, const void *a, size_t n_H,
                 size_t n_a, unsigned flags, void *out);

/* ---- circom `.r1cs` / snarkjs `.zkey` readers (host side of the library; no GPU involved) ----------------
 *   dg16_r1cs_parse   <- R1CSFile::new              ark-circom/src/circom/r1cs_reader.rs:54-249
 *   dg16_zkey_parse   <- read_zkey / BinFile         ark-circom/src/zkey.rs:53-388
 * Same acceptance rules as the reference (magic, version 1, 32-byte fields, BN254 moduli, section sizes, wire 0).
 * On failure the status is non-zero and dg16_io_error() (thread-local) gives the reference's error text.
 * dg16_r1cs copies what it keeps.  dg16_zkey is ZERO-COPY for points -- a zkey stores x || y Montgomery limbs with
 * the identity as (0, 0), i.e. this library's base layout -- so `data` must outlive the handle and the pointers
 * of dg16_zkey_points go straight into dg16_pk_create.  Matrix coefficients of a zkey are value * R^2 as stored
 * (zkey.rs:332-337): one dg16_field_op(from_mont) gives the Montgomery values dg16_qap takes; the rows snarkjs
 * appends for the public inputs are dropped and num_constraints = max row - n_public (zkey.rs:176-198). */
typedef struct dg16_r1cs dg16_r1cs;
typedef struct dg16_zkey dg16_zkey;
typedef struct dg16_r1cs_header {
  uint32_t n_wires, n_pub_out, n_pub_in, n_prv_in, n_constraints, has_wire_map;
  uint64_t n_labels;
} dg16_r1cs_header;
typedef struct dg16_zkey_header {
  uint32_t n_vars, n_public, domain_size, num_constraints;
} dg16_zkey_header;
typedef struct dg16_csr {   /* owned by the handle; coeff: nnz x 32-byte little-endian field elements */
  uint64_t n_rows, nnz;
  const uint32_t *row_ptr, *col;
  const void *coeff;
} dg16_csr;
enum {
  DG16_ZKEY_ALPHA_G1 = 0, DG16_ZKEY_BETA_G1 = 1, DG16_ZKEY_BETA_G2 = 2, DG16_ZKEY_GAMMA_G2 = 3,
  DG16_ZKEY_DELTA_G1 = 4, DG16_ZKEY_DELTA_G2 = 5, DG16_ZKEY_IC = 6, DG16_ZKEY_A = 7, DG16_ZKEY_B1 = 8,
  DG16_ZKEY_B2 = 9, DG16_ZKEY_L = 10, DG16_ZKEY_H = 11
};
const char *dg16_io_error(void);
int dg16_r1cs_parse(const void *data, size_t bytes, dg16_r1cs **out);
int dg16_r1cs_header_get(const dg16_r1cs *f, dg16_r1cs_header *out);
int dg16_r1cs_matrix(const dg16_r1cs *f, int which /* 0 A, 1 B, 2 C; canonical coefficients */, dg16_csr *out);
int dg16_r1cs_wire_map(const dg16_r1cs *f, const uint64_t **map /* NULL when the file has none */);
void dg16_r1cs_free(dg16_r1cs *f);
int dg16_zkey_parse(const void *data, size_t bytes, dg16_zkey **out);
int dg16_zkey_header_get(const dg16_zkey *z, dg16_zkey_header *out);
int dg16_zkey_points(const dg16_zkey *z, int which /* DG16_ZKEY_* */, const void **ptr, size_t *count);
int dg16_zkey_matrix(const dg16_zkey *z, int which /* 0 A, 1 B; value * R^2 */, dg16_csr *out);
void dg16_zkey_free(dg16_zkey *z);


/* ---- arkworks compressed Proof<Bn254> (host side; no GPU involved) ---------------------------------------
 *   dg16_proof_compress    <- proof.serialize_compressed       mpc-api/src/main.rs:154-171 (proof.bin)
 *   dg16_proof_decompress  <- Proof::deserialize_compressed     zk-cli verify path, test-circuits/sha256/proof.bin
 * 128 bytes: A (G1, 32) || B (G2, 64) || C (G1, 32); little-endian x, flags in the two top bits of the last byte
 * (bit 7: y > -y, Fq2 compared on (c1, c0); bit 6: infinity).  compress takes the 12 field elements that
 * dg16_groth16_prove writes (A, B, C Jacobian, Montgomery limbs); decompress writes A.x A.y | B.x B.y | C.x C.y
 * (8 field elements, Montgomery limbs, identity = zeros) and, with validate != 0, checks like Validate::Yes:
 * reduced coordinates, on the curve, B in the order-r subgroup.  BN254 only (the reference's proof curve). */
const char *dg16_serialize_error(void);
int dg16_proof_compress(int curve, const void *proof_jacobian, void *out128);
int dg16_proof_decompress(int curve, const void *in128, int validate, void *proof_affine);

/* ---- arkworks compressed key files (BN254) and compressed points (BN254, BLS12-377, BLS12-381) ----------------------
 *   <- pk.serialize_with_mode(.., Compress::Yes) / ProvingKey::deserialize_with_mode(.., Compress::Yes, Validate::No)
 *      and the same for VerifyingKey                               mpc-api/src/main.rs:154-171, :459-512
 * dg16_arkkey_layout (host code) walks the container: struct field order of ark-groth16's derive, a u64 little-endian
 * length in front of every Vec; offsets are byte offsets into the file, counts are points.  The point sections are
 * then (de)compressed in batches ON THE GPU by dg16_points_compress / _decompress -- one lane per point running the
 * same routines as the proof.bin codec above (pinned by the reference's own proof.bin): affine x || y Montgomery limbs
 * with the identity as zeros on one side (the layout dg16_pk_create and dg16_bases_upload take), 32 (G1) / 64 (G2)
 * bytes per point on the other; for BLS12-377 (ark-bls12-377 uses the same default SWFlags encoding -- the group
 * elements the reference's d_msm tests put on the wire, dist-primitives/examples/dmsm_test.rs) 48 / 96 bytes, and
 * validate != 0 checks the subgroup for G1 as well (cofactor != 1).  BLS12-381 (BASELINE config 5's curve; not a
 * dependency of the reference): ark-bls12-381 0.4 overrides the format with the zcash / IETF encoding -- 48 / 96 bytes,
 * BIG-endian x (G2: x.c1 || x.c0), flags in the three top bits of the FIRST byte: 0x80 compressed (always written, and
 * required when reading), 0x40 infinity, 0x20 y is the larger of (y, -y).  In every form an infinity encoding must
 * carry x = 0 and no sign flag (stricter than arkworks 0.4, which ignores the rest of an infinity encoding).
 * dg16_points_decompress is synchronous: a coordinate that is not reduced, bad flags
 * or an x off the curve return DG16_ERR_BAD_ARG (dg16_codec_error names the first failing point), like the Err of
 * deserialize_with_mode; validate != 0 adds the order-r subgroup check for G2 (Validate::Yes). */
typedef struct dg16_arkkey_layout_t {
  uint64_t n_ic, n_a, n_b1, n_b2, n_h, n_l;
  uint64_t off_alpha_g1, off_beta_g2, off_gamma_g2, off_delta_g2, off_ic;              /* VerifyingKey */
  uint64_t off_beta_g1, off_delta_g1, off_a, off_b1, off_b2, off_h, off_l;             /* rest of ProvingKey */
  uint64_t bytes;
} dg16_arkkey_layout_t;
const char *dg16_codec_error(void);
int dg16_arkkey_layout(const void *data, size_t bytes, int verifying_key_only, dg16_arkkey_layout_t *out);
int dg16_points_compress(dg16_ctx *ctx, int curve, int group, const void *affine, size_t n, void *out,
                         unsigned flags, int channel);
int dg16_points_decompress(dg16_ctx *ctx, int curve, int group, const void *in, size_t n, int validate,
                           void *affine_out, unsigned flags, int channel);

/* Vec<F> as MpcSerNet puts it on the wire (`out.serialize_compressed`, dist-primitives/src/channel/mod.rs:14,49):
 * u64 little-endian length || canonical little-endian 32-byte elements.  Between GPUs of one node the payloads of
 * dg16_net stay in the HBM form; these two convert at the edge to a party that speaks ark-serialize (group elements:
 * dg16_points_compress above).  Decode checks the prefix against `bytes` and every element < r. */
size_t dg16_wire_fr_bytes(size_t n);
int dg16_wire_fr_encode(dg16_ctx *ctx, int curve, const void *mont, size_t n, void *out, unsigned flags, int channel);
int dg16_wire_fr_decode(dg16_ctx *ctx, int curve, const void *in, size_t bytes, void *out_mont, size_t *n_out,
                        unsigned flags, int channel);

/* ---- Groth16 verification, BN254 (host side; no GPU involved: four pairings) --------------------------------
 *   dg16_groth16_verify  <- Groth16::<Bn254>::verify_proof   groth16/examples/sha256.rs:228-254, mpc-api verify
 * e(A, B) = e(alpha, beta) e(IC_0 + sum x_i IC_i, gamma) e(C, delta).  Points are affine x || y Montgomery limbs
 * with the identity as zeros -- the layout of a zkey's header / IC section (dg16_zkey_points) and of
 * dg16_proof_decompress.  public_inputs: n_public scalars of 32 bytes, canonical or (DG16_F_SCALARS_MONT)
 * Montgomery.  n_ic != n_public + 1 returns DG16_ERR_LENGTH_MISMATCH (ark-groth16's MalformedVerifyingKey).
 * Validation (what arkworks' Validate::Yes deserialisation guarantees before verify_proof runs): a verifying-key
 * point with a non-reduced coordinate, off its curve or (G2) outside the order-r subgroup, or a public input >= r,
 * returns DG16_ERR_BAD_ARG (no input aliasing: x and x + r are not the same input); a PROOF point with a
 * non-reduced coordinate, off its curve, or B outside the subgroup is a rejection (*accepted = 0), not an error.
 * *accepted = 1 iff all checks pass and the equation holds. */
const char *dg16_verify_error(void);
int dg16_groth16_verify(int curve, const void *alpha_g1, const void *beta_g2, const void *gamma_g2,
                        const void *delta_g2, const void *ic, size_t n_ic, const void *public_inputs,
                        size_t n_public, const void *proof_affine, unsigned flags, int *accepted);

/* ---- Batched Groth16 verification on the GPU, BN254 and BLS12-381 -------------------------------------------------
 *   dg16_vk_create             <- ark_groth16::prepare_verifying_key / PreparedVerifyingKey
 *   dg16_groth16_verify_batch  <- Groth16::verify_proof / verify_proof_with_prepared_inputs, once per proof
 * The equation and the point layout of dg16_groth16_verify above (affine x || y Montgomery limbs, identity = zeros;
 * 32-byte Fq for BN254, 48-byte for BLS12-381), decided on the device by an optimal ate pairing, one proof per lane.
 * DG16_BLS12_377 returns DG16_ERR_UNSUPPORTED from dg16_vk_create: the reference proves on BN254, and there is no
 * independent BLS12-377 pairing to check a verifier against.
 * dg16_vk_create validates the key by the rules above -- a non-reduced coordinate, a point off its curve, a G2 point
 * outside the order-r subgroup: DG16_ERR_BAD_ARG; on BLS12-381 G1 has a cofactor, so alpha_g1 and every ic point are
 * subgroup-checked too -- and does the per-key work once: the Miller value of (alpha, beta) and the Miller-loop line
 * tables of gamma and delta.  The key's pointers are host pointers, or all device pointers with DG16_F_DEVICE_PTRS
 * (no other flag is accepted); the call is synchronous and the handle owns its device memory until dg16_vk_destroy.
 * With DG16_F_DEVICE_PTRS: synchronous; ordered behind the work enqueued on channel 0's stream; outputs complete on return.
 * dg16_groth16_verify_batch: public_inputs = n_proofs x n_public scalars (row i belongs to proof i), proofs_affine =
 * n_proofs x (A | B | C), verdict = n_proofs bytes.  verdict[i] = 1 iff proof i passes every check and the equation
 * holds, else 0.  n_public + 1 != n_ic returns DG16_ERR_LENGTH_MISMATCH; n_proofs = 0 is DG16_OK.  Whatever is wrong
 * with ONE proof rejects THAT proof and nothing else: a non-reduced proof coordinate, a proof point off its curve, B
 * outside the subgroup, on BLS12-381 also A or C outside the subgroup, and a public input >= r (the single-proof call
 * returns DG16_ERR_BAD_ARG for that; here x and x + r are still not the same input, but one sender's bad input does
 * not fail the batch).  Identity points in a proof are legal: the verdict is what the equation gives.
 * DG16_F_SCALARS_MONT as everywhere; host pointers: synchronous; DG16_F_DEVICE_PTRS: stream-ordered on `channel`,
 * verdict a device pointer (16-byte aligned inputs and proofs).  Temporaries come from the channel's workspace
 * (DG16_ERR_OOM leaves the context usable).  Per-proof verdicts only; dg16_groth16_verify_aggregate below gives ONE
 * verdict for the whole batch by random-linear-combination batching. */
typedef struct dg16_vk dg16_vk;
int dg16_vk_create(dg16_ctx *ctx, int curve, const void *alpha_g1, const void *beta_g2, const void *gamma_g2,
                   const void *delta_g2, const void *ic, size_t n_ic, unsigned flags, dg16_vk **out);
void dg16_vk_destroy(dg16_vk *vk);
int dg16_groth16_verify_batch(dg16_ctx *ctx, const dg16_vk *vk, const void *public_inputs, size_t n_public,
                              const void *proofs_affine, size_t n_proofs, unsigned flags, uint8_t *verdict,
                              int channel);

/* ---- Aggregate Groth16 verification: one verdict for a batch (BN254 and BLS12-381) ---------------------------------
 *   dg16_groth16_verify_aggregate  <- Groth16::verify_proof in a loop whose caller only asks "is the whole batch valid?"
 * The small-exponent test (what bellman's verify_proofs_batch does on the CPU): with coefficients rho_i,
 *   prod_i e(rho_i A_i, B_i) * e(-sum_j s_j IC_j, gamma) * e(-sum_i rho_i C_i, delta) * e(-s_0 alpha, beta) == 1,
 *   s_j = sum_i rho_i x_ij mod r, x_i0 = 1 (so s_0 = sum_i rho_i)
 * -- per proof one Miller loop, per batch two MSMs, three Miller loops from the key's line tables and ONE final
 * exponentiation.  Key handle, point layout, input layout, curves and DG16_F_SCALARS_MONT / DG16_F_DEVICE_PTRS (the only
 * flags accepted) are those of dg16_groth16_verify_batch; coeffs = n_proofs x 16 bytes, each a little-endian unsigned
 * 128-bit integer; accepted = ONE byte.  With DG16_F_DEVICE_PTRS the call is stream-ordered on `channel` and coeffs and
 * accepted are device pointers too (16-byte aligned coeffs).  Temporaries come from the channel's workspace
 * (DG16_ERR_OOM leaves the context usable).
 * *accepted = 1 iff (a) EVERY proof passes the per-proof input checks of dg16_groth16_verify_batch (reduced coordinates,
 * points on their curves, B in G2, on BLS12-381 A and C in G1, every public input < r) and (b) the combined equation
 * holds.  Anything wrong with any proof is *accepted = 0 and DG16_OK, not an error.  A zero coefficient is
 * *accepted = 0 (a proof is never silently skipped); n_proofs = 0 is *accepted = 1; n_public + 1 != n_ic returns
 * DG16_ERR_LENGTH_MISMATCH.  Identity points in a proof are legal: the equation decides.
 * THE COEFFICIENTS ARE THE CALLER'S: the library draws no randomness (as dg16_groth16_prove takes r and s).  The
 * contract: the rho_i are independent and uniform in [1, 2^128), and they are chosen AFTER the proofs are fixed.  A batch
 * that holds an invalid proof is then accepted with probability about 2^-128.  Equal or predictable coefficients void
 * the guarantee (two tampered proofs whose errors cancel under equal coefficients pass).  On *accepted = 0,
 * dg16_groth16_verify_batch says which proofs are bad. */
int dg16_groth16_verify_aggregate(dg16_ctx *ctx, const dg16_vk *vk, const void *public_inputs, size_t n_public,
                                  const void *proofs_affine, size_t n_proofs,
                                  const void *coeffs /* n_proofs x 16 bytes, little-endian unsigned */, unsigned flags,
                                  uint8_t *accepted /* ONE byte */, int channel);

/* ---- Batched point multiplication and Groth16 proof re-randomization ------------------------------------------------
 * out[i] = scalars[i] * points[i], i < n.  points / out: affine x || y Montgomery limbs of the group's coordinate
 * field, identity = all-zero bytes (the layout of dg16_fixed_base_mul's output and of dg16_groth16_verify_batch's
 * proofs).  scalars: n x 32 bytes, integers below 2^255 (canonical field elements are), or Montgomery form with
 * DG16_F_SCALARS_MONT.  All three curves, group 1 or 2.  Correct for ANY point of the curve, like dg16_msm; the points
 * are neither checked to be on the curve nor in the subgroup (dg16_points_decompress(validate) does that).  With
 * DG16_F_BASES_IN_SUBGROUP the library splits the scalars with the curve's endomorphism (half or a quarter of the
 * doublings); without it only the cofactor-one group (BN254 G1) is split: the rule of dg16_msm.  Host pointers:
 * synchronous.  DG16_F_DEVICE_PTRS: stream-ordered on `channel`.  out may be the same buffer as points, not a partial
 * overlap.  n = 0 is DG16_OK; a null pointer with n > 0 or a group other than 1 or 2 is DG16_ERR_BAD_ARG, an unknown
 * curve DG16_ERR_BAD_CURVE.  Temporaries come from the channel's workspace (DG16_ERR_OOM leaves the context usable); a
 * large n is processed in slices of 2^16 products (dg16_ctx_set_points_mul_slice changes that for contexts short of
 * memory and for tests: 0 = default, at most 2^20; rounded up to a multiple of 64). */
int dg16_points_mul(dg16_ctx *ctx, int curve, int group, const void *points_affine, const void *scalars, size_t n,
                    void *out_affine, unsigned flags, int channel);
int dg16_ctx_set_points_mul_slice(dg16_ctx *ctx, size_t products);
/* proofs_out[i] = (A', B', C'),  A' = r1^-1 A,  B' = r1 B + (r1 r2) delta_g2,  C' = C + r2 A
 * (ark_groth16::Groth16::rerandomize_proof; figure 1 of Baghery-Kohlweiss-Siim-Volkhov).  Key handle, proof layout
 * (n_proofs x (A | B | C), affine), curves (BN254, BLS12-381) and flags (DG16_F_SCALARS_MONT, DG16_F_DEVICE_PTRS only)
 * are those of dg16_groth16_verify_batch.  r1_r2: n_proofs x (r1 | r2), 2 x 32 bytes, each in [1, r).
 * THE RANDOMNESS IS THE CALLER'S (as r, s of the prover and the aggregate verifier's coefficients): independent and
 * uniform per proof.  The proofs are NOT verified or validated here: (A', B', C') satisfies the verification equation
 * for the same public inputs exactly when (A, B, C) does (both sides gain the factor e(r2 A, delta)); verify first.
 * The caller guarantees that the points are on their curves and in the order-r subgroups (true of any proof
 * dg16_groth16_verify_batch accepted): the products use the endomorphism split.  Identity points are legal (A = 0 gives
 * A' = 0 and C' = C).  proofs_out may be proofs_affine.  n_proofs = 0 is DG16_OK.
 * An r1 or r2 that is zero or >= r: with host pointers DG16_ERR_BAD_ARG, checked before any work; with
 * DG16_F_DEVICE_PTRS the kernel checks, writes an ALL-ZERO proof (three identities, which no verifier accepts for a
 * real key) at that index, and the call returns DG16_OK. */
int dg16_groth16_rerandomize(dg16_ctx *ctx, const dg16_vk *vk, const void *proofs_affine, size_t n_proofs,
                             const void *r1_r2, unsigned flags, void *proofs_out, int channel);

/* ---- Phase 2 of the key ceremony: one scalar times n points, a contribution to delta, and its verification ----------
 * dg16_groth16_setup_srs ends at a key with gamma = delta = 1, which must not be deployed: with delta public the
 * l_query and h_query terms are unprotected.  The reference's recipe for a production key
 * (scripts/phase2_proving_key.sh:16-20) is `groth16 setup` -> `zkey contribute` -> `zkey verify`; these are the last two.
 *
 * dg16_points_scale: out[i] = k * points[i], i < n, ONE scalar for all points.  Layouts, curves and groups are those of
 * dg16_points_mul.  scalar: 32 bytes, a canonical little-endian integer below 2^255 (DG16_ERR_BAD_ARG otherwise).  The
 * scalar is split and recoded on the host once -- a width-5 non-adjacent form per part -- and every lane walks the same
 * digits: a zero digit is a doubling and nothing else, the table holds the odd multiples only.  The
 * split rule is dg16_msm's: the endomorphism split for the cofactor-one group (BN254 G1) always, for the others only
 * with in_subgroup = 1, the caller's word that every point has order r; without it the call is correct for ANY point of
 * the curve.  out may be the same buffer as points, not a partial overlap.  n = 0 is DG16_OK; a null pointer with n > 0,
 * n >= 2^30 or a group other than 1 or 2 is DG16_ERR_BAD_ARG, an unknown curve DG16_ERR_BAD_CURVE.  points, scalar, out:
 * host pointers only.  Synchronous; runs on channel 0.  A large n runs in slices of the size
 * dg16_ctx_set_points_mul_slice sets (default 2^16 points); the device copy of a slice, its table and its accumulators
 * come from channel 0's workspace, the buffers dg16_points_mul uses at the same sizes (DG16_ERR_OOM leaves the context
 * usable). */
int dg16_points_scale(dg16_ctx *ctx, int curve, int group, const void *points_affine, const void *scalar /* 32 bytes */,
                      size_t n, void *out_affine, int in_subgroup);

/* One phase-2 contribution (snarkjs `zkey contribute`, the arithmetic of it): with d = delta,
 *   l_out = d^-1 * l_query (n_l points)      h_out = d^-1 * h_query (n_h points)
 *   fixed_out = fixed_points (the dg16_pk_create layout alpha_g1 | beta_g1 | delta_g1 | beta_g2 | delta_g2) with
 *               delta_g1 and delta_g2 multiplied by d and the other three copied.
 * Every other array of the key is unchanged by a contribution.  d^-1 is taken mod r on the host; both arrays go through
 * dg16_points_scale's path with in_subgroup = 1: THE CALLER VOUCHES FOR THE KEY (every point on its curve and of order
 * r), as for dg16_groth16_rerandomize.  Identity entries (zero bytes; a LibsnarkReduction key's last h_query entry is
 * one) stay identities.  l_out, h_out, fixed_out may be the inputs.  n_l = 0 and n_h = 0 are legal.  All three curves; no
 * pairing is involved.
 * THE RANDOMNESS IS THE CALLER'S, as everywhere in this library: delta is 32 bytes, canonical, in [1, r) -- uniform, and
 * forgotten by the caller afterwards; the call draws nothing and keeps nothing.  delta = 0 or delta >= r is
 * DG16_ERR_BAD_ARG, checked before any work, as is a NULL pointer (l_query / h_query may be NULL with a zero count); an
 * unknown curve is DG16_ERR_BAD_CURVE.  Host pointers only.  Synchronous; runs on channel 0. */
int dg16_groth16_contribute(dg16_ctx *ctx, int curve, size_t n_l, size_t n_h, const void *l_query, const void *h_query,
                            const void *fixed_points, const void *delta /* 32 bytes, canonical, in [1, r) */,
                            void *l_out, void *h_out, void *fixed_out);

/* Bits of dg16_phase2_report::failed. */
#define DG16_P2_BAD_POINT 1u   /* a point with an unreduced coordinate, off its curve or outside the subgroup */
#define DG16_P2_IDENTITY 2u    /* delta_g1 or delta_g2 of either key is O */
#define DG16_P2_CHANGED 4u     /* an array a contribution does not touch differs between the keys */
#define DG16_P2_DELTA 8u       /* delta_g1 and delta_g2 were not multiplied by the same d */
#define DG16_P2_L 16u          /* l_query was not divided by that d */
#define DG16_P2_H 32u          /* h_query was not divided by that d */
typedef struct dg16_groth16_key {   /* the eight outputs of dg16_groth16_setup, host pointers */
  const void *a_query, *b_g1_query, *b_g2_query, *h_query, *l_query, *fixed_points, *gamma_g2, *gamma_abc_g1;
} dg16_groth16_key;
typedef struct dg16_phase2_report {
  uint32_t failed;        /* 0 = accepted; bits above */
  uint32_t bad_array;     /* with DG16_P2_BAD_POINT: 0 l_query, 1 h_query, 2 delta_g1, 3 delta_g2 of `before`, 4 .. 7 of `after` */
  uint64_t bad_index;     /* the smallest bad index in that array (the first array that has one) */
  uint64_t n_bad_points;  /* over all eight arrays */
} dg16_phase2_report;
/* Is `after` the key `before` with delta replaced by d * delta for SOME d (snarkjs `zkey verify`, without the contribution chain)?  BN254
 * and BLS12-381.  Both keys have the sizes of dg16_groth16_setup: l_query num_vars - num_inputs points, h_query
 * domain_size.  With D1, D2, L, H the delta_g1, delta_g2, l_query, h_query of `before`, primes for `after`, and
 * coefficients rho_k, a bit of report->failed is CLEAR when:
 *   DG16_P2_BAD_POINT  dg16_points_check(subgroup = 1) finds nothing in L, H, D1, D2, L', H', D1', D2'
 *   DG16_P2_IDENTITY   none of D1, D2, D1', D2' is the identity
 *   DG16_P2_CHANGED    a_query, b_g1_query, b_g2_query, gamma_g2, gamma_abc_g1, and alpha_g1, beta_g1, beta_g2 of
 *                      fixed_points, are byte-equal in both keys (a host memcmp)
 *   DG16_P2_DELTA      e(D1', D2) = e(D1, D2')
 *   DG16_P2_L          e(sum_k rho_k L'_k, D2') = e(sum_k rho_k L_k, D2)      (skipped for an empty l_query)
 *   DG16_P2_H          the same with H over domain_size terms
 * Membership runs first: with DG16_P2_BAD_POINT or DG16_P2_IDENTITY set the three pairing checks are skipped and
 * their bits stay clear (the sums use the endomorphism split and the pairing assumes subgroup points).  The four sums
 * are the library's MSM on the device; the three equalities are two Miller loops and one final exponentiation each, on
 * the host.  The relation is transitive in d: a key any number of contributions after `before` is accepted.
 * report->failed != 0 comes with DG16_OK: a rejected key is a result, not an error.
 * THE COEFFICIENTS ARE THE CALLER'S, as in dg16_groth16_verify_aggregate: coeffs = max(num_vars - num_inputs,
 * domain_size) x 16 bytes, each a little-endian unsigned 128-bit integer; each sum uses the first of them.  The
 * contract: the rho_k are independent and uniform in [1, 2^128), and they are chosen AFTER both keys are fixed.  A key
 * that fails an equation is then accepted with probability about 2^-128 per equation.  A zero coefficient is
 * DG16_ERR_BAD_ARG, checked before any work.
 * NOT CHECKED: a contributor's proof of knowledge of d and the hash chain of a ceremony transcript (snarkjs' `zkey
 * verify` with the contribution chain) -- they need a hash-to-curve this library does not have.
 * before, after, coeffs, report and every array: host pointers only.  Synchronous; runs on channel 0; the device copies
 * are temporary (DG16_ERR_OOM leaves the context usable).  num_inputs = 0, num_inputs > num_vars, domain_size = 0, sizes
 * of 2^28 or more, or a NULL pointer (l_query may be NULL when it is empty): DG16_ERR_BAD_ARG.  DG16_BLS12_377 (no pairing
 * here): DG16_ERR_UNSUPPORTED.  An unknown curve: DG16_ERR_BAD_CURVE. */
int dg16_groth16_verify_contribution(dg16_ctx *ctx, int curve, size_t num_inputs, size_t num_vars, size_t domain_size,
                                     const dg16_groth16_key *before, const dg16_groth16_key *after,
                                     const void *coeffs /* max(num_vars - num_inputs, domain_size) x 16 bytes */,
                                     dg16_phase2_report *report);

/* ---- Phase 1 of the key ceremony: a series of scalars times n points, a contribution to powers of tau, its check -----
 * dg16_srs_verify checks a transcript and dg16_srs_prepare turns it into a reference string; these three make a
 * contribution to one (snarkjs `powersoftau contribute`) and decide whether one transcript is a contribution to another
 * (the contribution part of `powersoftau verify`).
 *
 * dg16_points_mul_series: out[i] = (first * ratio^(start + i) mod r) * points[i], i < n.  Layouts, curves and groups are
 * those of dg16_points_mul, all six groups.  first, ratio: 32 bytes each, canonical little-endian integers in [0, r)
 * (anything else is DG16_ERR_BAD_ARG, checked before any work).  ratio = 0 is legal: the term of exponent 0 is `first`
 * and every other term is 0, the identity; first = 0 gives all identities; ratio = 1 gives what dg16_points_scale gives
 * for `first`, byte for byte.  start + n must not exceed 2^64 - 1 (DG16_ERR_BAD_ARG).  The scalars are never on the host:
 * a kernel writes each slice's terms, in Montgomery form, into the buffer dg16_points_mul's kernel reads -- a lane raises
 * ratio to the first of its 16 consecutive exponents, a full 64-bit number, and multiplies on.
 * in_subgroup has the meaning it has for dg16_points_scale: without it the call is correct for ANY point of the curve.
 * out may be the same buffer as points, not a partial overlap.  n = 0 is DG16_OK; a null pointer with n > 0, n >= 2^30 or
 * a group other than 1 or 2 is DG16_ERR_BAD_ARG, an unknown curve DG16_ERR_BAD_CURVE.  points, first, ratio, out: host
 * pointers only.  Synchronous; runs on channel 0.  A large n runs in slices of the size dg16_ctx_set_points_mul_slice
 * sets (default 2^16 points); the device copy of a slice and its scalars come from channel 0's workspace (DG16_ERR_OOM
 * leaves the context usable). */
int dg16_points_mul_series(dg16_ctx *ctx, int curve, int group, const void *points_affine, size_t n,
                           const void *first /* 32 bytes */, const void *ratio /* 32 bytes */, uint64_t start,
                           void *out_affine, int in_subgroup);

/* Where dg16_srs_contribute writes: caller-allocated host buffers with the sizes of dg16_srs_powers. */
typedef struct dg16_srs_powers_out {
  void *tau_g1, *tau_g2, *alpha_tau_g1, *beta_tau_g1, *beta_g2;
} dg16_srs_powers_out;
/* One phase-1 contribution (snarkjs `powersoftau contribute`, the arithmetic of it).  With m = 2^log_m:
 *   tau_g1'[j] = tau^j tau_g1[j] (j < 2m - 1)            tau_g2'[j] = tau^j tau_g2[j] (j < m)
 *   alpha_tau_g1'[j] = alpha tau^j alpha_tau_g1[j]       beta_tau_g1'[j] = beta tau^j beta_tau_g1[j] (j < m)
 *   beta_g2' = beta beta_g2
 * The four arrays are four runs of dg16_points_mul_series' path with in_subgroup = 1, beta_g2 goes through
 * dg16_points_scale's: THE CALLER VOUCHES FOR THE TRANSCRIPT (every point on its curve and of order r), as for
 * dg16_groth16_contribute -- run dg16_srs_verify first.  Every output array may be its input array.  All three curves;
 * no pairing is involved.  The log_m limits are dg16_srs_prepare's.
 * secrets: tau | alpha | beta, 3 x 32 bytes, canonical, each in [1, r).  THE RANDOMNESS IS THE CALLER'S, and so is the
 * challenge: the library draws nothing, hashes nothing and keeps nothing.
 * The key is a proof of knowledge per secret.  blinds: s_tau | s_alpha | s_beta in the same form; challenge_g2: SP_tau |
 * SP_alpha | SP_beta, three G2 affine points (how they are derived from the previous transcript is the caller's
 * protocol; snarkjs hashes a challenge to G2).  With G = powers->tau_g1[0] and x over tau, alpha, beta, key_out holds
 * s_x G | s_x x G | x SP_x for each x in that order: 6 G1 and 3 G2 affine points, each x's two G1 points followed by its
 * G2 point.  blinds, challenge_g2 and key_out are all three NULL (no key is made) or none of them is; a partial triple is
 * DG16_ERR_BAD_ARG.  A secret or blind that is zero or not below r is DG16_ERR_BAD_ARG, checked before any work, as is a
 * NULL pointer; an unknown curve is DG16_ERR_BAD_CURVE.  Host pointers only.  Synchronous; runs on channel 0.
 * Not here: the contribution hashes and the hash-to-G2 of a challenge, a .ptau reader, device-pointer forms. */
int dg16_srs_contribute(dg16_ctx *ctx, int curve, unsigned log_m, const dg16_srs_powers *powers,
                        const void *secrets /* tau | alpha | beta, 3 x 32 bytes */,
                        const void *blinds /* s_tau | s_alpha | s_beta; NULL: no key is made */,
                        const void *challenge_g2 /* SP_tau | SP_alpha | SP_beta; NULL with blinds */,
                        const dg16_srs_powers_out *out, void *key_out /* NULL with blinds */);

/* Bits of dg16_srs_contribution_report::failed. */
#define DG16_P1_AFTER 1u          /* `after` is not a transcript: report->after says why */
#define DG16_P1_BAD_POINT 2u      /* a key point, a challenge point or a head of `before` is unreduced, off its curve or outside the subgroup */
#define DG16_P1_IDENTITY 4u       /* one of those points is O */
#define DG16_P1_BASE 8u           /* tau_g1[0] or tau_g2[0] differs between the transcripts */
#define DG16_P1_KEY_TAU 16u       /* the tau key is not a proof of knowledge under SP_tau */
#define DG16_P1_KEY_ALPHA 32u     /* the alpha key, SP_alpha */
#define DG16_P1_KEY_BETA 64u      /* the beta key, SP_beta */
#define DG16_P1_LINK_TAU_G1 128u  /* tau_g1[1] did not move by the tau of the key */
#define DG16_P1_LINK_TAU_G2 256u  /* tau_g2[1] did not */
#define DG16_P1_LINK_ALPHA 512u   /* alpha_tau_g1[0] did not move by the alpha of the key */
#define DG16_P1_LINK_BETA 1024u   /* beta_tau_g1[0] did not move by the beta of the key */
#define DG16_P1_LINK_BETA_G2 2048u /* beta_g2 did not */
typedef struct dg16_srs_contribution_report {
  uint32_t failed;        /* 0 = accepted; bits above */
  uint32_t n_bad_points;  /* with DG16_P1_BAD_POINT: how many of the 19 points (9 key, 3 challenge, 7 heads) */
  dg16_srs_report after;  /* what dg16_srs_verify says about `after` */
} dg16_srs_contribution_report;
/* Is `after` a contribution to `before` by whoever holds this key (the contribution part of snarkjs `powersoftau
 * verify`)?  BN254 and BLS12-381.  key: the 9 points dg16_srs_contribute writes; challenge_g2: the three points the
 * contributor was given.  The call reads `after` in full (dg16_srs_verify's checks, same coeffs) and of `before` only
 * the heads T0 = tau_g1[0], T1 = tau_g1[1], U0 = tau_g2[0], U1 = tau_g2[1], A0 = alpha_tau_g1[0], B0 = beta_tau_g1[0]
 * and beta_g2 (the other entries of `before` may be absent: each array needs its first two, or its first one, point).
 * Write R(a, b; c, d) for e(a, d) = e(b, c), and key.x = (g1_s, g1_sx, g2_spx).  A bit of report->failed is CLEAR when:
 *   DG16_P1_AFTER         report->after.failed == 0
 *   DG16_P1_BAD_POINT     dg16_points_check(subgroup = 1) finds nothing among the 9 key points, the 3 challenge points
 *                         and the 7 heads of `before`
 *   DG16_P1_IDENTITY      none of those 19 points is the identity
 *   DG16_P1_BASE          tau_g1[0] and tau_g2[0] of `after` equal those of `before`, byte for byte
 *   DG16_P1_KEY_TAU       R(key.tau.g1_s, key.tau.g1_sx; SP_tau, key.tau.g2_spx)        (KEY_ALPHA, KEY_BETA alike)
 *   DG16_P1_LINK_TAU_G1   R(before.T1, after.T1; SP_tau, key.tau.g2_spx)
 *   DG16_P1_LINK_TAU_G2   R(key.tau.g1_s, key.tau.g1_sx; before.U1, after.U1)
 *   DG16_P1_LINK_ALPHA    R(before.A0, after.A0; SP_alpha, key.alpha.g2_spx)
 *   DG16_P1_LINK_BETA     R(before.B0, after.B0; SP_beta, key.beta.g2_spx)
 *   DG16_P1_LINK_BETA_G2  R(key.beta.g1_s, key.beta.g1_sx; before.beta_g2, after.beta_g2)
 * The eight equalities are two Miller loops and one final exponentiation each, on the host.  They are skipped, and their
 * bits stay clear, with DG16_P1_BAD_POINT or DG16_P1_IDENTITY set here or DG16_SRS_BAD_POINT or DG16_SRS_IDENTITY set in
 * report->after: the pairing assumes subgroup points (dg16_srs_verify's rule).  Together with a clean report->after the
 * links at the heads fix every entry: `after` is then a progression in ONE tau', alpha', beta', and the heads say which.
 * report->failed != 0 comes with DG16_OK: a bad contribution is a result, not an error.
 * coeffs: (2m - 2) x 16 bytes under dg16_srs_verify's contract; a zero coefficient is DG16_ERR_BAD_ARG, checked before
 * any work, as are a NULL pointer and a log_m outside dg16_srs_verify's range.  DG16_BLS12_377 (no pairing here):
 * DG16_ERR_UNSUPPORTED.  An unknown curve: DG16_ERR_BAD_CURVE.  Host pointers only.  Synchronous; runs on channel 0.
 * NOT CHECKED: that challenge_g2 is the hash of the previous transcript -- the caller's protocol. */
int dg16_srs_verify_contribution(dg16_ctx *ctx, int curve, unsigned log_m, const dg16_srs_powers *before,
                                 const dg16_srs_powers *after, const void *key /* 3 x (G1 | G1 | G2) */,
                                 const void *challenge_g2 /* 3 G2 points */,
                                 const void *coeffs /* (2m - 2) x 16 bytes, as dg16_srs_verify */,
                                 dg16_srs_contribution_report *report);

/* Duration in milliseconds of the dominant kernel(s) of the most recent call on `channel`
 * (HIP events recorded on the channel's stream); 0 if none.  which: 0 = whole call,
 * 1 = bucket accumulation (MSM) / butterfly passes (NTT); 2 = NOT a duration: the shader clock in MHz the chip held
 * under the bucket accumulation of `which = 1` (the kernel measures it: s_memtime against the 100-MHz s_memrealtime,
 * summed over its workgroups), 0 if that call had none. */
int dg16_last_kernel_ms(dg16_ctx *ctx, int channel, int which, float *ms);

#ifdef __cplusplus
}
#endif
#endif /* DG16_H */
