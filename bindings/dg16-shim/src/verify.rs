//! Batched verification: `Groth16::<E>::verify_proof(&pvk, &proof, &inputs)` for many proofs of one key in ONE call of
//! `dg16_groth16_verify_batch` (the reference verifies after every proof: groth16/examples/sha256.rs:228-254, the verify
//! endpoint of mpc-api/src/main.rs).  `PreparedVk::new` is `prepare_verifying_key`: it validates the key and builds its
//! Miller-loop tables once.  BN254 and BLS12-381.
//!
//! Like the rest of this crate: never compiled here (bindings/README.md) -- source for a maintainer's box with cargo.
use crate::pack::{pack_affine, scalars_as_bytes, FieldBytes};
use crate::{check, sys, Dg16Config, Dg16Error, CTX};
use ark_ec::pairing::Pairing;
use ark_ec::short_weierstrass::Affine;
use ark_groth16::{Proof, VerifyingKey};

pub struct PreparedVk {
    h: *mut sys::Dg16Vk,
    n_public: usize,
}
unsafe impl Send for PreparedVk {}
unsafe impl Sync for PreparedVk {}
impl Drop for PreparedVk {
    fn drop(&mut self) {
        unsafe { sys::dg16_vk_destroy(self.h) }
    }
}

impl PreparedVk {
    pub fn new<E, P1, P2>(vk: &VerifyingKey<E>) -> Result<Self, Dg16Error>
    where
        E: Pairing<G1Affine = Affine<P1>, G2Affine = Affine<P2>>,
        P1: Dg16Config<ScalarField = E::ScalarField>,
        P2: Dg16Config<ScalarField = E::ScalarField>,
        P1::BaseField: FieldBytes,
        P2::BaseField: FieldBytes,
    {
        let (alpha, ic) = (pack_affine(&[vk.alpha_g1]), pack_affine(&vk.gamma_abc_g1));
        let (beta, gamma, delta) = (pack_affine(&[vk.beta_g2]), pack_affine(&[vk.gamma_g2]), pack_affine(&[vk.delta_g2]));
        let mut h = core::ptr::null_mut();
        check(unsafe {
            sys::dg16_vk_create(
                CTX.0, P1::CURVE, alpha.as_ptr().cast(), beta.as_ptr().cast(), gamma.as_ptr().cast(),
                delta.as_ptr().cast(), ic.as_ptr().cast(), vk.gamma_abc_g1.len(), 0, &mut h,
            )
        })?;
        Ok(PreparedVk { h, n_public: vk.gamma_abc_g1.len() - 1 })
    }
}

/// One verdict per proof; `inputs[i]` are proof i's public inputs (without the constant 1).  A malformed proof or input
/// is `false` for that proof, never an error of the call.
pub fn verify_batch<E, P1, P2>(pvk: &PreparedVk, inputs: &[Vec<E::ScalarField>], proofs: &[Proof<E>])
    -> Result<Vec<bool>, Dg16Error>
where
    E: Pairing<G1Affine = Affine<P1>, G2Affine = Affine<P2>>,
    P1: Dg16Config<ScalarField = E::ScalarField>,
    P2: Dg16Config<ScalarField = E::ScalarField>,
    P1::BaseField: FieldBytes,
    P2::BaseField: FieldBytes,
{
    if inputs.len() != proofs.len() {
        return Err(Dg16Error::LengthMismatch(inputs.len().min(proofs.len())));
    }
    let mut x = Vec::with_capacity(proofs.len() * pvk.n_public * 32);
    for row in inputs {
        if row.len() != pvk.n_public {
            return Err(Dg16Error::LengthMismatch(row.len().min(pvk.n_public)));
        }
        x.extend_from_slice(scalars_as_bytes(row));
    }
    let mut p = Vec::new();
    for pr in proofs {
        p.extend(pack_affine(&[pr.a]));
        p.extend(pack_affine(&[pr.b]));
        p.extend(pack_affine(&[pr.c]));
    }
    let mut verdict = vec![0u8; proofs.len()];
    check(unsafe {
        sys::dg16_groth16_verify_batch(
            CTX.0, pvk.h, x.as_ptr().cast(), pvk.n_public, p.as_ptr().cast(), proofs.len(),
            sys::DG16_F_SCALARS_MONT, verdict.as_mut_ptr(), 0,
        )
    })?;
    Ok(verdict.into_iter().map(|v| v == 1).collect())
}

/// One verdict for the whole batch (`dg16_groth16_verify_aggregate`): `Groth16::verify_proof` in a loop becomes one
/// call.  `coeffs[i]` is proof i's 128-bit coefficient: the caller draws them independently and uniformly from
/// [1, 2^128) AFTER the proofs are fixed (the library draws no randomness); a batch with an invalid proof is then
/// accepted with probability about 2^-128, and equal or predictable coefficients void that.  A zero coefficient, a
/// malformed proof or input is `false`, never an error of the call; on `false`, [`verify_batch`] says which proofs are bad.
pub fn verify_aggregate<E, P1, P2>(pvk: &PreparedVk, inputs: &[Vec<E::ScalarField>], proofs: &[Proof<E>],
                                   coeffs: &[u128]) -> Result<bool, Dg16Error>
where
    E: Pairing<G1Affine = Affine<P1>, G2Affine = Affine<P2>>,
    P1: Dg16Config<ScalarField = E::ScalarField>,
    P2: Dg16Config<ScalarField = E::ScalarField>,
    P1::BaseField: FieldBytes,
    P2::BaseField: FieldBytes,
{
    if inputs.len() != proofs.len() || coeffs.len() != proofs.len() {
        return Err(Dg16Error::LengthMismatch(inputs.len().min(proofs.len()).min(coeffs.len())));
    }
    let mut x = Vec::with_capacity(proofs.len() * pvk.n_public * 32);
    for row in inputs {
        if row.len() != pvk.n_public {
            return Err(Dg16Error::LengthMismatch(row.len().min(pvk.n_public)));
        }
        x.extend_from_slice(scalars_as_bytes(row));
    }
    let mut p = Vec::new();
    for pr in proofs {
        p.extend(pack_affine(&[pr.a]));
        p.extend(pack_affine(&[pr.b]));
        p.extend(pack_affine(&[pr.c]));
    }
    let mut rho = Vec::with_capacity(coeffs.len() * 16);
    for c in coeffs {
        rho.extend_from_slice(&c.to_le_bytes());
    }
    let mut accepted = 0u8;
    check(unsafe {
        sys::dg16_groth16_verify_aggregate(
            CTX.0, pvk.h, x.as_ptr().cast(), pvk.n_public, p.as_ptr().cast(), proofs.len(), rho.as_ptr().cast(),
            sys::DG16_F_SCALARS_MONT, &mut accepted, 0,
        )
    })?;
    Ok(accepted == 1)
}

/// `Groth16::<E>::rerandomize_proof(vk, proof, rng)` for a batch in ONE call of `dg16_groth16_rerandomize`:
/// `(A, B, C) -> (r1^-1 A, r1 B + r1 r2 delta_g2, C + r2 A)` with `rerandomizers[i] = (r1, r2)`, both nonzero, drawn by
/// the caller independently and uniformly per proof (the library draws no randomness; a zero is `Err`).  The proofs are
/// not verified here and must hold subgroup points -- true of anything [`verify_batch`] accepted; the new proof
/// verifies for the same public inputs exactly when the old one does.
pub fn rerandomize_proofs<E, P1, P2>(pvk: &PreparedVk, proofs: &[Proof<E>],
                                     rerandomizers: &[(E::ScalarField, E::ScalarField)])
                                     -> Result<Vec<Proof<E>>, Dg16Error>
where
    E: Pairing<G1Affine = Affine<P1>, G2Affine = Affine<P2>>,
    P1: Dg16Config<ScalarField = E::ScalarField>,
    P2: Dg16Config<ScalarField = E::ScalarField>,
    P1::BaseField: FieldBytes,
    P2::BaseField: FieldBytes,
{
    if rerandomizers.len() != proofs.len() {
        return Err(Dg16Error::LengthMismatch(rerandomizers.len().min(proofs.len())));
    }
    let mut p = Vec::new();
    for pr in proofs {
        p.extend(pack_affine(&[pr.a]));
        p.extend(pack_affine(&[pr.b]));
        p.extend(pack_affine(&[pr.c]));
    }
    let mut r = Vec::with_capacity(proofs.len() * 64);
    for (r1, r2) in rerandomizers {
        r.extend_from_slice(scalars_as_bytes(&[*r1, *r2]));
    }
    let mut out = vec![0u8; p.len()];
    check(unsafe {
        sys::dg16_groth16_rerandomize(
            CTX.0, pvk.h, p.as_ptr().cast(), proofs.len(), r.as_ptr().cast(), sys::DG16_F_SCALARS_MONT,
            out.as_mut_ptr().cast(), 0,
        )
    })?;
    let g1 = 2 * <P1::BaseField as FieldBytes>::BYTES;
    let g2 = 2 * <P2::BaseField as FieldBytes>::BYTES;
    Ok(out
        .chunks_exact(2 * g1 + g2)
        .map(|c| Proof {
            a: crate::setup::unpack_affine::<P1>(&c[..g1])[0],
            b: crate::setup::unpack_affine::<P2>(&c[g1..g1 + g2])[0],
            c: crate::setup::unpack_affine::<P1>(&c[g1 + g2..])[0],
        })
        .collect())
}
