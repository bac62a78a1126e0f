//! Key generation: `Groth16::<E, CircomReduction>::circuit_specific_setup(circuit, rng)` (groth16/examples/sha256.rs:137,
//! million.rs:137, d_sha256.rs:138, mpc-api/src/main.rs:151) from the point where the constraint matrices exist, as ONE
//! call of `dg16_groth16_setup` (which runs `FixedBase::msm`'s job through `dg16_fixed_base_mul`'s kernels).
//!
//! Like the rest of this crate: never compiled here (bindings/README.md) -- source for a maintainer's box with cargo.
use crate::pack::{pack_affine, scalars_as_bytes, FieldBytes};
use crate::prove::Csr;
use crate::{check, sys, Dg16Config, Dg16Error, CTX};
use ark_ec::pairing::Pairing;
use ark_ec::short_weierstrass::{Affine, SWCurveConfig};
use ark_ec::AffineRepr;
use ark_ff::{BigInteger, PrimeField, UniformRand, Zero};
use ark_groth16::{ProvingKey, VerifyingKey};
use ark_relations::r1cs::ConstraintMatrices;
use ark_std::rand::RngCore;

/// x || y Montgomery limbs with the identity as zeros (the library's output layout) -> `Affine<P>`.
pub(crate) fn unpack_affine<P: SWCurveConfig>(buf: &[u8]) -> Vec<Affine<P>>
where
    P::BaseField: FieldBytes,
{
    let fe = <P::BaseField as FieldBytes>::BYTES;
    buf.chunks_exact(2 * fe)
        .map(|c| {
            if c.iter().all(|b| *b == 0) {
                Affine::<P>::zero()
            } else {
                Affine::<P>::new_unchecked(<P::BaseField>::read_mont(&c[..fe]), <P::BaseField>::read_mont(&c[fe..]))
            }
        })
        .collect()
}

/// `generate_random_parameters_with_reduction` with the library doing everything after the trapdoor is drawn.
/// `num_inputs` counts the constant 1 (`matrices.num_instance_variables`).
pub fn circuit_specific_setup<E, P1, P2, R: RngCore>(m: &ConstraintMatrices<E::ScalarField>, rng: &mut R)
    -> Result<ProvingKey<E>, Dg16Error>
where
    E: Pairing<G1Affine = Affine<P1>, G2Affine = Affine<P2>>,
    P1: Dg16Config<ScalarField = E::ScalarField>,
    P2: Dg16Config<ScalarField = E::ScalarField>,
    P1::BaseField: FieldBytes,
    P2::BaseField: FieldBytes,
{
    let (nc, ni) = (m.num_constraints, m.num_instance_variables);
    let nv = ni + m.num_witness_variables;
    let log_m = (nc + ni).next_power_of_two().trailing_zeros();
    let domain = 1usize << log_m;
    // alpha | beta | gamma | delta | tau, canonical little-endian (the caller owns the randomness)
    let mut td = Vec::with_capacity(5 * 32);
    for _ in 0..5 {
        let mut x = E::ScalarField::rand(rng);
        while x.is_zero() {
            x = E::ScalarField::rand(rng);
        }
        td.extend(x.into_bigint().to_bytes_le());
    }
    let gens = {
        let mut g = pack_affine(&[E::G1Affine::generator()]);
        g.extend(pack_affine(&[E::G2Affine::generator()]));
        g
    };
    let (ca, cb, cc) = (Csr::from_rows(&m.a), Csr::from_rows(&m.b), Csr::from_rows(&m.c));
    let (f1, f2) = (2 * <P1::BaseField as FieldBytes>::BYTES, 2 * <P2::BaseField as FieldBytes>::BYTES);
    let (mut a, mut b1, mut b2) = (vec![0u8; nv * f1], vec![0u8; nv * f1], vec![0u8; nv * f2]);
    let (mut h, mut l) = (vec![0u8; domain * f1], vec![0u8; (nv - ni) * f1]);
    let (mut fixed, mut gamma_g2, mut ic) = (vec![0u8; 3 * f1 + 2 * f2], vec![0u8; f2], vec![0u8; ni * f1]);
    check(unsafe {
        sys::dg16_groth16_setup(
            CTX.0, P1::CURVE, nc, ni, nv, log_m,
            ca.row_ptr.as_ptr(), ca.col.as_ptr(), scalars_as_bytes(&ca.coeff).as_ptr().cast(),
            cb.row_ptr.as_ptr(), cb.col.as_ptr(), scalars_as_bytes(&cb.coeff).as_ptr().cast(),
            cc.row_ptr.as_ptr(), cc.col.as_ptr(), scalars_as_bytes(&cc.coeff).as_ptr().cast(),
            td.as_ptr().cast(), gens.as_ptr().cast(), a.as_mut_ptr().cast(), b1.as_mut_ptr().cast(),
            b2.as_mut_ptr().cast(), h.as_mut_ptr().cast(), l.as_mut_ptr().cast(), fixed.as_mut_ptr().cast(),
            gamma_g2.as_mut_ptr().cast(), ic.as_mut_ptr().cast(), 0,
        )
    })?;
    let g1_fixed = unpack_affine::<P1>(&fixed[..3 * f1]);
    let g2_fixed = unpack_affine::<P2>(&fixed[3 * f1..]);
    let vk = VerifyingKey::<E> {
        alpha_g1: g1_fixed[0],
        beta_g2: g2_fixed[0],
        gamma_g2: unpack_affine::<P2>(&gamma_g2)[0],
        delta_g2: g2_fixed[1],
        gamma_abc_g1: unpack_affine::<P1>(&ic),
    };
    Ok(ProvingKey::<E> {
        vk,
        beta_g1: g1_fixed[1],
        delta_g1: g1_fixed[2],
        a_query: unpack_affine::<P1>(&a),
        b_g1_query: unpack_affine::<P1>(&b1),
        b_g2_query: unpack_affine::<P2>(&b2),
        h_query: unpack_affine::<P1>(&h),
        l_query: unpack_affine::<P1>(&l),
    })
}

/// A structured reference string for the domain of size `lag_g1.len()`: the Lagrange-basis points of a powers-of-tau
/// ceremony (include/dg16.h names the sections of a prepared `.ptau` file).  The caller vouches that every point is on
/// its curve and of order r.
pub struct Srs<E: Pairing> {
    pub lag_g1: Vec<E::G1Affine>,
    pub lag_g2: Vec<E::G2Affine>,
    pub alpha_lag_g1: Vec<E::G1Affine>,
    pub beta_lag_g1: Vec<E::G1Affine>,
    /// the h basis of the reduction the key will be proved with, delta = 1 (copied to `h_query`)
    pub h_g1: Vec<E::G1Affine>,
    pub alpha_g1: E::G1Affine,
    pub beta_g1: E::G1Affine,
    pub g1: E::G1Affine,
    pub beta_g2: E::G2Affine,
    pub g2: E::G2Affine,
}

/// The monomial powers a powers-of-tau ceremony publishes for a domain of size m = `tau_g2.len()` (a power of two):
/// `tau_g1` holds 2m - 1 points, the other arrays m.  The caller vouches that every point is of order r.
pub struct SrsPowers<E: Pairing> {
    pub tau_g1: Vec<E::G1Affine>,
    pub tau_g2: Vec<E::G2Affine>,
    pub alpha_tau_g1: Vec<E::G1Affine>,
    pub beta_tau_g1: Vec<E::G1Affine>,
    pub beta_g2: E::G2Affine,
}

/// From ceremony output to the reference string `setup_from_srs` takes (`dg16_srs_prepare`; snarkjs' `powersoftau
/// prepare phase2`): four inverse group FFTs of size m and the h basis of the chosen reduction (`libsnark` false:
/// CircomReduction).
pub fn srs_prepare<E, P1, P2>(powers: &SrsPowers<E>, libsnark: bool) -> Result<Srs<E>, Dg16Error>
where
    E: Pairing<G1Affine = Affine<P1>, G2Affine = Affine<P2>>,
    P1: Dg16Config<ScalarField = E::ScalarField>,
    P2: Dg16Config<ScalarField = E::ScalarField>,
    P1::BaseField: FieldBytes,
    P2::BaseField: FieldBytes,
{
    let m = powers.tau_g2.len();
    if !m.is_power_of_two() || powers.tau_g1.len() != 2 * m - 1 || powers.alpha_tau_g1.len() != m
        || powers.beta_tau_g1.len() != m
    {
        return Err(Dg16Error::Status(sys::DG16_ERR_BAD_ARG, "powers: tau_g1 holds 2m - 1 points, the others m = 2^k".into()));
    }
    let log_m = m.trailing_zeros();
    let (t1, t2) = (pack_affine(&powers.tau_g1), pack_affine(&powers.tau_g2));
    let (at, bt, b2) = (pack_affine(&powers.alpha_tau_g1), pack_affine(&powers.beta_tau_g1), pack_affine(&[powers.beta_g2]));
    let raw_in = sys::Dg16SrsPowers {
        tau_g1: t1.as_ptr().cast(),
        tau_g2: t2.as_ptr().cast(),
        alpha_tau_g1: at.as_ptr().cast(),
        beta_tau_g1: bt.as_ptr().cast(),
        beta_g2: b2.as_ptr().cast(),
    };
    let (f1, f2) = (2 * <P1::BaseField as FieldBytes>::BYTES, 2 * <P2::BaseField as FieldBytes>::BYTES);
    let (mut l1, mut l2) = (vec![0u8; m * f1], vec![0u8; m * f2]);
    let (mut al, mut bl, mut hb) = (vec![0u8; m * f1], vec![0u8; m * f1], vec![0u8; m * f1]);
    let mut fixed = vec![0u8; 3 * f1 + 2 * f2];
    let mut raw_out = sys::Dg16SrsPrepared {
        lag_g1: l1.as_mut_ptr().cast(),
        lag_g2: l2.as_mut_ptr().cast(),
        alpha_lag_g1: al.as_mut_ptr().cast(),
        beta_lag_g1: bl.as_mut_ptr().cast(),
        h_g1: hb.as_mut_ptr().cast(),
        fixed: fixed.as_mut_ptr().cast(),
    };
    check(unsafe { sys::dg16_srs_prepare(CTX.0, P1::CURVE, log_m, if libsnark { 1 } else { 0 }, &raw_in, &mut raw_out) })?;
    let g1_fixed = unpack_affine::<P1>(&fixed[..3 * f1]);
    let g2_fixed = unpack_affine::<P2>(&fixed[3 * f1..]);
    Ok(Srs::<E> {
        lag_g1: unpack_affine::<P1>(&l1),
        lag_g2: unpack_affine::<P2>(&l2),
        alpha_lag_g1: unpack_affine::<P1>(&al),
        beta_lag_g1: unpack_affine::<P1>(&bl),
        h_g1: unpack_affine::<P1>(&hb),
        alpha_g1: g1_fixed[0],
        beta_g1: g1_fixed[1],
        g1: g1_fixed[2],
        beta_g2: g2_fixed[0],
        g2: g2_fixed[1],
    })
}

/// Curve and subgroup membership of affine points (`dg16_points_check`): `(bad points, smallest bad index)`, the index
/// being `points.len()` when there is none.  A point is bad when a coordinate is not reduced, when it is off its curve
/// or -- with `subgroup` -- when it is outside the subgroup of order r.  The identity is good.
pub fn points_check<P>(points: &[Affine<P>], subgroup: bool) -> Result<(usize, usize), Dg16Error>
where
    P: Dg16Config,
    P::BaseField: FieldBytes,
{
    let raw = pack_affine(points);
    let (mut n_bad, mut first_bad) = (0usize, 0usize);
    check(unsafe {
        sys::dg16_points_check(CTX.0, P::CURVE, P::GROUP, raw.as_ptr().cast(), points.len(), if subgroup { 1 } else { 0 },
                               &mut n_bad, &mut first_bad)
    })?;
    Ok((n_bad, first_bad))
}

/// Is this a powers-of-tau transcript (`dg16_srs_verify`)?  `coeffs`: 2m - 2 integers in [1, 2^128), independent,
/// uniform and drawn AFTER the transcript was fixed -- the caller's randomness, as for the aggregate verifier.
/// `report.failed == 0` accepts; its bits are `sys::DG16_SRS_*`.  A rejected transcript is `Ok` with the bits set; a
/// zero coefficient is an error.  `srs_prepare` trusts its input: verify first.
pub fn srs_verify<E, P1, P2>(powers: &SrsPowers<E>, coeffs: &[u128]) -> Result<sys::Dg16SrsReport, Dg16Error>
where
    E: Pairing<G1Affine = Affine<P1>, G2Affine = Affine<P2>>,
    P1: Dg16Config<ScalarField = E::ScalarField>,
    P2: Dg16Config<ScalarField = E::ScalarField>,
    P1::BaseField: FieldBytes,
    P2::BaseField: FieldBytes,
{
    let m = powers.tau_g2.len();
    if !m.is_power_of_two() || m < 2 || powers.tau_g1.len() != 2 * m - 1 || powers.alpha_tau_g1.len() != m
        || powers.beta_tau_g1.len() != m || coeffs.len() != 2 * m - 2
    {
        return Err(Dg16Error::Status(sys::DG16_ERR_BAD_ARG,
                                     "powers: tau_g1 holds 2m - 1 points, the others m = 2^k >= 2; 2m - 2 coefficients".into()));
    }
    let log_m = m.trailing_zeros();
    let (t1, t2) = (pack_affine(&powers.tau_g1), pack_affine(&powers.tau_g2));
    let (at, bt, b2) = (pack_affine(&powers.alpha_tau_g1), pack_affine(&powers.beta_tau_g1), pack_affine(&[powers.beta_g2]));
    let raw_in = sys::Dg16SrsPowers {
        tau_g1: t1.as_ptr().cast(),
        tau_g2: t2.as_ptr().cast(),
        alpha_tau_g1: at.as_ptr().cast(),
        beta_tau_g1: bt.as_ptr().cast(),
        beta_g2: b2.as_ptr().cast(),
    };
    let rho: Vec<u8> = coeffs.iter().flat_map(|c| c.to_le_bytes()).collect();
    let mut report = sys::Dg16SrsReport::default();
    check(unsafe { sys::dg16_srs_verify(CTX.0, P1::CURVE, log_m, &raw_in, rho.as_ptr().cast(), &mut report) })?;
    Ok(report)
}

/// `k * P_i` for ONE scalar and all the points (`dg16_points_scale`).  `in_subgroup`: the caller's word that every point
/// has order r, which allows the endomorphism split; without it the call is correct for any point of the curve.
pub fn points_scale<P>(points: &[Affine<P>], k: &P::ScalarField, in_subgroup: bool) -> Result<Vec<Affine<P>>, Dg16Error>
where
    P: Dg16Config,
    P::BaseField: FieldBytes,
{
    let raw = pack_affine(points);
    let mut out = vec![0u8; raw.len()];
    let mut scalar = k.into_bigint().to_bytes_le();
    scalar.resize(32, 0);
    check(unsafe {
        sys::dg16_points_scale(CTX.0, P::CURVE, P::GROUP, raw.as_ptr().cast(), scalar.as_ptr().cast(), points.len(),
                               out.as_mut_ptr().cast(), if in_subgroup { 1 } else { 0 })
    })?;
    Ok(unpack_affine::<P>(&out))
}

fn scalar_bytes<F: PrimeField>(x: &F) -> Vec<u8> {
    let mut b = x.into_bigint().to_bytes_le();
    b.resize(32, 0);
    b
}

/// `(first * ratio^(start + i)) * P_i` (`dg16_points_mul_series`): the scalars are a geometric series made on the
/// device, nothing but `first` and `ratio` is uploaded.  `start + points.len()` must fit 64 bits.  `in_subgroup` as for
/// `points_scale`.
pub fn points_mul_series<P>(points: &[Affine<P>], first: &P::ScalarField, ratio: &P::ScalarField, start: u64,
                            in_subgroup: bool) -> Result<Vec<Affine<P>>, Dg16Error>
where
    P: Dg16Config,
    P::BaseField: FieldBytes,
{
    let raw = pack_affine(points);
    let mut out = vec![0u8; raw.len()];
    let (f, q) = (scalar_bytes(first), scalar_bytes(ratio));
    check(unsafe {
        sys::dg16_points_mul_series(CTX.0, P::CURVE, P::GROUP, raw.as_ptr().cast(), points.len(), f.as_ptr().cast(),
                                    q.as_ptr().cast(), start, out.as_mut_ptr().cast(), if in_subgroup { 1 } else { 0 })
    })?;
    Ok(unpack_affine::<P>(&out))
}

/// The proof of knowledge of one phase-1 contribution: per secret x (tau, alpha, beta) `s_x G`, `s_x x G` and `x SP_x`.
pub struct SrsContributionKey<E: Pairing> {
    pub g1_s: [E::G1Affine; 3],
    pub g1_sx: [E::G1Affine; 3],
    pub g2_spx: [E::G2Affine; 3],
}

fn pack_contribution_key<E, P1, P2>(key: &SrsContributionKey<E>) -> Vec<u8>
where
    E: Pairing<G1Affine = Affine<P1>, G2Affine = Affine<P2>>,
    P1: Dg16Config<ScalarField = E::ScalarField>,
    P2: Dg16Config<ScalarField = E::ScalarField>,
    P1::BaseField: FieldBytes,
    P2::BaseField: FieldBytes,
{
    let mut raw = Vec::new();
    for j in 0..3 {
        raw.extend(pack_affine(&[key.g1_s[j], key.g1_sx[j]]));
        raw.extend(pack_affine(&[key.g2_spx[j]]));
    }
    raw
}

/// One phase-1 contribution to a powers-of-tau transcript (`dg16_srs_contribute`): entry j of the four arrays times
/// tau^j (and alpha, beta), `beta_g2` times beta.  `secrets` = [tau, alpha, beta], non-zero.  THE RANDOMNESS IS THE
/// CALLER'S, and so is the challenge: with `proof` = (blinds [s_tau, s_alpha, s_beta], challenge points [SP_tau,
/// SP_alpha, SP_beta]) the key is made too.  The caller vouches that the transcript's points have order r
/// (`srs_verify` first).
pub fn srs_contribute<E, P1, P2>(powers: &SrsPowers<E>, secrets: &[E::ScalarField; 3],
                                 proof: Option<(&[E::ScalarField; 3], &[E::G2Affine; 3])>)
    -> Result<(SrsPowers<E>, Option<SrsContributionKey<E>>), Dg16Error>
where
    E: Pairing<G1Affine = Affine<P1>, G2Affine = Affine<P2>>,
    P1: Dg16Config<ScalarField = E::ScalarField>,
    P2: Dg16Config<ScalarField = E::ScalarField>,
    P1::BaseField: FieldBytes,
    P2::BaseField: FieldBytes,
{
    let m = powers.tau_g2.len();
    if !m.is_power_of_two() || powers.tau_g1.len() != 2 * m - 1 || powers.alpha_tau_g1.len() != m
        || powers.beta_tau_g1.len() != m
    {
        return Err(Dg16Error::Status(sys::DG16_ERR_BAD_ARG, "powers: tau_g1 holds 2m - 1 points, the others m = 2^k".into()));
    }
    let log_m = m.trailing_zeros();
    let (mut t1, mut t2) = (pack_affine(&powers.tau_g1), pack_affine(&powers.tau_g2));
    let (mut at, mut bt, mut b2) =
        (pack_affine(&powers.alpha_tau_g1), pack_affine(&powers.beta_tau_g1), pack_affine(&[powers.beta_g2]));
    // every output is its input: the library allows it
    let raw_in = sys::Dg16SrsPowers {
        tau_g1: t1.as_ptr().cast(),
        tau_g2: t2.as_ptr().cast(),
        alpha_tau_g1: at.as_ptr().cast(),
        beta_tau_g1: bt.as_ptr().cast(),
        beta_g2: b2.as_ptr().cast(),
    };
    let raw_out = sys::Dg16SrsPowersOut {
        tau_g1: t1.as_mut_ptr().cast(),
        tau_g2: t2.as_mut_ptr().cast(),
        alpha_tau_g1: at.as_mut_ptr().cast(),
        beta_tau_g1: bt.as_mut_ptr().cast(),
        beta_g2: b2.as_mut_ptr().cast(),
    };
    let sec: Vec<u8> = secrets.iter().flat_map(scalar_bytes).collect();
    let (f1, f2) = (2 * <P1::BaseField as FieldBytes>::BYTES, 2 * <P2::BaseField as FieldBytes>::BYTES);
    let mut key_raw = vec![0u8; 3 * (2 * f1 + f2)];
    let (blinds, challenge): (Vec<u8>, Vec<u8>) = match proof {
        Some((s, sp)) => (s.iter().flat_map(scalar_bytes).collect(), pack_affine(&sp[..])),
        None => (Vec::new(), Vec::new()),
    };
    let opt = |v: &Vec<u8>| -> *const core::ffi::c_void {
        if proof.is_some() { v.as_ptr().cast() } else { std::ptr::null() }
    };
    check(unsafe {
        sys::dg16_srs_contribute(CTX.0, P1::CURVE, log_m, &raw_in, sec.as_ptr().cast(), opt(&blinds), opt(&challenge),
                                 &raw_out, if proof.is_some() { key_raw.as_mut_ptr().cast() } else { std::ptr::null_mut() })
    })?;
    let out = SrsPowers::<E> {
        tau_g1: unpack_affine::<P1>(&t1),
        tau_g2: unpack_affine::<P2>(&t2),
        alpha_tau_g1: unpack_affine::<P1>(&at),
        beta_tau_g1: unpack_affine::<P1>(&bt),
        beta_g2: unpack_affine::<P2>(&b2)[0],
    };
    let key = proof.map(|_| {
        let part = |j: usize| &key_raw[j * (2 * f1 + f2)..(j + 1) * (2 * f1 + f2)];
        let g1: Vec<Vec<Affine<P1>>> = (0..3).map(|j| unpack_affine::<P1>(&part(j)[..2 * f1])).collect();
        let g2: Vec<Affine<P2>> = (0..3).map(|j| unpack_affine::<P2>(&part(j)[2 * f1..])[0]).collect();
        SrsContributionKey::<E> {
            g1_s: [g1[0][0], g1[1][0], g1[2][0]],
            g1_sx: [g1[0][1], g1[1][1], g1[2][1]],
            g2_spx: [g2[0], g2[1], g2[2]],
        }
    });
    Ok((out, key))
}

/// Is `after` a contribution to `before` by whoever holds `key` under the challenge points
/// (`dg16_srs_verify_contribution`)?  `after` is checked in full like `srs_verify` does (same `coeffs`: 2m - 2 integers
/// in [1, 2^128) drawn AFTER `after` was fixed); of `before` only the head points are read.  `report.failed == 0`
/// accepts; its bits are `sys::DG16_P1_*`.  A rejected contribution is `Ok` with the bits set.  Not checked: that the
/// challenge is the hash of `before` -- the caller's protocol.
pub fn srs_verify_contribution<E, P1, P2>(before: &SrsPowers<E>, after: &SrsPowers<E>, key: &SrsContributionKey<E>,
                                          challenge: &[E::G2Affine; 3], coeffs: &[u128])
    -> Result<sys::Dg16SrsContributionReport, Dg16Error>
where
    E: Pairing<G1Affine = Affine<P1>, G2Affine = Affine<P2>>,
    P1: Dg16Config<ScalarField = E::ScalarField>,
    P2: Dg16Config<ScalarField = E::ScalarField>,
    P1::BaseField: FieldBytes,
    P2::BaseField: FieldBytes,
{
    let m = after.tau_g2.len();
    if !m.is_power_of_two() || m < 2 || after.tau_g1.len() != 2 * m - 1 || after.alpha_tau_g1.len() != m
        || after.beta_tau_g1.len() != m || coeffs.len() != 2 * m - 2 || before.tau_g1.len() < 2 || before.tau_g2.len() < 2
        || before.alpha_tau_g1.is_empty() || before.beta_tau_g1.is_empty()
    {
        return Err(Dg16Error::Status(sys::DG16_ERR_BAD_ARG,
                                     "after: tau_g1 holds 2m - 1 points, the others m = 2^k >= 2; 2m - 2 coefficients; before: its heads".into()));
    }
    let log_m = m.trailing_zeros();
    // of `before` the heads only
    let (bt1, bt2) = (pack_affine(&before.tau_g1[..2]), pack_affine(&before.tau_g2[..2]));
    let (bat, bbt, bb2) =
        (pack_affine(&before.alpha_tau_g1[..1]), pack_affine(&before.beta_tau_g1[..1]), pack_affine(&[before.beta_g2]));
    let raw_before = sys::Dg16SrsPowers {
        tau_g1: bt1.as_ptr().cast(),
        tau_g2: bt2.as_ptr().cast(),
        alpha_tau_g1: bat.as_ptr().cast(),
        beta_tau_g1: bbt.as_ptr().cast(),
        beta_g2: bb2.as_ptr().cast(),
    };
    let (t1, t2) = (pack_affine(&after.tau_g1), pack_affine(&after.tau_g2));
    let (at, bt, b2) = (pack_affine(&after.alpha_tau_g1), pack_affine(&after.beta_tau_g1), pack_affine(&[after.beta_g2]));
    let raw_after = sys::Dg16SrsPowers {
        tau_g1: t1.as_ptr().cast(),
        tau_g2: t2.as_ptr().cast(),
        alpha_tau_g1: at.as_ptr().cast(),
        beta_tau_g1: bt.as_ptr().cast(),
        beta_g2: b2.as_ptr().cast(),
    };
    let key_raw = pack_contribution_key::<E, P1, P2>(key);
    let sp = pack_affine(&challenge[..]);
    let rho: Vec<u8> = coeffs.iter().flat_map(|c| c.to_le_bytes()).collect();
    let mut report = sys::Dg16SrsContributionReport::default();
    check(unsafe {
        sys::dg16_srs_verify_contribution(CTX.0, P1::CURVE, log_m, &raw_before, &raw_after, key_raw.as_ptr().cast(),
                                          sp.as_ptr().cast(), rho.as_ptr().cast(), &mut report)
    })?;
    Ok(report)
}

/// One phase-2 contribution to `pk` (`dg16_groth16_contribute`): `delta_g1`, `delta_g2` times `delta`, `l_query` and
/// `h_query` divided by it, everything else as it is.  THE RANDOMNESS IS THE CALLER'S: `delta` non-zero, uniform, and
/// forgotten afterwards.  The caller vouches that the key's points have order r.
pub fn contribute<E, P1, P2>(pk: &ProvingKey<E>, delta: &E::ScalarField) -> Result<ProvingKey<E>, Dg16Error>
where
    E: Pairing<G1Affine = Affine<P1>, G2Affine = Affine<P2>>,
    P1: Dg16Config<ScalarField = E::ScalarField>,
    P2: Dg16Config<ScalarField = E::ScalarField>,
    P1::BaseField: FieldBytes,
    P2::BaseField: FieldBytes,
{
    let f1 = 2 * <P1::BaseField as FieldBytes>::BYTES;
    let (mut l, mut h) = (pack_affine(&pk.l_query), pack_affine(&pk.h_query));
    let mut fixed = pack_affine(&[pk.vk.alpha_g1, pk.beta_g1, pk.delta_g1]);
    fixed.extend(pack_affine(&[pk.vk.beta_g2, pk.vk.delta_g2]));
    let mut d = delta.into_bigint().to_bytes_le();
    d.resize(32, 0);
    check(unsafe {
        sys::dg16_groth16_contribute(CTX.0, P1::CURVE, pk.l_query.len(), pk.h_query.len(), l.as_ptr().cast(),
                                     h.as_ptr().cast(), fixed.as_ptr().cast(), d.as_ptr().cast(), l.as_mut_ptr().cast(),
                                     h.as_mut_ptr().cast(), fixed.as_mut_ptr().cast())
    })?;
    let mut out = pk.clone();
    out.l_query = unpack_affine::<P1>(&l);
    out.h_query = unpack_affine::<P1>(&h);
    out.delta_g1 = unpack_affine::<P1>(&fixed[2 * f1..3 * f1])[0];
    out.vk.delta_g2 = unpack_affine::<P2>(&fixed[3 * f1..])[1];
    Ok(out)
}

/// One party's share of a proving key, with the field names of the reference's `PackedProvingKeyShare`
/// (groth16/src/proving_key.rs:26-33); a call site moves the five vectors into that struct.
pub struct PackedKeyShare<E: Pairing> {
    pub s: Vec<E::G1Affine>,
    pub u: Vec<E::G1Affine>,
    pub v: Vec<E::G2Affine>,
    pub w: Vec<E::G1Affine>,
    pub h: Vec<E::G1Affine>,
}

/// `PackedProvingKeyShare::pack_from_arkworks_proving_key` for ALL parties in one `dg16_pk_pack`: s <- a_query[1..],
/// u <- h_query, w <- l_query, h <- b_g1_query[1..], v <- b_g2_query[1..], each cut into l-chunks (the last one padded
/// with identities) and packed in the exponent.  Element i of the result is party i's share; the points are those the
/// reference computes.  `in_subgroup`: a key's points have order r, so a caller who
/// trusts its key sets it and the cofactor groups take the endomorphism split too.
pub fn pack_proving_key<E, P1, P2>(pk: &ProvingKey<E>, pp: &crate::net::Pss, n_parties: usize, in_subgroup: bool)
    -> Result<Vec<PackedKeyShare<E>>, Dg16Error>
where
    E: Pairing<G1Affine = Affine<P1>, G2Affine = Affine<P2>>,
    P1: Dg16Config<ScalarField = E::ScalarField>,
    P2: Dg16Config<ScalarField = E::ScalarField>,
    P1::BaseField: FieldBytes,
    P2::BaseField: FieldBytes,
{
    let (nv, m) = (pk.a_query.len(), pk.h_query.len());
    if nv == 0 || pk.b_g1_query.len() != nv || pk.b_g2_query.len() != nv || pk.l_query.len() >= nv {
        return Err(Dg16Error::Status(sys::DG16_ERR_BAD_ARG, "a proving key with queries of unequal lengths".into()));
    }
    let ni = nv - pk.l_query.len();
    let (f1, f2) = (2 * <P1::BaseField as FieldBytes>::BYTES, 2 * <P2::BaseField as FieldBytes>::BYTES);
    let chunks = |n: usize| unsafe { sys::dg16_pss_pack_chunks(pp.0, n) };
    let (cq, cu, cw) = (chunks(nv - 1), chunks(m), chunks(nv - ni));
    let (a, b1, b2) = (pack_affine(&pk.a_query), pack_affine(&pk.b_g1_query), pack_affine(&pk.b_g2_query));
    let (hq, lq) = (pack_affine(&pk.h_query), pack_affine(&pk.l_query));
    let (mut s, mut u, mut w) = (vec![0u8; n_parties * cq * f1], vec![0u8; n_parties * cu * f1], vec![0u8; n_parties * cw * f1]);
    let (mut h, mut v) = (vec![0u8; n_parties * cq * f1], vec![0u8; n_parties * cq * f2]);
    let out = sys::Dg16PkShares { s: s.as_mut_ptr().cast(), u: u.as_mut_ptr().cast(), v: v.as_mut_ptr().cast(),
                                  w: w.as_mut_ptr().cast(), h: h.as_mut_ptr().cast() };
    check(unsafe {
        sys::dg16_pk_pack(CTX.0, pp.0, nv, ni, m, a.as_ptr().cast(), b1.as_ptr().cast(), b2.as_ptr().cast(),
                          hq.as_ptr().cast(), lq.as_ptr().cast(), &out,
                          if in_subgroup { 1 } else { 0 })
    })?;
    Ok((0..n_parties)
        .map(|i| PackedKeyShare {
            s: unpack_affine::<P1>(&s[i * cq * f1..(i + 1) * cq * f1]),
            u: unpack_affine::<P1>(&u[i * cu * f1..(i + 1) * cu * f1]),
            v: unpack_affine::<P2>(&v[i * cq * f2..(i + 1) * cq * f2]),
            w: unpack_affine::<P1>(&w[i * cw * f1..(i + 1) * cw * f1]),
            h: unpack_affine::<P1>(&h[i * cq * f1..(i + 1) * cq * f1]),
        })
        .collect())
}

struct PackedKey {
    arrays: [Vec<u8>; 8],
}
impl PackedKey {
    fn new<E, P1, P2>(pk: &ProvingKey<E>) -> Self
    where
        E: Pairing<G1Affine = Affine<P1>, G2Affine = Affine<P2>>,
        P1: Dg16Config<ScalarField = E::ScalarField>,
        P2: Dg16Config<ScalarField = E::ScalarField>,
        P1::BaseField: FieldBytes,
        P2::BaseField: FieldBytes,
    {
        let mut fixed = pack_affine(&[pk.vk.alpha_g1, pk.beta_g1, pk.delta_g1]);
        fixed.extend(pack_affine(&[pk.vk.beta_g2, pk.vk.delta_g2]));
        PackedKey {
            arrays: [pack_affine(&pk.a_query), pack_affine(&pk.b_g1_query), pack_affine(&pk.b_g2_query),
                     pack_affine(&pk.h_query), pack_affine(&pk.l_query), fixed, pack_affine(&[pk.vk.gamma_g2]),
                     pack_affine(&pk.vk.gamma_abc_g1)],
        }
    }
    fn raw(&self) -> sys::Dg16Groth16Key {
        let p = |i: usize| self.arrays[i].as_ptr().cast();
        sys::Dg16Groth16Key { a_query: p(0), b_g1_query: p(1), b_g2_query: p(2), h_query: p(3), l_query: p(4),
                              fixed_points: p(5), gamma_g2: p(6), gamma_abc_g1: p(7) }
    }
}

/// Is `after` the key `before` with delta replaced by d * delta for some d (`dg16_groth16_verify_contribution`)?
/// `coeffs`: max(l_query.len(), h_query.len()) integers in [1, 2^128), independent, uniform and drawn AFTER both keys
/// were fixed -- the caller's randomness.  `report.failed == 0` accepts; its bits are `sys::DG16_P2_*`.  A rejected key is
/// `Ok` with the bits set; a zero coefficient is an error.  Not checked: a contributor's proof of knowledge and a
/// transcript's hash chain.
pub fn verify_contribution<E, P1, P2>(before: &ProvingKey<E>, after: &ProvingKey<E>, coeffs: &[u128])
    -> Result<sys::Dg16Phase2Report, Dg16Error>
where
    E: Pairing<G1Affine = Affine<P1>, G2Affine = Affine<P2>>,
    P1: Dg16Config<ScalarField = E::ScalarField>,
    P2: Dg16Config<ScalarField = E::ScalarField>,
    P1::BaseField: FieldBytes,
    P2::BaseField: FieldBytes,
{
    let (ni, nv, m) = (before.vk.gamma_abc_g1.len(), before.a_query.len(), before.h_query.len());
    if after.vk.gamma_abc_g1.len() != ni || after.a_query.len() != nv || after.h_query.len() != m
        || before.l_query.len() != nv - ni || after.l_query.len() != nv - ni || before.b_g1_query.len() != nv
        || after.b_g1_query.len() != nv || before.b_g2_query.len() != nv || after.b_g2_query.len() != nv
        || coeffs.len() != (nv - ni).max(m)
    {
        return Err(Dg16Error::Status(sys::DG16_ERR_BAD_ARG,
                                     "keys of different shapes, or not max(l_query, h_query) coefficients".into()));
    }
    let (kb, ka) = (PackedKey::new(before), PackedKey::new(after));
    let (rb, ra) = (kb.raw(), ka.raw());
    let rho: Vec<u8> = coeffs.iter().flat_map(|c| c.to_le_bytes()).collect();
    let mut report = sys::Dg16Phase2Report::default();
    check(unsafe {
        sys::dg16_groth16_verify_contribution(CTX.0, P1::CURVE, ni, nv, m, &rb, &ra, rho.as_ptr().cast(), &mut report)
    })?;
    Ok(report)
}

/// The key of `m` computed in the exponent from `srs` (`dg16_groth16_setup_srs`): gamma = delta = 1, no trapdoor.
/// `in_subgroup` passes DG16_F_BASES_IN_SUBGROUP (the endomorphism split of the coefficients).
pub fn setup_from_srs<E, P1, P2>(m: &ConstraintMatrices<E::ScalarField>, srs: &Srs<E>, in_subgroup: bool)
    -> Result<ProvingKey<E>, Dg16Error>
where
    E: Pairing<G1Affine = Affine<P1>, G2Affine = Affine<P2>>,
    P1: Dg16Config<ScalarField = E::ScalarField>,
    P2: Dg16Config<ScalarField = E::ScalarField>,
    P1::BaseField: FieldBytes,
    P2::BaseField: FieldBytes,
{
    let (nc, ni) = (m.num_constraints, m.num_instance_variables);
    let nv = ni + m.num_witness_variables;
    let log_m = (nc + ni).next_power_of_two().trailing_zeros();
    let domain = 1usize << log_m;
    for n in [srs.lag_g1.len(), srs.lag_g2.len(), srs.alpha_lag_g1.len(), srs.beta_lag_g1.len(), srs.h_g1.len()] {
        if n != domain {
            return Err(Dg16Error::Status(sys::DG16_ERR_BAD_ARG, "the reference string is for another domain size".into()));
        }
    }
    let (l1, l2) = (pack_affine(&srs.lag_g1), pack_affine(&srs.lag_g2));
    let (al, bl, hb) = (pack_affine(&srs.alpha_lag_g1), pack_affine(&srs.beta_lag_g1), pack_affine(&srs.h_g1));
    let fixed_in = {
        let mut f = pack_affine(&[srs.alpha_g1, srs.beta_g1, srs.g1]);
        f.extend(pack_affine(&[srs.beta_g2, srs.g2]));
        f
    };
    let raw = sys::Dg16Srs {
        lag_g1: l1.as_ptr().cast(),
        lag_g2: l2.as_ptr().cast(),
        alpha_lag_g1: al.as_ptr().cast(),
        beta_lag_g1: bl.as_ptr().cast(),
        h_g1: hb.as_ptr().cast(),
        fixed: fixed_in.as_ptr().cast(),
    };
    let (ca, cb, cc) = (Csr::from_rows(&m.a), Csr::from_rows(&m.b), Csr::from_rows(&m.c));
    let (f1, f2) = (2 * <P1::BaseField as FieldBytes>::BYTES, 2 * <P2::BaseField as FieldBytes>::BYTES);
    let (mut a, mut b1, mut b2) = (vec![0u8; nv * f1], vec![0u8; nv * f1], vec![0u8; nv * f2]);
    let (mut h, mut l) = (vec![0u8; domain * f1], vec![0u8; (nv - ni) * f1]);
    let (mut fixed, mut gamma_g2, mut ic) = (vec![0u8; 3 * f1 + 2 * f2], vec![0u8; f2], vec![0u8; ni * f1]);
    check(unsafe {
        sys::dg16_groth16_setup_srs(
            CTX.0, P1::CURVE, nc, ni, nv, log_m,
            ca.row_ptr.as_ptr(), ca.col.as_ptr(), scalars_as_bytes(&ca.coeff).as_ptr().cast(),
            cb.row_ptr.as_ptr(), cb.col.as_ptr(), scalars_as_bytes(&cb.coeff).as_ptr().cast(),
            cc.row_ptr.as_ptr(), cc.col.as_ptr(), scalars_as_bytes(&cc.coeff).as_ptr().cast(),
            &raw, a.as_mut_ptr().cast(), b1.as_mut_ptr().cast(), b2.as_mut_ptr().cast(), h.as_mut_ptr().cast(),
            l.as_mut_ptr().cast(), fixed.as_mut_ptr().cast(), gamma_g2.as_mut_ptr().cast(), ic.as_mut_ptr().cast(),
            if in_subgroup { sys::DG16_F_BASES_IN_SUBGROUP } else { 0 },
        )
    })?;
    let g1_fixed = unpack_affine::<P1>(&fixed[..3 * f1]);
    let g2_fixed = unpack_affine::<P2>(&fixed[3 * f1..]);
    let vk = VerifyingKey::<E> {
        alpha_g1: g1_fixed[0],
        beta_g2: g2_fixed[0],
        gamma_g2: unpack_affine::<P2>(&gamma_g2)[0],
        delta_g2: g2_fixed[1],
        gamma_abc_g1: unpack_affine::<P1>(&ic),
    };
    Ok(ProvingKey::<E> {
        vk,
        beta_g1: g1_fixed[1],
        delta_g1: g1_fixed[2],
        a_query: unpack_affine::<P1>(&a),
        b_g1_query: unpack_affine::<P1>(&b1),
        b_g2_query: unpack_affine::<P2>(&b2),
        h_query: unpack_affine::<P1>(&h),
        l_query: unpack_affine::<P1>(&l),
    })
}
