//! arkworks values <-> the byte layout of `include/dg16.h` ("Conventions").
use ark_ec::short_weierstrass::{Affine, Projective, SWCurveConfig};
use ark_ff::{BigInt, Field, Fp, MontBackend, MontConfig, PrimeField};

/// Montgomery limbs of a prime-field element as they lie in memory: `Fp<MontBackend<_, N>>.0` is `BigInt<N>([u64; N])`
/// (pinned by ark-circom/src/zkey.rs:417-427, which reads the same limbs from a `.zkey`).
#[inline]
pub fn fp_limbs<T: MontConfig<N>, const N: usize>(x: &Fp<MontBackend<T, N>, N>) -> &[u64; N] {
    &x.0 .0
}
#[inline]
pub fn fp_from_limbs<T: MontConfig<N>, const N: usize>(l: [u64; N]) -> Fp<MontBackend<T, N>, N> {
    Fp::new_unchecked(BigInt::new(l))
}

/// Base-field elements (prime field, or the quadratic extension as `c0 || c1`) to little-endian Montgomery bytes.
pub trait FieldBytes: Field {
    const BYTES: usize;
    fn write_mont(&self, out: &mut [u8]);
    fn read_mont(inp: &[u8]) -> Self;
}
impl<T: MontConfig<N>, const N: usize> FieldBytes for Fp<MontBackend<T, N>, N> {
    const BYTES: usize = 8 * N;
    fn write_mont(&self, out: &mut [u8]) {
        for (i, l) in fp_limbs(self).iter().enumerate() {
            out[8 * i..8 * i + 8].copy_from_slice(&l.to_le_bytes());
        }
    }
    fn read_mont(inp: &[u8]) -> Self {
        let mut l = [0u64; N];
        for i in 0..N {
            l[i] = u64::from_le_bytes(inp[8 * i..8 * i + 8].try_into().unwrap());
        }
        fp_from_limbs(l)
    }
}
impl<P: ark_ff::Fp2Config> FieldBytes for ark_ff::Fp2<P>
where
    P::Fp: FieldBytes,
{
    const BYTES: usize = 2 * <P::Fp as FieldBytes>::BYTES;
    fn write_mont(&self, out: &mut [u8]) {
        let h = Self::BYTES / 2;
        self.c0.write_mont(&mut out[..h]);
        self.c1.write_mont(&mut out[h..]);
    }
    fn read_mont(inp: &[u8]) -> Self {
        let h = Self::BYTES / 2;
        ark_ff::Fp2::<P>::new(<P::Fp>::read_mont(&inp[..h]), <P::Fp>::read_mont(&inp[h..]))
    }
}

/// `x || y`, identity = all-zero bytes (the convention of ark-circom/src/zkey.rs:353-361): 64 / 96 bytes per G1 point,
/// 128 / 192 per G2 point.
pub fn pack_affine<P: SWCurveConfig>(pts: &[Affine<P>]) -> Vec<u8>
where
    P::BaseField: FieldBytes,
{
    let fe = <P::BaseField as FieldBytes>::BYTES;
    let mut out = vec![0u8; pts.len() * 2 * fe];
    for (i, p) in pts.iter().enumerate() {
        if p.infinity {
            continue;
        }
        p.x.write_mont(&mut out[i * 2 * fe..][..fe]);
        p.y.write_mont(&mut out[i * 2 * fe + fe..][..fe]);
    }
    out
}

/// Jacobian `(x, y, z)` Montgomery limbs (what every group-valued entry point writes) -> `Projective`.
/// z = 0 encodes the identity, like ark-ec.
pub fn unpack_projective<P: SWCurveConfig>(buf: &[u8]) -> Projective<P>
where
    P::BaseField: FieldBytes,
{
    let fe = <P::BaseField as FieldBytes>::BYTES;
    Projective::new_unchecked(
        <P::BaseField>::read_mont(&buf[..fe]),
        <P::BaseField>::read_mont(&buf[fe..2 * fe]),
        <P::BaseField>::read_mont(&buf[2 * fe..3 * fe]),
    )
}

/// `&[F]` of a 256-bit scalar field as the bytes the library reads with `DG16_F_SCALARS_MONT` -- no copy.
pub fn scalars_as_bytes<F: PrimeField>(s: &[F]) -> &[u8] {
    assert_eq!(core::mem::size_of::<F>(), 32, "Fr of BN254 / BLS12-381 / BLS12-377 is 4 x u64");
    unsafe { core::slice::from_raw_parts(s.as_ptr().cast::<u8>(), s.len() * 32) }
}
pub fn scalars_as_bytes_mut<F: PrimeField>(s: &mut [F]) -> &mut [u8] {
    assert_eq!(core::mem::size_of::<F>(), 32);
    unsafe { core::slice::from_raw_parts_mut(s.as_mut_ptr().cast::<u8>(), s.len() * 32) }
}

// ---- packing scalars into party shares (`dg16_fr_expand`, `dg16_pss_pack_scalars`, `dg16_request_pack`) ---------------

/// How a vector is cut into the l-tuples that are packed (`DG16_PACK_CHUNKS` / `DG16_PACK_DFFT`).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum PackLayout {
    /// consecutive l-chunks, the last one zero-padded (`pack_from_witness`, groth16/examples/sha256.rs:97-121)
    Chunks = 0,
    /// bit-reversed, then `(x[e], x[e + m/l], ..)` (`QAP::pss`, groth16/src/qap.rs:151-165)
    Dfft = 1,
}

/// Elements `first .. first + n` of stream `stream` of a 32-byte seed, made on the device (`dg16_fr_expand`).
pub fn fr_expand<F: crate::Dg16Scalar>(seed: &[u8; 32], stream: u64, first: u64, n: usize) -> Result<Vec<F>, crate::Dg16Error> {
    let mut out = vec![F::zero(); n];
    crate::check(unsafe {
        crate::sys::dg16_fr_expand(crate::CTX.0, F::CURVE, seed.as_ptr().cast(), stream, first, n, 1,
                                   scalars_as_bytes_mut(&mut out).as_mut_ptr().cast())
    })?;
    Ok(out)
}

/// `pack_from_public` (blinds = None) or `pack_from_public_rand` with the caller's randomness
/// (secret-sharing/src/pss.rs:72-92) over a whole vector for ALL parties: element i of the result is party i's share
/// vector.  `blinds`: `chunks * l` elements, slot k of chunk e at `e * l + k`.
#[cfg(feature = "mpc")]
pub fn pack_scalars<F: PrimeField>(values: &[F], layout: PackLayout, blinds: Option<&[F]>, pp: &crate::net::Pss,
                                   n_parties: usize) -> Result<Vec<Vec<F>>, crate::Dg16Error> {
    use crate::sys;
    if values.is_empty() {
        return Ok(vec![Vec::new(); n_parties]);
    }
    let chunks = unsafe { sys::dg16_pss_scalar_chunks(pp.0, layout as i32, values.len()) };
    // n = 4 l parties: a blind vector holds chunks * l elements
    if blinds.map_or(false, |b| b.len() * 4 != chunks * n_parties) {
        return Err(crate::Dg16Error::LengthMismatch(blinds.map_or(0, |b| b.len())));
    }
    let mut flat = vec![F::zero(); n_parties * chunks];
    crate::check(unsafe {
        sys::dg16_pss_pack_scalars(crate::CTX.0, pp.0, layout as i32, scalars_as_bytes(values).as_ptr().cast(), values.len(),
                                   blinds.map_or(core::ptr::null(), |b| scalars_as_bytes(b).as_ptr().cast()),
                                   scalars_as_bytes_mut(&mut flat).as_mut_ptr().cast())
    })?;
    Ok(flat.chunks(chunks.max(1)).take(n_parties).map(|c| c.to_vec()).collect())
}

/// One party's part of a packed proof request: the `PackedQAPShare` vectors and the two witness share vectors.
#[cfg(feature = "mpc")]
pub struct RequestShare<F> {
    pub a: Vec<F>,
    pub b: Vec<F>,
    pub c: Vec<F>,
    pub a_share: Vec<F>,
    pub ax_share: Vec<F>,
}

/// `QAP::pss` (qap.rs:143-187) and the two `pack_from_witness` (sha256.rs:97-121) of a proof request for ALL parties in
/// one `dg16_request_pack`.  `seed`: 32 uniform bytes of the caller's randomness, used for this request only; every
/// chunk is then packed as by `pack_from_public_rand` with blinds expanded from the seed on the device.  None packs
/// plainly.
#[cfg(feature = "mpc")]
pub fn pack_request<F: PrimeField>(a: &[F], b: &[F], c: &[F], full_assignment: &[F], num_inputs: usize,
                                   seed: Option<&[u8; 32]>, pp: &crate::net::Pss, n_parties: usize)
    -> Result<Vec<RequestShare<F>>, crate::Dg16Error> {
    use crate::sys;
    let (m, l) = (a.len(), n_parties / 4);      // n = 4 l (pss.rs:36)
    if b.len() != m || c.len() != m {
        return Err(crate::Dg16Error::LengthMismatch(m.min(b.len()).min(c.len())));
    }
    if m == 0 || !m.is_power_of_two() || full_assignment.is_empty() || l == 0 {
        return Err(crate::Dg16Error::Status(sys::DG16_ERR_BAD_ARG, "a, b, c: a power of two; a non-empty assignment".into()));
    }
    let num_vars = full_assignment.len();
    let (cq, ca, cx) = (m / l, (num_vars - 1 + l - 1) / l, (num_vars.saturating_sub(num_inputs) + l - 1) / l);
    let mut bufs = [vec![F::zero(); n_parties * cq], vec![F::zero(); n_parties * cq], vec![F::zero(); n_parties * cq],
                    vec![F::zero(); n_parties * ca], vec![F::zero(); n_parties * cx]];
    let out = {
        let [oa, ob, oc, os, ox] = &mut bufs;
        sys::Dg16RequestShares {
            a: scalars_as_bytes_mut(oa).as_mut_ptr().cast(),
            b: scalars_as_bytes_mut(ob).as_mut_ptr().cast(),
            c: scalars_as_bytes_mut(oc).as_mut_ptr().cast(),
            a_share: scalars_as_bytes_mut(os).as_mut_ptr().cast(),
            ax_share: scalars_as_bytes_mut(ox).as_mut_ptr().cast(),
        }
    };
    crate::check(unsafe {
        sys::dg16_request_pack(crate::CTX.0, pp.0, m.trailing_zeros(), scalars_as_bytes(a).as_ptr().cast(),
                               scalars_as_bytes(b).as_ptr().cast(), scalars_as_bytes(c).as_ptr().cast(),
                               scalars_as_bytes(full_assignment).as_ptr().cast(), num_vars, num_inputs,
                               seed.map_or(core::ptr::null(), |s| s.as_ptr().cast()), 1, &out)
    })?;
    let row = |v: &Vec<F>, per: usize, i: usize| v[i * per..(i + 1) * per].to_vec();
    Ok((0..n_parties)
        .map(|i| RequestShare {
            a: row(&bufs[0], cq, i),
            b: row(&bufs[1], cq, i),
            c: row(&bufs[2], cq, i),
            a_share: row(&bufs[3], ca, i),
            ax_share: row(&bufs[4], cx, i),
        })
        .collect())
}
