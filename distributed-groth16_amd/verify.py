"""Groth16 verification through libdg16 -- the counterpart of `Groth16::<E>::verify_proof` as the reference calls it
(groth16/examples/sha256.rs:228-254, the verify endpoint of mpc-api/src/main.rs, zk-cli verify).  Two paths:
`verify_proof` / `verify_with_zkey`: the host verifier (`dg16_groth16_verify`, csrc/verify.hip; BN254, one proof per
call); `PreparedVerifyingKey`: batches on the GPU (`dg16_vk_create` + `dg16_groth16_verify_batch` for one verdict
per proof, `dg16_groth16_verify_aggregate` for one verdict per batch; BN254 and BLS12-381).  Points are affine x || y Montgomery limbs (uint64), the layout of a zkey's header / IC section and of
`serialize.decompress_to_limbs`."""

import ctypes
import secrets

import numpy as np

from . import lib as _lib


def verify_proof(alpha_g1, beta_g2, gamma_g2, delta_g2, ic, public_inputs, proof_affine, scalars_mont=False):
    """ic: (n_public + 1) x 8 uint64; public_inputs: n_public x 4 uint64; proof_affine: 32 uint64
    (A.x A.y | B.x B.y | C.x C.y).  Returns True / False; raises on a malformed verification key."""
    L = _lib.load()
    arr = lambda x: np.ascontiguousarray(x, dtype=np.uint64)
    alpha_g1, beta_g2, gamma_g2, delta_g2 = arr(alpha_g1), arr(beta_g2), arr(gamma_g2), arr(delta_g2)
    ic = arr(ic).reshape(-1, 8)
    pub = arr(public_inputs).reshape(-1, 4)
    proof = arr(proof_affine).reshape(-1)
    if proof.size != 32:
        raise ValueError("a BN254 proof is 8 field elements in affine form")
    ok = ctypes.c_int(0)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    rc = L.dg16_groth16_verify(0, p(alpha_g1), p(beta_g2), p(gamma_g2), p(delta_g2), p(ic), ic.shape[0], p(pub),
                               pub.shape[0], p(proof), _lib.F_SCALARS_MONT if scalars_mont else 0, ctypes.byref(ok))
    if rc != 0:
        raise _lib.Dg16Error(rc, L.dg16_verify_error().decode())
    return bool(ok.value)


def verify_with_zkey(zkey, public_inputs, proof_affine, scalars_mont=False):
    """Verification key taken from a parsed `.zkey` (zkey.ZKey): alpha, beta, gamma, delta and IC as they lie in it."""
    return verify_proof(zkey.alpha_g1, zkey.beta_g2, zkey.gamma_g2, zkey.delta_g2, zkey.ic, public_inputs,
                        proof_affine, scalars_mont=scalars_mont)


def random_coefficients(n):
    """n nonzero 128-bit coefficients for `verify_aggregate` from the operating system's generator: n x 2 uint64."""
    buf = bytearray(secrets.token_bytes(16 * n))
    for i in range(n):
        while not any(buf[16 * i:16 * i + 16]):
            buf[16 * i:16 * i + 16] = secrets.token_bytes(16)
    return np.frombuffer(bytes(buf), dtype=np.uint64).reshape(n, 2)


def random_rerandomizers(curve, n):
    """n pairs (r1, r2) for `PreparedVerifyingKey.rerandomize`, each uniform in [1, r) by rejection from the operating
    system's generator: n x 2 x 4 uint64, canonical."""
    from .keygen import FR_MODULUS
    r = FR_MODULUS[curve]
    nbits = r.bit_length()
    out = np.zeros((n, 2, 4), dtype=np.uint64)
    for i in range(n):
        for j in range(2):
            v = 0
            while not 1 <= v < r:
                v = secrets.randbits(nbits)
            out[i, j] = np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint64)
    return out


class PreparedVerifyingKey:
    """A verifying key validated and prepared once on `ctx`'s GPU (`ark_groth16::PreparedVerifyingKey`): the Miller value
    of (alpha, beta) and the Miller-loop line tables of gamma and delta.  Raises Dg16Error(BAD_ARG) for a malformed key
    (non-reduced coordinate, point off its curve or outside the order-r subgroup), UNSUPPORTED for BLS12-377."""

    def __init__(self, ctx, curve, alpha_g1, beta_g2, gamma_g2, delta_g2, ic):
        self.ctx, self.curve = ctx, curve
        self.fq = _lib.FQ_LIMBS64[curve]
        arr = lambda x: np.ascontiguousarray(x, dtype=np.uint64)
        alpha_g1, beta_g2, gamma_g2, delta_g2 = (arr(x).reshape(-1) for x in (alpha_g1, beta_g2, gamma_g2, delta_g2))
        ic = arr(ic).reshape(-1, 2 * self.fq)
        if alpha_g1.size != 2 * self.fq or any(x.size != 4 * self.fq for x in (beta_g2, gamma_g2, delta_g2)):
            raise ValueError("verifying key points have the wrong size for %s" % curve)
        self.n_public = ic.shape[0] - 1
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        h = ctypes.c_void_p()
        ctx._chk(ctx.L.dg16_vk_create(ctx.h, _lib.CURVES[curve], p(alpha_g1), p(beta_g2), p(gamma_g2), p(delta_g2),
                                      p(ic), ic.shape[0], 0, ctypes.byref(h)))
        self.h = h

    @classmethod
    def from_zkey(cls, ctx, zkey):
        """Key material as it lies in a parsed `.zkey` (zkey.ZKey; BN254)."""
        return cls(ctx, "bn254", zkey.alpha_g1, zkey.beta_g2, zkey.gamma_g2, zkey.delta_g2, zkey.ic)

    @classmethod
    def from_parameters(cls, ctx, params):
        """The verifying key of a `keygen.generate_parameters` result."""
        return cls(ctx, params.curve, *params.verifying_key())

    def verify_batch(self, public_inputs, proofs, scalars_mont=False, device=False, channel=0, n_proofs=None):
        """public_inputs: n_proofs x n_public scalars (4 uint64 each); proofs: n_proofs x (A | B | C) affine
        (8 field elements each).  Returns one bool per proof.  device=True: both are raw device pointers (ints) or
        objects with data_ptr(), n_proofs is required, and the verdicts are read back after the channel has drained."""
        flags = _lib.F_SCALARS_MONT if scalars_mont else 0
        L, ctx = self.ctx.L, self.ctx
        if device:
            import torch
            ptr = lambda x: x.data_ptr() if hasattr(x, "data_ptr") else int(x or 0)
            if n_proofs is None:
                raise ValueError("n_proofs is required with device pointers")
            out = torch.zeros(max(n_proofs, 1), dtype=torch.uint8, device="cuda:%d" % self.ctx.device)
            ctx._chk(L.dg16_groth16_verify_batch(ctx.h, self.h, ctypes.c_void_p(ptr(public_inputs)), self.n_public,
                                                 ctypes.c_void_p(ptr(proofs)), n_proofs, flags | _lib.F_DEVICE_PTRS,
                                                 ctypes.c_void_p(out.data_ptr()), channel))
            ctx.sync(channel)
            return out[:n_proofs].cpu().numpy().astype(bool)
        proofs = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 8 * self.fq)
        n = proofs.shape[0]
        pub = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        if n == 0:
            n_public = self.n_public
        elif pub.size % (4 * n):
            raise ValueError("public_inputs is not n_proofs x n_public scalars")
        else:
            n_public = pub.size // (4 * n)      # the library compares it with the key (LENGTH_MISMATCH)
        out = np.zeros(max(n, 1), dtype=np.uint8)
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        ctx._chk(L.dg16_groth16_verify_batch(ctx.h, self.h, p(pub), n_public, p(proofs), n, flags, p(out), channel))
        return out[:n].astype(bool)

    def verify_aggregate(self, public_inputs, proofs, coeffs=None, scalars_mont=False, device=False, channel=0,
                         n_proofs=None):
        """One verdict for the whole batch (`dg16_groth16_verify_aggregate`): True iff every proof passes the input
        checks and the random linear combination of the verification equations holds.  Layouts as `verify_batch`.
        coeffs: n_proofs x 2 uint64 (128-bit little-endian coefficients); None draws nonzero ones from `secrets` --
        coefficients must be unpredictable and chosen after the proofs are fixed, or the verdict guarantees nothing
        (include/dg16.h).  device=True: public_inputs, proofs and coeffs are device pointers, coeffs and n_proofs are
        required, and the verdict is read back after the channel has drained.  On False, `verify_batch` says which
        proofs are bad."""
        flags = _lib.F_SCALARS_MONT if scalars_mont else 0
        L, ctx = self.ctx.L, self.ctx
        if device:
            import torch
            ptr = lambda x: x.data_ptr() if hasattr(x, "data_ptr") else int(x or 0)
            if n_proofs is None or coeffs is None:
                raise ValueError("n_proofs and coeffs are required with device pointers")
            out = torch.zeros(1, dtype=torch.uint8, device="cuda:%d" % self.ctx.device)
            ctx._chk(L.dg16_groth16_verify_aggregate(ctx.h, self.h, ctypes.c_void_p(ptr(public_inputs)), self.n_public,
                                                     ctypes.c_void_p(ptr(proofs)), n_proofs,
                                                     ctypes.c_void_p(ptr(coeffs)), flags | _lib.F_DEVICE_PTRS,
                                                     ctypes.c_void_p(out.data_ptr()), channel))
            ctx.sync(channel)
            return bool(out.cpu()[0])
        proofs = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 8 * self.fq)
        n = proofs.shape[0]
        pub = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        if n == 0:
            n_public = self.n_public
        elif pub.size % (4 * n):
            raise ValueError("public_inputs is not n_proofs x n_public scalars")
        else:
            n_public = pub.size // (4 * n)      # the library compares it with the key (LENGTH_MISMATCH)
        if coeffs is None:
            coeffs = random_coefficients(n)
        coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 2)
        if coeffs.shape[0] != n:
            raise ValueError("coeffs is not n_proofs x 2 uint64")
        out = np.zeros(1, dtype=np.uint8)
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        ctx._chk(L.dg16_groth16_verify_aggregate(ctx.h, self.h, p(pub), n_public, p(proofs), n, p(coeffs), flags,
                                                 p(out), channel))
        return bool(out[0])

    def rerandomize(self, proofs, r1_r2=None, scalars_mont=False, device=False, channel=0, n_proofs=None, out=None):
        """`Groth16::rerandomize_proof` for a batch (`dg16_groth16_rerandomize`): (A, B, C) -> (r1^-1 A,
        r1 B + r1 r2 delta_g2, C + r2 A), which verifies for the same public inputs exactly when (A, B, C) does and cannot
        be linked to it.  proofs as in `verify_batch`; r1_r2: n_proofs x 2 scalars in [1, r) (4 uint64 each), None draws
        them with `random_rerandomizers`.  The proofs are not verified here and must hold subgroup points: verify first.
        Host arrays: a zero or non-reduced r1 / r2 raises Dg16Error(BAD_ARG).  device=True: proofs, r1_r2 and out are
        device pointers, r1_r2 and n_proofs are required, out=None means in place, the call is stream-ordered on the
        channel, and a bad r1 / r2 turns its proof into all-zero bytes instead of an error.  Returns the new proofs."""
        flags = _lib.F_SCALARS_MONT if scalars_mont else 0
        L, ctx = self.ctx.L, self.ctx
        if device:
            ptr = lambda x: x.data_ptr() if hasattr(x, "data_ptr") else int(x or 0)
            if n_proofs is None or r1_r2 is None:
                raise ValueError("n_proofs and r1_r2 are required with device pointers")
            if out is None:
                out = proofs
            ctx._chk(L.dg16_groth16_rerandomize(ctx.h, self.h, ctypes.c_void_p(ptr(proofs)), n_proofs,
                                                ctypes.c_void_p(ptr(r1_r2)), flags | _lib.F_DEVICE_PTRS,
                                                ctypes.c_void_p(ptr(out)), channel))
            return out
        proofs = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 8 * self.fq)
        n = proofs.shape[0]
        if r1_r2 is None:
            if scalars_mont:
                raise ValueError("drawn r1, r2 are canonical: pass scalars_mont=False")
            r1_r2 = random_rerandomizers(self.curve, n)
        r1_r2 = np.ascontiguousarray(r1_r2, dtype=np.uint64).reshape(-1, 2, 4)
        if r1_r2.shape[0] != n:
            raise ValueError("r1_r2 is not n_proofs x 2 scalars")
        res = np.zeros_like(proofs)
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        ctx._chk(L.dg16_groth16_rerandomize(ctx.h, self.h, p(proofs), n, p(r1_r2), flags, p(res), channel))
        return res

    def close(self):
        if self.h:
            self.ctx.L.dg16_vk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
