"""Groth16 key generation on the GPU (`dg16_groth16_setup`, csrc/setup_curve.hip) -- the counterpart of
`Groth16::<Bn254, CircomReduction>::circuit_specific_setup(circuit, rng)` as every program of the reference starts
(groth16/examples/sha256.rs:137, million.rs:137, mpc-api/src/main.rs:151).

    params = generate_parameters(ctx, "bn254", r1cs)          # R1CS of r1cs.py, or a dict of CSR arrays
    pk = params.proving_key(ctx)                              # resident key (dg16_pk_create on device pointers)
    ok = verify.verify_proof(*params.verifying_key(), public_inputs, proof_affine)

A key nobody holds the trapdoor of is computed in the exponent, from the Lagrange-basis points of a powers-of-tau
ceremony (`dg16_groth16_setup_srs`, csrc/setup_srs_curve.hip); it has gamma = delta = 1:

    params = generate_parameters_from_srs(ctx, "bn254", r1cs, srs)      # srs: an Srs, e.g. decoded from a prepared .ptau

and an Srs comes from the monomial powers a ceremony publishes through the group transform (`dg16_srs_prepare`,
csrc/group_ntt_curve.hip; snarkjs' `powersoftau prepare phase2`):

    srs = srs_from_powers(ctx, "bn254", log_m, tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, beta_g2)

Before a transcript is trusted anybody may add randomness of their own to it, phase 1 of the ceremony: every power is
multiplied by the matching power of a secret tau, alpha, beta (`dg16_srs_contribute`, csrc/points_series.h: the scalars
are a geometric series made on the device), with a proof of knowledge per secret, and anybody can check that one
transcript is such a contribution to another (`dg16_srs_verify_contribution`; snarkjs' `powersoftau contribute` and the
contribution part of `powersoftau verify`, without the hashes, which stay with the caller):

    powers2, key = contribute_powers(ctx, "bn254", log_m, powers, tau, alpha, beta, blinds=(s1, s2, s3), challenge=sp)
    report = verify_powers_contribution(ctx, "bn254", log_m, powers, powers2, key, sp)      # report.accepted

Such a key becomes one anybody may use through phase 2 of the ceremony -- every participant multiplies delta by a secret
of their own (`dg16_groth16_contribute`, csrc/points_scale.h), and anybody can check the result against the circuit and
the reference string (`dg16_groth16_verify_contribution`; snarkjs' `zkey contribute` and the key part of `zkey verify`):

    params = contribute(ctx, params, 1 + secrets.randbelow(r - 1))      # the contributor forgets the secret
    report = verify_parameters(ctx, "bn254", r1cs, srs, params)         # report.accepted

The trapdoor (alpha, beta, gamma, delta, tau) is drawn from `secrets` unless the caller passes one; it is returned with
the parameters only when it was passed in.  torch is the device-memory plumbing; there is no CPU path."""

import secrets

import numpy as np

from . import lib as _lib

FR_MODULUS = {
    "bn254": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
    "bls12_381": 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001,
    "bls12_377": 0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001,
}
TWO_ADICITY = {"bn254": 28, "bls12_381": 32, "bls12_377": 47}


def draw_trapdoor(curve):
    """Five uniform non-zero scalars (alpha, beta, gamma, delta, tau)."""
    r = FR_MODULUS[curve]
    return tuple(1 + secrets.randbelow(r - 1) for _ in range(5))


def _trapdoor_array(curve, trapdoor):
    r = FR_MODULUS[curve]
    td = [int(x) for x in trapdoor]
    if len(td) != 5:
        raise ValueError("trapdoor = (alpha, beta, gamma, delta, tau)")
    if any(not 0 < x < r for x in td):
        raise ValueError("every trapdoor element must be non-zero and below r")
    return np.array([[(x >> (64 * j)) & (2**64 - 1) for j in range(4)] for x in td], dtype=np.uint64)


def _is_tensor(x):
    return hasattr(x, "data_ptr")


def _check_csr(name, csr, nc, nv):
    ptr, col, coeff = csr
    if any(_is_tensor(x) for x in csr):
        if not all(_is_tensor(x) for x in csr):
            raise ValueError("matrix %s mixes device tensors and host arrays" % name)
        if ptr.numel() != nc + 1:
            raise ValueError("matrix %s: row_ptr must have num_constraints + 1 entries" % name)
        return csr            # indices on the device are checked by the library (DG16_ERR_BAD_ARG)
    ptr = np.ascontiguousarray(ptr, dtype=np.uint32)
    col = np.ascontiguousarray(col, dtype=np.uint32)
    coeff = np.ascontiguousarray(coeff, dtype=np.uint64).reshape(-1, 4)
    if ptr.shape != (nc + 1,):
        raise ValueError("matrix %s: row_ptr must have num_constraints + 1 entries" % name)
    if nc and (ptr[0] != 0 or np.any(ptr[1:] < ptr[:-1])):
        raise ValueError("matrix %s: row_ptr must start at 0 and not decrease" % name)
    nnz = int(ptr[-1]) if nc else 0
    if col.shape[0] != nnz or coeff.shape[0] != nnz:
        raise ValueError("matrix %s: col / coeff length differs from row_ptr[-1]" % name)
    if nnz and int(col.max()) >= nv:
        raise ValueError("matrix %s: column index >= num_vars" % name)
    return ptr, col, coeff


def prepare(curve, r1cs, trapdoor=None):
    """Host-side argument handling of generate_parameters (no GPU involved): shapes of the constraint system, CSR
    validation, the trapdoor.  r1cs: an `r1cs.R1CS` (canonical coefficients) or a dict with num_constraints,
    num_inputs (incl. the constant 1), num_vars, a / b / c = (row_ptr, col, coeff) and coeff_mont (default True:
    coefficients already in Montgomery form, the layout dg16_qap takes).
    -> dict(nc, ni, nv, log_m, csr=[a, b, c], coeff_mont, trapdoor=uint64 [5][4], trapdoor_given)."""
    if curve not in FR_MODULUS:
        raise ValueError("unknown curve %r" % (curve,))
    if isinstance(r1cs, dict):
        nc, ni, nv = int(r1cs["num_constraints"]), int(r1cs["num_inputs"]), int(r1cs["num_vars"])
        csr = [r1cs["a"], r1cs["b"], r1cs["c"]]
        coeff_mont = bool(r1cs.get("coeff_mont", True))
    else:
        nc, ni, nv = int(r1cs.n_constraints), int(r1cs.num_inputs), int(r1cs.num_variables)
        csr = list(r1cs.csr)
        coeff_mont = False
    if not (1 <= ni <= nv) or nc < 0:
        raise ValueError("need 1 <= num_inputs <= num_vars")
    log_m = max(nc + ni - 1, 0).bit_length()          # D::new(num_constraints + num_inputs).size()
    if log_m + 1 > TWO_ADICITY[curve] or log_m > 26:
        raise ValueError("domain larger than the field's 2-adic subgroup")
    csr = [_check_csr(n, m, nc, nv) for n, m in zip("abc", csr)]
    given = trapdoor is not None
    td = _trapdoor_array(curve, trapdoor if given else draw_trapdoor(curve))
    return dict(nc=nc, ni=ni, nv=nv, log_m=log_m, csr=csr, coeff_mont=coeff_mont, trapdoor=td, trapdoor_given=given)


class Parameters:
    """The generated key as device arrays (torch uint8 tensors, affine points, identity = zero bytes):
    a_query, b_g1_query, b_g2_query, h_query, l_query, fixed_points (alpha_g1 | beta_g1 | delta_g1 | beta_g2 |
    delta_g2), gamma_g2, gamma_abc_g1."""

    NAMES = ("a_query", "b_g1_query", "b_g2_query", "h_query", "l_query", "fixed_points", "gamma_g2", "gamma_abc_g1")

    def __init__(self, curve, nc, ni, nv, log_m, arrays, trapdoor=None):
        self.curve, self.num_constraints, self.num_inputs, self.num_vars = curve, nc, ni, nv
        self.log_m, self.domain_size = log_m, 1 << log_m
        self.trapdoor = trapdoor
        for n, t in zip(self.NAMES, arrays):
            setattr(self, n, t)

    def proving_key(self, ctx, shard=0, n_shards=1, h_cyclic=False):
        """Resident proving key over the device arrays (no host round trip)."""
        return ctx.pk_create(self.curve, self.num_vars, self.num_inputs, self.domain_size, self.a_query.data_ptr(),
                             self.b_g1_query.data_ptr(), self.b_g2_query.data_ptr(), self.h_query.data_ptr(),
                             self.l_query.data_ptr(), self.fixed_points.data_ptr(), device_ptrs=True, shard=shard,
                             n_shards=n_shards, h_cyclic=h_cyclic)

    def host(self, name):
        """One array as numpy uint64 [points][limbs]."""
        fq = _lib.FQ_LIMBS64[self.curve]
        cols = {"b_g2_query": 4 * fq, "gamma_g2": 4 * fq, "fixed_points": fq}.get(name, 2 * fq)
        return getattr(self, name).cpu().numpy().view(np.uint64).reshape(-1, cols)

    def verifying_key(self):
        """(alpha_g1, beta_g2, gamma_g2, delta_g2, ic): the first five arguments of verify.verify_proof."""
        fq = _lib.FQ_LIMBS64[self.curve]
        f = self.host("fixed_points").reshape(-1)
        g2 = f[6 * fq:]
        return f[:2 * fq].copy(), g2[:4 * fq].copy(), self.host("gamma_g2").reshape(-1), g2[4 * fq:].copy(), \
            self.host("gamma_abc_g1")


def generate_parameters(ctx, curve, r1cs, trapdoor=None, generators=None, reduction="circom"):
    """ctx: a Context (None: one is made on device 0 -- without a GPU that raises Dg16Error, there is no CPU path).
    generators: None, or (g1 affine, g2 affine) as uint64 arrays.  reduction: "circom" (CircomReduction, the snarkjs
    h_query) or "libsnark" (ark-groth16's default LibsnarkReduction: h_query[i] = tau^i Z(tau) / delta, the last entry
    the identity); prove with the same reduction.  Returns Parameters."""
    _lib._reduction_flag(reduction)
    p = prepare(curve, r1cs, trapdoor)
    if ctx is None:
        ctx = _lib.Context(0)
    import torch
    dev = torch.device("cuda", ctx.device)
    nc, ni, nv, log_m = p["nc"], p["ni"], p["nv"], p["log_m"]

    def up(x, dtype):
        if _is_tensor(x):
            return x
        x = np.ascontiguousarray(x, dtype=dtype)
        if x.size == 0:
            return torch.zeros(16, dtype=torch.uint8, device=dev)
        return torch.from_numpy(x.view(np.uint8).reshape(-1)).to(dev)

    mats = []
    for ptr, col, coeff in p["csr"]:
        d = (up(ptr, np.uint32), up(col, np.uint32), up(coeff, np.uint64))
        if not p["coeff_mont"]:
            nnz = d[2].numel() * d[2].element_size() // 32
            if _is_tensor(coeff):
                d = (d[0], d[1], d[2].clone())
            torch.cuda.synchronize(dev)
            ctx.field_op_dev(curve, "fr", 5, d[2].data_ptr(), None, d[2].data_ptr(), nnz)      # to Montgomery form
        mats.append(d)
    fqb = 8 * _lib.FQ_LIMBS64[curve]
    g1b, g2b = 2 * fqb, 4 * fqb
    sizes = (nv * g1b, nv * g1b, nv * g2b, (1 << log_m) * g1b, (nv - ni) * g1b, 3 * g1b + 2 * g2b, g2b, ni * g1b)
    arrays = [torch.empty(max(s, 16), dtype=torch.uint8, device=dev)[:s] for s in sizes]
    gens = None
    if generators is not None:
        gens = np.concatenate([np.ascontiguousarray(g, dtype=np.uint64).reshape(-1) for g in generators])
        if gens.size * 8 != g1b + g2b:
            raise ValueError("generators = (g1 affine, g2 affine)")
    torch.cuda.synchronize(dev)        # the uploads ran on torch's stream, the generator runs on the library's
    ctx.sync(0)
    ctx.groth16_setup(curve, nc, ni, nv, log_m, *[[t.data_ptr() for t in m] for m in mats], p["trapdoor"],
                      [t.data_ptr() for t in arrays], generators=gens, device_ptrs=True, reduction=reduction)
    params = Parameters(curve, nc, ni, nv, log_m, arrays, trapdoor=tuple(trapdoor) if p["trapdoor_given"] else None)
    params.reduction = reduction
    return params


class Srs:
    """A structured reference string for the domain of size 2^log_m, as `dg16_groth16_setup_srs` takes it: lag_g1,
    lag_g2, alpha_lag_g1, beta_lag_g1, h_g1 -- 2^log_m affine points each (numpy uint64 arrays, or device tensors; identity
    = zeros) -- and fixed = alpha_g1 | beta_g1 | g1 | beta_g2 | g2 (host array).  include/dg16.h names the sections of a
    prepared .ptau file they come from.  The points must be on their curves and of order r: nothing here checks that."""

    ARRAYS = ("lag_g1", "lag_g2", "alpha_lag_g1", "beta_lag_g1", "h_g1")

    def __init__(self, curve, log_m, lag_g1, lag_g2, alpha_lag_g1, beta_lag_g1, h_g1, fixed, reduction=None):
        self.curve, self.log_m, self.reduction = curve, log_m, reduction
        self.lag_g1, self.lag_g2, self.alpha_lag_g1, self.beta_lag_g1, self.h_g1 = \
            lag_g1, lag_g2, alpha_lag_g1, beta_lag_g1, h_g1
        self.fixed = np.ascontiguousarray(fixed, dtype=np.uint64).reshape(-1)
        fq = _lib.FQ_LIMBS64[curve]
        if self.fixed.size != 3 * 2 * fq + 2 * 4 * fq:
            raise ValueError("fixed = alpha_g1 | beta_g1 | g1 | beta_g2 | g2")


def _ints_to_arr(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def srs_scalars(ctx, curve, log_m, tau, reduction="circom"):
    """(u, h) as canonical uint64 [m][4] arrays, made the way dg16_groth16_setup makes them, with delta = 1:
    u_i = L_i(tau) is the inverse NTT of [tau^j]; h is, for "circom", the odd-indexed entries of the inverse NTT of size
    2m of [tau^j]_{j < 2m - 1} | 0 and, for "libsnark", tau^i Z(tau) for i < m - 1, then 0."""
    _lib._reduction_flag(reduction)
    r = FR_MODULUS[curve]
    m = 1 << log_m
    pw = [1] * (2 * m)
    for j in range(1, 2 * m):
        pw[j] = pw[j - 1] * tau % r
    u = ctx.ntt(curve, _ints_to_arr(pw[:m]), inverse=True)
    if reduction == "libsnark":
        z = (pw[m] - 1) % r
        h = _ints_to_arr([pw[i] * z % r for i in range(m - 1)] + [0])
    else:
        h = ctx.ntt(curve, _ints_to_arr(pw[:2 * m - 1] + [0]), inverse=True)[1::2].copy()
    return u, h


def srs_from_trapdoor(ctx, curve, log_m, alpha, beta, tau, reduction="circom"):
    """FOR TESTS AND BENCHMARKS ONLY: the reference string a ceremony with the KNOWN secrets alpha, beta, tau would
    publish, over the standard generators.  A key made from it is as worthless as its trapdoor is public; a real one
    comes from a ceremony's output.  The five arrays are dg16_fixed_base_mul products of the scalars of srs_scalars
    (which stay on the result as `u` and `h`, canonical, for a test to check).  Host arrays."""
    r = FR_MODULUS[curve]
    alpha, beta, tau = int(alpha), int(beta), int(tau)
    if any(not 0 < x < r for x in (alpha, beta, tau)) or pow(tau, 1 << log_m, r) == 1:
        raise ValueError("alpha, beta, tau must be non-zero and below r, tau outside the domain")
    if log_m + 1 > TWO_ADICITY[curve] or log_m > 26:
        raise ValueError("domain larger than the field's 2-adic subgroup")
    u, h = srs_scalars(ctx, curve, log_m, tau, reduction)
    ab = ctx.fixed_base_mul(curve, 1, _ints_to_arr([alpha, beta, 1]))
    b2 = ctx.fixed_base_mul(curve, 2, _ints_to_arr([beta, 1]))
    srs = Srs(curve, log_m, ctx.fixed_base_mul(curve, 1, u), ctx.fixed_base_mul(curve, 2, u),
              ctx.fixed_base_mul(curve, 1, u, base=ab[0]), ctx.fixed_base_mul(curve, 1, u, base=ab[1]),
              ctx.fixed_base_mul(curve, 1, h), np.concatenate([ab.reshape(-1), b2.reshape(-1)]), reduction=reduction)
    srs.u, srs.h = u, h
    return srs


def powers_from_trapdoor(ctx, curve, log_m, alpha, beta, tau):
    """FOR TESTS AND BENCHMARKS ONLY, like srs_from_trapdoor: the monomial powers a ceremony with the KNOWN secrets alpha,
    beta, tau would publish over the standard generators, as dg16_fixed_base_mul products of tau^j.
    -> (tau_g1 [2m - 1], tau_g2 [m], alpha_tau_g1 [m], beta_tau_g1 [m], beta_g2 [1]), host arrays."""
    r = FR_MODULUS[curve]
    alpha, beta, tau = int(alpha), int(beta), int(tau)
    if any(not 0 < x < r for x in (alpha, beta, tau)):
        raise ValueError("alpha, beta, tau must be non-zero and below r")
    if log_m + 1 > TWO_ADICITY[curve] or log_m > 26:
        raise ValueError("domain larger than the field's 2-adic subgroup")
    m = 1 << log_m
    pw = [1] * (2 * m - 1)
    for j in range(1, 2 * m - 1):
        pw[j] = pw[j - 1] * tau % r
    ab = ctx.fixed_base_mul(curve, 1, _ints_to_arr([alpha, beta]))
    first = _ints_to_arr(pw[:m])
    return (ctx.fixed_base_mul(curve, 1, _ints_to_arr(pw)), ctx.fixed_base_mul(curve, 2, first),
            ctx.fixed_base_mul(curve, 1, first, base=ab[0]), ctx.fixed_base_mul(curve, 1, first, base=ab[1]),
            ctx.fixed_base_mul(curve, 2, _ints_to_arr([beta])))


def srs_from_powers(ctx, curve, log_m, tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, beta_g2, reduction="circom"):
    """The reference string of the domain of size 2^log_m from a ceremony's monomial powers (`dg16_srs_prepare`): host
    arrays tau_g1 [2m - 1] G1, tau_g2 [m] G2, alpha_tau_g1 and beta_tau_g1 [m] G1, beta_g2 one G2 point, in this
    library's affine Montgomery layout.  reduction names the QAP reduction the h basis is made for; it is recorded on
    the result.  The points must be on their curves and of order r: nothing here checks that.  Returns an Srs of host
    arrays."""
    _lib._reduction_flag(reduction)
    if curve not in FR_MODULUS:
        raise ValueError("unknown curve %r" % (curve,))
    if log_m + 1 > TWO_ADICITY[curve] or log_m > 26:
        raise ValueError("domain larger than the field's 2-adic subgroup")
    out = ctx.srs_prepare(curve, log_m, tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, beta_g2, reduction=reduction)
    return Srs(curve, log_m, *out, reduction=reduction)


class SrsReport:
    """What `verify_powers` found: `.accepted`, the word `.failed` (0 = accepted) and a name per bit of it, the bits of
    dg16_srs_report in include/dg16.h.  With BAD_POINT: `.bad_array` (the name of the first array that holds a bad point),
    `.bad_index` (the smallest bad index in it) and `.n_bad_points` (over all five arrays).  `.generators_match` is None
    unless `verify_powers` was given generators to compare with."""

    BAD_POINT, IDENTITY, TAU_G1, TAU_G2, ALPHA, BETA, BETA_G2 = 1, 2, 4, 8, 16, 32, 64
    NAMES = {1: "bad_point", 2: "identity", 4: "tau_g1", 8: "tau_g2", 16: "alpha", 32: "beta", 64: "beta_g2"}
    ARRAYS = ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2")

    def __init__(self, failed, bad_array=0, bad_index=0, n_bad_points=0, generators_match=None):
        self.failed = int(failed)
        self.n_bad_points = int(n_bad_points)
        self.bad_array = self.ARRAYS[bad_array] if self.failed & self.BAD_POINT else None
        self.bad_index = int(bad_index) if self.failed & self.BAD_POINT else None
        self.generators_match = generators_match
        for bit, name in self.NAMES.items():
            setattr(self, name, bool(self.failed & bit))

    @property
    def accepted(self):
        return self.failed == 0 and self.generators_match is not False

    @property
    def reasons(self):
        return [name for bit, name in self.NAMES.items() if self.failed & bit]

    def __repr__(self):
        return "SrsReport(accepted=%r, failed=%d %r)" % (self.accepted, self.failed, self.reasons)


def verify_powers(ctx, curve, log_m, tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, beta_g2, coeffs=None, generators=None):
    """Is this the output of a powers-of-tau ceremony (`dg16_srs_verify`; snarkjs' `powersoftau verify` without the
    contribution chain)?  The arrays are those of `srs_from_powers`, which trusts them: verify first.  Every point must
    be reduced, on its curve and of order r; the seven head points must not be the identity; and tau_g1, tau_g2,
    alpha_tau_g1, beta_tau_g1 must be geometric progressions in one tau, beta_g2 holding beta_tau_g1's beta -- each
    decided by one pairing equation on a random linear combination.  coeffs: uint64 [2m - 2][2], independent and uniform
    in [1, 2^128) and drawn AFTER the transcript was fixed; None draws them with `verify.random_coefficients`.  A
    transcript that fails an equation is then accepted with probability about 2^-128.  generators = (g1, g2) packed
    affine points: tau_g1[0] and tau_g2[0] are also compared with them (a byte comparison), and a difference makes
    `.accepted` False.  BN254 and BLS12-381.  Returns an SrsReport."""
    if curve not in FR_MODULUS:
        raise ValueError("unknown curve %r" % (curve,))
    if coeffs is None:
        from .verify import random_coefficients
        coeffs = random_coefficients(2 * (1 << log_m) - 2)
    rep = ctx.srs_verify(curve, log_m, tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, beta_g2, coeffs)
    match = None
    if generators is not None:
        g1 = np.ascontiguousarray(generators[0], dtype=np.uint64).reshape(-1)
        g2 = np.ascontiguousarray(generators[1], dtype=np.uint64).reshape(-1)
        t = np.ascontiguousarray(tau_g1, dtype=np.uint64).reshape(-1)
        u = np.ascontiguousarray(tau_g2, dtype=np.uint64).reshape(-1)
        match = bool(np.array_equal(t[:g1.size], g1) and np.array_equal(u[:g2.size], g2))
    return SrsReport(*rep, generators_match=match)


def contribute_powers(ctx, curve, log_m, powers, tau, alpha, beta, blinds=None, challenge=None):
    """One phase-1 contribution to a powers-of-tau transcript (`dg16_srs_contribute`; snarkjs' `powersoftau contribute`
    without its hashes).  powers = (tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, beta_g2), the host arrays of
    `srs_from_powers`; entry j of the first four is multiplied by tau^j (and by alpha, by beta), beta_g2 by beta.  THE
    RANDOMNESS IS THE CALLER'S: tau, alpha, beta are ints in [1, r), uniform, and to be forgotten afterwards -- the
    transcript is sound as long as ONE contributor did.  The caller vouches that the transcript's points have order r:
    `verify_powers` first.  blinds = (s_tau, s_alpha, s_beta), ints in [1, r), and challenge = three G2 affine points
    (uint64 [3][4 fq]; how they follow from the previous transcript is the caller's protocol) make the proof of
    knowledge: key = s_x G | s_x x G | x SP_x per secret as one uint64 array, G = tau_g1[0]; without them no key is
    made.  Returns (powers', key or None)."""
    if curve not in FR_MODULUS:
        raise ValueError("unknown curve %r" % (curve,))
    r = FR_MODULUS[curve]
    secrets_ = [int(x) for x in (tau, alpha, beta)]
    if any(not 0 < x < r for x in secrets_):
        raise ValueError("tau, alpha, beta must be non-zero and below r")
    if log_m + 1 > TWO_ADICITY[curve] or log_m > 26:
        raise ValueError("domain larger than the field's 2-adic subgroup")
    if (blinds is None) != (challenge is None):
        raise ValueError("blinds and challenge come together")
    if blinds is not None:
        blinds = [int(x) for x in blinds]
        if len(blinds) != 3 or any(not 0 < x < r for x in blinds):
            raise ValueError("blinds = (s_tau, s_alpha, s_beta), non-zero and below r")
    return ctx.srs_contribute(curve, log_m, powers, secrets_, blinds=blinds, challenge_g2=challenge)


class Phase1Report:
    """What `verify_powers_contribution` found: `.accepted`, the word `.failed` (0 = accepted) and a name per bit of it,
    the bits of dg16_srs_contribution_report in include/dg16.h.  `.after` is the SrsReport of the new transcript (bit
    `after` is set when it is not clean); `.n_bad_points` counts the bad points among the key, the challenge and the
    heads of the old transcript."""

    AFTER, BAD_POINT, IDENTITY, BASE = 1, 2, 4, 8
    KEY_TAU, KEY_ALPHA, KEY_BETA = 16, 32, 64
    LINK_TAU_G1, LINK_TAU_G2, LINK_ALPHA, LINK_BETA, LINK_BETA_G2 = 128, 256, 512, 1024, 2048
    NAMES = {1: "after", 2: "bad_point", 4: "identity", 8: "base", 16: "key_tau", 32: "key_alpha", 64: "key_beta",
             128: "link_tau_g1", 256: "link_tau_g2", 512: "link_alpha", 1024: "link_beta", 2048: "link_beta_g2"}

    def __init__(self, failed, n_bad_points=0, after=None):
        self.failed = int(failed)
        self.n_bad_points = int(n_bad_points)
        self.after = after if isinstance(after, SrsReport) else SrsReport(*(after or (0,)))
        for bit, name in self.NAMES.items():
            if name != "after":
                setattr(self, name, bool(self.failed & bit))

    @property
    def accepted(self):
        return self.failed == 0

    @property
    def reasons(self):
        return [name for bit, name in self.NAMES.items() if self.failed & bit]

    def __repr__(self):
        return "Phase1Report(accepted=%r, failed=%d %r)" % (self.accepted, self.failed, self.reasons)


def verify_powers_contribution(ctx, curve, log_m, before, after, key, challenge, coeffs=None):
    """Is the transcript `after` a contribution to `before` by whoever holds `key` (`dg16_srs_verify_contribution`; the
    contribution part of snarkjs' `powersoftau verify`)?  before, after: five host arrays each, as for `verify_powers`;
    `after` is checked in full the way `verify_powers` checks it, of `before` only the head points are read.  key: what
    `contribute_powers` returned; challenge: the three G2 points the contributor was given.  The key must prove
    knowledge of tau, alpha, beta under the challenge, and the heads of `after` must be those of `before` moved by
    exactly these -- eight pairing equations.  coeffs: as for `verify_powers`, drawn AFTER `after` was fixed; None draws
    them.  Not checked: that the challenge is the hash of `before` -- the caller's protocol.  BN254 and BLS12-381.
    Returns a Phase1Report."""
    if curve not in FR_MODULUS:
        raise ValueError("unknown curve %r" % (curve,))
    if coeffs is None:
        from .verify import random_coefficients
        coeffs = random_coefficients(2 * (1 << log_m) - 2)
    failed, n_bad, rep = ctx.srs_verify_contribution(curve, log_m, before, after, key, challenge, coeffs)
    return Phase1Report(failed, n_bad, rep)


def generate_parameters_from_srs(ctx, curve, r1cs, srs, reduction="circom", in_subgroup=False):
    """The key of `r1cs` from a structured reference string (an Srs for the domain of the system: log_m must match), in
    the exponent: gamma = delta = 1 and no trapdoor anywhere.  reduction names the QAP reduction srs.h_g1 was made for
    (it is recorded on the result; prove with the same one).  in_subgroup=True passes DG16_F_BASES_IN_SUBGROUP: the
    caller vouches that every point of the string has order r, and the coefficients may then be split with the curve's
    endomorphism.  Returns Parameters (trapdoor None); proving_key() and verifying_key() work as for generate_parameters."""
    _lib._reduction_flag(reduction)
    if srs.reduction is not None and srs.reduction != reduction:
        raise ValueError("the reference string's h basis was made for reduction %r" % (srs.reduction,))
    p = prepare(curve, r1cs, trapdoor=(1, 1, 1, 1, 2))       # shapes and CSR validation only: no trapdoor is used
    if srs.curve != curve or srs.log_m != p["log_m"]:
        raise ValueError("the reference string is for %s, 2^%d; the system needs %s, 2^%d"
                         % (srs.curve, srs.log_m, curve, p["log_m"]))
    if ctx is None:
        ctx = _lib.Context(0)
    import torch
    dev = torch.device("cuda", ctx.device)
    nc, ni, nv, log_m = p["nc"], p["ni"], p["nv"], p["log_m"]
    m = 1 << log_m

    def up(x, dtype=np.uint64):
        if _is_tensor(x):
            return x
        x = np.ascontiguousarray(x, dtype=dtype)
        if x.size == 0:
            return torch.zeros(16, dtype=torch.uint8, device=dev)
        return torch.from_numpy(x.view(np.uint8).reshape(-1)).to(dev)

    mats = []
    for ptr, col, coeff in p["csr"]:
        d = (up(ptr, np.uint32), up(col, np.uint32), up(coeff))
        if not p["coeff_mont"]:
            nnz = d[2].numel() * d[2].element_size() // 32
            if _is_tensor(coeff):
                d = (d[0], d[1], d[2].clone())
            torch.cuda.synchronize(dev)
            ctx.field_op_dev(curve, "fr", 5, d[2].data_ptr(), None, d[2].data_ptr(), nnz)      # to Montgomery form
        mats.append(d)
    fqb = 8 * _lib.FQ_LIMBS64[curve]
    g1b, g2b = 2 * fqb, 4 * fqb
    tabs = [up(getattr(srs, n)) for n in Srs.ARRAYS]
    for t, n, b in zip(tabs, Srs.ARRAYS, (g1b, g2b, g1b, g1b, g1b)):
        if t.numel() * t.element_size() != m * b:
            raise ValueError("srs.%s must hold 2^%d points" % (n, log_m))
    sizes = (nv * g1b, nv * g1b, nv * g2b, m * g1b, (nv - ni) * g1b, 3 * g1b + 2 * g2b, g2b, ni * g1b)
    arrays = [torch.empty(max(s, 16), dtype=torch.uint8, device=dev)[:s] for s in sizes]
    torch.cuda.synchronize(dev)        # the uploads ran on torch's stream, the generator runs on the library's
    ctx.sync(0)
    ctx.groth16_setup_srs(curve, nc, ni, nv, log_m, *[[t.data_ptr() for t in mt] for mt in mats],
                          [t.data_ptr() for t in tabs] + [srs.fixed], [t.data_ptr() for t in arrays], device_ptrs=True,
                          in_subgroup=in_subgroup)
    params = Parameters(curve, nc, ni, nv, log_m, arrays, trapdoor=None)
    params.reduction = reduction
    return params


def contribute(ctx, params, delta):
    """One phase-2 contribution to a key (`dg16_groth16_contribute`; snarkjs' `zkey contribute` without its transcript):
    l_query and h_query are divided by d = delta, delta_g1 and delta_g2 multiplied by it, every other array is shared
    with `params`.  THE RANDOMNESS IS THE CALLER'S: delta is an int in [1, r), uniform, and to be forgotten afterwards --
    the key is sound as long as ONE contributor did.  The caller vouches that the key's points have order r.  The three
    arrays go through the host (`.host()`) and are uploaded again.  Returns new Parameters with `reduction` kept and
    trapdoor None."""
    import torch
    curve = params.curve
    delta = int(delta)
    if not 0 < delta < FR_MODULUS[curve]:
        raise ValueError("delta must be non-zero and below r")
    l, h, f = ctx.groth16_contribute(curve, params.host("l_query"), params.host("h_query"),
                                     params.host("fixed_points").reshape(-1), delta)
    dev = params.fixed_points.device

    def up(x):
        if x.size == 0:
            return torch.zeros(16, dtype=torch.uint8, device=dev)[:0]
        return torch.from_numpy(x.view(np.uint8).reshape(-1)).to(dev)

    new = {"l_query": up(l), "h_query": up(h), "fixed_points": up(f)}
    arrays = [new.get(n, getattr(params, n)) for n in Parameters.NAMES]
    out = Parameters(curve, params.num_constraints, params.num_inputs, params.num_vars, params.log_m, arrays,
                     trapdoor=None)
    out.reduction = getattr(params, "reduction", None)
    return out


class Phase2Report:
    """What `verify_contribution` found: `.accepted`, the word `.failed` (0 = accepted) and a name per bit of it, the
    bits of dg16_phase2_report in include/dg16.h.  With BAD_POINT: `.bad_array` (the name of the first array that holds a
    bad point), `.bad_index` (the smallest bad index in it) and `.n_bad_points` (over all eight arrays)."""

    BAD_POINT, IDENTITY, CHANGED, DELTA, L, H = 1, 2, 4, 8, 16, 32
    NAMES = {1: "bad_point", 2: "identity", 4: "changed", 8: "delta", 16: "l", 32: "h"}
    ARRAYS = ("before.l_query", "before.h_query", "before.delta_g1", "before.delta_g2",
              "after.l_query", "after.h_query", "after.delta_g1", "after.delta_g2")

    def __init__(self, failed, bad_array=0, bad_index=0, n_bad_points=0):
        self.failed = int(failed)
        self.n_bad_points = int(n_bad_points)
        self.bad_array = self.ARRAYS[bad_array] if self.failed & self.BAD_POINT else None
        self.bad_index = int(bad_index) if self.failed & self.BAD_POINT else None
        for bit, name in self.NAMES.items():
            setattr(self, name, bool(self.failed & bit))

    @property
    def accepted(self):
        return self.failed == 0

    @property
    def reasons(self):
        return [name for bit, name in self.NAMES.items() if self.failed & bit]

    def __repr__(self):
        return "Phase2Report(accepted=%r, failed=%d %r)" % (self.accepted, self.failed, self.reasons)


def verify_contribution(ctx, before, after, coeffs=None):
    """Is `after` the key `before` with delta replaced by d * delta for some d (`dg16_groth16_verify_contribution`)?  Both
    are Parameters of the same system.  Every point of l_query, h_query, delta_g1, delta_g2 of both keys must be
    reduced, on its curve and of order r; no delta may be the identity; the arrays a contribution leaves alone must be
    byte-equal; and the deltas, l_query and h_query must have moved by one d -- each decided by one pairing equation,
    the last two on a random linear combination.  coeffs: uint64 [max(num_vars - num_inputs, domain_size)][2],
    independent and uniform in [1, 2^128) and drawn AFTER both keys were fixed; None draws them with
    `verify.random_coefficients`.  A key that fails an equation is then accepted with probability about 2^-128.  Not
    checked: a contributor's proof of knowledge and a transcript's hash chain.  BN254 and BLS12-381.  Returns a
    Phase2Report."""
    shape = lambda p: (p.curve, p.num_inputs, p.num_vars, p.domain_size)      # noqa: E731
    if shape(before) != shape(after):
        raise ValueError("the keys are of different systems: %r, %r" % (shape(before), shape(after)))
    if coeffs is None:
        from .verify import random_coefficients
        coeffs = random_coefficients(max(before.num_vars - before.num_inputs, before.domain_size))
    keys = [[p.host(n).reshape(-1) for n in Parameters.NAMES] for p in (before, after)]
    return Phase2Report(*ctx.groth16_verify_contribution(before.curve, before.num_inputs, before.num_vars,
                                                         before.domain_size, keys[0], keys[1], coeffs))


def verify_parameters(ctx, curve, r1cs, srs, params, reduction="circom", coeffs=None):
    """Is `params` a key of THIS R1CS over THIS reference string (the key part of snarkjs' `zkey verify`)?  The
    uncontributed key is computed again (`generate_parameters_from_srs`, in_subgroup as the caller of that would pass
    for a verified string: False here, the plain loops) and `params` is held against it with `verify_contribution`;
    the relation is transitive in d, so any number of contributions is covered.  Returns a Phase2Report."""
    initial = generate_parameters_from_srs(ctx, curve, r1cs, srs, reduction=reduction)
    return verify_contribution(ctx, initial, params, coeffs=coeffs)
