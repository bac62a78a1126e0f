"""GPU: dg16_group_ntt (Context.group_ntt) and dg16_srs_prepare (Context.srs_prepare, keygen.srs_from_powers).  Expected
values come from the oracle alone: corc.ntt on the scalars and corc.point_mul / corc.msm for the points; the prepared
reference string is also compared, byte for byte, with the one keygen.srs_from_trapdoor makes from the same secrets by
another route (scalar NTT, then fixed-base products)."""

import ctypes
import functools
import random

import numpy as np
import pytest

from oracle import corc
from oracle.pyref.fields import FQ, FR
from oracle.pyref import groth16 as G
from gpu_util import ctx
from test_gpu_prover import enc_fr, enc_g1, enc_g2
from test_gpu_setup import system_of
from test_gpu_setup_srs import lagrange_at, oracle_key, trapdoor

pytestmark = pytest.mark.gpu

ALL = ["bn254", "bls12_381", "bls12_377"]
GROUPS = [(c, g) for c in ALL for g in (1, 2)]
LOGS = [0, 1, 2, 3, 6, 7, 8]           # 2^7: one full wave of butterflies; 2^8: the first size with two


def _mont(curve, ks):
    return corc.field_op(curve, "fr", "to_mont", corc.ints_to_arr(ks, 4))


def _ntt_ints(curve, ks, inverse):
    return corc.arr_to_ints(corc.field_op(curve, "fr", "from_mont", corc.ntt(curve, _mont(curve, ks), inverse=inverse)))


def _multiples(curve, group, base, ks):
    return np.concatenate([corc.point_mul(curve, group, base, k) for k in ks])


@functools.lru_cache(maxsize=None)
def _inputs(curve, group):
    """256 scalars (a zero and a repeated value among them) and the points s_j G, made once per group"""
    rng = random.Random(100 + 2 * corc.CURVES[curve] + group)
    r = FR[curve].p
    ks = [rng.randrange(r) for _ in range(256)]
    ks[1], ks[5] = 0, ks[4]
    return ks, _multiples(curve, group, corc.generator(curve, group), ks)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("log_n", LOGS)
@pytest.mark.parametrize("curve,group", GROUPS)
def test_multiples_of_the_generator_transform_like_their_scalars(curve, group, log_n, inverse):
    ks, pts = _inputs(curve, group)
    n = 1 << log_n
    exp = _multiples(curve, group, corc.generator(curve, group), _ntt_ints(curve, ks[:n], inverse))
    got = ctx().group_ntt(curve, group, pts[:n], inverse=inverse)
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("curve,group", GROUPS)
def test_random_subgroup_points_against_the_dft_rows(curve, group):
    """n = 8, points without a known discrete logarithm: out[i] = msm(P, [w^(i j)]_j), and n^-1 w^(-i j) for the inverse."""
    r = FR[curve].p
    n = 8
    pts = corc.gen_points(curve, group, 77, n)
    w = corc.arr_to_ints(corc.field_op(curve, "fr", "from_mont", corc.root_of_unity(curve, 3)))[0]
    assert pow(w, 8, r) == 1 and pow(w, 4, r) == r - 1
    for inverse in (False, True):
        base = pow(w, r - 2, r) if inverse else w
        scale = pow(n, r - 2, r) if inverse else 1
        exp = np.concatenate([corc.msm(curve, group, pts, corc.ints_to_arr([pow(base, i * j, r) * scale % r for j in range(n)], 4))
                              for i in range(n)])
        assert np.array_equal(ctx().group_ntt(curve, group, pts, inverse=inverse), exp), inverse


def _structured(curve, n):
    r = FR[curve].p
    rng = random.Random(9)
    third = [0 if j % 3 == 0 else rng.randrange(1, r) for j in range(n)]
    return {"all equal": [1] * n, "one point": [1] + [0] * (n - 1), "P, -P alternating": [1, r - 1] * (n // 2),
            "identities at a third": third}


@pytest.mark.parametrize("name", ["all equal", "one point", "P, -P alternating", "identities at a third"])
@pytest.mark.parametrize("curve,group", [("bn254", 1), ("bls12_377", 2)])
def test_structured_inputs(curve, group, name):
    """n = 64 inputs s_j P for a random subgroup point P: a + a, a - a and identity operands in every stage."""
    n = 64
    r = FR[curve].p
    p = corc.gen_points(curve, group, 13, 1)
    ks = _structured(curve, n)[name]
    pts = _multiples(curve, group, p, ks)
    for inverse in (False, True):
        t = _ntt_ints(curve, ks, inverse)
        if name == "all equal":
            assert t == [1 if inverse else n] + [0] * (n - 1)
        if name == "P, -P alternating":
            assert [i for i, v in enumerate(t) if v] == [n // 2]
        if name == "one point":
            assert len(set(t)) == 1 and t[0] == (pow(n, r - 2, r) if inverse else 1)
        got = ctx().group_ntt(curve, group, pts, inverse=inverse)
        assert np.array_equal(got, _multiples(curve, group, p, t)), inverse


def test_slices_do_not_change_the_result_and_the_inverse_undoes_the_transform():
    """log_n = 9, BLS12-381 G1: slices of 64 and 192 butterflies against the default (one launch per kind and stage)."""
    curve, group = "bls12_381", 1
    x = corc.gen_points(curve, group, 5, 512)
    c_ = ctx()
    ref = c_.group_ntt(curve, group, x)
    assert np.array_equal(c_.group_ntt(curve, group, ref, inverse=True), x)
    try:
        for slc in (64, 192):
            c_.set_points_mul_slice(slc)
            got = c_.group_ntt(curve, group, x)
            assert np.array_equal(got, ref), slc
            assert np.array_equal(c_.group_ntt(curve, group, got, inverse=True), x), slc
    finally:
        c_.set_points_mul_slice(0)


# ---- srs_prepare -----------------------------------------------------------------------------------------------------
SRS_NAMES = ("lag_g1", "lag_g2", "alpha_lag_g1", "beta_lag_g1", "h_g1", "fixed")


def _prepared_both_ways(curve, log_m, alpha, beta, tau, reduction):
    import dg16_amd
    powers = dg16_amd.powers_from_trapdoor(ctx(), curve, log_m, alpha, beta, tau)
    got = dg16_amd.srs_from_powers(ctx(), curve, log_m, *powers, reduction=reduction)
    want = dg16_amd.srs_from_trapdoor(ctx(), curve, log_m, alpha, beta, tau, reduction=reduction)
    assert got.reduction == reduction and got.log_m == log_m and got.curve == curve
    return got, want


@pytest.mark.parametrize("reduction", ["circom", "libsnark"])
@pytest.mark.parametrize("log_m", [3, 6])
@pytest.mark.parametrize("curve", ALL)
def test_prepared_string_equals_the_one_made_from_the_trapdoor(curve, log_m, reduction):
    td = trapdoor(curve, log_m)
    got, want = _prepared_both_ways(curve, log_m, td[0], td[1], td[4], reduction)
    for name in SRS_NAMES:
        assert np.array_equal(np.asarray(getattr(got, name)).reshape(-1), np.asarray(getattr(want, name)).reshape(-1)), name
    if (curve, log_m, reduction) == ("bls12_381", 3, "circom"):
        # ... and against the oracle directly: L_i(tau) G from Python integers
        lag = lagrange_at(FR[curve], 1 << log_m, td[4])
        assert np.array_equal(got.lag_g1, _multiples(curve, 1, corc.generator(curve, 1), lag))


@pytest.mark.parametrize("curve", ["bn254", "bls12_377"])
def test_tau_inside_the_doubled_domain(curve):
    """tau = w_2m^3 lies inside the doubled domain: tau^m = -1, so the difference stage meets p_j - p_(j+m) = 2 p_j and
    the size-2m Lagrange basis at tau is one 1 among zeros.  The h basis is the transform of the 2m - 1 published powers
    and the identity, NOT of all 2m powers, so it is that unit vector less the share of the missing power tau^(2m-1):
    h_i = [i = 1] - tau^(2m-1) w_2m^(-(2i+1)(2m-1)) / 2m.  Checked against the string from the trapdoor and against
    these integers through the oracle."""
    log_m = 3
    m = 1 << log_m
    r = FR[curve].p
    w2m = corc.arr_to_ints(corc.field_op(curve, "fr", "from_mont", corc.root_of_unity(curve, log_m + 1)))[0]
    tau = pow(w2m, 3, r)
    assert pow(tau, m, r) == r - 1
    td = trapdoor(curve, 21)
    got, want = _prepared_both_ways(curve, log_m, td[0], td[1], tau, "circom")
    for name in SRS_NAMES:
        assert np.array_equal(np.asarray(getattr(got, name)).reshape(-1), np.asarray(getattr(want, name)).reshape(-1)), name
    winv, ninv = pow(w2m, r - 2, r), pow(2 * m, r - 2, r)
    h = [sum(pow(winv, (2 * i + 1) * j, r) * pow(tau, j, r) for j in range(2 * m - 1)) * ninv % r for i in range(m)]
    last = pow(tau, 2 * m - 1, r)
    assert h == [((1 if i == 1 else 0) - last * pow(winv, (2 * i + 1) * (2 * m - 1), r) * ninv) % r for i in range(m)]
    assert np.array_equal(got.h_g1, _multiples(curve, 1, corc.generator(curve, 1), h))


def test_powers_to_a_verified_proof():
    """BN254: powers -> srs_from_powers -> generate_parameters_from_srs -> proving key -> prove -> verify_batch; the proof
    equals the oracle's under (alpha, beta, 1, 1, tau), is accepted, and is rejected under a changed public input."""
    import dg16_amd
    curve, log_m = "bn254", 6
    F, Fq = FR[curve], FQ[curve]
    p = F.p
    r1cs, w, td, pk = oracle_key(curve, log_m)
    ni = r1cs["num_instance"]
    powers = dg16_amd.powers_from_trapdoor(ctx(), curve, log_m, td[0], td[1], td[4])
    srs = dg16_amd.srs_from_powers(ctx(), curve, log_m, *powers)
    params = dg16_amd.generate_parameters_from_srs(ctx(), curve, system_of(F, r1cs), srs, in_subgroup=True)
    rng = random.Random(17)
    r, s = rng.randrange(1, p), rng.randrange(1, p)
    dpk = params.proving_key(ctx())
    pvk = dg16_amd.PreparedVerifyingKey.from_parameters(ctx(), params)
    try:
        a, b, c, dom = G.qap(r1cs, w, F)
        A, B, C = ctx().prove(dpk, enc_fr(F, a), enc_fr(F, b), enc_fr(F, c), enc_fr(F, w), enc_fr(F, [r]), enc_fr(F, [s]))
        proof = np.concatenate([np.asarray(corc.jac_to_affine(curve, 1, A)).reshape(-1),
                                np.asarray(corc.jac_to_affine(curve, 2, B)).reshape(-1),
                                np.asarray(corc.jac_to_affine(curve, 1, C)).reshape(-1)])
        eA, eB, eC = G.create_proof(curve, pk, r, s, r1cs, w)
        exp = np.concatenate([enc_g1(Fq, [eA]).reshape(-1), enc_g2(Fq, [eB]).reshape(-1), enc_g1(Fq, [eC]).reshape(-1)])
        assert np.array_equal(proof, exp)
        pub = [x % p for x in w[1:ni]]
        assert list(pvk.verify_batch(corc.ints_to_arr(pub, 4), proof)) == [True]
        pub[0] = (pub[0] + 1) % p
        assert list(pvk.verify_batch(corc.ints_to_arr(pub, 4), proof)) == [False]
    finally:
        dpk.close()
        pvk.close()


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_refusals_and_the_context_transforms_afterwards():
    from dg16_amd.lib import SrsPowers, SrsPrepared
    c_ = ctx()
    L, h = c_.L, c_.h
    buf = np.zeros((8, 8), dtype=np.uint64)
    ptr = buf.ctypes.data_as(ctypes.c_void_p)
    assert L.dg16_group_ntt(h, 7, 1, ptr, 3, 0) == 2                       # curve
    assert L.dg16_group_ntt(h, -1, 1, ptr, 3, 0) == 2
    assert L.dg16_group_ntt(h, 0, 3, ptr, 3, 0) == 3                       # group
    assert L.dg16_group_ntt(h, 0, 0, ptr, 3, 0) == 3
    assert L.dg16_group_ntt(h, 0, 1, None, 3, 0) == 3                      # NULL
    assert L.dg16_group_ntt(h, 0, 1, ptr, 28, 0) == 3                      # beyond 27 (BN254: two-adicity 28)
    assert L.dg16_group_ntt(h, 2, 1, ptr, 28, 1) == 3                      # beyond 27 (BLS12-377: two-adicity 47)
    assert L.dg16_group_ntt(None, 0, 1, ptr, 3, 0) == 3
    assert L.dg16_group_ntt(h, 0, 1, ptr, 0, 0) == 0 and not buf.any()     # log_n = 0: nothing to do
    big = np.zeros(64, dtype=np.uint64)
    a = big.ctypes.data
    pw, pr = SrsPowers(a, a, a, a, a), SrsPrepared(a, a, a, a, a, a)
    ok = lambda *args: L.dg16_srs_prepare(h, *args)                        # noqa: E731
    assert ok(5, 3, 0, ctypes.byref(pw), ctypes.byref(pr)) == 2            # curve
    assert ok(0, 3, 2, ctypes.byref(pw), ctypes.byref(pr)) == 3            # reduction
    assert ok(0, 3, -1, ctypes.byref(pw), ctypes.byref(pr)) == 3
    assert ok(0, 27, 0, ctypes.byref(pw), ctypes.byref(pr)) == 3           # log_m > 26
    assert ok(0, 28, 0, ctypes.byref(pw), ctypes.byref(pr)) == 3           # log_m + 1 > two-adicity
    assert ok(0, 3, 0, None, ctypes.byref(pr)) == 3                        # NULL structs
    assert ok(0, 3, 0, ctypes.byref(pw), None) == 3
    for j in range(5):                                                     # a NULL array in either
        f = [a] * 5
        f[j] = None
        assert ok(0, 3, 0, ctypes.byref(SrsPowers(*f)), ctypes.byref(pr)) == 3, j
    for j in range(6):
        f = [a] * 6
        f[j] = None
        assert ok(0, 3, 0, ctypes.byref(pw), ctypes.byref(SrsPrepared(*f))) == 3, j
    assert not big.any()                                                   # nothing was written
    # ... and the same context transforms correctly afterwards
    ks, pts = _inputs("bn254", 1)
    exp = _multiples("bn254", 1, corc.generator("bn254", 1), _ntt_ints("bn254", ks[:8], True))
    assert np.array_equal(c_.group_ntt("bn254", 1, pts[:8], inverse=True), exp)
