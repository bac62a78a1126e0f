"""GPU: phase 2 of the key ceremony -- dg16_groth16_contribute (keygen.contribute) and dg16_groth16_verify_contribution
(keygen.verify_contribution, keygen.verify_parameters).  The yardstick of the key is existing code that the oracle pins:
dg16_groth16_setup under the trapdoor (alpha, beta, 1, d1 d2, tau).  Systems come from the helpers
tests/test_gpu_setup_srs.py uses."""

import ctypes
import functools
import random

import numpy as np
import pytest

import points_check_cases as PC
from oracle import corc
from oracle.pyref import groth16 as G
from oracle.pyref import pairing as PR
from oracle.pyref.curves import CURVES
from oracle.pyref.fields import FQ, FR
from gpu_util import ctx
from test_gpu_prover import enc_fr, dec_g1, dec_g2
from test_gpu_setup import system_of
from test_gpu_srs_verify import bad_kinds, coeff_arr
import test_libsnark_model as M

pytestmark = pytest.mark.gpu

BOTH = ["bn254", "bls12_381"]
SMALL = [1, 2, 5]
NAMES = ("a_query", "b_g1_query", "b_g2_query", "h_query", "l_query", "fixed_points", "gamma_g2", "gamma_abc_g1")
A_Q, B1_Q, B2_Q, H_Q, L_Q, FIXED, GAMMA, IC = range(8)
BAD_POINT, IDENTITY, CHANGED, DELTA, L_BIT, H_BIT = 1, 2, 4, 8, 16, 32


@functools.lru_cache(maxsize=None)
def instance(curve, log_m):
    """log_m = 1: one constraint and the constant alone; log_m = 2: two public inputs; log_m = 5: the synthetic system of
    the reference-string tests"""
    F = FR[curve]
    if log_m == 1:
        return G.synthetic_r1cs(F, num_constraints=1, num_instance=1, num_witness=3, seed=51)
    if log_m == 2:
        return G.synthetic_r1cs(F, num_constraints=1, num_instance=3, num_witness=4, seed=52)
    return M.instance(F, 1 << log_m, seed=log_m + 50)


def secrets_of(curve, log_m):
    """alpha, beta, tau, d1, d2"""
    rng = random.Random(2000 + 10 * log_m + corc.CURVES[curve])
    r = FR[curve].p
    return tuple(rng.randrange(2, r) for _ in range(5))


@functools.lru_cache(maxsize=None)
def srs_of(curve, log_m, reduction, tau_shift=0):
    import dg16_amd
    alpha, beta, tau, _, _ = secrets_of(curve, log_m)
    return dg16_amd.srs_from_trapdoor(ctx(), curve, log_m, alpha, beta, tau + tau_shift, reduction=reduction)


def keys(curve, log_m, reduction="circom"):
    """(the uncontributed key, after d1, after d1 and d2) as Parameters"""
    return _keys(curve, log_m, reduction)


@functools.lru_cache(maxsize=None)
def _keys(curve, log_m, reduction):
    import dg16_amd
    r1cs, _ = instance(curve, log_m)
    _, _, _, d1, d2 = secrets_of(curve, log_m)
    p0 = dg16_amd.generate_parameters_from_srs(ctx(), curve, system_of(FR[curve], r1cs), srs_of(curve, log_m, reduction),
                                               reduction=reduction)
    assert p0.log_m == log_m
    p1 = dg16_amd.contribute(ctx(), p0, d1)
    p2 = dg16_amd.contribute(ctx(), p1, d2)
    return p0, p1, p2


def host_key(params):
    """the eight arrays as writable host copies, [points][limbs]"""
    return [params.host(n).copy() for n in NAMES]


def coefficients(params, seed):
    rng = random.Random(seed)
    return [rng.randrange(1, 1 << 128) for _ in range(max(params.num_vars - params.num_inputs, params.domain_size))]


def verify(params, before, after, rho):
    return ctx().groth16_verify_contribution(params.curve, params.num_inputs, params.num_vars, params.domain_size,
                                             before, after, coeff_arr(rho))


def g1_of(curve, k):
    return ctx().fixed_base_mul(curve, 1, corc.ints_to_arr([k % FR[curve].p], 4))[0]


def fixed_view(curve, fixed):
    """fixed_points [.][fq limbs] -> views of alpha_g1, beta_g1, delta_g1, beta_g2, delta_g2"""
    fq = FQ[curve].limbs64
    f = fixed.reshape(-1)
    return f[:2 * fq], f[2 * fq:4 * fq], f[4 * fq:6 * fq], f[6 * fq:10 * fq], f[10 * fq:14 * fq]


# ---- the key itself ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduction", ["circom", "libsnark"])
@pytest.mark.parametrize("log_m", SMALL)
@pytest.mark.parametrize("curve", BOTH)
def test_two_contributions_equal_the_trapdoor_key(curve, log_m, reduction):
    """contribute(contribute(key from the reference string, d1), d2) is, array by array and byte for byte, the key
    dg16_groth16_setup makes under (alpha, beta, 1, d1 d2, tau)."""
    import dg16_amd
    r = FR[curve].p
    r1cs, _ = instance(curve, log_m)
    alpha, beta, tau, d1, d2 = secrets_of(curve, log_m)
    p0, _, p2 = keys(curve, log_m, reduction)
    ref = dg16_amd.generate_parameters(ctx(), curve, system_of(FR[curve], r1cs), trapdoor=(alpha, beta, 1, d1 * d2 % r, tau),
                                       reduction=reduction)
    assert p2.trapdoor is None and p2.reduction == reduction
    for name in NAMES:
        assert np.array_equal(p2.host(name), ref.host(name)), (curve, log_m, reduction, name)
    if reduction == "libsnark":
        m = 1 << log_m
        assert not p0.host("h_query")[m - 1].any() and not p2.host("h_query")[m - 1].any()
        assert p2.host("h_query")[0].any()


@pytest.mark.parametrize("curve", BOTH)
def test_a_proof_under_the_contributed_key(curve):
    """A proof made with the contributed key is accepted under its verifying key and rejected under the uncontributed
    one."""
    import dg16_amd
    log_m = 5
    F = FR[curve]
    r1cs, w = instance(curve, log_m)
    ni = r1cs["num_instance"]
    p0, _, p2 = keys(curve, log_m)
    rng = random.Random(7)
    r, s = rng.randrange(1, F.p), rng.randrange(1, F.p)
    dpk = p2.proving_key(ctx())
    pvk = dg16_amd.PreparedVerifyingKey.from_parameters(ctx(), p2)
    pvk0 = dg16_amd.PreparedVerifyingKey.from_parameters(ctx(), p0)
    try:
        a, b, c, dom = G.qap(r1cs, w, F)
        assert dom.size == p2.domain_size
        A, B, C = ctx().prove(dpk, enc_fr(F, a), enc_fr(F, b), enc_fr(F, c), enc_fr(F, w), enc_fr(F, [r]), enc_fr(F, [s]))
        proof = np.concatenate([np.asarray(corc.jac_to_affine(curve, 1, A)).reshape(-1),
                                np.asarray(corc.jac_to_affine(curve, 2, B)).reshape(-1),
                                np.asarray(corc.jac_to_affine(curve, 1, C)).reshape(-1)])
        pub = corc.ints_to_arr([x % F.p for x in w[1:ni]], 4)
        assert list(pvk.verify_batch(pub, proof)) == [True]
        assert list(pvk0.verify_batch(pub, proof)) == [False]
    finally:
        dpk.close()
        pvk.close()
        pvk0.close()


# ---- contribute: edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", ["bn254", "bls12_381", "bls12_377"])
def test_contribute_edges(curve):
    """d = 1 is the identity map on the bytes; outputs may be the inputs; n_l = 0 is legal; d = 0 and d = r are refused.
    BLS12-377 (no pairing, no verifier) is held against the oracle's products on a few entries."""
    from dg16_amd.lib import Dg16Error
    r = FR[curve].p
    c = ctx()
    rng = random.Random(5)
    d = rng.randrange(2, r)
    l = corc.gen_points(curve, 1, 91, 70)
    h = corc.gen_points(curve, 1, 92, 33)
    h[32] = 0                                                      # an identity entry stays one
    fixed = np.concatenate([corc.gen_points(curve, 1, 93, 3).reshape(-1), corc.gen_points(curve, 2, 94, 2).reshape(-1)])
    same = c.groth16_contribute(curve, l, h, fixed, 1)
    assert np.array_equal(same[0], l) and np.array_equal(same[1], h) and np.array_equal(same[2], fixed)
    lo, ho, fo = c.groth16_contribute(curve, l, h, fixed, d)
    dinv = pow(d, r - 2, r)
    for i in (0, 35, 69):
        assert np.array_equal(lo[i], corc.point_mul(curve, 1, l[i:i + 1], dinv)[0])
    for i in (0, 31):
        assert np.array_equal(ho[i], corc.point_mul(curve, 1, h[i:i + 1], dinv)[0])
    assert not ho[32].any()
    f_in, f_out = fixed_view(curve, fixed), fixed_view(curve, fo)
    for j in (0, 1, 3):
        assert np.array_equal(f_in[j], f_out[j])
    assert np.array_equal(f_out[2], corc.point_mul(curve, 1, f_in[2][None, :], d)[0])
    assert np.array_equal(f_out[4], corc.point_mul(curve, 2, f_in[4][None, :], d)[0])
    # aliased outputs
    l2, h2, f2 = l.copy(), h.copy(), fixed.copy()
    got = c.groth16_contribute(curve, l2, h2, f2, d, in_place=True)
    assert got[0] is l2 and np.array_equal(l2, lo) and np.array_equal(h2, ho) and np.array_equal(f2, fo)
    # n_l = 0
    e, ho2, fo2 = c.groth16_contribute(curve, l[:0], h, fixed, d)
    assert e.size == 0 and np.array_equal(ho2, ho) and np.array_equal(fo2, fo)
    for bad in (0, r):
        with pytest.raises(Dg16Error) as err:
            c.groth16_contribute(curve, l, h, fixed, bad)
        assert err.value.code == 3


# ---- verify_contribution -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_m", SMALL)
@pytest.mark.parametrize("curve", BOTH)
def test_honest_pairs_are_accepted(curve, log_m):
    import dg16_amd
    p0, p1, p2 = keys(curve, log_m)
    rho = coefficients(p0, 3)
    k0, k1, k2 = host_key(p0), host_key(p1), host_key(p2)
    assert verify(p0, k0, k1, rho) == (0, 0, 0, 0)
    assert verify(p0, k0, k2, rho) == (0, 0, 0, 0)             # two contributions apart
    assert verify(p0, k1, k2, rho) == (0, 0, 0, 0)
    assert verify(p0, k0, k0, rho) == (0, 0, 0, 0)             # d = 1
    rep = dg16_amd.verify_contribution(ctx(), p0, p2)          # coefficients drawn by the library's helper
    assert rep.accepted and rep.failed == 0 and rep.reasons == [] and rep.bad_array is None


@pytest.mark.parametrize("log_m", SMALL)
@pytest.mark.parametrize("curve", BOTH)
def test_each_tampering_sets_exactly_its_bit(curve, log_m):
    r = FR[curve].p
    fq = FQ[curve].limbs64
    p0, p1, _ = keys(curve, log_m)
    _, _, _, d1, _ = secrets_of(curve, log_m)
    rho = coefficients(p0, 4)
    k0 = host_key(p0)
    n_l, m = p0.num_vars - p0.num_inputs, p0.domain_size
    other = g1_of(curve, 987654321)

    def tampered(change):
        k1 = host_key(p1)
        change(k1)
        return verify(p0, k0, k1, rho)

    def put(array, index, words):
        def change(k):
            k[array][index] = words
        return change

    # one entry of l_query' / h_query' replaced by another subgroup point
    for i in sorted({0, n_l // 2, n_l - 1}):
        assert tampered(put(L_Q, i, other)) == (L_BIT, 0, 0, 0), i
    for i in sorted({0, m // 2, m - 1}):
        assert tampered(put(H_Q, i, other)) == (H_BIT, 0, 0, 0), i
    # delta_g1' and delta_g2' from different d
    def other_delta_g1(k):
        fixed_view(curve, k[FIXED])[2][:] = corc.point_mul(curve, 1, fixed_view(curve, k0[FIXED])[2][None, :], d1 + 1)[0]
    assert tampered(other_delta_g1) == (DELTA, 0, 0, 0)
    # l_query' scaled by another d than delta
    def other_l(k):
        k[L_Q][:] = ctx().points_scale(curve, 1, k0[L_Q], pow(d1 + 1, r - 2, r), in_subgroup=True)
    assert tampered(other_l) == (L_BIT, 0, 0, 0)
    # the arrays a contribution leaves alone
    assert tampered(put(A_Q, p0.num_vars - 1, other)) == (CHANGED, 0, 0, 0)
    assert tampered(put(IC, 0, other)) == (CHANGED, 0, 0, 0)
    def other_beta_g2(k):
        fixed_view(curve, k[FIXED])[3][:] = corc.generator(curve, 2)[0]
    assert tampered(other_beta_g2) == (CHANGED, 0, 0, 0)
    # delta_g1' = O
    def no_delta_g1(k):
        fixed_view(curve, k[FIXED])[2][:] = 0
    assert tampered(no_delta_g1) == (IDENTITY, 0, 0, 0)
    # bad points: unreduced, off the curve, off the subgroup, in l_query', h_query' and delta_g2'
    for array, report_as, n in ((L_Q, 4, n_l), (H_Q, 5, m)):
        kinds = bad_kinds(curve, 1)
        assert len(kinds) == (2 if curve == "bn254" else 3)
        for j, w in enumerate(kinds):
            index = sorted({0, n // 2, n - 1})[j % len({0, n // 2, n - 1})]
            assert tampered(put(array, index, w)) == (BAD_POINT, report_as, index, 1), (array, j)
    kinds = bad_kinds(curve, 2)
    assert len(kinds) == 3
    for w in kinds:
        def bad_delta_g2(k, w=w):
            fixed_view(curve, k[FIXED])[4][:] = w
        assert tampered(bad_delta_g2) == (BAD_POINT, 7, 0, 1)
    # two arrays with bad points: the first array and its smallest index, the count over all
    def several(k):
        k[H_Q][m - 1] = bad_kinds(curve, 1)[0]
        k[H_Q][0] = bad_kinds(curve, 1)[1]
        fixed_view(curve, k[FIXED])[4][:] = bad_kinds(curve, 2)[0]
    assert tampered(several) == (BAD_POINT, 5, 0, 3)
    # a bad point in `before`
    kb = host_key(p0)
    kb[L_Q][n_l - 1] = bad_kinds(curve, 1)[0]
    assert verify(p0, kb, host_key(p1), rho) == (BAD_POINT, 0, n_l - 1, 1)


@pytest.mark.parametrize("log_m", SMALL)
@pytest.mark.parametrize("curve", BOTH)
def test_why_the_coefficients_must_be_unpredictable(curve, log_m):
    """L'_0 += rho_1 X and L'_1 -= rho_0 X cancel in sum rho_k L'_k: accepted under the rho the forger knew, rejected under
    fresh ones."""
    r = FR[curve].p
    p0, p1, _ = keys(curve, log_m)
    rho = coefficients(p0, 5)
    k0, k1 = host_key(p0), host_key(p1)
    X = g1_of(curve, 424242)[None, :]
    k1[L_Q][0] = corc.point_add(curve, 1, k1[L_Q][0:1], corc.point_mul(curve, 1, X, rho[1]))[0]
    k1[L_Q][1] = corc.point_add(curve, 1, k1[L_Q][1:2], corc.point_mul(curve, 1, X, r - rho[0]))[0]
    assert not np.array_equal(k1[L_Q][:2], p1.host("l_query")[:2])
    assert verify(p0, k0, k1, rho) == (0, 0, 0, 0)
    assert verify(p0, k0, k1, coefficients(p0, 6)) == (L_BIT, 0, 0, 0)


def test_the_equalities_against_the_oracles_pairing():
    """BN254, log_m = 1: the three equations evaluated by oracle.pyref.pairing on the decoded points -- the sums made by
    the oracle's group law -- agree bit by bit with the library, for the honest pair and for a tampered one."""
    curve, log_m = "bn254", 1
    Fq = FQ[curve]
    c1 = CURVES[curve, "g1"]
    p0, p1, _ = keys(curve, log_m)
    rho = coefficients(p0, 9)
    k0 = host_key(p0)
    words = []
    for tamper in (False, True):
        k1 = host_key(p1)
        if tamper:
            k1[L_Q][1] = g1_of(curve, 31337)
        d1 = [dec_g1(Fq, fixed_view(curve, k[FIXED])[2]) for k in (k0, k1)]
        d2 = [dec_g2(Fq, fixed_view(curve, k[FIXED])[4]) for k in (k0, k1)]
        comb = lambda arr: c1.msm([dec_g1(Fq, row) for row in arr], rho[:len(arr)])      # noqa: E731
        eqs = {DELTA: ((d1[1], d2[0]), (d1[0], d2[1])),
               L_BIT: ((comb(k1[L_Q]), d2[1]), (comb(k0[L_Q]), d2[0])),
               H_BIT: ((comb(k1[H_Q]), d2[1]), (comb(k0[H_Q]), d2[0]))}
        word = 0
        for bit, ((a1, b1), (a2, b2)) in eqs.items():
            if not PR.pairing_product_is_one(curve, [(a1, b1), (c1.neg(a2), b2)]):
                word |= bit
        assert verify(p0, k0, k1, rho) == (word, 0, 0, 0)
        words.append(word)
    assert words == [0, L_BIT]


def test_refusals_and_the_context_proves_afterwards():
    from dg16_amd.lib import Groth16Key, Phase2ReportC
    from test_gpu_srs_verify import context_still_proves
    c_ = ctx()
    L, h = c_.L, c_.h
    p0, p1, _ = keys("bn254", 2)
    k0, k1 = host_key(p0), host_key(p1)
    rho = coeff_arr(coefficients(p0, 11))
    a0, a1 = [a.ctypes.data for a in k0], [a.ctypes.data for a in k1]
    kb, ka, rep = Groth16Key(*a0), Groth16Key(*a1), Phase2ReportC()
    cp = rho.ctypes.data_as(ctypes.c_void_p)
    ni, nv, m = p0.num_inputs, p0.num_vars, p0.domain_size
    call = lambda curve, b, a, c, rp, ni_=ni: L.dg16_groth16_verify_contribution(h, curve, ni_, nv, m, b, a, c, rp)  # noqa: E731
    assert call(0, ctypes.byref(kb), ctypes.byref(ka), cp, ctypes.byref(rep)) == 0 and rep.failed == 0
    for j in (0, len(rho) - 1):
        zero = rho.copy()
        zero[j] = 0                                                              # a zero coefficient
        assert call(0, ctypes.byref(kb), ctypes.byref(ka), zero.ctypes.data_as(ctypes.c_void_p), ctypes.byref(rep)) == 3
    assert call(0, None, ctypes.byref(ka), cp, ctypes.byref(rep)) == 3           # NULL pointers
    assert call(0, ctypes.byref(kb), None, cp, ctypes.byref(rep)) == 3
    assert call(0, ctypes.byref(kb), ctypes.byref(ka), None, ctypes.byref(rep)) == 3
    assert call(0, ctypes.byref(kb), ctypes.byref(ka), cp, None) == 3
    for j in range(8):
        f = list(a1)
        f[j] = None
        assert call(0, ctypes.byref(kb), ctypes.byref(Groth16Key(*f)), cp, ctypes.byref(rep)) == 3, j
    assert call(0, ctypes.byref(kb), ctypes.byref(ka), cp, ctypes.byref(rep), 0) == 3        # num_inputs = 0
    assert call(0, ctypes.byref(kb), ctypes.byref(ka), cp, ctypes.byref(rep), nv + 1) == 3   # num_inputs > num_vars
    assert call(2, ctypes.byref(kb), ctypes.byref(ka), cp, ctypes.byref(rep)) == 7           # BLS12-377: no pairing here
    assert call(5, ctypes.byref(kb), ctypes.byref(ka), cp, ctypes.byref(rep)) == 2           # unknown curve
    # contribute's refusals through the C ABI: NULL pointers, an unknown curve
    d = np.frombuffer((5).to_bytes(32, "little"), dtype=np.uint64).copy()
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    lq, hq, fx = k0[L_Q], k0[H_Q], k0[FIXED]
    lo, ho, fo = lq.copy(), hq.copy(), fx.copy()
    con = lambda curve, l, hh, f, dd, o1, o2, o3: L.dg16_groth16_contribute(      # noqa: E731
        h, curve, len(lq), len(hq), vp(l), vp(hh), vp(f), vp(dd), vp(o1), vp(o2), vp(o3))
    assert con(0, lq, hq, fx, d, lo, ho, fo) == 0
    for j in range(7):
        args = [lq, hq, fx, d, lo, ho, fo]
        args[j] = None
        assert con(0, *args) == 3, j
    assert con(4, lq, hq, fx, d, lo, ho, fo) == 2
    context_still_proves()
    assert verify(p0, k0, k1, coefficients(p0, 11)) == (0, 0, 0, 0)


# ---- verify_parameters -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", BOTH)
def test_verify_parameters(curve):
    """A twice-contributed key is accepted against its R1CS and reference string, and rejected against an R1CS with one
    changed coefficient and against a reference string from another tau."""
    import dg16_amd
    log_m = 5
    F = FR[curve]
    r1cs, _ = instance(curve, log_m)
    _, _, p2 = keys(curve, log_m)
    srs = srs_of(curve, log_m, "circom")
    rep = dg16_amd.verify_parameters(ctx(), curve, system_of(F, r1cs), srs, p2)
    assert rep.accepted, rep
    changed = dict(r1cs)
    rows = [list(row) for row in r1cs["a"]]
    coeff, col = rows[3][0]
    rows[3][0] = ((coeff + 1) % F.p, col)
    changed["a"] = rows
    rep = dg16_amd.verify_parameters(ctx(), curve, system_of(F, changed), srs, p2)
    assert not rep.accepted and rep.changed, rep
    rep = dg16_amd.verify_parameters(ctx(), curve, system_of(F, r1cs), srs_of(curve, log_m, "circom", 1), p2)
    assert not rep.accepted and rep.failed & (CHANGED | L_BIT | H_BIT), rep
