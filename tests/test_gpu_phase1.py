"""GPU: phase 1 of the key ceremony -- dg16_srs_contribute (keygen.contribute_powers) and dg16_srs_verify_contribution
(keygen.verify_powers_contribution).  Expected values come from elsewhere: a contribution to the transcript of a known
trapdoor is the transcript of the product trapdoor (powers_from_trapdoor: dg16_fixed_base_mul on Python-made powers), the
key's points are the oracle's products, and the verifier's word is the eight relations evaluated by oracle.pyref.pairing."""

import ctypes
import functools
import random

import numpy as np
import pytest

import phase1_cases as P1
import points_mul_cases as PM
from oracle import corc
from oracle.pyref.fields import FR
from gpu_util import ctx
from test_gpu_srs_verify import coeff_arr, coefficients, context_still_proves

pytestmark = pytest.mark.gpu

BOTH = ["bn254", "bls12_381"]
ALL = BOTH + ["bls12_377"]


def secrets_of(curve, log_m, which):
    """(alpha, beta, tau) of transcript number `which`"""
    rng = random.Random(7000 + 100 * which + 10 * log_m + corc.CURVES[curve])
    r = FR[curve].p
    return rng.randrange(2, r), rng.randrange(2, r), rng.randrange(2, r)


def blinds_of(curve):
    rng = random.Random(8100 + corc.CURVES[curve])
    r = FR[curve].p
    return [rng.randrange(2, r) for _ in range(3)]


@functools.lru_cache(maxsize=None)
def _challenge(curve):
    return corc.gen_points(curve, 2, 4242, 3)


def challenge(curve):
    return _challenge(curve).copy()


@functools.lru_cache(maxsize=None)
def _trapdoor_powers(curve, log_m, alpha, beta, tau):
    import dg16_amd
    return dg16_amd.powers_from_trapdoor(ctx(), curve, log_m, alpha, beta, tau)


def trapdoor_powers(curve, log_m, alpha, beta, tau):
    return tuple(a.copy() for a in _trapdoor_powers(curve, log_m, alpha, beta, tau))


def product(curve, x, y):
    r = FR[curve].p
    return tuple(a * b % r for a, b in zip(x, y))


def contribute(curve, log_m, powers, abt, with_key=False):
    """keygen's argument order is (tau, alpha, beta); the trapdoors here are (alpha, beta, tau)"""
    import dg16_amd
    a, b, t = abt
    if with_key:
        return dg16_amd.contribute_powers(ctx(), curve, log_m, powers, t, a, b, blinds=blinds_of(curve),
                                          challenge=challenge(curve))
    return dg16_amd.contribute_powers(ctx(), curve, log_m, powers, t, a, b)


def assert_same(got, want, what):
    for name, g, w in zip(("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (what, name)


# ---- contributions against known secrets ----------------------------------------------------------------------------------
@pytest.mark.parametrize("log_m", [1, 2, 3, 6])
@pytest.mark.parametrize("curve", BOTH)
def test_a_contribution_is_the_product_trapdoor(curve, log_m):
    """contribute_powers(powers(a, b, t), t', a', b') = powers(a a', b b', t t') in all five arrays, and verify_powers
    accepts it.  At log_m = 6 tau_g1 has 127 points: a partial last wave and a partial last chunk."""
    import dg16_amd
    x, y = secrets_of(curve, log_m, 0), secrets_of(curve, log_m, 1)
    before = trapdoor_powers(curve, log_m, *x)
    after, key = contribute(curve, log_m, before, y)
    assert key is None
    assert_same(after, trapdoor_powers(curve, log_m, *product(curve, x, y)), (curve, log_m))
    assert_same(before, trapdoor_powers(curve, log_m, *x), "the input is untouched")
    rep = dg16_amd.verify_powers(ctx(), curve, log_m, *after, coeffs=coeff_arr(coefficients(log_m, 21)),
                                 generators=(corc.generator(curve, 1)[0], corc.generator(curve, 2)[0]))
    assert rep.accepted and rep.failed == 0


@pytest.mark.parametrize("curve", BOTH)
def test_log_7_in_slices_of_64(curve):
    """tau_g1 = 255 points in four slices, the others 128 in two: the exponent carries over every slice boundary."""
    log_m = 7
    x, y = secrets_of(curve, log_m, 0), secrets_of(curve, log_m, 1)
    c = ctx()
    c.set_points_mul_slice(64)
    try:
        after, _ = contribute(curve, log_m, trapdoor_powers(curve, log_m, *x), y)
    finally:
        c.set_points_mul_slice(0)
    assert_same(after, trapdoor_powers(curve, log_m, *product(curve, x, y)), curve)


def test_bls12_377_at_log_3():
    curve, log_m = "bls12_377", 3
    x, y = secrets_of(curve, log_m, 0), secrets_of(curve, log_m, 1)
    after, key = contribute(curve, log_m, trapdoor_powers(curve, log_m, *x), y, with_key=True)
    assert_same(after, trapdoor_powers(curve, log_m, *product(curve, x, y)), curve)
    a, b, t = y
    assert np.array_equal(key, P1.oracle_key(curve, corc.generator(curve, 1)[0], (t, a, b), blinds_of(curve),
                                             challenge(curve)))


@pytest.mark.parametrize("curve", BOTH)
def test_in_place_and_two_in_a_row(curve):
    """Two contributions, the second one written over its input, equal the product of the three trapdoors; the key of
    the in-place call is the key of the out-of-place one (G is read before tau_g1 is overwritten)."""
    log_m = 3
    x, y, z = (secrets_of(curve, log_m, j) for j in range(3))
    mid, _ = contribute(curve, log_m, trapdoor_powers(curve, log_m, *x), y)
    buf = [np.ascontiguousarray(a.copy()) for a in mid]
    a, b, t = z
    out, key = ctx().srs_contribute(curve, log_m, buf, (t, a, b), blinds=blinds_of(curve), challenge_g2=challenge(curve),
                                    in_place=True)
    assert all(o is i for o, i in zip(out, buf))
    assert_same(buf, trapdoor_powers(curve, log_m, *product(curve, product(curve, x, y), z)), curve)
    _, key2 = contribute(curve, log_m, mid, z, with_key=True)
    assert np.array_equal(key, key2)


# ---- from a contributed transcript to a key --------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", ALL)
def test_contributed_powers_to_the_key_of_the_product_trapdoor(curve):
    """log_m = 3: srs_from_powers and generate_parameters_from_srs on the contributed transcript give the key
    dg16_groth16_setup makes under (a a', b b', 1, 1, t t')."""
    import dg16_amd
    import test_libsnark_model as M
    from test_gpu_setup import system_of
    from test_gpu_setup_srs import NAMES as KEY_NAMES
    log_m = 3
    F = FR[curve]
    x, y = secrets_of(curve, log_m, 0), secrets_of(curve, log_m, 1)
    after, _ = contribute(curve, log_m, trapdoor_powers(curve, log_m, *x), y)
    if curve in BOTH:
        assert dg16_amd.verify_powers(ctx(), curve, log_m, *after, coeffs=coeff_arr(coefficients(log_m, 22))).accepted
    r1cs, _ = M.instance(F, 1 << log_m, seed=log_m + 90)
    system = system_of(F, r1cs)
    srs = dg16_amd.srs_from_powers(ctx(), curve, log_m, *after)
    got = dg16_amd.generate_parameters_from_srs(ctx(), curve, system, srs, in_subgroup=True)
    a, b, t = product(curve, x, y)
    ref = dg16_amd.generate_parameters(ctx(), curve, system, trapdoor=(a, b, 1, 1, t))
    assert got.log_m == ref.log_m == log_m
    for name in KEY_NAMES:
        assert np.array_equal(got.host(name), ref.host(name)), (curve, name)


# ---- the verifier ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _honest(curve, log_m):
    x, y = secrets_of(curve, log_m, 0), secrets_of(curve, log_m, 1)
    before = trapdoor_powers(curve, log_m, *x)
    after, key = contribute(curve, log_m, before, y, with_key=True)
    return before, after, key


def honest(curve, log_m):
    before, after, key = _honest(curve, log_m)
    return [a.copy() for a in before], [a.copy() for a in after], key.copy()


def verify(curve, log_m, before, after, key, sp, seed=23):
    """-> (failed, n_bad_points, after's report) and, beside it, dg16_srs_verify's own report of `after`"""
    rho = coeff_arr(coefficients(log_m, seed))
    got = ctx().srs_verify_contribution(curve, log_m, before, after, key, sp, rho)
    assert got[2] == ctx().srs_verify(curve, log_m, *after, rho)
    return got


def g1_of(curve, k):
    return ctx().fixed_base_mul(curve, 1, corc.ints_to_arr([k % FR[curve].p], 4))[0]


@pytest.mark.parametrize("log_m", [1, 2, 5])
@pytest.mark.parametrize("curve", BOTH)
def test_an_honest_contribution_is_accepted(curve, log_m):
    import dg16_amd
    before, after, key = honest(curve, log_m)
    a, b, t = secrets_of(curve, log_m, 1)
    assert np.array_equal(key, P1.oracle_key(curve, before[0][0], (t, a, b), blinds_of(curve), challenge(curve)))
    assert verify(curve, log_m, before, after, key, challenge(curve)) == (0, 0, (0, 0, 0, 0))
    # of `before` the heads are enough
    heads = [before[0][:2], before[1][:2], before[2][:1], before[3][:1], before[4]]
    assert verify(curve, log_m, heads, after, key, challenge(curve)) == (0, 0, (0, 0, 0, 0))
    rep = dg16_amd.verify_powers_contribution(ctx(), curve, log_m, before, after, key, challenge(curve))
    assert rep.accepted and rep.failed == 0 and rep.reasons == [] and rep.after.accepted


TAMPERINGS = ("none", "g1_sx", "g2_spx", "other_tau_key", "other_beta", "base", "other_sp_tau")
# what each tampering must set (the test computes the pairing bits with the oracle; this table keeps it honest)
WANT = {"none": 0, "g1_sx": P1.KEY_TAU | P1.LINK_TAU_G2, "g2_spx": P1.KEY_TAU | P1.LINK_TAU_G1,
        "other_tau_key": P1.LINK_TAU_G1 | P1.LINK_TAU_G2, "other_beta": P1.LINK_BETA | P1.LINK_BETA_G2,
        "base": P1.AFTER | P1.BASE, "other_sp_tau": P1.KEY_TAU | P1.LINK_TAU_G1}


def tampered(curve, log_m, kind):
    before, after, key = honest(curve, log_m)
    sp = challenge(curve)
    fq = corc.FQ_LIMBS[curve]
    a, b, t = secrets_of(curve, log_m, 1)
    s = blinds_of(curve)
    if kind == "g1_sx":                  # s (tau + 1) G in the place of s tau G
        key[2 * fq:4 * fq] = g1_of(curve, s[0] * (t + 1))
    elif kind == "g2_spx":               # (tau + 1) SP_tau
        key[4 * fq:8 * fq] = corc.point_mul(curve, 2, sp[0:1], t + 1)[0]
    elif kind == "other_tau_key":        # an honest key, for another tau
        _, key = contribute(curve, log_m, before, (a, b, t + 5), with_key=True)
    elif kind == "other_beta":           # a transcript by another beta under the key of this one
        after, _ = contribute(curve, log_m, before, (a, b + 5, t))
        after = list(after)
    elif kind == "base":
        after[0][0] = g1_of(curve, 2)
    elif kind == "other_sp_tau":
        sp[0] = corc.point_mul(curve, 2, sp[0:1], 3)[0]
    return before, after, key, sp


def check_tampering(curve, log_m, kind):
    before, after, key, sp = tampered(curve, log_m, kind)
    want = P1.expected_pairing_bits(curve, before, after, key, sp)
    rho = coeff_arr(coefficients(log_m, 23))
    if ctx().srs_verify(curve, log_m, *after, rho)[0]:
        want |= P1.AFTER
    if not (np.array_equal(before[0][0], after[0][0]) and np.array_equal(before[1][0], after[1][0])):
        want |= P1.BASE
    assert want == WANT[kind], (kind, want)
    got = verify(curve, log_m, before, after, key, sp)
    assert got[:2] == (want, 0), (kind, got)


@pytest.mark.parametrize("kind", TAMPERINGS)
def test_each_tampering_against_the_oracles_pairing(kind):
    check_tampering("bn254", 2, kind)


def test_one_tampering_on_bls12_381():
    check_tampering("bls12_381", 2, "other_tau_key")


# ---- bad input ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", BOTH)
def test_bad_and_identity_points_skip_the_pairings(curve):
    """A G2 key point outside the subgroup, an identity key point, an identity challenge point and an identity head of
    `before`: their bit, and no pairing bit although the relations they are part of cannot hold."""
    log_m = 2
    fq = corc.FQ_LIMBS[curve]
    before, after, key, sp = tampered(curve, log_m, "none")
    bad = key.copy()
    bad[4 * fq:8 * fq] = PM.pack_point(curve, 2, PM.outside_point(curve, 2))
    assert verify(curve, log_m, before, after, bad, sp)[:2] == (P1.BAD_POINT, 1)
    off = key.copy()
    off[0] ^= 1                                        # g1_s of tau leaves the curve
    assert verify(curve, log_m, before, after, off, sp)[:2] == (P1.BAD_POINT, 1)
    for lo, hi in ((0, 2 * fq), (2 * fq, 4 * fq), (3 * 8 * fq - 4 * fq, 3 * 8 * fq)):
        ident = key.copy()
        ident[lo:hi] = 0
        assert verify(curve, log_m, before, after, ident, sp)[:2] == (P1.IDENTITY, 0), lo
    sp0 = sp.copy()
    sp0[1] = 0
    assert verify(curve, log_m, before, after, key, sp0)[:2] == (P1.IDENTITY, 0)
    b0 = [a.copy() for a in before]
    b0[2][0] = 0                                       # alpha_tau_g1[0] of `before`
    assert verify(curve, log_m, b0, after, key, sp)[:2] == (P1.IDENTITY, 0)
    a0 = [a.copy() for a in after]
    a0[3][0] = 0                                       # beta_tau_g1[0] of `after`: its own report says so
    got = verify(curve, log_m, before, a0, key, sp)
    assert got[0] == P1.AFTER and got[2][0] == 2       # DG16_SRS_IDENTITY, and no pairing bit


def test_refusals_and_the_context_proves_afterwards():
    from dg16_amd.lib import SrsPowers, SrsPowersOut, SrsContributionReportC
    c_ = ctx()
    L, h = c_.L, c_.h
    curve, log_m = "bn254", 2
    before, after, key, sp = tampered(curve, log_m, "none")
    rho = coeff_arr(coefficients(log_m, 24))
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    pb, pa = SrsPowers(*[a.ctypes.data for a in before]), SrsPowers(*[a.ctypes.data for a in after])
    rep = SrsContributionReportC()
    ver = lambda cv, lm, b, a, k, s, c, rp: L.dg16_srs_verify_contribution(h, cv, lm, b, a, vp(k), vp(s), vp(c), rp)  # noqa: E731
    assert ver(0, log_m, ctypes.byref(pb), ctypes.byref(pa), key, sp, rho, ctypes.byref(rep)) == 0 and rep.failed == 0
    assert ver(2, log_m, ctypes.byref(pb), ctypes.byref(pa), key, sp, rho, ctypes.byref(rep)) == 7     # BLS12-377
    assert ver(5, log_m, ctypes.byref(pb), ctypes.byref(pa), key, sp, rho, ctypes.byref(rep)) == 2     # unknown curve
    for j in (0, len(rho) - 1):
        zero = rho.copy()
        zero[j] = 0                                                                # a zero coefficient
        assert ver(0, log_m, ctypes.byref(pb), ctypes.byref(pa), key, sp, zero, ctypes.byref(rep)) == 3
    assert ver(0, log_m, None, ctypes.byref(pa), key, sp, rho, ctypes.byref(rep)) == 3
    assert ver(0, log_m, ctypes.byref(pb), None, key, sp, rho, ctypes.byref(rep)) == 3
    assert ver(0, log_m, ctypes.byref(pb), ctypes.byref(pa), None, sp, rho, ctypes.byref(rep)) == 3
    assert ver(0, log_m, ctypes.byref(pb), ctypes.byref(pa), key, None, rho, ctypes.byref(rep)) == 3
    assert ver(0, log_m, ctypes.byref(pb), ctypes.byref(pa), key, sp, None, ctypes.byref(rep)) == 3
    assert ver(0, log_m, ctypes.byref(pb), ctypes.byref(pa), key, sp, rho, None) == 3
    assert ver(0, 0, ctypes.byref(pb), ctypes.byref(pa), key, sp, rho, ctypes.byref(rep)) == 3         # log_m = 0
    assert ver(0, 27, ctypes.byref(pb), ctypes.byref(pa), key, sp, rho, ctypes.byref(rep)) == 3
    # dg16_srs_contribute
    word = lambda *v: np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in v), dtype=np.uint64).copy()   # noqa: E731
    r = FR[curve].p
    outs = [np.zeros_like(a) for a in before]
    po = SrsPowersOut(*[a.ctypes.data for a in outs])
    kout = np.zeros_like(key)
    sec, bl = word(3, 5, 7), word(11, 13, 17)
    con = lambda cv, lm, p, s, b, c, o, k: L.dg16_srs_contribute(h, cv, lm, p, vp(s), vp(b), vp(c), o, vp(k))   # noqa: E731
    assert con(0, log_m, ctypes.byref(pb), sec, bl, sp, ctypes.byref(po), kout) == 0
    assert con(0, log_m, ctypes.byref(pb), sec, None, None, ctypes.byref(po), None) == 0
    for bad in (word(0, 5, 7), word(3, 0, 7), word(3, 5, 0), word(r, 5, 7), word(3, 5, r + 1)):
        assert con(0, log_m, ctypes.byref(pb), bad, bl, sp, ctypes.byref(po), kout) == 3               # a zero / large secret
        assert con(0, log_m, ctypes.byref(pb), sec, bad, sp, ctypes.byref(po), kout) == 3              # ... blind
    assert con(0, log_m, ctypes.byref(pb), sec, bl, None, ctypes.byref(po), kout) == 3                 # partial triples
    assert con(0, log_m, ctypes.byref(pb), sec, bl, sp, ctypes.byref(po), None) == 3
    assert con(0, log_m, ctypes.byref(pb), sec, None, sp, ctypes.byref(po), kout) == 3
    assert con(0, log_m, ctypes.byref(pb), sec, None, None, ctypes.byref(po), kout) == 3
    assert con(0, log_m, None, sec, bl, sp, ctypes.byref(po), kout) == 3
    assert con(0, log_m, ctypes.byref(pb), None, bl, sp, ctypes.byref(po), kout) == 3
    assert con(0, log_m, ctypes.byref(pb), sec, bl, sp, None, kout) == 3
    assert con(0, 27, ctypes.byref(pb), sec, bl, sp, ctypes.byref(po), kout) == 3
    assert con(5, log_m, ctypes.byref(pb), sec, bl, sp, ctypes.byref(po), kout) == 2
    import dg16_amd
    with pytest.raises(ValueError):
        dg16_amd.contribute_powers(ctx(), curve, log_m, before, 0, 5, 7)
    with pytest.raises(ValueError):
        dg16_amd.contribute_powers(ctx(), curve, log_m, before, 3, 5, 7, blinds=(1, 2, 3))
    context_still_proves()
    assert verify(curve, log_m, before, after, key, sp)[:2] == (0, 0)
