"""GPU: dg16_srs_verify (Context.srs_verify, keygen.verify_powers) for BN254 and BLS12-381.  Every transcript is made of
multiples of the generators whose discrete logarithms the test knows: the powers come from keygen.powers_from_trapdoor
with known (alpha, beta, tau), a tampering adds k G to a point.  The expected `failed` word is computed here, from the
exponents and the test's own fixed-seed coefficients (e(x G1, y G2) = e(x' G1, y' G2) iff x y = x' y' mod r), never
taken from the library; once, at log_m = 2, the same five equations are also evaluated by the oracle's pairing."""

import ctypes
import functools
import random

import numpy as np
import pytest

import points_check_cases as PC
from oracle import corc
from oracle.pyref import pairing as PR
from oracle.pyref.curves import CURVES
from oracle.pyref.fields import FR
from gpu_util import ctx

pytestmark = pytest.mark.gpu

BOTH = ["bn254", "bls12_381"]
SMALL = [1, 2, 5]
BAD_POINT, IDENTITY, TAU_G1, TAU_G2, ALPHA, BETA, BETA_G2 = 1, 2, 4, 8, 16, 32, 64
NAMES = ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2")
GROUP_OF = (1, 2, 1, 1, 2)


def context_still_proves():
    """A small proof through the resident prover equals the oracle's: the context is usable after an error."""
    import bench
    import torch
    _, ok = bench.cpu_baseline_and_parity(ctx(), torch.device("cuda", 0), 8)
    assert ok


def coefficients(log_m, seed):
    """2m - 2 integers in [1, 2^128), fixed by the seed"""
    rng = random.Random(seed)
    return [rng.randrange(1, 1 << 128) for _ in range(2 * (1 << log_m) - 2)]


def coeff_arr(rho):
    return np.frombuffer(b"".join(v.to_bytes(16, "little") for v in rho), dtype=np.uint64).reshape(-1, 2).copy()


def secrets_of(curve, log_m):
    rng = random.Random(1000 + 10 * log_m + corc.CURVES[curve])
    r = FR[curve].p
    return rng.randrange(2, r), rng.randrange(2, r), rng.randrange(2, r)


class Transcript:
    """The exponents of the five arrays and the packed points that go with them."""

    def __init__(self, curve, log_m, exps, arrays):
        self.curve, self.log_m = curve, log_m
        self.exps = [list(e) for e in exps]                # t [2m - 1], u [m], a [m], b [m], [beta]
        self.arrays = [np.array(a, dtype=np.uint64, copy=True) for a in arrays]

    def copy(self):
        return Transcript(self.curve, self.log_m, self.exps, self.arrays)

    def set_exponent(self, array, index, value):
        """the point becomes value * G"""
        value %= FR[self.curve].p
        self.exps[array][index] = value
        self.arrays[array][index] = ctx().fixed_base_mul(self.curve, GROUP_OF[array], corc.ints_to_arr([value], 4))[0]
        return self

    def add_multiple(self, array, index, k):
        return self.set_exponent(array, index, self.exps[array][index] + k)

    def set_point(self, array, index, words):
        """a point with no exponent (bad points only)"""
        self.exps[array][index] = None
        self.arrays[array][index] = words
        return self

    def expected(self, rho):
        """the word the exponents give under the coefficients rho (no bad point in the transcript)"""
        r = FR[self.curve].p
        t, u, a, b, (bg,) = self.exps
        m = 1 << self.log_m
        if 0 in (t[0], t[1], u[0], u[1], a[0], b[0], bg):
            return IDENTITY
        comb = lambda v, n, shift: sum(rho[j] * v[j + shift] for j in range(n)) % r     # noqa: E731
        word = 0
        if comb(t, 2 * m - 2, 0) * u[1] % r != comb(t, 2 * m - 2, 1) * u[0] % r:
            word |= TAU_G1
        if t[1] * comb(u, m - 1, 0) % r != t[0] * comb(u, m - 1, 1) % r:
            word |= TAU_G2
        if comb(a, m - 1, 0) * u[1] % r != comb(a, m - 1, 1) * u[0] % r:
            word |= ALPHA
        if comb(b, m - 1, 0) * u[1] % r != comb(b, m - 1, 1) * u[0] % r:
            word |= BETA
        if b[0] * u[0] % r != t[0] * bg % r:
            word |= BETA_G2
        return word

    def verify(self, rho):
        return ctx().srs_verify(self.curve, self.log_m, *self.arrays, coeff_arr(rho))


@functools.lru_cache(maxsize=None)
def _valid(curve, log_m):
    import dg16_amd
    r = FR[curve].p
    alpha, beta, tau = secrets_of(curve, log_m)
    m = 1 << log_m
    pw = [pow(tau, j, r) for j in range(2 * m - 1)]
    exps = (pw, pw[:m], [alpha * x % r for x in pw[:m]], [beta * x % r for x in pw[:m]], [beta])
    return Transcript(curve, log_m, exps, dg16_amd.powers_from_trapdoor(ctx(), curve, log_m, alpha, beta, tau))


def valid(curve, log_m):
    return _valid(curve, log_m).copy()


def indices(n):
    return sorted({0, n // 2, n - 1})


@pytest.mark.parametrize("log_m", SMALL)
@pytest.mark.parametrize("curve", BOTH)
def test_valid_transcript_is_accepted(curve, log_m):
    tr = valid(curve, log_m)
    rho = coefficients(log_m, 1)
    assert tr.expected(rho) == 0
    assert tr.verify(rho) == (0, 0, 0, 0)


@pytest.mark.parametrize("log_m", SMALL)
@pytest.mark.parametrize("curve", BOTH)
def test_one_tampered_point(curve, log_m):
    """Each of T, U, A, B tampered at its first, a middle and its last index (T's last is 2m - 2: where an off-by-one of
    the shifted sum would hide): the whole word is the one the exponents give."""
    rho = coefficients(log_m, 2)
    rng = random.Random(3)
    for array in range(4):
        n = len(valid(curve, log_m).exps[array])
        for index in indices(n):
            tr = valid(curve, log_m).add_multiple(array, index, rng.randrange(1, 1 << 64))
            want = tr.expected(rho)
            assert want != 0, (array, index)
            assert tr.verify(rho) == (want, 0, 0, 0), (NAMES[array], index)
    # the words are not all alike: T_1 also enters the TAU_G2 equation, T's last index only TAU_G1
    m = 1 << log_m
    assert valid(curve, log_m).add_multiple(0, 1, 5).expected(rho) & TAU_G2
    assert valid(curve, log_m).add_multiple(0, 2 * m - 2, 5).expected(rho) == TAU_G1


@pytest.mark.parametrize("log_m", SMALL)
@pytest.mark.parametrize("curve", BOTH)
def test_other_tau_in_g2_and_other_beta(curve, log_m):
    r = FR[curve].p
    rho = coefficients(log_m, 4)
    tr = valid(curve, log_m)
    other = secrets_of(curve, log_m + 50)[2]
    for j in range(1, 1 << log_m):
        tr.set_exponent(1, j, pow(other, j, r))
    want = tr.expected(rho)
    assert want & TAU_G1 and want & TAU_G2 and not want & BETA_G2
    assert tr.verify(rho) == (want, 0, 0, 0)
    tr = valid(curve, log_m).add_multiple(4, 0, 1)
    assert tr.expected(rho) == BETA_G2
    assert tr.verify(rho) == (BETA_G2, 0, 0, 0)


@pytest.mark.parametrize("log_m", SMALL)
@pytest.mark.parametrize("curve", BOTH)
def test_identity_heads(curve, log_m):
    """Each of T_0, T_1, U_0, U_1, A_0, B_0, beta_g2 as the identity: bit 2, and the pairing bits stay clear."""
    rho = coefficients(log_m, 5)
    for array, index in ((0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (3, 0), (4, 0)):
        tr = valid(curve, log_m).set_exponent(array, index, 0)
        assert not tr.arrays[array][index].any()
        assert tr.expected(rho) == IDENTITY
        assert tr.verify(rho) == (IDENTITY, 0, 0, 0), (NAMES[array], index)


def bad_kinds(curve, group):
    """one unreduced, one off-curve and (where the group has a cofactor) one off-subgroup point"""
    out = {}
    for _, w, v0, v1 in PC.cases(curve, group):
        if v1 != PC.GOOD:
            out.setdefault(v1, w)
    return [out[k] for k in sorted(out)]


@pytest.mark.parametrize("log_m", SMALL)
@pytest.mark.parametrize("curve", BOTH)
def test_bad_points(curve, log_m):
    """One off-subgroup, one off-curve and one unreduced point, in each array in turn: bit 1 alone with the array, the
    index and the count; the pairing bits stay clear."""
    rho = coefficients(log_m, 6)
    for array in range(5):
        kinds = bad_kinds(curve, GROUP_OF[array])
        assert len(kinds) == (2 if (curve, GROUP_OF[array]) == ("bn254", 1) else 3)
        n = len(valid(curve, log_m).exps[array])
        for k, w in enumerate(kinds):
            index = indices(n)[k % len(indices(n))]
            tr = valid(curve, log_m).set_point(array, index, w)
            assert tr.verify(rho) == (BAD_POINT, array, index, 1), (NAMES[array], index, k)
    # two arrays with bad points, one of them with two: the first array and its smallest index are reported
    tr = valid(curve, log_m)
    tr.set_point(3, 1, bad_kinds(curve, 1)[0]).set_point(3, 0, bad_kinds(curve, 1)[1]).set_point(1, 1, bad_kinds(curve, 2)[0])
    assert tr.verify(rho) == (BAD_POINT, 1, 1, 3)
    # a bad point and an identity head together: both bits, nothing else
    tr = valid(curve, log_m).set_point(2, 1, bad_kinds(curve, 1)[0]).set_exponent(4, 0, 0)
    assert tr.verify(rho) == (BAD_POINT | IDENTITY, 2, 1, 1)


@pytest.mark.parametrize("log_m", [2, 5])
@pytest.mark.parametrize("curve", BOTH)
def test_a_tampering_that_cancels_under_the_known_coefficients(curve, log_m):
    """T_i += d_i G and T_k += d_k G with d_i c_i + d_k c_k = 0, c_j = rho_j tau - rho_(j-1) the weight of T_j in the
    TAU_G1 equation: accepted under rho, rejected under other coefficients -- the library computes the stated combination
    and nothing else.  (log_m = 1 has no such pair: T_0 and T_1 enter other equations, which leaves one index.)"""
    r = FR[curve].p
    tau = secrets_of(curve, log_m)[2]
    rho = coefficients(log_m, 7)
    m = 1 << log_m
    i, k = 2, 2 * m - 3
    c = lambda j: (rho[j] * tau - rho[j - 1]) % r     # noqa: E731
    tr = valid(curve, log_m).add_multiple(0, i, c(k)).add_multiple(0, k, -c(i))
    assert tr.expected(rho) == 0
    assert tr.verify(rho) == (0, 0, 0, 0)
    other = coefficients(log_m, 8)
    assert tr.expected(other) == TAU_G1
    assert tr.verify(other) == (TAU_G1, 0, 0, 0)


def test_the_exponent_argument_against_the_oracles_pairing():
    """BN254, log_m = 2: the five equations evaluated by oracle.pyref.pairing on points the oracle's group law makes
    from the exponents agree, bit by bit, with the words computed from the exponents -- for the valid transcript and a
    tampered one -- and with the library."""
    curve, log_m = "bn254", 2
    r = FR[curve].p
    c1, c2 = CURVES[curve, "g1"], CURVES[curve, "g2"]
    rho = coefficients(log_m, 9)
    m = 1 << log_m
    g1 = lambda k: c1.mul(c1.gen, k % r)      # noqa: E731
    g2 = lambda k: c2.mul(c2.gen, k % r)      # noqa: E731
    for tr in (valid(curve, log_m), valid(curve, log_m).add_multiple(0, 1, 77)):
        t, u, a, b, (bg,) = tr.exps
        comb = lambda v, n, shift: sum(rho[j] * v[j + shift] for j in range(n)) % r     # noqa: E731
        eqs = {TAU_G1: ((g1(comb(t, 2 * m - 2, 0)), g2(u[1])), (g1(comb(t, 2 * m - 2, 1)), g2(u[0]))),
               TAU_G2: ((g1(t[1]), g2(comb(u, m - 1, 0))), (g1(t[0]), g2(comb(u, m - 1, 1)))),
               ALPHA: ((g1(comb(a, m - 1, 0)), g2(u[1])), (g1(comb(a, m - 1, 1)), g2(u[0]))),
               BETA: ((g1(comb(b, m - 1, 0)), g2(u[1])), (g1(comb(b, m - 1, 1)), g2(u[0]))),
               BETA_G2: ((g1(b[0]), g2(u[0])), (g1(t[0]), g2(bg)))}
        word = 0
        for bit, ((p1, q1), (p2, q2)) in eqs.items():
            if not PR.pairing_product_is_one(curve, [(p1, q1), (c1.neg(p2), q2)]):
                word |= bit
        assert word == tr.expected(rho)
        assert tr.verify(rho) == (word, 0, 0, 0)
    assert word == TAU_G1 | TAU_G2


@pytest.mark.parametrize("curve", BOTH)
def test_log_12(curve):
    """Sums of 8190 and 4095 terms (the bucket path proper): the valid transcript and two tamperings."""
    log_m = 12
    rho = coefficients(log_m, 10)
    tr = valid(curve, log_m)
    assert tr.expected(rho) == 0
    assert tr.verify(rho) == (0, 0, 0, 0)
    m = 1 << log_m
    for array, index in ((0, 2 * m - 2), (2, m // 2 + 1)):
        bad = valid(curve, log_m).add_multiple(array, index, 1)
        want = bad.expected(rho)
        assert want == (TAU_G1, 0, ALPHA)[array]
        assert bad.verify(rho) == (want, 0, 0, 0), (array, index)


def test_refusals_and_the_context_proves_afterwards():
    from dg16_amd.lib import SrsPowers, SrsReportC
    c_ = ctx()
    L, h = c_.L, c_.h
    log_m = 2
    tr = valid("bn254", log_m)
    rho = coeff_arr(coefficients(log_m, 11))
    addr = [a.ctypes.data for a in tr.arrays]
    pw, rep = SrsPowers(*addr), SrsReportC()
    cp = rho.ctypes.data_as(ctypes.c_void_p)
    call = lambda curve, lm, p, c, rp: L.dg16_srs_verify(h, curve, lm, p, c, rp)     # noqa: E731
    assert call(0, log_m, ctypes.byref(pw), cp, ctypes.byref(rep)) == 0 and rep.failed == 0
    zero = rho.copy()
    zero[len(zero) - 1] = 0                                                  # the last coefficient is zero
    assert call(0, log_m, ctypes.byref(pw), zero.ctypes.data_as(ctypes.c_void_p), ctypes.byref(rep)) == 3
    zero = rho.copy()
    zero[0] = 0
    assert call(0, log_m, ctypes.byref(pw), zero.ctypes.data_as(ctypes.c_void_p), ctypes.byref(rep)) == 3
    assert call(0, log_m, None, cp, ctypes.byref(rep)) == 3                  # NULL pointers
    assert call(0, log_m, ctypes.byref(pw), None, ctypes.byref(rep)) == 3
    assert call(0, log_m, ctypes.byref(pw), cp, None) == 3
    for j in range(5):
        f = list(addr)
        f[j] = None
        assert call(0, log_m, ctypes.byref(SrsPowers(*f)), cp, ctypes.byref(rep)) == 3, j
    assert call(0, 0, ctypes.byref(pw), cp, ctypes.byref(rep)) == 3          # log_m = 0
    assert call(0, 27, ctypes.byref(pw), cp, ctypes.byref(rep)) == 3         # log_m = 27
    assert call(2, log_m, ctypes.byref(pw), cp, ctypes.byref(rep)) == 7      # BLS12-377: no pairing here
    assert call(5, log_m, ctypes.byref(pw), cp, ctypes.byref(rep)) == 2      # unknown curve
    assert L.dg16_srs_verify(None, 0, log_m, ctypes.byref(pw), cp, ctypes.byref(rep)) == 3
    context_still_proves()
    assert tr.verify(coefficients(log_m, 11)) == (0, 0, 0, 0)


def test_verify_powers_report_and_generators():
    import dg16_amd
    from dg16_amd import keygen
    curve, log_m = "bls12_381", 2
    tr = valid(curve, log_m)
    gens = (corc.generator(curve, 1)[0], corc.generator(curve, 2)[0])
    rep = keygen.verify_powers(ctx(), curve, log_m, *tr.arrays, generators=gens)        # coefficients drawn here
    assert rep.accepted and rep.failed == 0 and rep.generators_match is True and rep.reasons == []
    rep = keygen.verify_powers(ctx(), curve, log_m, *tr.arrays, generators=(gens[0], tr.arrays[1][1]))
    assert not rep.accepted and rep.failed == 0 and rep.generators_match is False
    bad = valid(curve, log_m).add_multiple(3, 2, 9)
    rep = keygen.verify_powers(ctx(), curve, log_m, *bad.arrays)
    assert not rep.accepted and rep.failed == keygen.SrsReport.BETA and rep.beta and not rep.tau_g1
    assert rep.reasons == ["beta"] and rep.generators_match is None and rep.bad_array is None
    off = valid(curve, log_m).set_point(1, 3, bad_kinds(curve, 2)[-1])
    rep = keygen.verify_powers(ctx(), curve, log_m, *off.arrays)
    assert rep.failed == 1 and rep.bad_point and (rep.bad_array, rep.bad_index, rep.n_bad_points) == ("tau_g2", 3, 1)
    assert dg16_amd.verify_powers is keygen.verify_powers and dg16_amd.SrsReport is keygen.SrsReport


def test_verified_powers_to_the_oracles_key():
    """verify_powers accepted -> srs_from_powers -> generate_parameters_from_srs: the key equals the oracle's at log 5."""
    import dg16_amd
    from test_gpu_setup import system_of, expected_arrays
    from test_gpu_setup_srs import NAMES as KEY_NAMES, oracle_key
    curve, log_m = "bn254", 5
    F = FR[curve]
    r1cs, _, td, pk = oracle_key(curve, log_m)
    powers = dg16_amd.powers_from_trapdoor(ctx(), curve, log_m, td[0], td[1], td[4])
    rep = dg16_amd.verify_powers(ctx(), curve, log_m, *powers, coeffs=coeff_arr(coefficients(log_m, 12)),
                                 generators=(corc.generator(curve, 1)[0], corc.generator(curve, 2)[0]))
    assert rep.accepted
    srs = dg16_amd.srs_from_powers(ctx(), curve, log_m, *powers)
    params = dg16_amd.generate_parameters_from_srs(ctx(), curve, system_of(F, r1cs), srs, in_subgroup=True)
    exp = expected_arrays(curve, pk)
    for name in KEY_NAMES:
        assert np.array_equal(params.host(name), exp[name]), name
