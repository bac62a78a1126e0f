"""The Libsnark QAP reduction (ark-groth16's default `LibsnarkReduction`; DG16_F_QAP_LIBSNARK) restated on Python big
ints, and the checks that pin the restatement itself.  tests/test_gpu_libsnark.py measures the GPU against this model.

Definition (include/dg16.h, "The two QAP reductions"): with m = D::new(num_constraints + num_inputs).size(), a, b, c the
length-m vectors of <A_i, w>, <B_i, w>, <C_i, w> on the constraint rows, w[j] in a[num_constraints + j] and zeros
elsewhere, A, B, C their interpolants on the domain and Z = X^m - 1: h is the polynomial of degree <= m - 2 with
h Z = A B - C, given by its m coefficients (the top one zero); the key's h_query[i] = tau^i Z(tau) / delta, i < m - 1.

The model computes h the way arkworks does (iNTT, coset NTT at g = F::GENERATOR, divide by Z(g), coset iNTT) with the
oracle's Domain.  The checks below do NOT use a transform: A(x), B(x), C(x) at a random x come from the domain values by
the barycentric formula, h(x) by Horner."""

import random

import pytest

from oracle.pyref import groth16 as G
from oracle.pyref.fields import FR
from oracle.pyref.poly import Domain

GENERATORS = {"bn254": 5, "bls12_381": 7, "bls12_377": 22}


def libsnark_abc(r1cs, w, F):
    """a, b, c, domain: G.qap's a and b, and c from the C matrix."""
    a, b, _, dom = G.qap(r1cs, w, F)
    c = [0] * dom.size
    for i in range(r1cs["num_constraints"]):
        c[i] = G.evaluate_constraint(r1cs["c"][i], w, F.p)
    return a, b, c, dom


def libsnark_h(a, b, c, dom):
    """The m coefficients of (A B - C) / Z from the domain values a, b, c."""
    F, p, m = dom.F, dom.p, dom.size
    g = F.generator
    coset = dom.get_coset(g)
    ea, eb, ec = (coset.fft(dom.ifft(v)) for v in (a, b, c))
    zg_inv = F.inv((pow(g, m, p) - 1) % p)
    return coset.ifft([(x * y - z) * zg_inv % p for x, y, z in zip(ea, eb, ec)])


def libsnark_setup_scalars(r1cs, F, trapdoor):
    """G.setup_scalars with the LibsnarkReduction h_query scalars: tau^i Z(tau) / delta for i < m - 1, then 0."""
    p = F.p
    delta, tau = trapdoor[3], trapdoor[4]
    sc = dict(G.setup_scalars(r1cs, F, trapdoor))
    m = sc["m"]
    k = sc["zt"] * F.inv(delta) % p
    sc["h"] = [pow(tau, i, p) * k % p for i in range(m - 1)] + [0]
    return sc


def libsnark_proof_scalars(r1cs, F, trapdoor, sc, r, s, w, h):
    """Discrete logs of (A, B, C) of prove.rs:21-136 over a Libsnark key, with the H term as the MSM computes it:
    sum_i h_i h_query_i."""
    p = F.p
    alpha, beta, _, delta, _ = trapdoor
    ni = r1cs["num_instance"]
    w = [x % p for x in w]
    a = (alpha + sum(x * y for x, y in zip(sc["a"], w)) + r * delta) % p
    b = (beta + sum(x * y for x, y in zip(sc["b"], w)) + s * delta) % p
    aux = sum(x * y for x, y in zip(sc["l"], w[ni:])) % p
    hq = sum(x * y for x, y in zip(sc["h"], h)) % p
    c = (aux + hq + s * a + r * b - r * s % p * delta) % p
    return a, b, c


def barycentric(vals, dom, x):
    """The interpolant of `vals` on the domain, evaluated at x off the domain: (x^m - 1) / m * sum_i v_i w^i / (x - w^i)."""
    p, m = dom.p, dom.size
    acc, wi = 0, 1
    for v in vals:
        acc = (acc + v * wi % p * pow((x - wi) % p, p - 2, p)) % p
        wi = wi * dom.group_gen % p
    return (pow(x, m, p) - 1) * dom.size_inv % p * acc % p


def horner(coeffs, x, p):
    acc = 0
    for cf in reversed(coeffs):
        acc = (acc * x + cf) % p
    return acc


def quotient_identity_holds(h, a, b, c, dom, x):
    """h(x) (x^m - 1) == A(x) B(x) - C(x) at the point x."""
    p = dom.p
    lhs = horner(h, x, p) * (pow(x, dom.size, p) - 1) % p
    return lhs == (barycentric(a, dom, x) * barycentric(b, dom, x) - barycentric(c, dom, x)) % p


def instance(F, m, seed, slack=0):
    """A satisfied synthetic system whose domain has exactly m points (num_constraints + num_instance = m - slack)."""
    ni = 2
    nc = m - ni - slack
    r1cs, w = G.synthetic_r1cs(F, num_constraints=nc, num_instance=ni, num_witness=nc + 3, seed=seed)
    assert Domain(F, nc + ni).size == m
    return r1cs, w


def test_generators_are_the_oracles():
    for curve, g in GENERATORS.items():
        assert FR[curve].generator == g


@pytest.mark.parametrize("curve", ["bn254", "bls12_381", "bls12_377"])
@pytest.mark.parametrize("m,slack", [(8, 0), (16, 3), (64, 0), (64, 20)])
def test_quotient_identity_at_a_random_point(curve, m, slack):
    F = FR[curve]
    r1cs, w = instance(F, m, seed=m + slack, slack=slack)
    assert G.is_satisfied(r1cs, w, F.p)
    a, b, c, dom = libsnark_abc(r1cs, w, F)
    assert dom.size == m and c[:len(r1cs["c"])] == [x * y % F.p for x, y in zip(a, b)][:len(r1cs["c"])]
    h = libsnark_h(a, b, c, dom)
    assert len(h) == m and h[m - 1] == 0
    rng = random.Random(m)
    for _ in range(2):
        x = rng.randrange(2, F.p)
        assert pow(x, m, F.p) != 1
        assert quotient_identity_holds(h, a, b, c, dom, x)
    # the identity is a check: a perturbed coefficient fails it
    h2 = list(h)
    h2[1] = (h2[1] + 1) % F.p
    assert not quotient_identity_holds(h2, a, b, c, dom, x)


def test_unsatisfied_witness_has_no_exact_quotient():
    """For a witness that violates a row, A B - C is not a multiple of Z: whatever the pipeline returns fails the identity
    (the reason dg16_qap_r1cs reports violations)."""
    F = FR["bn254"]
    r1cs, w = instance(F, 16, seed=3)
    w = list(w)
    w[-1] = (w[-1] + 1) % F.p
    assert not G.is_satisfied(r1cs, w, F.p)
    a, b, c, dom = libsnark_abc(r1cs, w, F)
    h = libsnark_h(a, b, c, dom)
    assert not quotient_identity_holds(h, a, b, c, dom, 123456789)


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
@pytest.mark.parametrize("m", [8, 64])
def test_model_proof_satisfies_groth16_in_the_exponent(curve, m):
    F = FR[curve]
    p = F.p
    r1cs, w = instance(F, m, seed=7 * m, slack=1)
    rng = random.Random(m)
    td = tuple(rng.randrange(2, p) for _ in range(5))
    r, s = rng.randrange(p), rng.randrange(p)
    sc = libsnark_setup_scalars(r1cs, F, td)
    assert len(sc["h"]) == m and sc["h"][m - 1] == 0
    a, b, c, dom = libsnark_abc(r1cs, w, F)
    h = libsnark_h(a, b, c, dom)
    # the H term of the proof is h(tau) Z(tau) / delta
    delta, tau = td[3], td[4]
    assert sum(x * y for x, y in zip(sc["h"], h)) % p == horner(h, tau, p) * sc["zt"] % p * F.inv(delta) % p
    abc = libsnark_proof_scalars(r1cs, F, td, sc, r, s, w, h)
    assert G.verify_in_exponent(r1cs, F, td, sc, abc, w)
    # ... and equals the closed form the oracle derives from the trapdoor, which knows nothing of h
    assert abc == G.proof_scalars_from_trapdoor(r1cs, F, td, sc, r, s, w)
    # the circom witness map against the Libsnark key is not a proof: the flag selects something
    h_circom = G.witness_map_from_abc(a, b, c, dom)
    assert not G.verify_in_exponent(r1cs, F, td, sc, libsnark_proof_scalars(r1cs, F, td, sc, r, s, w, h_circom), w)
    # an unsatisfying witness is not accepted either
    w_bad = list(w)
    w_bad[-1] = (w_bad[-1] + 1) % p
    a2, b2, c2, _ = libsnark_abc(r1cs, w_bad, F)
    bad = libsnark_proof_scalars(r1cs, F, td, sc, r, s, w_bad, libsnark_h(a2, b2, c2, dom))
    assert not G.verify_in_exponent(r1cs, F, td, sc, bad, w_bad)
