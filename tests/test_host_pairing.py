"""CPU: distributed-groth16_amd/csrc/pairing.h (the Fq12 tower, the optimal ate Miller loop, the final
exponentiation and the Groth16 decision the batch verifier's kernels run) instantiated with the host compiler for
BN254 and BLS12-381 and compared with the oracle (`oracle.pyref.pairing`, pinned by the reference's snarkjs triple).
The tower is the oracle's flat Fq2[w] / (w^6 - xi), so elements compare coefficient by coefficient."""

import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import verify_cases as VC
from oracle.pyref import pairing as PR
from oracle.pyref.curves import CURVES
from oracle.pyref.fields import FQ, FR

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_pairing", "host_pairing.cpp")
SO = os.path.join(HERE, "host_pairing", "libhost_pairing.so")
BOTH = ["bn254", "bls12_381"]


@pytest.fixture(scope="module")
def hp():
    csrc = os.path.join(HERE, "..", "distributed-groth16_amd", "csrc")
    hdrs = [os.path.join(csrc, f) for f in ("pairing.h", "pairing_consts_gen.h", "fp.h", "fp2.h", "ec.h", "types.h",
                                            "consts_gen.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(SO) < os.path.getmtime(p) for p in [SRC] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    L = ctypes.CDLL(SO)
    vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.hp_fq12_op.argtypes = [i, i, vp, vp, vp, sz]
    L.hp_sparse.argtypes = [i, vp, vp, vp, vp, vp]
    L.hp_pairing.argtypes = [i, vp, vp, vp, i]
    L.hp_verify.argtypes = [i, vp, vp, vp, vp, vp, sz, vp, sz, i, vp, sz, vp]
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def pack12(curve, elems):
    F = FQ[curve]
    return np.stack([np.concatenate([VC.fq(curve, c) for pair in e for c in pair]) for e in elems])


def unpack12(curve, arr):
    F = FQ[curve]
    n = F.limbs64
    out = []
    for row in arr:
        v = [F.from_mont(int.from_bytes(row[k * n:(k + 1) * n].tobytes(), "little")) for k in range(12)]
        out.append([(v[2 * k], v[2 * k + 1]) for k in range(6)])
    return out


def rand12(curve, rng):
    q = FQ[curve].p
    return [(rng.randrange(q), rng.randrange(q)) for _ in range(6)]


def op12(hp, curve, op, a, b=None):
    A = pack12(curve, a)
    B = pack12(curve, b) if b is not None else A
    out = np.empty_like(A)
    assert hp.hp_fq12_op(VC.CURVE_ID[curve], op, _p(A), _p(B), _p(out), len(a)) == 0
    return unpack12(curve, out)


def pairing(hp, curve, P, Q, final=True):
    p, q = VC.g1(curve, P), VC.g2(curve, Q)
    out = np.zeros((1, 12 * FQ[curve].limbs64), dtype=np.uint64)
    assert hp.hp_pairing(VC.CURVE_ID[curve], _p(p), _p(q), _p(out), int(final)) == 0
    return unpack12(curve, out)[0]


@pytest.mark.parametrize("curve", BOTH)
def test_fq12_tower_against_the_oracle(hp, curve):
    K = PR.Fq12(curve)
    q = K.q
    rng = random.Random(5)
    a = [rand12(curve, rng) for _ in range(6)] + [K.one, [(q - 1, q - 1)] * 6]
    b = [rand12(curve, rng) for _ in range(7)] + [[(q - 1, 0)] + [(0, q - 1)] * 5]
    assert op12(hp, curve, 0, a, b) == [K.mul(x, y) for x, y in zip(a, b)]
    assert op12(hp, curve, 1, a) == [K.mul(x, x) for x in a]
    inv = op12(hp, curve, 2, a)
    assert all(K.mul(x, y) == K.one for x, y in zip(a, inv))
    assert op12(hp, curve, 3, a[:3]) == [K.pow(x, q) for x in a[:3]]                   # Frobenius
    assert op12(hp, curve, 5, a[:2]) == [K.pow(x, q ** 6) for x in a[:2]]              # conjugation = q^6 Frobenius
    # the easy part maps into the cyclotomic subgroup; there the Granger-Scott squaring is the square
    cyc = op12(hp, curve, 6, a[:4])
    assert cyc[:1] == [K.pow(a[0], (q ** 6 - 1) * (q ** 2 + 1))]
    assert all(K.pow(c, q ** 4 - q ** 2 + 1) == K.one for c in cyc[:2])
    assert op12(hp, curve, 4, cyc) == [K.mul(c, c) for c in cyc]
    x = {"bn254": 4965661367192848881, "bls12_381": -0xd201000000010000}[curve]
    exp = [K.pow(c, abs(x)) for c in cyc[:2]]
    if x < 0:
        exp = [K.pow(e, q ** 6) for e in exp]
    assert op12(hp, curve, 7, cyc[:2]) == exp


@pytest.mark.parametrize("curve", BOTH)
def test_sparse_line_product_equals_dense_product(hp, curve):
    rng = random.Random(6)
    q = FQ[curve].p
    n = FQ[curve].limbs64
    for _ in range(4):
        f = pack12(curve, [rand12(curve, rng)])
        line = np.concatenate([VC.fq(curve, rng.randrange(q)) for _ in range(6)])
        p = np.concatenate([VC.fq(curve, rng.randrange(q)) for _ in range(2)])
        s, d = np.zeros(12 * n, dtype=np.uint64), np.zeros(12 * n, dtype=np.uint64)
        assert hp.hp_sparse(VC.CURVE_ID[curve], _p(f), _p(line), _p(p), _p(s), _p(d)) == 0
        assert s.any() and np.array_equal(s, d)


@pytest.mark.parametrize("curve", BOTH)
def test_pairing_is_bilinear_non_degenerate_and_of_order_r(hp, curve):
    K = PR.Fq12(curve)
    r = FR[curve].p
    c1, c2 = CURVES[curve, "g1"], CURVES[curve, "g2"]
    rng = random.Random(8)
    P, Q = c1.mul(c1.gen, rng.randrange(1, r)), c2.mul(c2.gen, rng.randrange(1, r))
    e = pairing(hp, curve, P, Q)
    assert e != K.one
    assert K.pow(e, r) == K.one
    for a, b in ((2, 3), (rng.randrange(1, r), rng.randrange(1, r)), (r - 1, 1)):
        assert pairing(hp, curve, c1.mul(P, a), c2.mul(Q, b)) == K.pow(e, a * b % r)
    assert pairing(hp, curve, None, Q) == K.one and pairing(hp, curve, P, None) == K.one
    # the final exponentiation raises to a multiple of (q^12 - 1) / r: anything at all lands in the r-torsion
    f = op12(hp, curve, 8, [rand12(curve, rng)])[0]
    assert K.pow(f, r) == K.one


def decide(hp, curve, vk, rows, proofs, mont=False):
    al, be, ga, de, ic = VC.pack_vk(curve, vk)
    x = VC.scalars(curve, rows, mont=mont)
    pr = VC.pack_proofs(curve, proofs)
    out = np.full(len(proofs), 7, dtype=np.uint8)
    rc = hp.hp_verify(VC.CURVE_ID[curve], _p(al), _p(be), _p(ga), _p(de), _p(ic), len(vk["ic"]), _p(x),
                      len(rows[0]) if rows else 0, int(mont), _p(pr), len(proofs), _p(out))
    return rc, [bool(v) for v in out]


def test_decision_on_the_reference_snarkjs_triple_and_its_perturbations(hp):
    vk, cases = VC.snarkjs_cases()
    rc, got = decide(hp, "bn254", vk, [c[0] for c in cases], [c[1] for c in cases])
    assert rc == 0 and got == [c[2] for c in cases]
    vk2, public2, proof2 = VC.snarkjs("snarkjs_test_vectors")        # the reference's mismatched triple
    assert decide(hp, "bn254", vk2, [public2], [proof2]) == (0, [False])
    assert decide(hp, "bn254", vk, [cases[0][0] + [1]], [cases[0][1]])[0] == 1      # LENGTH_MISMATCH


@pytest.mark.parametrize("curve", BOTH)
def test_decision_equals_the_oracle_on_oracle_proofs(hp, curve):
    F = FR[curve]
    r1cs, w, pk = VC.oracle_key(curve, seed=3)
    vk = VC.vk_of(pk)
    proof = VC.oracle_proof(curve, pk, r1cs, w, seed=9)
    other = VC.oracle_proof(curve, pk, r1cs, w, seed=10)
    public = w[1:r1cs["num_instance"]]
    wrong = [public[0], (public[1] + 5) % F.p]
    cases = [(public, proof), (wrong, proof), (public, (proof[0], proof[1], other[2])),
             (public, VC.rerandomise(curve, proof, 12345)), (public, (None, proof[1], proof[2])),
             (public, (proof[0], proof[1], None))]
    want = [PR.groth16_verify(curve, vk, x, p) for x, p in cases]
    assert want[:4] == [True, False, False, True]
    rc, got = decide(hp, curve, vk, [c[0] for c in cases], [c[1] for c in cases])
    assert rc == 0 and got == want
    # Montgomery-form inputs; an input + r is a rejection of that proof, not the same input
    assert decide(hp, curve, vk, [public], [proof], mont=True) == (0, [True])
    assert decide(hp, curve, vk, [[public[0] + F.p, public[1]]], [proof]) == (0, [False])
    # malformed keys: a point outside the subgroup
    Q = VC.twist_point_outside_g2(curve)
    assert decide(hp, curve, dict(vk, gamma_g2=Q), [public], [proof])[0] == 3
    assert decide(hp, curve, vk, [public], [(proof[0], Q, proof[2])]) == (0, [False])
    if curve == "bls12_381":
        P = VC.g1_point_outside_subgroup(curve)
        assert decide(hp, curve, dict(vk, alpha_g1=P), [public], [proof])[0] == 3
        assert decide(hp, curve, vk, [public, public], [(P, proof[1], proof[2]), (proof[0], proof[1], P)]) == \
            (0, [False, False])
