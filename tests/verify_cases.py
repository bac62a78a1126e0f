"""Shared by tests/test_host_pairing.py and tests/test_gpu_verify.py: packing of oracle values (Python ints) into
the C ABI's layout for any curve, and makers of Groth16 verification cases whose expected verdicts come from the
oracle (`oracle.pyref.pairing.groth16_verify`) and the validation rules of include/dg16.h."""

import json
import os
import random

import numpy as np

from oracle.pyref import groth16 as G
from oracle.pyref import pairing as PR
from oracle.pyref.curves import CURVES
from oracle.pyref.fields import FQ, FR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CURVE_ID = {"bn254": 0, "bls12_381": 1, "bls12_377": 2}


def raw(v, nbytes):
    """v as little-endian limbs, NOT reduced."""
    return np.frombuffer(int(v).to_bytes(nbytes, "little"), dtype=np.uint64)


def fq(curve, v):
    return np.frombuffer(FQ[curve].to_bytes(v, mont=True), dtype=np.uint64)


def g1(curve, P):
    n = FQ[curve].limbs64
    return np.zeros(2 * n, dtype=np.uint64) if P is None else np.concatenate([fq(curve, P[0]), fq(curve, P[1])])


def g2(curve, P):
    n = FQ[curve].limbs64
    if P is None:
        return np.zeros(4 * n, dtype=np.uint64)
    return np.concatenate([fq(curve, P[0][0]), fq(curve, P[0][1]), fq(curve, P[1][0]), fq(curve, P[1][1])])


def scalars(curve, rows, mont=False):
    """rows of public inputs -> [n_proofs][n_public][4] uint64; values are taken as they are (no reduction) unless
    mont."""
    F = FR[curve]
    n_public = len(rows[0]) if rows else 0
    out = np.zeros((len(rows), n_public, 4), dtype=np.uint64)
    for i, row in enumerate(rows):
        for j, v in enumerate(row):
            out[i, j] = raw(F.to_mont(v % F.p) if mont else v, 32)
    return out


def pack_vk(curve, vk):
    return (g1(curve, vk["alpha_g1"]), g2(curve, vk["beta_g2"]), g2(curve, vk["gamma_g2"]), g2(curve, vk["delta_g2"]),
            np.stack([g1(curve, P) for P in vk["ic"]]))


def pack_proof(curve, proof):
    A, B, C = proof
    return np.concatenate([g1(curve, A), g2(curve, B), g1(curve, C)])


def pack_proofs(curve, proofs):
    n = 8 * FQ[curve].limbs64
    return np.stack([pack_proof(curve, p) for p in proofs]) if proofs else np.zeros((0, n), dtype=np.uint64)


def snarkjs(d="snarkjs_million"):
    vk = PR.snarkjs_vk(json.load(open(os.path.join(GOLD, d, "verification_key.json"))))
    proof = PR.snarkjs_proof(json.load(open(os.path.join(GOLD, d, "proof.json"))))
    public = [int(x) for x in json.load(open(os.path.join(GOLD, d, "public.json")))]
    return vk, public, proof


def snarkjs_cases():
    """The reference's `million` triple and the perturbations tests/test_verify.py applies to it: (public, proof,
    expected verdict)."""
    q = FQ["bn254"].p
    vk, public, (A, B, C) = snarkjs()
    return vk, [
        (public, (A, B, C), True),
        ([public[0] + 1], (A, B, C), False),
        (public, ((A[0], q - A[1]), B, C), False),
        (public, (A, B, A), False),                                  # C replaced by another curve point
        (public, ((A[0], (A[1] + 1) % q), B, C), False),             # off the curve: a rejection
    ]


def vk_of(pk):
    return {"alpha_g1": pk["alpha_g1"], "beta_g2": pk["beta_g2"], "gamma_g2": pk["gamma_g2"],
            "delta_g2": pk["delta_g2"], "ic": pk["gamma_abc_g1"]}


def oracle_key(curve, seed, nc=11, ni=3, nw=9):
    """A small satisfied R1CS, its key from the oracle's setup, and K witnesses' worth of material."""
    F = FR[curve]
    r1cs, w = G.synthetic_r1cs(F, nc, ni, nw, seed=seed)
    rng = random.Random(seed + 100)
    td = tuple(rng.randrange(1, F.p) for _ in range(5))
    pk, _ = G.setup(curve, r1cs, td)
    return r1cs, w, pk


def oracle_proof(curve, pk, r1cs, w, seed):
    F = FR[curve]
    rng = random.Random(seed)
    return G.create_proof(curve, pk, rng.randrange(1, F.p), rng.randrange(1, F.p), r1cs, w)


def rerandomise(curve, proof, t):
    """(tA, t^-1 B, C) verifies whenever (A, B, C) does."""
    r = FR[curve].p
    c1, c2 = CURVES[curve, "g1"], CURVES[curve, "g2"]
    A, B, C = proof
    return c1.mul(A, t % r), c2.mul(B, pow(t, r - 2, r)), C


def twist_point_outside_g2(curve, seed=1):
    """A point of E'(Fq2) that is not in the order-r subgroup (found by trial; membership decided by the oracle)."""
    c2 = CURVES[curve, "g2"]
    q, r = FQ[curve].p, FR[curve].p
    rng = random.Random(seed)
    while True:
        x = (rng.randrange(q), rng.randrange(q))
        y = _sqrt_fq2(curve, c2, x)
        if y is not None and c2.on_curve((x, y)) and c2.mul((x, y), r) is not None:
            return (x, y)


def _sqrt_fq2(curve, c2, x):
    """Square root in Fq2 = Fq[u] / (u^2 + 1) for q = 3 mod 4 (complex method), None for a non-square."""
    q = FQ[curve].p
    F2 = c2.F
    a = F2.add(F2.mul(F2.mul(x, x), x), c2.b)
    if a == (0, 0):
        return (0, 0)
    n = (a[0] * a[0] + a[1] * a[1]) % q            # norm
    s = pow(n, (q + 1) // 4, q)
    if s * s % q != n:
        return None
    inv2 = pow(2, q - 2, q)
    for sg in (s, q - s):
        t = (a[0] + sg) * inv2 % q
        y0 = pow(t, (q + 1) // 4, q)
        if y0 * y0 % q == t and y0:
            y = (y0, a[1] * pow(2 * y0, q - 2, q) % q)
            if F2.mul(y, y) == a:
                return y
    return None


def g1_point_outside_subgroup(curve, seed=1):
    """BLS12-381: a point of E(Fq) outside the order-r subgroup."""
    c1 = CURVES[curve, "g1"]
    q, r = FQ[curve].p, FR[curve].p
    assert q % 4 == 3
    rng = random.Random(seed)
    while True:
        x = rng.randrange(q)
        a = (x * x * x + c1.b) % q
        y = pow(a, (q + 1) // 4, q)
        if y * y % q == a and c1.mul((x, y), r) is not None:
            return (x, y)
