"""The recoding, the per-product loops and the re-randomization arithmetic of distributed-groth16_amd/csrc/points_mul.h,
compiled with the host compiler (tests/host_arith/host_points_mul.cpp) and compared with the oracle: the CPU runs the
text the kernel runs.  Group operations are counted by the shim's Ops and held to the budgets of DESIGN.md 2.9."""

import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import points_mul_cases as PM
import verify_cases as VC
from oracle import corc
from oracle.pyref.fields import FR

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_arith", "host_points_mul.cpp")
SO = os.path.join(HERE, "host_arith", "libhost_points_mul.so")
CSRC = os.path.join(HERE, "..", "distributed-groth16_amd", "csrc")

# the budgets of the issue: (doublings, additions) per product, table construction included
BUDGET_PLAIN = (256, 72)
BUDGET_SPLIT = (136, 80)


@pytest.fixture(scope="module")
def hp():
    hdrs = [os.path.join(CSRC, f) for f in ("points_mul.h", "glv_endo.h", "glv.h", "fp.h", "fp2.h", "ec.h", "types.h",
                                            "consts_gen.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(SO) < os.path.getmtime(p) for p in [SRC] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-o", SO, SRC])
    L = ctypes.CDLL(SO)
    vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.hp_params.argtypes = [vp]
    L.hp_digits.argtypes = [vp, vp]
    L.hp_split.argtypes = [i, vp, vp, vp, vp, vp]
    L.hp_lambda.argtypes = [i, vp]
    L.hp_may_split.argtypes = [i, i]
    L.hp_mul.argtypes = [i, i, vp, vp, sz, vp, vp]
    L.hp_rerandomize.argtypes = [i, vp, vp, vp, i, vp]
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _params(hp):
    out = np.zeros(3, dtype=np.int32)
    hp.hp_params(_p(out))
    return [int(v) for v in out]


def _words(k):
    return np.frombuffer(int(k).to_bytes(32, "little"), dtype=np.uint32).copy()


def test_window_width_is_the_one_the_scalar_list_assumes(hp):
    w, table, nwin = _params(hp)
    assert w == PM.W and table == 1 << (w - 1) and nwin * w >= 256


@pytest.mark.parametrize("curve", ["bn254", "bls12_381", "bls12_377"])
def test_plain_digits_are_regular_and_exact(hp, curve):
    """sum d_i 2^(w i) = k with every digit in [-2^(w-1), 2^(w-1)], for S and 10 000 random 255-bit scalars."""
    w, table, nwin = _params(hp)
    below, above = PM.scalar_list(curve)
    rng = random.Random(11)
    ks = below + above + [rng.randrange(1 << 255) for _ in range(10000)]
    d = np.zeros(nwin, dtype=np.int8)
    for k in ks:
        kw = _words(k)
        hp.hp_digits(_p(kw), _p(d))
        assert int(np.abs(d).max()) <= table, hex(k)
        assert sum(int(v) << (w * i) for i, v in enumerate(d)) == k, hex(k)


@pytest.mark.parametrize("curve,group", PM.GROUPS)
def test_split_digits_are_exact_and_within_the_window_count(hp, curve, group):
    """k = sum_j k_j LAMBDA^j (mod r), |k_j| < 2^(w nwin - 1) -- the bound that rules out a carry from the top window --
    and the digits of every part reconstruct it.  S (values >= r included: canonical input may hold them) and 10 000
    random scalars per curve."""
    w, table, _ = _params(hp)
    r = FR[curve].p
    g = PM.gid(curve, group)
    lw = np.zeros(8, dtype=np.uint32)
    assert hp.hp_lambda(g, _p(lw)) == 0
    lam = int.from_bytes(lw.tobytes(), "little")
    below, above = PM.scalar_list(curve)
    rng = random.Random(12 + g)
    ks = below + above + [rng.randrange(r) for _ in range(9000)] + [rng.randrange(1 << 255) for _ in range(1000)]
    mags = np.zeros((4, 8), dtype=np.uint32)
    negs = np.zeros(4, dtype=np.int32)
    digits = np.zeros(4 * 64, dtype=np.int8)
    nwin = ctypes.c_int(0)
    for k in ks:
        kw = _words(k)
        dim = hp.hp_split(g, _p(kw), _p(mags), _p(negs), _p(digits), ctypes.byref(nwin))
        assert dim in (2, 4)
        nw = nwin.value
        total = 0
        for j in range(dim):
            m = int.from_bytes(mags[j].tobytes(), "little")
            assert m < 1 << (w * nw - 1), (hex(k), j)
            dj = digits[j * nw:(j + 1) * nw]
            assert int(np.abs(dj).max()) <= table
            assert sum(int(v) << (w * i) for i, v in enumerate(dj)) == m
            total += (-m if negs[j] else m) * pow(lam, j, r)
        assert (total - k) % r == 0, hex(k)


def _points(curve, group):
    """generator, a random subgroup point, the identity; then (cofactor groups) a point outside the subgroup"""
    pts = [corc.generator(curve, group)[0], corc.gen_points(curve, group, 21, 3)[2],
           np.zeros(corc.point_limbs(curve, group), dtype=np.uint64)]
    outside = None
    if (curve, group) in PM.COFACTOR_GROUPS:
        outside = PM.outside_point(curve, group)
    return pts, outside


@pytest.mark.parametrize("curve,group", PM.GROUPS)
def test_products_equal_the_oracle_within_the_budget(hp, curve, group):
    """S x {generator, random subgroup point, identity} through the plain loop and through the split loop, S x {a point
    outside the subgroup} through the plain loop only; every product byte-equal to the oracle's and within the budget of
    doublings and additions."""
    g = PM.gid(curve, group)
    below, above = PM.scalar_list(curve)
    ks = below + above
    pts, outside = _points(curve, group)
    K = corc.ints_to_arr(ks, 4)
    for split, budget in ((0, BUDGET_PLAIN), (1, BUDGET_SPLIT)):
        for P in pts:
            bases = np.ascontiguousarray(np.tile(P, (len(ks), 1)))
            out = np.zeros_like(bases)
            counts = np.zeros((len(ks), 4), dtype=np.uint32)
            assert hp.hp_mul(g, split, _p(bases), _p(K), len(ks), _p(out), _p(counts)) == 0
            for i, k in enumerate(ks):
                assert np.array_equal(out[i], corc.point_mul(curve, group, P[None, :], k)[0]), (split, hex(k))
            assert int(counts[:, 0].max()) <= budget[0] and int(counts[:, 1].max()) <= budget[1], counts.max(axis=0)
    if outside is not None:
        P = PM.pack_point(curve, group, outside)
        bases = np.ascontiguousarray(np.tile(P, (len(ks), 1)))
        out = np.zeros_like(bases)
        counts = np.zeros((len(ks), 4), dtype=np.uint32)
        assert hp.hp_mul(g, 0, _p(bases), _p(K), len(ks), _p(out), _p(counts)) == 0
        for i, k in enumerate(ks):
            assert np.array_equal(out[i], PM.ref_mul_any(curve, group, outside, k)), hex(k)
        assert int(counts[:, 0].max()) <= BUDGET_PLAIN[0] and int(counts[:, 1].max()) <= BUDGET_PLAIN[1]


@pytest.mark.parametrize("curve,group", PM.GROUPS)
def test_the_forcing_scalars_reach_the_exceptional_additions(hp, curve, group):
    """On the generator the plain loop meets P - P at k = r and -P - P (a doubling inside the addition) at k = r - 2:
    the list S really holds the cases the header's comment names, and they come out right (previous test)."""
    g = PM.gid(curve, group)
    r = FR[curve].p
    P = corc.generator(curve, group)
    K = corc.ints_to_arr([r, r - 2, 5], 4)
    bases = np.ascontiguousarray(np.tile(P[0], (3, 1)))
    out = np.zeros_like(bases)
    counts = np.zeros((3, 4), dtype=np.uint32)
    assert hp.hp_mul(g, 0, _p(bases), _p(K), 3, _p(out), _p(counts)) == 0
    assert counts[0, 3] >= 1 and counts[1, 2] >= 1
    assert counts[2, 2] == 0 and counts[2, 3] == 0
    assert not out[0].any()                                       # r G = identity = zero bytes


def test_split_rule_is_the_msm_rule(hp):
    for curve, group in PM.GROUPS:
        g = PM.gid(curve, group)
        assert hp.hp_may_split(g, 1) == 1
        assert hp.hp_may_split(g, 0) == (1 if (curve, group) == ("bn254", 1) else 0)


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_rerandomize_one_proof_equals_the_oracle(hp, curve):
    """The header's arithmetic of one proof: (r1^-1 A, r1 B + r1 r2 delta, C + r2 A), canonical and Montgomery r1, r2;
    A = identity; r1 = 0 gives three identities."""
    F = FR[curve]
    r1cs, w, pk = VC.oracle_key(curve, 5)
    proof = VC.oracle_proof(curve, pk, r1cs, w, 9)
    delta = VC.g2(curve, pk["delta_g2"])
    rng = random.Random(3)
    for pr in (proof, (None, proof[1], proof[2])):
        r1, r2 = rng.randrange(1, F.p), rng.randrange(1, F.p)
        exp = VC.pack_proof(curve, PM.oracle_rerandomize(curve, pr, pk["delta_g2"], r1, r2))
        packed = np.ascontiguousarray(VC.pack_proof(curve, pr))
        for mont in (0, 1):
            rr = PM.scalars_arr(curve, [r1, r2], mont=bool(mont))
            out = np.zeros_like(packed)
            assert hp.hp_rerandomize(corc.CURVES[curve], _p(packed), _p(delta), _p(rr), mont, _p(out)) == 0
            assert np.array_equal(out, exp), mont
    rr = PM.scalars_arr(curve, [0, 5])
    out = np.ones_like(packed)
    assert hp.hp_rerandomize(corc.CURVES[curve], _p(packed), _p(delta), _p(rr), 0, _p(out)) == 0
    assert not out.any()
