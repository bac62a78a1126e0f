"""dg16_groth16_setup_srs / keygen.generate_parameters_from_srs on the GPU: the Groth16 key computed in the exponent from
a structured reference string, against the CPU oracle (oracle.pyref.groth16.setup under the trapdoor (alpha, beta, 1, 1,
tau), corc.point_mul) and, at a size the oracle is too slow for, against dg16_groth16_setup.  Every comparison is on
affine bytes: the result does not depend on the order the terms were added in."""

import functools
import random

import numpy as np
import pytest

from oracle import corc
from oracle.pyref.fields import FQ, FR
from oracle.pyref.poly import Domain
from oracle.pyref import groth16 as G
from gpu_util import ctx
from test_gpu_prover import enc_fr, enc_g1, enc_g2
from test_gpu_setup import csr_of, system_of, expected_arrays
import test_libsnark_model as M

pytestmark = pytest.mark.gpu

ALL = ["bn254", "bls12_381", "bls12_377"]
PROVER_CURVES = ["bn254", "bls12_381"]
NAMES = ("a_query", "b_g1_query", "b_g2_query", "h_query", "l_query", "fixed_points", "gamma_g2", "gamma_abc_g1")


def trapdoor(curve, seed):
    """(alpha, beta, 1, 1, tau): the trapdoor a key from a reference string has."""
    rng = random.Random(seed)
    p = FR[curve].p
    return (rng.randrange(2, p), rng.randrange(2, p), 1, 1, rng.randrange(2, p))


@functools.lru_cache(maxsize=None)
def srs_of(curve, log_m, seed, reduction):
    import dg16_amd
    td = trapdoor(curve, seed)
    return dg16_amd.srs_from_trapdoor(ctx(), curve, log_m, td[0], td[1], td[4], reduction=reduction)


def limits():
    import ctypes
    from dg16_amd.lib import load
    a, b = ctypes.c_uint(), ctypes.c_uint()
    load().dg16_setup_srs_limits(ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def lagrange_at(F, m, tau):
    """L_i(tau) on the size-m domain by the closed form Z(tau) w^i / (m (tau - w^i)) -- big integers, no NTT."""
    p = F.p
    dom = Domain(F, m)
    zt = (pow(tau, m, p) - 1) % p
    return [zt * dom.element(i) % p * F.inv(m * (tau - dom.element(i)) % p) % p for i in range(m)]


def h_scalars(F, m, tau, reduction):
    p = F.p
    if reduction == "libsnark":
        z = (pow(tau, m, p) - 1) % p
        return [pow(tau, i, p) * z % p for i in range(m - 1)] + [0]
    return G.h_query_scalars(m - 1, tau, 1, F)


@functools.lru_cache(maxsize=None)
def oracle_key(curve, log_m):
    F = FR[curve]
    r1cs, w = M.instance(F, 1 << log_m, seed=log_m + 40)
    td = trapdoor(curve, log_m)
    pk, sc = G.setup(curve, r1cs, td)
    assert sc["m"] == 1 << log_m
    return r1cs, w, td, pk


# ---- against the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduction", ["circom", "libsnark"])
@pytest.mark.parametrize("log_m", [3, 6])
@pytest.mark.parametrize("curve", ALL)
def test_key_equals_the_oracles(curve, log_m, reduction):
    import dg16_amd
    F, Fq = FR[curve], FQ[curve]
    m = 1 << log_m
    r1cs, _, td, pk = oracle_key(curve, log_m)
    srs = srs_of(curve, log_m, log_m, reduction)
    # the reference string's scalars against big integers
    assert corc.arr_to_ints(srs.u) == lagrange_at(F, m, td[4])
    hs = h_scalars(F, m, td[4], reduction)
    assert corc.arr_to_ints(srs.h) == hs
    params = dg16_amd.generate_parameters_from_srs(ctx(), curve, system_of(F, r1cs), srs, reduction=reduction)
    assert params.trapdoor is None and params.domain_size == m and params.reduction == reduction
    exp = expected_arrays(curve, pk)
    if reduction == "libsnark":
        gen = corc.generator(curve, 1)
        exp["h_query"] = np.stack([np.asarray(corc.point_mul(curve, 1, gen, s)).reshape(-1) for s in hs])
        assert not exp["h_query"][m - 1].any() and not params.host("h_query")[m - 1].any()
    for name in NAMES:
        assert np.array_equal(params.host(name), exp[name]), (curve, log_m, reduction, name)


# ---- against dg16_groth16_setup --------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_subgroup", [False, True])
@pytest.mark.parametrize("curve", ALL)
def test_key_equals_the_trapdoor_generators(curve, in_subgroup):
    """log_m = 10 with almost half the domain padding rows: all eight outputs equal dg16_groth16_setup's under
    (alpha, beta, 1, 1, tau).  Synthetic coefficients are full-width, so every term is a multiplication: in_subgroup
    selects between the plain loop and the endomorphism split."""
    import dg16_amd
    F = FR[curve]
    log_m, m = 10, 1 << 10
    r1cs, _ = M.instance(F, m, seed=77, slack=m // 2 - 1)
    assert r1cs["num_constraints"] + r1cs["num_instance"] == m // 2 + 1
    td = trapdoor(curve, 10)
    system = system_of(F, r1cs)
    ref = dg16_amd.generate_parameters(ctx(), curve, system, trapdoor=td)
    got = dg16_amd.generate_parameters_from_srs(ctx(), curve, system, srs_of(curve, log_m, 10, "circom"),
                                                in_subgroup=in_subgroup)
    for name in NAMES:
        assert np.array_equal(got.host(name), ref.host(name)), (curve, name)


# ---- column shapes ---------------------------------------------------------------------------------------------------
SHAPE_CURVE = "bls12_381"      # 12-limb base field, a cofactor in both groups, the four-dimensional split in G2


@functools.lru_cache(maxsize=None)
def shapes():
    """A hand-built system whose wires cover every shape of a column, the same in A, B and C (with other coefficients),
    over point tables with INDEPENDENT known discrete logs: lag_g1 / lag_g2 = s_i G, alpha_lag_g1 = t_i G,
    beta_lag_g1 = v_i G (not a ceremony's output: the sums do not care).  Expected points: the sums over Z_r, times the
    generator by the oracle."""
    curve = SHAPE_CURVE
    F = FR[curve]
    p = F.p
    wave_from, msm_from = limits()
    assert 2 < wave_from < msm_from
    nc, ni = msm_from + 2, 2
    log_m = (nc + ni - 1).bit_length()
    assert log_m >= 6
    m = 1 << log_m
    rng = random.Random(5)
    full = lambda: rng.randrange(1 << 200, p)                                   # noqa: E731
    mixed = lambda i: 1 if i % 3 == 0 else p - 1 if i % 3 == 1 else full() if i % 7 == 2 else 1     # noqa: E731

    def column(n):
        """n entries in n different rows, every third a full-width coefficient's neighbour of +-1 terms."""
        assert n <= nc
        return [(i, mixed(i)) for i in range(n)]

    v = full()
    wires = [
        [(i, 1) for i in range(nc)],                          # 0  the constant one: an entry in every constraint
        [],                                                   # 1  an instance wire nothing reads: only its instance term
        [],                                                   # 2  no entry
        [(7, full())],                                        # 3  one entry
        column(wave_from - 1), column(wave_from), column(wave_from + 1),             # 4 5 6
        column(msm_from - 1), column(msm_from), column(msm_from + 1),                # 7 8 9
        [(11, 3), (11, 5), (12, 1)],                          # 10 a duplicate (row, column) pair
        [(20, 0), (21, 1), (22, p - 1), (23, full())],        # 11 coefficients 0, 1, r - 1 and a full-width value
        [(30, v), (30, p - v), (31, 1), (31, p - 1)],         # 12 terms that cancel to the identity
        [(40, 1), (40, 1)],                                   # 13 two equal terms: the doubling
        [(41, v), (41, v), (5, 1)],                           # 14 two equal products, and the identity point's row
        [(i % 3, mixed(i + 1)) for i in range(wave_from + 9)],        # 15 a wave segment of repeated rows
    ]
    nv = len(wires)

    def matrix(shift):
        rows = [[] for _ in range(nc)]
        for k, col in enumerate(wires):
            for i, c in col:
                c = c if c in (0, 1, p - 1) or shift == 0 else (c * (shift + 1)) % p
                rows[i].append((c, k))
        return rows

    r1cs = dict(num_constraints=nc, num_instance=ni, num_witness=nv - ni, a=matrix(0), b=matrix(1), c=matrix(2))
    s, t, u = ([rng.randrange(1, p) for _ in range(m)] for _ in range(3))
    s[5] = 0                                                  # an identity in the table
    c_ = ctx()
    arr = lambda x: corc.ints_to_arr(x, 4)                    # noqa: E731
    tabs = dict(lag_g1=c_.fixed_base_mul(curve, 1, arr(s)), lag_g2=c_.fixed_base_mul(curve, 2, arr(s)),
                alpha_lag_g1=c_.fixed_base_mul(curve, 1, arr(t)), beta_lag_g1=c_.fixed_base_mul(curve, 1, arr(u)))
    g1, g2 = corc.generator(curve, 1), corc.generator(curve, 2)
    for i in (0, 5, nc, m - 1):                               # the tables themselves, against the oracle
        assert np.array_equal(tabs["lag_g1"][i:i + 1], corc.point_mul(curve, 1, g1, s[i]))
        assert np.array_equal(tabs["lag_g2"][i:i + 1], corc.point_mul(curve, 2, g2, s[i]))
        assert np.array_equal(tabs["beta_lag_g1"][i:i + 1], corc.point_mul(curve, 1, g1, u[i]))
    assert not tabs["lag_g1"][5].any()
    tabs["h_g1"] = np.ascontiguousarray(tabs["alpha_lag_g1"][::-1])
    tabs["fixed"] = np.concatenate([tabs["lag_g1"][1:4].reshape(-1), tabs["lag_g2"][1:3].reshape(-1)])

    def col_sum(rows, table):
        acc = [0] * nv
        for i, row in enumerate(rows):
            for c, k in row:
                acc[k] = (acc[k] + c * table[i]) % p
        return acc

    a = col_sum(r1cs["a"], s)
    b = col_sum(r1cs["b"], s)
    kk = [(x + y + z) % p for x, y, z in zip(col_sum(r1cs["a"], u), col_sum(r1cs["b"], t), col_sum(r1cs["c"], s))]
    for k in range(ni):
        a[k] = (a[k] + s[nc + k]) % p
        kk[k] = (kk[k] + u[nc + k]) % p
    assert b[2] == 0 and a[12] == 0 and b[12] == 0 and kk[12] == 0 and a[13] == 2 * s[40] % p
    mul = lambda g, gen, xs: np.concatenate([corc.point_mul(curve, g, gen, x) for x in xs])      # noqa: E731
    exp = dict(a_query=mul(1, g1, a), b_g1_query=mul(1, g1, b), b_g2_query=mul(2, g2, b), h_query=tabs["h_g1"],
               l_query=mul(1, g1, kk[ni:]), fixed_points=tabs["fixed"], gamma_g2=tabs["lag_g2"][2:3],
               gamma_abc_g1=mul(1, g1, kk[:ni]))
    return dict(curve=curve, r1cs=r1cs, nc=nc, ni=ni, nv=nv, log_m=log_m, m=m, tabs=tabs, exp=exp)


def run_shapes(sh, in_subgroup=False, srs="all", mats=None):
    curve, F = sh["curve"], FR[sh["curve"]]
    fq = FQ[curve].limbs64
    nv, ni, m = sh["nv"], sh["ni"], sh["m"]
    outs = [np.zeros(n, dtype=np.uint64) for n in (nv * 2 * fq, nv * 2 * fq, nv * 4 * fq, m * 2 * fq, (nv - ni) * 2 * fq,
                                                  3 * 2 * fq + 2 * 4 * fq, 4 * fq, ni * 2 * fq)]
    if mats is None:
        mats = [csr_of(F, sh["r1cs"][k]) for k in "abc"]
    t = sh["tabs"]
    if srs == "all":
        srs = [t["lag_g1"], t["lag_g2"], t["alpha_lag_g1"], t["beta_lag_g1"], t["h_g1"], t["fixed"]]
    ctx().groth16_setup_srs(curve, sh["nc"], ni, nv, sh["log_m"], *mats, srs, outs, in_subgroup=in_subgroup)
    return dict(zip(NAMES, outs))


@pytest.mark.parametrize("in_subgroup", [False, True])
def test_column_shapes(in_subgroup):
    sh = shapes()
    got = run_shapes(sh, in_subgroup=in_subgroup)
    for name in NAMES:
        assert np.array_equal(got[name].reshape(-1), np.asarray(sh["exp"][name]).reshape(-1)), name


# ---- slicing ---------------------------------------------------------------------------------------------------------
def test_term_slices():
    """A slice of 1000 terms: every output of the shapes system takes several launches (a_query: the 3 * msm_from + ~100
    lane and wave entries in 13, the last one short; K three times as many), and segments straddle the cuts."""
    sh = shapes()
    c_ = ctx()
    c_.set_points_mul_slice(1000)
    try:
        got = run_shapes(sh)
    finally:
        c_.set_points_mul_slice(0)
    for name in NAMES:
        assert np.array_equal(got[name].reshape(-1), np.asarray(sh["exp"][name]).reshape(-1)), name


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_refusals_and_the_context_proves_afterwards():
    import dg16_amd
    import torch
    sh = shapes()
    curve, F = sh["curve"], FR[sh["curve"]]
    good = [csr_of(F, sh["r1cs"][k]) for k in "abc"]

    def refused(**kw):
        with pytest.raises(dg16_amd.Dg16Error) as e:
            run_shapes(sh, **kw)
        assert e.value.code == 3, kw.keys()

    for j in range(3):
        ptr, col, coeff = good[j]
        bad_col = col.copy()
        bad_col[len(col) // 2] = sh["nv"]                     # a column that is not a wire
        refused(mats=good[:j] + [(ptr, bad_col, coeff)] + good[j + 1:])
        bad_ptr = ptr.copy()
        bad_ptr[3], bad_ptr[4] = ptr[4], ptr[3]               # row 3 ends before it starts
        assert bad_ptr[3] > bad_ptr[4]
        refused(mats=good[:j] + [(bad_ptr, col, coeff)] + good[j + 1:])
    refused(srs=None)
    t = sh["tabs"]
    full = [t["lag_g1"], t["lag_g2"], t["alpha_lag_g1"], t["beta_lag_g1"], t["h_g1"], t["fixed"]]
    for j in range(6):
        refused(srs=full[:j] + [None] + full[j + 1:])
    # the same two index errors on device pointers, where the kernels find them
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int32 if x.dtype == np.uint32 else np.int64)).to(dev)   # noqa: E731
    srs = dg16_amd.Srs(curve, sh["log_m"], *full)
    ptr, col, coeff = good[1]
    bad_col = col.copy()
    bad_col[-1] = sh["nv"] + 5
    bad_ptr = ptr.copy()
    bad_ptr[3], bad_ptr[4] = ptr[4], ptr[3]
    for b in ((ptr, bad_col, coeff), (bad_ptr, col, coeff)):
        system = dict(num_constraints=sh["nc"], num_inputs=sh["ni"], num_vars=sh["nv"],
                      a=tuple(up(x) for x in good[0]), b=tuple(up(x) for x in b), c=tuple(up(x) for x in good[2]))
        with pytest.raises(dg16_amd.Dg16Error) as e:
            dg16_amd.generate_parameters_from_srs(ctx(), curve, system, srs)
        assert e.value.code == 3
    # ... and the context generates a key and proves correctly afterwards
    _end_to_end("bn254", 3)


# ---- end to end ------------------------------------------------------------------------------------------------------
def _end_to_end(curve, log_m):
    import dg16_amd
    F, Fq = FR[curve], FQ[curve]
    p = F.p
    r1cs, w, td, pk = oracle_key(curve, log_m)
    ni = r1cs["num_instance"]
    params = dg16_amd.generate_parameters_from_srs(ctx(), curve, system_of(F, r1cs), srs_of(curve, log_m, log_m, "circom"))
    rng = random.Random(log_m)
    r, s = rng.randrange(1, p), rng.randrange(1, p)
    dpk = params.proving_key(ctx())
    pvk = dg16_amd.PreparedVerifyingKey.from_parameters(ctx(), params)
    try:
        a, b, c, dom = G.qap(r1cs, w, F)
        assert dom.size == params.domain_size
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


@pytest.mark.parametrize("curve", PROVER_CURVES)
def test_key_from_srs_proves_and_verifies(curve):
    """Key from the reference string -> resident key -> proof == the oracle's proof under (alpha, beta, 1, 1, tau) with the
    same r and s; the pairing verifier accepts it and rejects it for a changed public input."""
    _end_to_end(curve, 6)
