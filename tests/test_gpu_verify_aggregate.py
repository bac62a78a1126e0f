"""GPU: dg16_groth16_verify_aggregate (verify.PreparedVerifyingKey.verify_aggregate) for BN254 and BLS12-381: one
verdict for a batch of proofs under caller-supplied 128-bit coefficients.  Expected verdicts never come from either
GPU verifier: they come from the oracle -- `oracle.pyref.pairing.groth16_verify` per proof, or
`pairing_product_is_one` on the aggregated pairs [(rho_i A_i, B_i)..., (-ACC, gamma), (-CS, delta), (-s_0 alpha, beta)]
built with `oracle.pyref.curves` and the same coefficients -- and from the validation rules of include/dg16.h with
membership facts established by the oracle inside the test.  One Miller loop of the oracle costs a few tenths of a
second, so oracle-evaluated aggregates stay at n <= 8 and larger batches repeat and permute oracle-decided cases."""

import ctypes
import random

import numpy as np
import pytest

import verify_cases as VC
from oracle.pyref import groth16 as G
from oracle.pyref import pairing as PR
from oracle.pyref.curves import CURVES
from oracle.pyref.fields import FQ, FR
from gpu_util import ctx

pytestmark = pytest.mark.gpu

BOTH = ["bn254", "bls12_381"]
TOP = (1 << 128) - 1


def prepared(curve, vk):
    from dg16_amd import verify
    return verify.PreparedVerifyingKey(ctx(), curve, *VC.pack_vk(curve, vk))


def coeff_array(rhos):
    return np.array([[r & ((1 << 64) - 1), r >> 64] for r in rhos], dtype=np.uint64).reshape(-1, 2)


def seeded_coeffs(n, seed):
    rng = random.Random(seed)
    return [rng.randrange(1, 1 << 128) for _ in range(n)]


def run(pvk, curve, rows, proofs, rhos, **kw):
    xs = VC.scalars(curve, rows, mont=kw.get("scalars_mont", False))
    return pvk.verify_aggregate(xs, VC.pack_proofs(curve, proofs), coeffs=None if rhos is None else coeff_array(rhos),
                                **kw)


def oracle_aggregate(curve, vk, rows, proofs, rhos):
    """The combined equation on the CPU: every point on its curve is the caller's business."""
    r = FR[curve].p
    g1 = CURVES[curve, "g1"]
    n_ic = len(vk["ic"])
    s = [0] * n_ic
    for rho, row in zip(rhos, rows):
        assert len(row) + 1 == n_ic
        for j, x in enumerate([1] + list(row)):
            s[j] = (s[j] + rho * x) % r
    acc = cs = None
    for sj, pt in zip(s, vk["ic"]):
        acc = g1.add(acc, g1.mul(pt, sj))
    pairs = []
    for rho, (A, B, C) in zip(rhos, proofs):
        pairs.append((g1.mul(A, rho), B))
        cs = g1.add(cs, g1.mul(C, rho))
    pairs += [(g1.neg(acc), vk["gamma_g2"]), (g1.neg(cs), vk["delta_g2"]),
              (g1.neg(g1.mul(vk["alpha_g1"], s[0])), vk["beta_g2"])]
    return PR.pairing_product_is_one(curve, pairs)


def context_still_proves():
    """A small proof through the resident prover equals the oracle's: the context is usable after an error."""
    import bench
    import torch
    _, ok = bench.cpu_baseline_and_parity(ctx(), torch.device("cuda", 0), 8)
    assert ok


def _another_witness(F, r1cs, w0, seed):
    """Another satisfying assignment of the same `synthetic_r1cs` system: redraw the free variables and recompute the
    output wires in order (the caller checks satisfaction)."""
    rng = random.Random(seed)
    p = F.p
    outs = [rc[0][1] for rc in r1cs["c"]]
    assert all(len(rc) == 1 and rc[0][0] == 1 for rc in r1cs["c"]) and outs == sorted(set(outs))
    w = list(w0)
    for i in range(1, outs[0]):
        w[i] = rng.randrange(p)
    for ra, rb, o in zip(r1cs["a"], r1cs["b"], outs):
        w[o] = G.evaluate_constraint(ra, w, p) * G.evaluate_constraint(rb, w, p) % p
    return w


_INST = {}


def instances(curve, K=4):
    """(vk, [(public inputs, proof)] * K): K witnesses of one small system with the oracle's key and proofs; the oracle's
    per-proof verifier accepts the first two (its cost), the others are made the same way."""
    if curve not in _INST:
        F = FR[curve]
        r1cs, w0, pk = VC.oracle_key(curve, seed=131, nc=11, ni=3, nw=12)
        vk = VC.vk_of(pk)
        ni = r1cs["num_instance"]
        inst = []
        for k in range(K):
            w = w0 if k == 0 else _another_witness(F, r1cs, w0, seed=140 + k)
            assert G.is_satisfied(r1cs, w, F.p)
            inst.append((w[1:ni], VC.oracle_proof(curve, pk, r1cs, w, seed=150 + k)))
        for pub, proof in inst[:2]:
            assert PR.groth16_verify(curve, vk, pub, proof)
        _INST[curve] = (vk, inst)
    return _INST[curve]


def packed_batch(curve, cases, order):
    """Public inputs and proofs of cases[order[i]] as arrays (every distinct case is packed once)."""
    xs = VC.scalars(curve, [c[0] for c in cases])
    pr = VC.pack_proofs(curve, [c[1] for c in cases])
    idx = np.asarray(order)
    return xs[idx], pr[idx]


SIZES = (1, 2, 63, 64, 65, 130, 5000)


@pytest.mark.parametrize("curve", BOTH)
def test_all_valid_batches_are_accepted(curve):
    """Completeness is exact: every all-valid batch is accepted, whatever the (nonzero) coefficients."""
    vk, inst = instances(curve)
    pvk = prepared(curve, vk)
    rng = random.Random(7)
    for n in SIZES:
        order = [rng.randrange(len(inst)) for _ in range(n)]
        xs, pr = packed_batch(curve, inst, order)
        assert pvk.verify_aggregate(xs, pr, coeffs=coeff_array(seeded_coeffs(n, 1000 + n))) is True, n
        assert pvk.verify_aggregate(xs, pr) is True, n                  # coefficients drawn from `secrets`
    pvk.close()


def test_snarkjs_triple_batches_are_accepted():
    vk, cases = VC.snarkjs_cases()
    public, proof, want = cases[0]
    assert want
    pvk = prepared("bn254", vk)
    for n in SIZES:
        xs, pr = packed_batch("bn254", [(public, proof)], [0] * n)
        assert pvk.verify_aggregate(xs, pr, coeffs=coeff_array(seeded_coeffs(n, 2000 + n))) is True, n
        assert pvk.verify_aggregate(xs, pr) is True, n
    # and its perturbations reject a batch they are part of
    for public_b, proof_b, want_b in cases[1:]:
        assert not want_b
        xs, pr = packed_batch("bn254", [(public, proof), (public_b, proof_b)], [0, 0, 1, 0])
        assert pvk.verify_aggregate(xs, pr, coeffs=coeff_array(seeded_coeffs(4, 2100))) is False
    pvk.close()


def bad_variants(curve, vk, inst):
    """Three ways to spoil instance 0, each rejected by the oracle's per-proof verifier."""
    F = FR[curve]
    g1 = CURVES[curve, "g1"]
    pub, (A, B, C) = inst[0]
    wrong = list(pub)
    wrong[0] = (wrong[0] + 1) % F.p
    bads = [(wrong, (A, B, C)), (pub, (A, B, inst[1][1][2])), (pub, (g1.add(A, g1.gen), B, C))]
    return bads


@pytest.mark.parametrize("curve", BOTH)
def test_one_bad_proof_rejects_the_batch(curve):
    vk, inst = instances(curve)
    bads = bad_variants(curve, vk, inst)
    for pub, proof in bads:
        assert not PR.groth16_verify(curve, vk, pub, proof)
    pvk = prepared(curve, vk)
    n = 130
    rng = random.Random(17)
    cases = inst + bads
    base = [rng.randrange(len(inst)) for _ in range(n)]
    rhos = coeff_array(seeded_coeffs(n, 3000))
    xs, pr = packed_batch(curve, cases, base)
    assert pvk.verify_aggregate(xs, pr, coeffs=rhos) is True
    for pos in (0, 63, 64, n - 1):
        for b in range(len(bads)):
            order = list(base)
            order[pos] = len(inst) + b
            xs, pr = packed_batch(curve, cases, order)
            assert pvk.verify_aggregate(xs, pr, coeffs=rhos) is False, (pos, b)
            assert pvk.verify_aggregate(xs, pr) is False, (pos, b)
    # an 8-batch: the oracle's aggregated product with the same coefficients agrees, accepted twin and rejected case
    rho8 = seeded_coeffs(8, 3100)
    good8 = [inst[k % len(inst)] for k in range(8)]
    bad8 = list(good8)
    bad8[5] = bads[1]
    for batch, want in ((good8, True), (bad8, False)):
        rows, proofs = [c[0] for c in batch], [c[1] for c in batch]
        assert oracle_aggregate(curve, vk, rows, proofs, rho8) is want
        assert run(pvk, curve, rows, proofs, rho8) is want
    pvk.close()


@pytest.mark.parametrize("curve", BOTH)
def test_coefficients_are_applied(curve):
    """Proofs 1 and 2 carry C + T and C - T: both are invalid, their errors cancel exactly when rho_1 == rho_2 -- so the
    verdict shows that each proof's own coefficient went into the combination."""
    vk, inst = instances(curve)
    g1 = CURVES[curve, "g1"]
    T = g1.mul(g1.gen, 0xC0FFEE)
    batch = [inst[0], inst[1], inst[2], inst[3]]
    (p1, (A1, B1, C1)), (p2, (A2, B2, C2)) = batch[1], batch[2]
    batch[1] = (p1, (A1, B1, g1.add(C1, T)))
    batch[2] = (p2, (A2, B2, g1.add(C2, g1.neg(T))))
    rows, proofs = [c[0] for c in batch], [c[1] for c in batch]
    assert not PR.groth16_verify(curve, vk, rows[1], proofs[1])
    pvk = prepared(curve, vk)
    rho = seeded_coeffs(4, 4000)
    equal = [rho[0], rho[1], rho[1], rho[3]]
    assert oracle_aggregate(curve, vk, rows, proofs, equal) is True
    assert run(pvk, curve, rows, proofs, equal) is True
    assert rho[1] != rho[2]
    assert run(pvk, curve, rows, proofs, rho) is False
    assert run(pvk, curve, rows, proofs, [rho[0], rho[1], rho[1] ^ 1, rho[3]]) is False
    per_proof = pvk.verify_batch(VC.scalars(curve, rows), VC.pack_proofs(curve, proofs)).tolist()
    assert per_proof == [True, False, False, True]
    # extreme and mixed coefficients against the oracle's product: a valid 3-batch and one with the tampered proof 1
    good3 = [inst[0], inst[1], inst[2]]
    bad3 = [inst[0], batch[1], inst[2]]
    for rhos in ([1, 1, 1], [1 << 127, 1 << 127, 1 << 127], [TOP, TOP, TOP], [1, 1 << 127, TOP], [TOP, 3, (1 << 64) + 1]):
        assert run(pvk, curve, [c[0] for c in good3], [c[1] for c in good3], rhos) is True, rhos
    for rhos in ([1, 1 << 127, TOP], [TOP, TOP, TOP]):
        want = oracle_aggregate(curve, vk, [c[0] for c in bad3], [c[1] for c in bad3], rhos)
        assert want is False
        assert run(pvk, curve, [c[0] for c in bad3], [c[1] for c in bad3], rhos) is want, rhos
    assert oracle_aggregate(curve, vk, [c[0] for c in good3], [c[1] for c in good3], [1, 1 << 127, TOP]) is True
    pvk.close()


@pytest.mark.parametrize("curve", BOTH)
def test_validation_rules(curve):
    from dg16_amd.lib import Dg16Error
    F, q = FR[curve], FQ[curve].p
    fb = FQ[curve].limbs64 * 8
    nl = FQ[curve].limbs64
    c1, c2 = CURVES[curve, "g1"], CURVES[curve, "g2"]
    r1cs, w, pk = VC.oracle_key(curve, seed=171, ni=2)
    vk = VC.vk_of(pk)
    proof = VC.oracle_proof(curve, pk, r1cs, w, seed=172)
    pub = w[1:2]
    A, B, C = proof
    assert PR.groth16_verify(curve, vk, pub, proof)
    pvk = prepared(curve, vk)
    x = VC.scalars(curve, [pub])
    good = VC.pack_proof(curve, proof)
    rho3 = coeff_array(seeded_coeffs(3, 5000))

    def between(xs_mid, pr_mid, coeffs=rho3, **kw):
        """good, the case, good"""
        x_good = VC.scalars(curve, [pub], mont=kw.get("scalars_mont", False))
        return pvk.verify_aggregate(np.concatenate([x_good, xs_mid, x_good]), np.stack([good, pr_mid, good]),
                                    coeffs=coeffs, **kw)

    assert between(x, good) is True
    # a proof coordinate + q (same residue, non-reduced limbs) where it fits the limbs
    for off in (0, nl, 2 * nl, 6 * nl):
        v = int.from_bytes(good[off:off + nl].tobytes(), "little") + q
        if v < 1 << (8 * fb):
            bad = good.copy()
            bad[off:off + nl] = VC.raw(v, fb)
            assert between(x, bad) is False
    # A off the curve
    assert between(x, VC.pack_proof(curve, ((A[0], (A[1] + 1) % q), B, C))) is False
    # B on the twist outside G2 (the oracle establishes the membership fact)
    Q = VC.twist_point_outside_g2(curve)
    assert c2.on_curve(Q) and c2.mul(Q, F.p) is not None
    assert between(x, VC.pack_proof(curve, (A, Q, C))) is False
    if curve == "bls12_381":
        P = VC.g1_point_outside_subgroup(curve)
        assert c1.on_curve(P) and c1.mul(P, F.p) is not None
        assert between(x, VC.pack_proof(curve, (P, B, C))) is False
        assert between(x, VC.pack_proof(curve, (A, B, P))) is False
    # x + r is not x
    if pub[0] + F.p < 1 << 256:
        assert between(VC.scalars(curve, [[pub[0] + F.p]]), good) is False
    # Montgomery limbs: right with the flag, read as canonical without it
    assert between(VC.scalars(curve, [pub], mont=True), good, scalars_mont=True) is True
    assert between(VC.scalars(curve, [pub], mont=True), good) is False
    # a zero coefficient never skips a proof: not a good one, not a bad one
    for at in range(3):
        z = rho3.copy()
        z[at] = 0
        assert between(x, good, coeffs=z) is False
    z = rho3.copy()
    z[1] = 0
    assert between(x, VC.pack_proof(curve, (A, B, c1.add(C, c1.gen))), coeffs=z) is False
    # identity points are inputs like any other: the equation decides
    rho2 = seeded_coeffs(2, 5100)
    for pr in ((None, B, C), (A, B, None), (A, None, C)):
        want = oracle_aggregate(curve, vk, [pub, pub], [proof, pr], rho2)
        assert run(pvk, curve, [pub, pub], [proof, pr], rho2) is want
    # the empty batch: the empty product is one
    assert pvk.verify_aggregate(np.zeros((0, 1, 4), dtype=np.uint64), VC.pack_proofs(curve, [])) is True
    assert pvk.verify_aggregate(np.zeros((0, 1, 4), dtype=np.uint64), VC.pack_proofs(curve, []),
                                coeffs=np.zeros((0, 2), dtype=np.uint64)) is True
    # errors of the call
    with pytest.raises(Dg16Error) as e:
        pvk.verify_aggregate(VC.scalars(curve, [pub + [1]]), good.reshape(1, -1), coeffs=rho3[:1])
    assert e.value.code == 1                                                       # LENGTH_MISMATCH
    context_still_proves()
    assert between(x, good) is True
    pvk.close()


@pytest.mark.parametrize("curve,n_public", [("bn254", 0), ("bn254", 40), ("bls12_381", 0), ("bls12_381", 40)])
def test_zero_and_forty_public_inputs(curve, n_public):
    """A key built directly from trapdoor scalars (no circuit): alpha, beta, gamma, delta and IC_j = u_j G1; a proof
    A = a G1, B = b G2, C = c G1 with c = (a b - alpha beta - gamma sum_j x_j u_j) / delta satisfies the equation by
    construction.  Three such proofs with their own inputs; the oracle's product evaluates the batches."""
    F = FR[curve]
    r = F.p
    c1, c2 = CURVES[curve, "g1"], CURVES[curve, "g2"]
    rng = random.Random(190 + n_public)
    al, be, ga, de = (rng.randrange(1, r) for _ in range(4))
    u = [rng.randrange(1, r) for _ in range(n_public + 1)]
    G1 = lambda k: c1.mul(c1.gen, k % r)       # noqa: E731
    G2 = lambda k: c2.mul(c2.gen, k % r)       # noqa: E731
    vk = {"alpha_g1": G1(al), "beta_g2": G2(be), "gamma_g2": G2(ga), "delta_g2": G2(de), "ic": [G1(k) for k in u]}
    rows, proofs = [], []
    for _ in range(3):
        a, b = rng.randrange(1, r), rng.randrange(1, r)
        x = [rng.randrange(r) for _ in range(n_public)]
        acc = (u[0] + sum(xi * ui for xi, ui in zip(x, u[1:]))) % r
        c = (a * b - al * be - ga * acc) * pow(de, r - 2, r) % r
        rows.append(x)
        proofs.append((G1(a), G2(b), G1(c)))
    assert PR.groth16_verify(curve, vk, rows[0], proofs[0])
    rhos = seeded_coeffs(3, 6000 + n_public)
    assert oracle_aggregate(curve, vk, rows, proofs, rhos) is True
    pvk = prepared(curve, vk)
    pr = VC.pack_proofs(curve, proofs)

    def call(rws):
        xs = VC.scalars(curve, rws) if n_public else np.zeros((len(rws), 0, 4), dtype=np.uint64)
        return pvk.verify_aggregate(xs, pr, coeffs=coeff_array(rhos))

    assert call(rows) is True
    if n_public:
        for k, j in ((1, 0), (2, n_public - 1)):
            changed = [list(x) for x in rows]
            changed[k][j] = (changed[k][j] + 1) % r
            if j == 0:
                assert oracle_aggregate(curve, vk, changed, proofs, rhos) is False
            assert call(changed) is False, (k, j)
    else:
        wrong = list(proofs)
        wrong[1] = (c1.add(proofs[1][0], c1.gen), proofs[1][1], proofs[1][2])
        assert oracle_aggregate(curve, vk, rows, wrong, rhos) is False
        xs = np.zeros((3, 0, 4), dtype=np.uint64)
        assert pvk.verify_aggregate(xs, VC.pack_proofs(curve, wrong), coeffs=coeff_array(rhos)) is False
        # no inputs at all through the C ABI: a null pointer with n_public = 0
        out = np.zeros(1, dtype=np.uint8)
        rho = coeff_array(rhos)
        p = lambda v: v.ctypes.data_as(ctypes.c_void_p)     # noqa: E731
        ctx()._chk(ctx().L.dg16_groth16_verify_aggregate(ctx().h, pvk.h, None, 0, p(pr), 3, p(rho), 0, p(out), 0))
        assert out[0] == 1
    pvk.close()


@pytest.mark.parametrize("curve", BOTH)
def test_setup_prove_verify_on_the_device(curve):
    """generate_parameters -> proving_key -> dg16_groth16_prove -> dg16_to_affine -> verify_aggregate, device pointers
    throughout and everything after the key on channel 0 with no host synchronisation in between; one public input
    changed -> rejected."""
    import torch
    import dg16_amd
    from dg16_amd import lib, verify
    from test_gpu_prover import enc_fr
    from test_gpu_setup import system_of
    F, Fq = FR[curve], FQ[curve]
    nl = Fq.limbs64
    r1cs, w = G.synthetic_r1cs(F, num_constraints=120, num_instance=3, num_witness=130, seed=161)
    rng = random.Random(162)
    td = tuple(rng.randrange(1, F.p) for _ in range(5))
    params = dg16_amd.generate_parameters(ctx(), curve, system_of(F, r1cs), trapdoor=td)
    a, b, c, dom = G.qap(r1cs, w, F)
    dev = torch.device("cuda", 0)
    up = lambda arr: torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to(dev)      # noqa: E731
    da, db, dc, dw = (up(enc_fr(F, v)) for v in (a, b, c, w))
    n = 3
    jac = torch.zeros((n, 12 * nl), dtype=torch.int64, device=dev)
    proofs = torch.zeros((n, 8 * nl), dtype=torch.int64, device=dev)
    pk = params.proving_key(ctx())
    pvk = verify.PreparedVerifyingKey.from_parameters(ctx(), params)
    pub = dw[1:3].repeat(n, 1).contiguous()                      # Montgomery form, as the prover takes them
    rho = up(coeff_array(seeded_coeffs(n, 7000)))
    out = torch.zeros(2, dtype=torch.uint8, device=dev)
    bad_pub = pub.clone()
    bad_pub[2] = up(enc_fr(F, [(w[1] + 1) % F.p]))[0]           # proof 1's first input
    torch.cuda.synchronize()
    L, h = ctx().L, ctx().h
    vp = ctypes.c_void_p
    for i in range(n):
        rs = enc_fr(F, [rng.randrange(1, F.p), rng.randrange(1, F.p)])
        ctx().prove_dev(pk, da.data_ptr(), db.data_ptr(), dc.data_ptr(), dw.data_ptr(), rs, jac[i].data_ptr())
        for group, joff, poff in ((1, 0, 0), (2, 3 * nl, 2 * nl), (1, 9 * nl, 6 * nl)):
            ctx()._chk(L.dg16_to_affine(h, lib.CURVES[curve], group, vp(jac[i].data_ptr() + 8 * joff),
                                        vp(proofs[i].data_ptr() + 8 * poff), 1, lib.F_DEVICE_PTRS, 0))
    flags = lib.F_DEVICE_PTRS | lib.F_SCALARS_MONT
    for k, x in enumerate((pub, bad_pub)):
        ctx()._chk(L.dg16_groth16_verify_aggregate(h, pvk.h, vp(x.data_ptr()), 2, vp(proofs.data_ptr()), n,
                                                   vp(rho.data_ptr()), flags, vp(out.data_ptr() + k), 0))
    ctx().sync(0)                                                # the first host synchronisation since the first proof
    assert out.cpu().tolist() == [1, 0]
    # the Python method on the same device buffers, and the per-proof verdicts for the record
    assert pvk.verify_aggregate(pub, proofs, coeffs=rho, scalars_mont=True, device=True, n_proofs=n) is True
    assert pvk.verify_aggregate(bad_pub, proofs, coeffs=rho, scalars_mont=True, device=True, n_proofs=n) is False
    assert pvk.verify_batch(bad_pub, proofs, scalars_mont=True, device=True, n_proofs=n).tolist() == [True, False, True]
    with pytest.raises(ValueError):
        pvk.verify_aggregate(pub, proofs, scalars_mont=True, device=True, n_proofs=n)      # coeffs are required
    pk.close()
    pvk.close()


@pytest.mark.parametrize("curve", BOTH)
def test_batch_of_two_to_the_eighteen(curve):
    """2^18 proofs in one call, built from two good proofs and one bad one: accepted with no bad proof, rejected with
    exactly one at a random position -- grid, workspace and depth of the product tree."""
    vk, inst = instances(curve)
    bad = bad_variants(curve, vk, inst)[1]
    n = 1 << 18
    cases = [inst[0], inst[1], bad]
    order = (np.arange(n) % 5 == 2).astype(np.int64)            # good pattern: instance 0 and instance 1
    xs, pr = packed_batch(curve, cases, order)
    rho = np.random.default_rng(18).integers(1, 1 << 63, size=(n, 2), dtype=np.uint64)
    pvk = prepared(curve, vk)
    assert pvk.verify_aggregate(xs, pr, coeffs=rho) is True
    pos = random.Random(19).randrange(n)
    xs[pos], pr[pos] = VC.scalars(curve, [bad[0]])[0], VC.pack_proof(curve, bad[1])
    assert pvk.verify_aggregate(xs, pr, coeffs=rho) is False
    pvk.close()


def test_faster_than_per_proof_verification_where_it_should_be():
    """Measured in this run by tools/verify_aggregate_timing.py (both calls on the same device buffers, interleaved in one
    process, HIP events around each call, median of 3): at (n = 262144, n_public = 1) and at (n = 1024, n_public = 40),
    on both curves, the aggregate call takes less time than dg16_groth16_verify_batch.  The points (1, 1) and (1024, 1)
    are printed, not asserted: there the call is a latency chain with no margin worth asserting."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("verify_aggregate_timing",
                                                  os.path.join(root, "tools", "verify_aggregate_timing.py"))
    vt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(vt)
    res = vt.measure(ctx(), grid=((1, 1), (1024, 1), (262144, 1), (1024, 40)))
    print("\n" + vt.table(res))
    for curve in BOTH:
        for p in res[curve]["points"]:
            if (p["n_proofs"], p["n_public"]) in ((262144, 1), (1024, 40)):
                assert p["aggregate_ms"] < p["batch_ms"], (curve, p)
