"""GPU: dg16_vk_create / dg16_groth16_verify_batch (verify.PreparedVerifyingKey) for BN254 and BLS12-381.  Expected
verdicts come from the oracle's pairing verifier (`oracle.pyref.pairing.groth16_verify`, pinned by the reference's
snarkjs triple), from the validation rules of include/dg16.h with membership facts established by the oracle inside
the test, and -- BN254 only -- from the unchanged host verifier as a second reference.  Never from the batch verifier
itself.  One oracle verification costs 0.6 s (BN254) / 1.4 s (BLS12-381), so distinct oracle-checked cases stay at a
few dozen per curve and large batches repeat and permute them."""

import ctypes
import random
import time

import numpy as np
import pytest

import verify_cases as VC
from oracle import corc
from oracle.pyref import groth16 as G
from oracle.pyref import pairing as PR
from oracle.pyref.curves import CURVES
from oracle.pyref.fields import FQ, FR
from gpu_util import ctx

pytestmark = pytest.mark.gpu

BOTH = ["bn254", "bls12_381"]


def prepared(curve, vk):
    from dg16_amd import verify
    return verify.PreparedVerifyingKey(ctx(), curve, *VC.pack_vk(curve, vk))


def run(pvk, curve, rows, proofs, **kw):
    return [bool(v) for v in pvk.verify_batch(VC.scalars(curve, rows, mont=kw.get("scalars_mont", False)),
                                              VC.pack_proofs(curve, proofs), **kw)]


def context_still_proves():
    """A small proof through the resident prover equals the oracle's: the context is usable after an error."""
    import bench
    import torch
    _, ok = bench.cpu_baseline_and_parity(ctx(), torch.device("cuda", 0), 8)
    assert ok


def test_snarkjs_triple_and_perturbations_interleaved_in_one_batch():
    """130 proofs, bad ones at 0, 63, 64, 129 (both sides of a wave boundary and both ends) and scattered between:
    every verdict is its own."""
    vk, cases = VC.snarkjs_cases()
    good, bads = cases[0], cases[1:]
    n = 130
    pick = [good] * n
    for k, i in enumerate([0, 63, 64, 129, 7, 31, 100, 101]):
        pick[i] = bads[k % len(bads)]
    pvk = prepared("bn254", vk)
    got = run(pvk, "bn254", [c[0] for c in pick], [c[1] for c in pick])
    assert got == [c[2] for c in pick]
    assert got.count(False) == 8 and not got[0] and not got[63] and not got[64] and not got[129] and got[1] and got[65]
    assert run(pvk, "bn254", [good[0]], [good[1]]) == [True]                      # a batch of one
    pvk.close()


@pytest.mark.parametrize("curve", BOTH)
def test_oracle_instances_then_five_thousand_in_one_call(curve):
    F = FR[curve]
    K = 8
    r1cs, w0, pk = VC.oracle_key(curve, seed=31, nc=11, ni=3, nw=12)
    vk = VC.vk_of(pk)
    ni = r1cs["num_instance"]
    rng = random.Random(32)
    inst = []
    for k in range(K):      # different witnesses of the same system, different r and s
        w = w0 if k == 0 else _another_witness(F, r1cs, w0, seed=40 + k)
        assert G.is_satisfied(r1cs, w, F.p)
        inst.append((w[1:ni], VC.oracle_proof(curve, pk, r1cs, w, seed=50 + k)))
    cases = []
    for k, (pub, proof) in enumerate(inst):
        cases.append((pub, proof))
        wrong = list(pub)
        wrong[k % len(pub)] = (wrong[k % len(pub)] + 1 + k) % F.p
        cases.append((wrong, proof))
        cases.append((pub, (proof[0], proof[1], inst[(k + 1) % K][1][2])))           # another instance's C
    cases.append((inst[0][0], VC.rerandomise(curve, inst[0][1], rng.randrange(1, F.p))))
    cases.append((inst[1][0], VC.rerandomise(curve, inst[0][1], rng.randrange(1, F.p))))
    # the oracle decides a subset directly (its cost); the rest follow from facts it has established: a valid proof
    # is accepted and stays valid re-randomised, inputs differ from the witness's -> rejected (checked for k = 0, 1)
    want = []
    for j, (pub, proof) in enumerate(cases):
        if j < 6 or j >= 3 * K:
            want.append(PR.groth16_verify(curve, vk, pub, proof))
        else:
            want.append(j % 3 == 0)
    assert want[:6] == [True, False, False, True, False, False] and want[3 * K:] == [True, False]
    pvk = prepared(curve, vk)
    assert run(pvk, curve, [c[0] for c in cases], [c[1] for c in cases]) == want
    n = 5000
    order = [rng.randrange(len(cases)) for _ in range(n)]
    t0 = time.perf_counter()
    got = run(pvk, curve, [cases[j][0] for j in order], [cases[j][1] for j in order])
    print("\n%s: 5000 proofs in one host-pointer call, %.3f s" % (curve, time.perf_counter() - t0))
    assert got == [want[j] for j in order]
    pvk.close()


def _another_witness(F, r1cs, w0, seed):
    """Another satisfying assignment of the SAME system: with num_witness >= num_constraints every constraint of
    `synthetic_r1cs` is <a, w> <b, w> = w_out with a fresh output wire that later rows may read, so redrawing the free
    variables and recomputing the outputs in order gives a new witness (checked by the caller)."""
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


@pytest.mark.parametrize("curve", BOTH)
def test_setup_prove_verify_on_the_device(curve):
    """generate_parameters -> proving_key -> dg16_groth16_prove -> dg16_to_affine -> verify_batch, device pointers
    throughout; one public input changed -> rejected; the oracle confirms both verdicts for this instance."""
    import torch
    import dg16_amd
    from dg16_amd import lib, verify
    from test_gpu_prover import enc_fr, dec_g1, dec_g2
    from test_gpu_setup import system_of
    F, Fq = FR[curve], FQ[curve]
    nl = Fq.limbs64
    r1cs, w = G.synthetic_r1cs(F, num_constraints=120, num_instance=3, num_witness=130, seed=61)
    rng = random.Random(62)
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
    torch.cuda.synchronize()
    L, h = ctx().L, ctx().h
    for i in range(n):
        rs = enc_fr(F, [rng.randrange(1, F.p), rng.randrange(1, F.p)])
        ctx().prove_dev(pk, da.data_ptr(), db.data_ptr(), dc.data_ptr(), dw.data_ptr(), rs, jac[i].data_ptr())
        for ch in range(3):
            ctx().sync(ch)
        vp = ctypes.c_void_p
        for group, joff, poff in ((1, 0, 0), (2, 3 * nl, 2 * nl), (1, 9 * nl, 6 * nl)):
            ctx()._chk(L.dg16_to_affine(h, lib.CURVES[curve], group, vp(jac[i].data_ptr() + 8 * joff),
                                        vp(proofs[i].data_ptr() + 8 * poff), 1, lib.F_DEVICE_PTRS, 0))
    ctx().sync(0)
    pvk = verify.PreparedVerifyingKey.from_parameters(ctx(), params)
    pub = dw[1:3].repeat(n, 1).contiguous()                      # Montgomery form, as the prover takes them
    torch.cuda.synchronize()
    good = pvk.verify_batch(pub, proofs, scalars_mont=True, device=True, n_proofs=n)
    assert good.tolist() == [True] * n
    bad_pub = pub.clone()
    bad_pub[2] = up(enc_fr(F, [(w[1] + 1) % F.p]))[0]           # proof 1's first input
    torch.cuda.synchronize()
    bad = pvk.verify_batch(bad_pub, proofs, scalars_mont=True, device=True, n_proofs=n)
    assert bad.tolist() == [True, False, True]
    # the oracle on proof 0 with the GPU-made key
    row = proofs[0].cpu().numpy().view(np.uint64)
    A, B, C = dec_g1(Fq, row[:2 * nl].reshape(1, -1)), dec_g2(Fq, row[2 * nl:6 * nl].reshape(1, -1)), \
        dec_g1(Fq, row[6 * nl:].reshape(1, -1))
    opk, _ = G.setup(curve, r1cs, td)
    vk = VC.vk_of(opk)
    assert PR.groth16_verify(curve, vk, w[1:3], (A, B, C))
    assert not PR.groth16_verify(curve, vk, [(w[1] + 1) % F.p, w[2]], (A, B, C))
    pk.close()
    pvk.close()


@pytest.mark.parametrize("curve", BOTH)
def test_validation_rules(curve):
    from dg16_amd import verify
    from dg16_amd.lib import Dg16Error
    F, q = FR[curve], FQ[curve].p
    fb = FQ[curve].limbs64 * 8
    nl = FQ[curve].limbs64
    c1, c2 = CURVES[curve, "g1"], CURVES[curve, "g2"]
    r1cs, w, pk = VC.oracle_key(curve, seed=71, ni=2)
    vk = VC.vk_of(pk)
    proof = VC.oracle_proof(curve, pk, r1cs, w, seed=72)
    pub = w[1:2]
    A, B, C = proof
    assert PR.groth16_verify(curve, vk, pub, proof)
    pvk = prepared(curve, vk)
    x = VC.scalars(curve, [pub])
    good = VC.pack_proof(curve, proof)

    def one(xs, pr, **kw):
        return bool(pvk.verify_batch(xs, pr.reshape(1, -1), **kw)[0])

    assert one(x, good)
    # a proof coordinate + q (same residue, non-reduced limbs) where it fits the limbs
    for off in (0, nl, 2 * nl):
        v = int.from_bytes(good[off:off + nl].tobytes(), "little") + q
        if v < 1 << (8 * fb):
            bad = good.copy()
            bad[off:off + nl] = VC.raw(v, fb)
            assert not one(x, bad)
    # A off the curve
    assert not one(x, VC.pack_proof(curve, ((A[0], (A[1] + 1) % q), B, C)))
    # B on the twist outside G2 (the oracle establishes the membership fact)
    Q = VC.twist_point_outside_g2(curve)
    assert c2.on_curve(Q) and c2.mul(Q, F.p) is not None
    assert not one(x, VC.pack_proof(curve, (A, Q, C)))
    if curve == "bls12_381":
        P = VC.g1_point_outside_subgroup(curve)
        assert c1.on_curve(P) and c1.mul(P, F.p) is not None
        assert not one(x, VC.pack_proof(curve, (P, B, C)))
        assert not one(x, VC.pack_proof(curve, (A, B, P)))
    # x + r is not x
    if pub[0] + F.p < 1 << 256:
        assert not one(VC.scalars(curve, [[pub[0] + F.p]]), good)
    assert one(VC.scalars(curve, [pub], mont=True), good, scalars_mont=True)
    assert not one(VC.scalars(curve, [pub], mont=True), good)                      # Montgomery limbs read as canonical
    # identity points are inputs like any other: the equation decides
    for pr in ((None, B, C), (A, B, None), (A, None, C)):
        assert one(x, VC.pack_proof(curve, pr)) == PR.groth16_verify(curve, vk, pub, pr)
    # neighbours: all of the above in one batch with good proofs between them
    mixed = [good, VC.pack_proof(curve, (A, Q, C)), good, VC.pack_proof(curve, ((A[0], (A[1] + 1) % q), B, C)), good]
    assert pvk.verify_batch(np.concatenate([x] * 5), np.stack(mixed)).tolist() == [True, False, True, False, True]
    # errors of the call
    with pytest.raises(Dg16Error) as e:
        pvk.verify_batch(VC.scalars(curve, [pub + [1]]), good.reshape(1, -1))
    assert e.value.code == 1                                                       # LENGTH_MISMATCH
    context_still_proves()
    assert pvk.verify_batch(np.zeros((0, 1, 4), dtype=np.uint64), VC.pack_proofs(curve, [])).tolist() == []
    # malformed keys
    al, be, ga, de, ic = VC.pack_vk(curve, vk)
    v = int.from_bytes(ic[0, :nl].tobytes(), "little") + q
    if v < 1 << (8 * fb):
        ic_bad = ic.copy()
        ic_bad[0, :nl] = VC.raw(v, fb)
        with pytest.raises(Dg16Error) as e:
            verify.PreparedVerifyingKey(ctx(), curve, al, be, ga, de, ic_bad)
        assert e.value.code == 3
    with pytest.raises(Dg16Error) as e:
        verify.PreparedVerifyingKey(ctx(), curve, al, be, VC.g2(curve, Q), de, ic)
    assert e.value.code == 3
    if curve == "bls12_381":
        with pytest.raises(Dg16Error) as e:
            verify.PreparedVerifyingKey(ctx(), curve, VC.g1(curve, P), be, ga, de, ic)
        assert e.value.code == 3
    context_still_proves()
    assert one(x, good)
    pvk.close()


def test_bls12_377_is_unsupported():
    from dg16_amd import verify
    from dg16_amd.lib import Dg16Error
    z = np.zeros(48, dtype=np.uint64)
    with pytest.raises(Dg16Error) as e:
        verify.PreparedVerifyingKey(ctx(), "bls12_377", z[:12], z[:24], z[:24], z[:24], z[:12].reshape(1, 12))
    assert e.value.code == 7
    context_still_proves()


@pytest.mark.parametrize("curve,n_public", [("bn254", 0), ("bn254", 40), ("bls12_381", 0), ("bls12_381", 40)])
def test_zero_and_forty_public_inputs(curve, n_public):
    """A key built directly from trapdoor scalars (no circuit): alpha, beta, gamma, delta and IC_j = u_j G1; the proof
    A = a G1, B = b G2, C = c G1 with c = (a b - alpha beta - gamma sum_j x_j u_j) / delta satisfies the equation by
    construction, and the oracle confirms it."""
    F = FR[curve]
    r = F.p
    c1, c2 = CURVES[curve, "g1"], CURVES[curve, "g2"]
    rng = random.Random(90 + n_public)
    al, be, ga, de, a, b = (rng.randrange(1, r) for _ in range(6))
    u = [rng.randrange(1, r) for _ in range(n_public + 1)]
    x = [rng.randrange(r) for _ in range(n_public)]
    acc = (u[0] + sum(xi * ui for xi, ui in zip(x, u[1:]))) % r
    c = (a * b - al * be - ga * acc) * pow(de, r - 2, r) % r
    G1 = lambda k: c1.mul(c1.gen, k % r)       # noqa: E731
    G2 = lambda k: c2.mul(c2.gen, k % r)       # noqa: E731
    vk = {"alpha_g1": G1(al), "beta_g2": G2(be), "gamma_g2": G2(ga), "delta_g2": G2(de), "ic": [G1(k) for k in u]}
    proof = (G1(a), G2(b), G1(c))
    assert PR.groth16_verify(curve, vk, x, proof)
    pvk = prepared(curve, vk)
    rows, proofs, want = [x], [proof], [True]
    if n_public:
        for j in (0, n_public - 1):
            y = list(x)
            y[j] = (y[j] + 1) % r
            rows.append(y)
            proofs.append(proof)
            want.append(False)
    rows.append(x)
    proofs.append((G1(a + 1), G2(b), G1(c)))
    want.append(False)
    pr = VC.pack_proofs(curve, proofs)
    xs = VC.scalars(curve, rows) if n_public else np.zeros((len(rows), 0, 4), dtype=np.uint64)
    if n_public:
        got = pvk.verify_batch(xs, pr)
    else:     # no inputs at all: the call takes n_public = 0 from the empty array
        out = np.zeros(len(rows), dtype=np.uint8)
        p = lambda v: v.ctypes.data_as(ctypes.c_void_p)     # noqa: E731
        ctx()._chk(ctx().L.dg16_groth16_verify_batch(ctx().h, pvk.h, None, 0, p(pr), len(rows), 0, p(out), 0))
        got = out.astype(bool)
    assert got.tolist() == want
    pvk.close()


def test_agreement_with_the_host_verifier_on_bit_flips():
    """~200 single-bit mutations of a valid BN254 proof and its input: verdict == (the unchanged host verifier accepts),
    where the host call raises BAD_ARG for a non-reduced input the batch says 0."""
    from dg16_amd import verify
    from dg16_amd.lib import Dg16Error
    curve = "bn254"
    vk, cases = VC.snarkjs_cases()
    public, proof = cases[0][0], cases[0][1]
    packed_vk = VC.pack_vk(curve, vk)
    good = VC.pack_proof(curve, proof)
    x = VC.scalars(curve, [public])[0]
    rng = random.Random(5)
    xs, prs = [x], [good]
    for _ in range(150):
        m = good.copy()
        bit = rng.randrange(32 * 64)
        m[bit // 64] ^= np.uint64(1 << (bit % 64))
        xs.append(x)
        prs.append(m)
    for _ in range(50):
        y = x.copy()
        bit = rng.randrange(256)
        y[0, bit // 64] ^= np.uint64(1 << (bit % 64))
        xs.append(y)
        prs.append(good)
    want = []
    for y, m in zip(xs, prs):
        try:
            want.append(bool(verify.verify_proof(*packed_vk, y, m)))
        except Dg16Error as e:
            assert e.code == 3
            want.append(False)
    assert want[0] and want.count(True) == 1
    pvk = prepared(curve, vk)
    got = pvk.verify_batch(np.stack(xs), np.stack(prs))
    assert got.tolist() == want
    pvk.close()


def test_batch_of_one_hundred_thousand():
    """10^5 proofs in one call (repeats of a good and a bad one): grid and workspace scale."""
    vk, cases = VC.snarkjs_cases()
    good, bad = cases[0], cases[2]
    n = 100000
    pattern = np.arange(n) % 7 != 3
    pr = np.where(pattern[:, None], VC.pack_proof("bn254", good[1])[None, :], VC.pack_proof("bn254", bad[1])[None, :])
    xs = np.repeat(VC.scalars("bn254", [good[0]]), n, axis=0)
    pvk = prepared("bn254", vk)
    got = pvk.verify_batch(xs, pr)
    assert np.array_equal(got, pattern)
    pvk.close()


def test_throughput_against_prover_and_host_verifier():
    """The two conditions of the feature, on values measured in this run (tools/verify_timing.py does the measuring):
    at 1 024 proofs the batch verifies more proofs per second than the prover of the same curve produces, and on BN254
    more than 16 x the host verifier's single-thread rate (16 CPUs is what a user of the host verifier has)."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("verify_timing", os.path.join(root, "tools", "verify_timing.py"))
    vt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(vt)
    res = vt.measure(ctx(), sizes=(1, 1024), prover_log_m=20, host_calls=10)
    print("\n" + vt.table(res))
    for curve in BOTH:
        v = res[curve]["verify_batch"]["1024"]["proofs_per_s"]
        p = res[curve]["prove_queued"]["proofs_per_s"]
        assert v > p, (curve, v, p)
    host = res["bn254"]["host_verify"]["proofs_per_s"]
    assert res["bn254"]["verify_batch"]["1024"]["proofs_per_s"] > 16 * host, host
