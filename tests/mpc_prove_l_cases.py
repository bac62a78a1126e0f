"""The n-party proofs of tests/test_gpu_mpc_prove_l.py: the shared material (circuit, key, expected proofs -- oracle only,
no GPU) and, run as a program, the GPU side of every case in a process of its own:

    python tests/mpc_prove_l_cases.py        ->  one line "RESULT <json>"

Why a process of its own: a 16- or 32-party party_prove is the first thing in a test run to drive channels 1 and 2 (the
three joined d_msm of prove::C) of party contexts 8 .. 31 -- 48 more streams in use, kept for the life of the process
like the pool of tests/dist_pool.py that owns them.  The test process is shared by the whole suite; what these cases need
beyond what the suite already had stays out of it.  Inside this program the parties are contexts of one process through
dist_pool.parties, as everywhere else.  The program only produces what the GPU computed (decoded points, verdicts); every
comparison is made by the test.
(test infrastructure: imports the oracle)"""

import functools
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import corc  # noqa: E402
from oracle.pyref import groth16 as G  # noqa: E402
from oracle.pyref.curves import CURVES  # noqa: E402
from oracle.pyref.fields import FQ, FR  # noqa: E402

SEED = bytes(range(32))
LS = [1, 4, 8]


def enc(F, vals):
    return corc.ints_to_arr([F.to_mont(v) for v in vals], 4)


def plain(x):
    """Points as JSON carries them: tuples -> lists, recursively."""
    if isinstance(x, (tuple, list)):
        return [plain(v) for v in x]
    return x


@functools.lru_cache(maxsize=None)
def material(curve):
    """The circuit, trapdoor and witness of test_mpc_prove_equals_single_prover (13 constraints, 2 instance and 17
    witness variables, domain 16), its key, the QAP evaluations, (r, s), the clear points that make the blinded proof, and
    both expected proofs from oracle.pyref.groth16.create_proof.  Read-only."""
    F = FR[curve]
    r1cs, w = G.synthetic_r1cs(F, num_constraints=13, num_instance=2, num_witness=17, seed=3)
    rng = random.Random(5)
    pk, _ = G.setup(curve, r1cs, tuple(rng.randrange(1, F.p) for _ in range(5)))
    a, b, c, dom = G.qap(r1cs, w, F)
    r, s = rng.randrange(1, F.p), rng.randrange(1, F.p)
    g1, g2 = CURVES[curve, "g1"], CURVES[curve, "g2"]
    fixed = dict(L=g1.add(pk["alpha_g1"], pk["a_query"][0]), N=pk["delta_g1"],
                 Z=g2.add(pk["beta_g2"], pk["b_g2_query"][0]), K=pk["delta_g2"],
                 M=g1.add(pk["beta_g1"], pk["b_g1_query"][0]))
    return dict(r1cs=r1cs, w=w, pk=pk, abc=(a, b, c), log_m=dom.size.bit_length() - 1, r=r, s=s, fixed=fixed,
                proof0=G.create_proof(curve, pk, 0, 0, r1cs, w), proof_rs=G.create_proof(curve, pk, r, s, r1cs, w))


def complete(curve, pk, proof):
    """The client's completion of an r = s = 0 proof (groth16/examples/sha256.rs:208-212)."""
    g1, g2 = CURVES[curve, "g1"], CURVES[curve, "g2"]
    A, B, C = proof
    return (g1.add(A, g1.add(pk["a_query"][0], pk["alpha_g1"])), g2.add(B, g2.add(pk["b_g2_query"][0], pk["beta_g2"])), C)


# ---- the GPU side ---------------------------------------------------------------------------------------------------------
def _hpk(curve):
    from test_gpu_prover import enc_g1, enc_g2
    Fq, pk = FQ[curve], material(curve)["pk"]
    hpk = {k: enc_g1(Fq, pk[k]) for k in ("a_query", "b_g1_query", "h_query", "l_query")}
    hpk["b_g2_query"] = enc_g2(Fq, pk["b_g2_query"])
    return hpk


def _decode(curve, res):
    from test_gpu_prover import dec_g1, dec_g2
    Fq = FQ[curve]
    return (dec_g1(Fq, corc.jac_to_affine(curve, 1, res[0])), dec_g2(Fq, corc.jac_to_affine(curve, 2, res[1])),
            dec_g1(Fq, corc.jac_to_affine(curve, 1, res[2])))


def _host_shares(curve, l):
    """Key and request shares through the per-vector host compositions, as test_mpc_prove_equals_single_prover makes
    them."""
    import dist_pool
    from dg16_amd import groth16_mpc as M
    F, m = FR[curve], material(curve)
    pp = dist_pool.params(curve, l)[0]
    a, b, c = m["abc"]
    w, ni = m["w"], m["r1cs"]["num_instance"]
    return (M.pack_from_arkworks_proving_key(pp, _hpk(curve)), M.qap_pss(pp, enc(F, a), enc(F, b), enc(F, c)),
            M.pack_from_witness(pp, enc(F, w[1:])), M.pack_from_witness(pp, enc(F, w[ni:])))


def _prove(curve, l, crs, qs, a_sh, ax_sh, **kw):
    """-> {"proof": the points every party holds (party 0's, decoded), "parties": how many, "same": identical on all}"""
    import dist_pool
    from dg16_amd import groth16_mpc as M
    ctxs, pps, net, _ = dist_pool.parties(curve, l)
    log_m = material(curve)["log_m"]
    res = net.simulate_network_round(
        lambda i, h: M.party_prove(ctxs[i], pps[i], h, crs[i], qs[i], a_sh[i], ax_sh[i], log_m, h_odd=True, **kw))
    same = all(np.array_equal(x, y) for rr in res for x, y in zip(rr, res[0]))
    return {"proof": plain(_decode(curve, res[0])), "parties": len(res), "same": bool(same)}, res


def _blinding(curve):
    from test_gpu_prover import enc_g1, enc_g2
    F, Fq, m = FR[curve], FQ[curve], material(curve)
    kw = {k: (enc_g2 if k in "ZK" else enc_g1)(Fq, [v]) for k, v in m["fixed"].items()}
    return dict(r=enc(F, [m["r"]]), s=enc(F, [m["s"]]), **kw)


def run_all():
    import dist_pool
    import verify_cases as VC
    from gpu_util import ctx
    from dg16_amd import groth16_mpc as M, verify
    out = {}
    curve = "bn254"
    F, m = FR[curve], material(curve)
    for l in LS:
        shares = _host_shares(curve, l)
        out["bn254_l%d_zero" % l], _ = _prove(curve, l, *shares)
        out["bn254_l%d_rs" % l], res = _prove(curve, l, *shares, **_blinding(curve))
        if l == 4:      # the proof as a verifier sees it, and after one public input is changed
            proof = VC.pack_proofs(curve, [_decode(curve, res[0])])
            ni = m["r1cs"]["num_instance"]
            pub = [x % F.p for x in m["w"][1:ni]]
            bad = [(pub[0] + 1) % F.p] + pub[1:]
            pvk = verify.PreparedVerifyingKey(ctx(), curve, *VC.pack_vk(curve, VC.vk_of(m["pk"])))
            try:
                out["bn254_l4_verify"] = [pvk.verify_batch(VC.scalars(curve, [pub]), proof).tolist(),
                                          pvk.verify_batch(VC.scalars(curve, [bad]), proof).tolist()]
            finally:
                pvk.close()
    # the whole client flow through the one-call packers, plain and blinded
    pp = dist_pool.params(curve, 4)[0]
    a, b, c = m["abc"]
    ni = m["r1cs"]["num_instance"]
    crs = M.pack_proving_key(pp, _hpk(curve), in_subgroup=True)
    reqs = {}
    for name, seed in (("plain", None), ("blinded", SEED)):
        req = reqs[name] = M.pack_request(pp, enc(F, a), enc(F, b), enc(F, c), enc(F, m["w"]), ni, seed=seed)
        out["bn254_l4_packers_" + name], _ = _prove(curve, 4, crs, [q[0] for q in req], [q[1] for q in req],
                                                    [q[2] for q in req])
    out["bn254_l4_blinded_shares_differ"] = not np.array_equal(reqs["plain"][0][1], reqs["blinded"][0][1])
    out["bls12_377_l4_zero"], _ = _prove("bls12_377", 4, *_host_shares("bls12_377", 4))
    return out


if __name__ == "__main__":
    print("RESULT " + json.dumps(run_all()))
