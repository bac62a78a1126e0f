"""An n-party Groth16 proof at EVERY packing factor: l = 1, 4, 8 (4, 16, 32 parties) beside the l = 2 of
tests/test_gpu_dist.py.  Everything around ext_wit::h already ran at these l; with `party_prove(..., h_odd=True)`
(DG16_F_H_ODD) the h shares are the witness map's and the three compute calls give the single prover's proof.

The circuit, the trapdoor and the witness are those of test_mpc_prove_equals_single_prover (13 constraints, 2 instance
variables, 17 witness variables, domain 16); the expected proofs come from oracle.pyref.groth16.create_proof, once per
curve.  The GPU side of all cases runs ONCE, in a process of its own (tests/mpc_prove_l_cases.py says why): parties are
contexts of that process through dist_pool.parties.  It reports the points and verdicts the GPU produced; the
comparisons are here."""

import json
import os
import subprocess
import sys

import pytest

import mpc_prove_l_cases as MC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mpc_prove_l_cases.py")], cwd=ROOT,
                         capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, out.stdout[-2000:]
    return json.loads(line[-1][7:])


def completed(curve, case):
    """The r = s = 0 proof of a case after the client's completion, as JSON carried it."""
    A, B, C = case["proof"]
    tup = lambda p: None if p is None else tuple(tuple(c) if isinstance(c, list) else c for c in p)      # noqa: E731
    return MC.plain(MC.complete(curve, MC.material(curve)["pk"], (tup(A), tup(B), tup(C))))


@pytest.mark.parametrize("l", MC.LS)
def test_mpc_proof_equals_the_single_provers(gpu, l):
    curve = "bn254"
    m = MC.material(curve)
    zero = gpu["bn254_l%d_zero" % l]
    assert zero["parties"] == 4 * l and zero["same"]                  # the three points are identical on every party
    assert completed(curve, zero) == MC.plain(m["proof0"])
    # every term live: r, s != 0 and the clear points L, N, Z, K, M that make the blinded single-prover proof
    rs = gpu["bn254_l%d_rs" % l]
    assert rs["parties"] == 4 * l and rs["same"]
    assert rs["proof"] == MC.plain(m["proof_rs"])


def test_the_l_4_proof_verifies_and_a_changed_input_does_not(gpu):
    assert gpu["bn254_l4_rs"]["proof"] == MC.plain(MC.material("bn254")["proof_rs"])        # the proof that was verified
    assert gpu["bn254_l4_verify"] == [[True], [False]]


def test_bls12_377_at_l_4(gpu):
    curve = "bls12_377"
    case = gpu["bls12_377_l4_zero"]
    assert case["parties"] == 16 and case["same"]
    assert completed(curve, case) == MC.plain(MC.material(curve)["proof0"])


@pytest.mark.parametrize("form", ["plain", "blinded"])
def test_the_one_call_packers_give_the_same_proof_at_l_4(gpu, form):
    """The whole client flow: dg16_pk_pack, dg16_request_pack (plain, then blinded from a seed), the 16 parties,
    completion."""
    curve = "bn254"
    case = gpu["bn254_l4_packers_" + form]
    assert case["parties"] == 16 and case["same"]
    assert completed(curve, case) == MC.plain(MC.material(curve)["proof0"])
    if form == "blinded":
        assert gpu["bn254_l4_blinded_shares_differ"]       # the blinded run did start from other shares
