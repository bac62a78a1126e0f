"""GPU: dg16_groth16_rerandomize (verify.PreparedVerifyingKey.rerandomize) on BN254 and BLS12-381.  The expected proofs
are the oracle's three formulas (r1^-1 A, r1 B + r1 r2 delta, C + r2 A) computed with `oracle.pyref.curves`; validity is
decided by the batch verifier on unchanged public inputs and, for two proofs per curve, by the oracle's pairing
verifier (`oracle.pyref.pairing.groth16_verify`).  Key and proofs: `verify_cases.oracle_key` / `oracle_proof`."""

import ctypes
import random

import numpy as np
import pytest

import points_mul_cases as PM
import verify_cases as VC
from oracle.pyref import pairing as PR
from oracle.pyref.curves import CURVES
from oracle.pyref.fields import FQ, FR
from gpu_util import ctx
from test_gpu_verify import context_still_proves

pytestmark = pytest.mark.gpu

BOTH = ["bn254", "bls12_381"]
_cases = {}


def case(curve):
    """One key, 65 proofs (five distinct ones, cycled), their (r1, r2) and the oracle's re-randomized proofs."""
    if curve not in _cases:
        from dg16_amd import verify
        F = FR[curve]
        r1cs, w, pk = VC.oracle_key(curve, 7)
        vk = VC.vk_of(pk)
        base = [VC.oracle_proof(curve, pk, r1cs, w, 20 + j) for j in range(5)]
        n = 65
        proofs = [base[i % 5] for i in range(n)]
        rng = random.Random(99)
        rs = [(rng.randrange(1, F.p), rng.randrange(1, F.p)) for _ in range(n)]
        rs[1] = (1, 1)
        rs[2] = (F.p - 1, F.p - 1)
        exp = [PM.oracle_rerandomize(curve, proofs[i], pk["delta_g2"], *rs[i]) for i in range(n)]
        pvk = verify.PreparedVerifyingKey(ctx(), curve, *VC.pack_vk(curve, vk))
        x = [w[1:3]] * n          # oracle_key: ni = 3 (the constant one and two public inputs)
        _cases[curve] = dict(vk=vk, pk=pk, proofs=proofs, rs=rs, exp=exp, pvk=pvk, x=x)
    return _cases[curve]


def rr_arr(curve, rs, mont=False):
    return np.stack([PM.scalars_arr(curve, list(p), mont=mont) for p in rs]) if rs else np.zeros((0, 2, 4), np.uint64)


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("curve", BOTH)
def test_output_is_the_oracles_and_verifies(curve, n):
    c = case(curve)
    packed = VC.pack_proofs(curve, c["proofs"][:n])
    got = c["pvk"].rerandomize(packed, rr_arr(curve, c["rs"][:n]))
    want = VC.pack_proofs(curve, c["exp"][:n])
    assert np.array_equal(got, want)
    assert all((got[i] != packed[i]).any() for i in range(n))
    assert c["pvk"].verify_batch(VC.scalars(curve, c["x"][:n]), got).all()
    if n == 65:
        for i in (0, 2):       # two per curve: the Python pairing is slow
            assert PR.groth16_verify(curve, c["vk"], c["x"][i], c["exp"][i])
    assert c["pvk"].rerandomize(VC.pack_proofs(curve, []), rr_arr(curve, [])).shape[0] == 0


@pytest.mark.parametrize("curve", BOTH)
def test_tampered_stays_rejected_and_twice_gives_two_valid_proofs(curve):
    c = case(curve)
    c1 = CURVES[curve, "g1"]
    A, B, C = c["proofs"][0]
    bad = (A, B, c1.add(C, c1.gen))
    x = VC.scalars(curve, c["x"][:2])
    rs = rr_arr(curve, c["rs"][3:5])
    out = c["pvk"].rerandomize(VC.pack_proofs(curve, [bad, c["proofs"][0]]), rs)
    assert c["pvk"].verify_batch(x, out).tolist() == [False, True]
    twice = c["pvk"].rerandomize(VC.pack_proofs(curve, [c["proofs"][0]] * 2), rs)
    assert (twice[0] != twice[1]).any()
    assert c["pvk"].verify_batch(x, twice).all()
    assert np.array_equal(twice[1], out[1])


@pytest.mark.parametrize("curve", BOTH)
def test_identity_a_in_one_proof(curve):
    c = case(curve)
    proofs = list(c["proofs"][:5])
    proofs[2] = (None, proofs[2][1], proofs[2][2])
    rs = c["rs"][10:15]
    got = c["pvk"].rerandomize(VC.pack_proofs(curve, proofs), rr_arr(curve, rs))
    want = VC.pack_proofs(curve, [PM.oracle_rerandomize(curve, proofs[i], c["pk"]["delta_g2"], *rs[i]) for i in range(5)])
    assert np.array_equal(got, want)
    g1w = 2 * FQ[curve].limbs64
    assert not got[2, :g1w].any()                                                     # A' = identity
    assert np.array_equal(got[2, -g1w:], VC.g1(curve, proofs[2][2]))                  # C' = C


@pytest.mark.parametrize("curve", BOTH)
def test_in_place_device_host_and_montgomery_agree(curve):
    import torch
    dev = torch.device("cuda", 0)
    c = case(curve)
    n = 65
    packed = VC.pack_proofs(curve, c["proofs"])
    want = VC.pack_proofs(curve, c["exp"])
    for mont in (False, True):
        rs = rr_arr(curve, c["rs"], mont=mont)
        assert np.array_equal(c["pvk"].rerandomize(packed, rs, scalars_mont=mont), want)
        # host pointers, in place (proofs_out is proofs)
        buf = packed.copy()
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        k = ctx()
        assert k.L.dg16_groth16_rerandomize(k.h, c["pvk"].h, p(buf), n, p(rs), 1 if mont else 0, p(buf), 0) == 0
        assert np.array_equal(buf, want)
        # device pointers, in place
        d_p = torch.from_numpy(packed.view(np.int64)).to(dev)
        d_r = torch.from_numpy(np.ascontiguousarray(rs).view(np.int64)).to(dev)
        torch.cuda.synchronize()
        c["pvk"].rerandomize(d_p, d_r, scalars_mont=mont, device=True, n_proofs=n)
        ctx().sync(0)
        assert np.array_equal(d_p.cpu().numpy().view(np.uint64), want)
        # device pointers, separate output
        d_p = torch.from_numpy(packed.view(np.int64)).to(dev)
        d_o = torch.zeros_like(d_p)
        torch.cuda.synchronize()
        c["pvk"].rerandomize(d_p, d_r, scalars_mont=mont, device=True, n_proofs=n, out=d_o)
        ctx().sync(0)
        assert np.array_equal(d_o.cpu().numpy().view(np.uint64), want)
        assert np.array_equal(d_p.cpu().numpy().view(np.uint64), packed)


@pytest.mark.parametrize("curve", BOTH)
def test_bad_randomness(curve):
    import torch
    from dg16_amd.lib import Dg16Error
    dev = torch.device("cuda", 0)
    c = case(curve)
    r = FR[curve].p
    n = 65
    packed = VC.pack_proofs(curve, c["proofs"])
    want = VC.pack_proofs(curve, c["exp"])
    for bad in ((0, 5), (5, 0), (r, 5)):
        rs = list(c["rs"])
        rs[3] = bad
        with pytest.raises(Dg16Error) as e:
            c["pvk"].rerandomize(packed, rr_arr(curve, rs))
        assert e.value.code == 3
    context_still_proves()
    rs = list(c["rs"])
    rs[3] = (0, 5)
    d_p = torch.from_numpy(packed.view(np.int64)).to(dev)
    d_r = torch.from_numpy(rr_arr(curve, rs).view(np.int64)).to(dev)
    torch.cuda.synchronize()
    c["pvk"].rerandomize(d_p, d_r, device=True, n_proofs=n)          # returns DG16_OK (a raise would fail the test)
    ctx().sync(0)
    got = d_p.cpu().numpy().view(np.uint64)
    assert not got[3].any()
    keep = [i for i in range(n) if i != 3]
    assert np.array_equal(got[keep], want[keep])


@pytest.mark.parametrize("curve", BOTH)
def test_drawn_randomness(curve):
    from dg16_amd import verify
    c = case(curve)
    n = 16
    rs = verify.random_rerandomizers(curve, n)
    r = FR[curve].p
    assert rs.shape == (n, 2, 4) and all(1 <= int.from_bytes(v.tobytes(), "little") < r for v in rs.reshape(-1, 4))
    out = c["pvk"].rerandomize(VC.pack_proofs(curve, [c["proofs"][0]] * n))
    assert c["pvk"].verify_batch(VC.scalars(curve, c["x"][:n]), out).all()
    assert len({o.tobytes() for o in out}) == n
