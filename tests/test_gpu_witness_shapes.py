"""GPU parity on witness-shaped scalars (tests/witness_shapes.py): bits, small integers, field negatives, one repeated
value, a sha256-like mix, zeros and scalars on the signed-digit recoding's edges -- through the plain MSM, the resident
(table) MSM and whole proofs, bit-exact against the oracle in affine form.  Such scalars put nearly every bucket entry
into one bucket: giant buckets through BN254 G1's stitch kernel, giants cut into slices of more than 512 partials, bucket
sets that are all identities but one (test_witness_shapes.py asserts which of these paths each case reaches)."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import corc
from gpu_util import ctx
import witness_shapes as ws

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = [("bn254", 1), ("bn254", 2), ("bls12_381", 1), ("bls12_381", 2), ("bls12_377", 1), ("bls12_377", 2)]


def _threads():
    import bench
    return bench.cpu_threads()


@functools.lru_cache(maxsize=8)
def _bases(curve, group, n, seed):
    b = ctx().gen_bases(curve, group, seed, n) if n >= 1 << 12 else corc.gen_points(curve, group, seed, n)
    b.setflags(write=False)
    return b


def _sum_points(curve, group, bases):
    """sum_i P_i by the oracle's double-and-add (algo 1: the definition, no bucket method)."""
    ones = np.zeros((len(bases), 4), dtype=np.uint64)
    ones[:, 0] = 1
    return corc.msm(curve, group, bases, ones, algo=1)


def _identities(curve, group, bases, sc, kind, got):
    """ones: sum_i P_i; const: v * sum_i P_i (corc.point_mul) -- results that do not go through any Pippenger."""
    if kind == "ones":
        assert np.array_equal(got, _sum_points(curve, group, bases))
    elif kind == "const":
        v = ws.to_ints(sc[:1])[0]
        assert np.array_equal(got, corc.point_mul(curve, group, _sum_points(curve, group, bases), v))
    elif kind == "zero":
        assert not got.any()


def _plain(curve, group, bases, sc, kind=None, in_subgroup=True):
    jac = ctx().msm(curve, group, bases, sc, in_subgroup=in_subgroup)
    got = corc.jac_to_affine(curve, group, jac)
    exp = corc.msm(curve, group, bases, sc, threads=_threads())
    assert np.array_equal(got, exp), (curve, group, len(sc), kind)
    _identities(curve, group, bases, sc, kind, got)


# ---- plain dg16_msm ----------------------------------------------------------------------------------------------
# 2^10: the direct atomic sort; 2^14 + 37: the LDS-partitioned sort; 2^16: 16-entry segments (test_witness_shapes.py)
PLAIN_KINDS = ("bits", "sparse", "u64", "neg_small", "const", "sha256_mix")
PLAIN = [(c, g, n, k) for (c, g) in GROUPS for n in (1 << 10, (1 << 14) + 37, 1 << 16) for k in PLAIN_KINDS]


@pytest.mark.parametrize("curve,group,n,kind", PLAIN)
def test_plain_msm_on_witness_shapes(curve, group, n, kind):
    _plain(curve, group, _bases(curve, group, n, 31), ws.shape(curve, n, kind, ws.SEEDS["plain"]), kind)


@pytest.mark.parametrize("curve,group", [("bn254", 1), ("bn254", 2), ("bls12_381", 1)])
@pytest.mark.parametrize("log_n", [17, 20])
@pytest.mark.parametrize("kind", ["bits", "ones"])
def test_plain_msm_one_giant_bucket(curve, group, log_n, kind):
    """2^17 (eight 16-bit windows) and 2^20: bits / ones put 2^(log_n - 1) / 2^log_n entries into ONE bucket -- at 2^20 a
    giant through BN254 G1's stitch kernel, and with `ones` a giant of > 32 768 partials (slices of > 512) in the groups
    without the tree."""
    n = 1 << log_n
    _plain(curve, group, _bases(curve, group, n, 40 + log_n), ws.shape(curve, n, kind, ws.SEEDS["giant"]), kind)


@pytest.mark.parametrize("group", [1, 2])
def test_plain_msm_without_the_split_on_bits(group):
    """BLS12-381 without DG16_F_BASES_IN_SUBGROUP: the full-width sort (255-bit scalars, no GLV) on a bits witness."""
    curve, n = "bls12_381", 1 << 14
    sc = ws.shape(curve, n, "bits", ws.SEEDS["subgroup"])
    _plain(curve, group, _bases(curve, group, n, 52), sc, "bits", in_subgroup=False)


_PINNED = r"""
import sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
from oracle import corc
import witness_shapes as ws
import dg16_amd
c = dg16_amd.Context(0)
for curve, group, n in (("bls12_381", 1, 1 << 12), ("bn254", 2, 1 << 10), ("bls12_377", 2, 1 << 10)):
    bases = corc.gen_points(curve, group, 60 + n, n)
    sc = ws.boundary_scalars(%(c)d, ws.SCALAR_BITS[curve], n, curve)
    got = corc.jac_to_affine(curve, group, c.msm(curve, group, bases, sc, in_subgroup=False))
    assert np.array_equal(got, corc.msm(curve, group, bases, sc)), (curve, group, n)
print("ok")
"""


@pytest.mark.parametrize("c", [13, 16])
def test_plain_msm_at_a_pinned_width_on_boundary_digits(c):
    """DG16_MSM_C pins the plain window width (read once per process: a child process).  On cofactor groups without the
    subgroup flag there is no GLV split, so the digits the library recodes are the crafted ones: +half, -(half - 1),
    carries through all-ones windows, r - 1 and r - 2."""
    env = dict(os.environ)
    env["DG16_MSM_C"] = str(c)
    out = subprocess.run([sys.executable, "-c", _PINNED % {"root": ROOT, "c": c}], capture_output=True, text=True,
                         timeout=300, env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


# ---- resident MSM (dg16_bases_upload + dg16_msm_resident) ------------------------------------------------------------
RESIDENT = [("bn254", 1, 1 << 13), ("bn254", 1, (1 << 15) + 7), ("bn254", 1, 1 << 16), ("bn254", 1, 1 << 20),
            ("bn254", 2, 1 << 20), ("bls12_381", 1, 1 << 16), ("bls12_377", 2, 1 << 12)]


def _boundary_padded(curve, c, n):
    """boundary_scalars at the key's width: 4096 of them, zeros after (keeps the oracle's dense work small at 2^20)."""
    sc = np.zeros((n, 4), dtype=np.uint64)
    m = min(n, 4096)
    sc[:m] = ws.boundary_scalars(c, ws.SCALAR_BITS[curve], m, curve)
    return sc


@pytest.mark.parametrize("curve,group,n", RESIDENT)
def test_resident_msm_on_witness_shapes(curve, group, n):
    c = ctx()
    bases = _bases(curve, group, n, 70)
    hb = c.bases_upload(curve, group, bases)
    try:
        wb = hb.info()["window_bits"]
        assert wb == ws.window_bits(n, True, ws.SCALAR_BITS[curve])
        for kind in ("bits", "ones", "sha256_mix", "zero", "boundary"):
            sc = _boundary_padded(curve, wb, n) if kind == "boundary" else ws.shape(curve, n, kind, ws.SEEDS["resident"])
            got = c.msm_resident(hb, sc, affine=True).reshape(1, -1)
            exp = corc.msm(curve, group, bases, sc, threads=_threads())
            assert np.array_equal(got, exp), (curve, group, n, kind)
            _identities(curve, group, bases, sc, kind, got)
    finally:
        hb.close()


def test_resident_msm_under_a_table_budget_on_bits():
    """A thinned table (stride > 1: several bucket sets and the Horner tail) on a bits witness and boundary digits."""
    import dg16_amd
    curve, group, n = "bn254", 1, 1 << 14
    bases = _bases(curve, group, n, 75)
    c = dg16_amd.Context(0)
    try:
        c.set_table_budget(bases.nbytes * 3)
        hb = c.bases_upload(curve, group, bases)
        info = hb.info()
        nwin = ws.nwin_of(info["window_bits"], 254)
        assert info["table_bytes"] <= bases.nbytes * 3 < nwin * bases.nbytes
        for sc in (ws.shape(curve, n, "bits", ws.SEEDS["budget"]), _boundary_padded(curve, info["window_bits"], n)):
            got = c.msm_resident(hb, sc, affine=True).reshape(1, -1)
            assert np.array_equal(got, corc.msm(curve, group, bases, sc, threads=_threads()))
        hb.close()
    finally:
        c.close()


def test_resident_msm_back_to_back_shapes():
    """dense, bits, dense, ones through ONE resident key: giant-list or bucket state of one call must not leak into the
    next."""
    curve, group, n = "bn254", 1, 1 << 16
    c = ctx()
    bases = _bases(curve, group, n, 80)
    hb = c.bases_upload(curve, group, bases)
    try:
        for i, kind in enumerate(("dense", "bits", "dense", "ones")):
            sc = ws.dense(curve, n, i) if kind == "dense" else ws.shape(curve, n, kind, i)
            got = c.msm_resident(hb, sc, affine=True).reshape(1, -1)
            assert np.array_equal(got, corc.msm(curve, group, bases, sc, threads=_threads())), (i, kind)
    finally:
        hb.close()


# ---- whole proofs against bench.oracle_prove ------------------------------------------------------------------------
def _set_witness(wl, w_rest):
    """wl.w[1:] <- w_rest in place (w[0] stays 1)."""
    import torch
    wl.w[1:] = torch.from_numpy(np.ascontiguousarray(w_rest).view(np.int64)).to(wl.dev)
    torch.cuda.synchronize()


def _prove_and_check(wl, label):
    import bench
    gp = bench.prove_once(ctx(), wl)
    (A, B, C), _ = bench.oracle_prove(wl, _threads())
    gA, gB, gC = bench.gpu_proof_affine(wl.curve, gp)
    assert np.array_equal(A, gA) and np.array_equal(B, gB) and np.array_equal(C, gC), label


def _workload(curve, log_m, seed, **shape):
    import torch
    import bench
    return bench.Workload(ctx(), torch.device("cuda", 0), log_m, 0, 1, seed=seed, curve=curve, **shape)


@pytest.mark.parametrize("curve,log_m,shape,kinds", [
    ("bn254", 15, dict(nv=29823, nc=29400, ni=2), ("sha256_mix", "bits")),    # config 4: the merged A / B1 / L launch
    ("bn254", 20, {}, ("bits", "ones")),                                       # stitch giants, separate launches
    ("bls12_381", 16, {}, ("sha256_mix",)),
    ("bn254", 12, {}, ("zero",)),
])
def test_proof_on_witness_shapes(curve, log_m, shape, kinds):
    wl = _workload(curve, log_m, 90 + log_m, **shape)
    try:
        for i, kind in enumerate(kinds):
            _set_witness(wl, ws.shape(curve, wl.nv - 1, kind, ws.SEEDS["proof"] + i))
            _prove_and_check(wl, (curve, log_m, kind))
    finally:
        wl.pk.close()


def test_proof_back_to_back_shapes():
    """dense, bits, dense, ones through one key and prove_once (BN254 2^16): each proof equals the oracle's."""
    curve = "bn254"
    wl = _workload(curve, 16, 96)
    try:
        for i, kind in enumerate(("dense", "bits", "dense", "ones")):
            rest = ws.dense(curve, wl.nv - 1, 20 + i) if kind == "dense" else ws.shape(curve, wl.nv - 1, kind, 20 + i)
            _set_witness(wl, rest)
            _prove_and_check(wl, (i, kind))
    finally:
        wl.pk.close()


def test_sharded_proof_on_bits():
    """Eight shard keys in one process (BN254 2^16): the shards share shards[0].w; every shard's qap runs inside
    prove()."""
    import torch
    import bench
    sp = bench.ShardedInProcess(ctx(), torch.device("cuda", 0), "bn254", 16, 8, seed=97)
    try:
        wl = sp.shards[0]
        assert all(s.w is wl.w for s in sp.shards)
        _set_witness(wl, ws.shape("bn254", wl.nv - 1, "bits", 30))
        proof, _, _ = sp.prove()
        (A, B, C), _ = bench.oracle_prove(wl, _threads())
        gA, gB, gC = bench.gpu_proof_affine("bn254", proof.cpu().numpy())
        assert np.array_equal(A, gA) and np.array_equal(B, gB) and np.array_equal(C, gC)
    finally:
        sp.close()
