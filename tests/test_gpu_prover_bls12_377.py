"""The resident Groth16 prover on BLS12-377 (curve id 2): dg16_pk_create* / dg16_groth16_prove / _msms / _msms_h /
_assemble with every flag and form the other two curves have.  The curve has no pairing here, so proofs are checked
against the big-integer prover (oracle.pyref.groth16), in the exponent (trapdoor scalars times the generators) and
against a proof assembled from the C oracle over the same key arrays (tests/prover377_cases.py) -- never against the
library.  Proofs are compared as affine points converted by the oracle: two schedules may leave different Jacobian
representatives of one point."""

import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from oracle import corc
from oracle.pyref.curves import CURVES
from oracle.pyref import groth16 as G
from gpu_util import ctx
from test_gpu_prover import enc_fr, dec_g1, dec_g2
from test_gpu_setup import csr_of, system_of
import test_libsnark_model as M
import witness_shapes as ws
import prover377_cases as P

pytestmark = pytest.mark.gpu

CURVE, F, Fq = P.CURVE, P.F, P.Fq
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _decoded(A, B, C):
    return (dec_g1(Fq, corc.jac_to_affine(CURVE, 1, A)), dec_g2(Fq, corc.jac_to_affine(CURVE, 2, B)),
            dec_g1(Fq, corc.jac_to_affine(CURVE, 1, C)))


# ---- 1. tiny keys against the big-integer prover ---------------------------------------------------------------------
@pytest.mark.parametrize("nc,nw", [(13, 20), (60, 30)])
def test_prove_matches_bigint_prover(nc, nw):
    """m = 16 and m = 64; (r, s) = (0, 0) and drawn, scalars in Montgomery form and plain.  The proof equals
    G.create_proof's and the trapdoor scalars times the generators, which satisfy the verifying equation in the exponent."""
    ni = 2
    r1cs, w = G.synthetic_r1cs(F, num_constraints=nc, num_instance=ni, num_witness=nw, seed=nc)
    assert G.is_satisfied(r1cs, w, F.p)
    rng = random.Random(5)
    td = tuple(rng.randrange(1, F.p) for _ in range(5))
    pk, sc = G.setup(CURVE, r1cs, td)
    a, b, c, dom = G.qap(r1cs, w, F)
    assert dom.size == (16 if nc == 13 else 64)
    dpk = ctx().pk_create(CURVE, ni + nw, ni, dom.size, *P.arrays_of_bigint_key(pk))
    g1, g2 = CURVES[CURVE, "g1"], CURVES[CURVE, "g2"]
    try:
        for r, s in ((0, 0), (rng.randrange(1, F.p), rng.randrange(1, F.p))):
            eA, eB, eC = G.create_proof(CURVE, pk, r, s, r1cs, w)
            for mont in (True, False):
                enc = (lambda v: enc_fr(F, v)) if mont else P.fr_arr
                got = _decoded(*ctx().prove(dpk, enc_fr(F, a), enc_fr(F, b), enc_fr(F, c), enc(w), enc([r]), enc([s]),
                                            scalars_mont=mont))
                assert got == (eA, eB, eC), (r != 0, mont)
            sa, sb, scc = G.proof_scalars_from_trapdoor(r1cs, F, td, sc, r, s, w)
            assert got == (g1.mul(g1.gen, sa), g2.mul(g2.gen, sb), g1.mul(g1.gen, scc))
            assert G.verify_in_exponent(r1cs, F, td, sc, (sa, sb, scc), w)
    finally:
        dpk.close()


# ---- 2. multi-block phases, in the exponent --------------------------------------------------------------------------
def test_proof_from_gpu_key_in_the_exponent():
    """nc = 8000, m = 8192: GPU key -> resident key -> ONE call with drawn r, s == proof_scalars_from_trapdoor * G."""
    import dg16_amd
    nc, ni, nw = 8000, 3, 8100
    r1cs, w = G.synthetic_r1cs(F, num_constraints=nc, num_instance=ni, num_witness=nw, seed=21)
    rng = random.Random(22)
    td = tuple(rng.randrange(1, F.p) for _ in range(5))
    sc = G.setup_scalars(r1cs, F, td)
    params = dg16_amd.generate_parameters(ctx(), CURVE, system_of(F, r1cs), trapdoor=td)
    a, b, c, dom = G.qap(r1cs, w, F)
    assert dom.size == params.domain_size == 8192
    r, s = rng.randrange(1, F.p), rng.randrange(1, F.p)
    dpk = params.proving_key(ctx())
    try:
        got = P.affine(*ctx().prove(dpk, enc_fr(F, a), enc_fr(F, b), enc_fr(F, c), enc_fr(F, w), enc_fr(F, [r]),
                                    enc_fr(F, [s])))
    finally:
        dpk.close()
    sa, sb, scc = G.proof_scalars_from_trapdoor(r1cs, F, td, sc, r, s, w)
    assert G.verify_in_exponent(r1cs, F, td, sc, (sa, sb, scc), w)
    assert np.array_equal(got, P.scalars_times_generators(sa, sb, scc))


# ---- 3. both sides of each planner boundary --------------------------------------------------------------------------
@pytest.mark.parametrize("log_m", [12, 13, 14])
def test_prove_on_both_sides_of_the_planner_boundaries(log_m):
    """The two thresholds of csrc/msm_geom.h at or under 2^14 points for this curve (prover377_cases.py):
      * msm_window_bits: tables of up to 6144 points take log2(n) + 1 window bits, larger ones (to 2^16) 15
        -- 2^12 is below (13 bits), 2^13 and 2^14 above;
      * msm_partition_plan: the partitioned digit sort from nwin * n >= 2^18, i.e. 15 421 points at 15 bits
        -- 2^13 is below (the direct atomic path), 2^14 above.
    nv = m, so the A / B1 / B / L tables have m + 2 points and H's m: both sorts are on the same side."""
    inst = P.Instance(ctx(), log_m, seed=30 + log_m)
    n_ab, n_h = inst.nv - 1 + 3, inst.m
    pk = inst.pk(ctx())
    try:
        info = pk.info()
        assert (info["n_ab"], info["n_h"]) == (n_ab, n_h)
        for n, c in ((n_ab, info["c_ab"]), (n_h, info["c_h"])):
            assert c == (15 if n >= P.WINDOW_15_FROM else log_m + 1) == ws.window_bits(n, True, ws.SCALAR_BITS[CURVE])
            g = ws.geometry(n, ws.SCALAR_BITS[CURVE], True, c)
            assert (g["nwin"] * n >= 1 << 18) == (n >= P.PARTITIONED_FROM) == (log_m == 14)
        w = inst.dense_witness()
        abc = inst.abc(w)
        rs = P.rand_fr(inst.rng, 2)
        got = P.affine(*ctx().prove(pk, *abc, w, rs[0], rs[1], scalars_mont=False))
    finally:
        pk.close()
    assert np.array_equal(got, inst.expected(abc, w, P.fr_int(rs[0]), P.fr_int(rs[1])))


# ---- 4. witness-shaped scalars ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,r_zero", [("bits", False), ("sparse", True)])
def test_prove_on_witness_shapes(kind, r_zero):
    """m = 2^12.  bits: half the entries of window 0 in ONE bucket, every other window empty; sparse: 98 % zeros -- the
    giant-bucket and the empty-bucket paths of the sort A, B1, B and L share.  r = 0 once: the B1 chain is skipped."""
    inst = P.Instance(ctx(), 12, seed=44)
    w = ws.shape(CURVE, inst.nv, kind, ws.SEEDS["proof"])
    w[0] = (1, 0, 0, 0)
    abc = inst.abc(w)
    rs = P.rand_fr(inst.rng, 2)
    if r_zero:
        rs[0] = 0
    pk = inst.pk(ctx())
    try:
        got = P.affine(*ctx().prove(pk, *abc, w, rs[0], rs[1], scalars_mont=False))
    finally:
        pk.close()
    assert np.array_equal(got, inst.expected(abc, w, P.fr_int(rs[0]), P.fr_int(rs[1])))


# ---- 5. table budget -------------------------------------------------------------------------------------------------
def test_prove_under_a_table_budget():
    """dg16_ctx_set_table_budget at 0.5 and 0.01 of the full tables, m = 2^12: a stride above 1, and the same proof as the
    full tables give (which is the oracle's)."""
    import dg16_amd
    c = dg16_amd.Context(0)               # a context of its own: the budget is a context setting
    try:
        inst = P.Instance(c, 12, seed=55)
        w = inst.dense_witness()
        abc = inst.abc(w)
        rs = P.rand_fr(inst.rng, 2)
        full = inst.pk(c)
        fi = full.info()
        assert fi["table_stride"] == 1
        want = P.affine(*c.prove(full, *abc, w, rs[0], rs[1], scalars_mont=False))
        full.close()
        assert np.array_equal(want, inst.expected(abc, w, P.fr_int(rs[0]), P.fr_int(rs[1])))
        for frac in (0.5, 0.01):
            c.set_table_budget(int(fi["table_bytes"] * frac))
            try:
                pk = inst.pk(c)
                info = pk.info()
                assert info["table_stride"] > 1 and info["table_bytes"] < fi["table_bytes"], frac
                got = P.affine(*c.prove(pk, *abc, w, rs[0], rs[1], scalars_mont=False))
                pk.close()
            finally:
                c.set_table_budget(0)
            assert np.array_equal(got, want), frac
    finally:
        c.close()


# ---- 6. shards -------------------------------------------------------------------------------------------------------
def test_sharded_prove_equals_the_bigint_prover():
    """The (nc, nw) = (45, 50) key split 1, 2, 3 and 8 ways: per-shard records concatenated as the all-gather would,
    assembled -> G.create_proof's proof."""
    ni, nc, nw = 2, 45, 50
    r1cs, w = G.synthetic_r1cs(F, num_constraints=nc, num_instance=ni, num_witness=nw, seed=11)
    rng = random.Random(8)
    td = tuple(rng.randrange(1, F.p) for _ in range(5))
    pk, _ = G.setup(CURVE, r1cs, td)
    a, b, c, dom = G.qap(r1cs, w, F)
    c_ = ctx()
    args = (CURVE, ni + nw, ni, dom.size) + P.arrays_of_bigint_key(pk)
    r, s = rng.randrange(1, F.p), rng.randrange(1, F.p)
    exp = G.create_proof(CURVE, pk, r, s, r1cs, w)
    rec_bytes = c_.results_bytes(CURVE)
    for world in (1, 2, 3, 8):
        keys = [c_.pk_create(*args, shard=k, n_shards=world) for k in range(world)]
        try:
            recs = [c_.groth16_msms(k, enc_fr(F, a), enc_fr(F, b), enc_fr(F, c), enc_fr(F, w), enc_fr(F, [r]), enc_fr(F, [s]))
                    for k in keys]
            assert all(rec.size == rec_bytes for rec in recs)
            got = _decoded(*c_.groth16_assemble(keys[0], np.concatenate(recs), enc_fr(F, [r]), enc_fr(F, [s])))
        finally:
            for k in keys:
                k.close()
        assert got == exp, world


def test_cyclic_shards_with_the_sharded_h_polynomial():
    """(log_m, world) = (11, 4): DG16_F_H_CYCLIC key shards, the three stages of the sharded h-polynomial (sharded_h),
    dg16_groth16_msms_h per shard, assembly == the unsharded proof of the same key and witness == the oracle's; and a
    cyclic shard refuses dg16_groth16_msms."""
    import torch
    import dg16_amd
    from test_gpu_hdist import sharded_h, dev_t
    log_m, world = 11, 4
    c_ = ctx()
    inst = P.Instance(c_, log_m, seed=66)
    w = inst.dense_witness()
    abc = inst.abc(w)
    rs = P.rand_fr(inst.rng, 2)
    want = inst.expected(abc, w, P.fr_int(rs[0]), P.fr_int(rs[1]))
    whole = inst.pk(c_)
    try:
        unsharded = P.affine(*c_.prove(whole, *abc, w, rs[0], rs[1], scalars_mont=False))
    finally:
        whole.close()
    assert np.array_equal(unsharded, want)
    hs = sharded_h(c_, CURVE, abc[0], abc[1], abc[2], world)
    keys = [inst.pk(c_, shard=k, n_shards=world, h_cyclic=True) for k in range(world)]
    try:
        assert all(k.info()["n_h"] == inst.m // world for k in keys)
        wd = dev_t(w)
        recs = []
        for k, key in enumerate(keys):
            hd = dev_t(hs[k])
            rec = torch.empty(c_.results_bytes(CURVE), dtype=torch.uint8, device=wd.device)
            torch.cuda.synchronize()
            c_.groth16_msms_h_dev(key, hd.data_ptr(), wd.data_ptr(), rs, rec.data_ptr(), scalars_mont=False)
            for ch in range(3):
                c_.sync(ch)
            recs.append(rec.cpu().numpy())
        got = P.affine(*c_.groth16_assemble(keys[0], np.concatenate(recs), rs[0], rs[1], scalars_mont=False))
        assert np.array_equal(got, want)
        with pytest.raises(dg16_amd.Dg16Error) as e:
            c_.groth16_msms(keys[0], *abc, w, rs[0], rs[1], scalars_mont=False)
        assert e.value.code == 3
    finally:
        for key in keys:
            key.close()


# ---- 7. the Libsnark reduction ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_m", [6, 10])
def test_libsnark_setup_and_prove_equal_the_model(log_m):
    """generate_parameters(reduction="libsnark") -> resident key -> prove(reduction="libsnark") == the model's discrete
    logs times the generators; without the prove flag the same witness gives another proof."""
    import dg16_amd
    p = F.p
    r1cs, w = M.instance(F, 1 << log_m, 3 * log_m, slack=((1 << log_m) // 2 - 1) if log_m == 10 else 0)
    rng = random.Random(log_m)
    td = tuple(rng.randrange(2, p) for _ in range(5))
    r, s = rng.randrange(1, p), rng.randrange(1, p)
    sc = M.libsnark_setup_scalars(r1cs, F, td)
    params = dg16_amd.generate_parameters(ctx(), CURVE, system_of(F, r1cs), trapdoor=td, reduction="libsnark")
    assert params.domain_size == 1 << log_m
    dpk = params.proving_key(ctx())
    try:
        a, b, c, viol = ctx().qap_r1cs(CURVE, r1cs["num_constraints"], r1cs["num_instance"], csr_of(F, r1cs["a"]),
                                       csr_of(F, r1cs["b"]), csr_of(F, r1cs["c"]), enc_fr(F, w))
        assert viol == (0, None)
        ma, mb, mc, dom = M.libsnark_abc(r1cs, w, F)
        assert np.array_equal(a, enc_fr(F, ma)) and np.array_equal(b, enc_fr(F, mb)) and np.array_equal(c, enc_fr(F, mc))
        proof = P.affine(*ctx().prove(dpk, a, b, c, enc_fr(F, w), enc_fr(F, [r]), enc_fr(F, [s]), reduction="libsnark"))
        sa, sb, scc = M.libsnark_proof_scalars(r1cs, F, td, sc, r, s, w, M.libsnark_h(ma, mb, mc, dom))
        assert G.verify_in_exponent(r1cs, F, td, sc, (sa, sb, scc), w)
        assert np.array_equal(proof, P.scalars_times_generators(sa, sb, scc))
        circom = P.affine(*ctx().prove(dpk, a, b, c, enc_fr(F, w), enc_fr(F, [r]), enc_fr(F, [s])))
        assert circom.any() and not np.array_equal(circom, proof)
    finally:
        dpk.close()


def test_sharded_entry_points_refuse_the_libsnark_flag():
    import torch
    import dg16_amd
    from dg16_amd import lib
    log_m = 4
    dev = torch.device("cuda", 0)
    c_ = ctx()
    r1cs, w = M.instance(F, 1 << log_m, 9, slack=0)
    params = dg16_amd.generate_parameters(c_, CURVE, system_of(F, r1cs), trapdoor=(3, 5, 7, 11, 13), reduction="libsnark")
    pk = params.proving_key(c_)
    m = 1 << log_m
    buf = [torch.zeros(m * 32, dtype=torch.uint8, device=dev) for _ in range(4)]
    wd = torch.zeros(len(w) * 32, dtype=torch.uint8, device=dev)
    rs = enc_fr(F, [1, 2])
    res = torch.zeros(4096, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    vp = ctypes.c_void_p
    T = lambda t: vp(t.data_ptr())          # noqa: E731
    flags = lib.F_DEVICE_PTRS | lib.F_SCALARS_MONT | lib.F_QAP_LIBSNARK
    rsp = rs.ctypes.data_as(vp)
    L = c_.L
    calls = {
        "dg16_groth16_msms": lambda: L.dg16_groth16_msms(c_.h, pk.h, T(buf[0]), T(buf[1]), T(buf[2]), T(wd), rsp, flags, T(res)),
        "dg16_groth16_msms_h": lambda: L.dg16_groth16_msms_h(c_.h, pk.h, T(buf[3]), T(wd), rsp, flags, T(res)),
        "dg16_groth16_prove_dist": lambda: L.dg16_groth16_prove_dist(c_.h, pk.h, None, T(buf[0]), T(buf[1]), T(buf[2]), T(wd),
                                                                     rsp, flags, T(res)),
    }
    try:
        for name, call in calls.items():
            assert call() == 7, name                                   # DG16_ERR_UNSUPPORTED
            assert b"LIBSNARK" in L.dg16_last_error(c_.h), name
        for ch in range(3):
            c_.sync(ch)
    finally:
        pk.close()


# ---- 8. a queue with the overlapped tail -----------------------------------------------------------------------------
def test_queue_with_the_overlapped_tail_across_curves():
    """Three witnesses and one of them again through one context with DG16_F_OVERLAP_TAIL and device pointers at m = 2^12,
    a BN254 proof between them (the persistent events and workspace slots are shared across curves): every queued proof
    equals the proof of the same inputs made one at a time, and the first of those the oracle's."""
    P.queue_case(ctx())


_QUEUE = r"""
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import dg16_amd
import prover377_cases
prover377_cases.queue_case(dg16_amd.Context(0))
print("ok")
"""


def test_queue_with_the_joined_schedule_in_a_child_process():
    """The same queue with DG16_QUEUE_JOIN=1 (read once per process: a child process)."""
    env = dict(os.environ)
    env["DG16_QUEUE_JOIN"] = "1"
    out = subprocess.run([sys.executable, "-c", _QUEUE % {"root": ROOT}], capture_output=True, text=True, timeout=300,
                         env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-4000:]


# ---- 9. contract -----------------------------------------------------------------------------------------------------
def test_pk_create_refuses_unknown_curves_and_foreign_keys():
    import dg16_amd
    c_ = ctx()
    inst = P.Instance(c_, 4, seed=77)
    k = inst.key
    arrs = [np.ascontiguousarray(k[n], dtype=np.uint64) for n in ("a_query", "b_g1_query", "b_g2_query", "h_query",
                                                                  "l_query", "fixed_points")]
    ptrs = [x.ctypes.data_as(ctypes.c_void_p) for x in arrs]
    for curve in (3, -1, 1 << 20):
        out = ctypes.c_void_p(0xDEAD)
        rc = c_.L.dg16_pk_create(c_.h, curve, inst.nv, inst.ni, inst.m, *ptrs, 0, ctypes.byref(out))
        assert rc == 2 and out.value is None, curve                    # DG16_ERR_BAD_CURVE, *out = NULL
        out = ctypes.c_void_p(0xDEAD)
        rc = c_.L.dg16_pk_create_shard(c_.h, curve, inst.nv, inst.ni, inst.m, *ptrs, 0, 2, 0, ctypes.byref(out))
        assert rc == 2 and out.value is None, curve
    # a key of one context handed to another
    other = dg16_amd.Context(0)
    pk = inst.pk(c_)
    try:
        w = inst.dense_witness()
        abc = inst.abc(w)
        with pytest.raises(dg16_amd.Dg16Error) as e:
            other.prove(pk, *abc, w, w[1], w[2], scalars_mont=False)
        assert e.value.code == 3                                       # DG16_ERR_BAD_ARG
        with pytest.raises(dg16_amd.Dg16Error) as e:
            other.groth16_msms(pk, *abc, w, w[1], w[2], scalars_mont=False)
        assert e.value.code == 3
        # ... and the owner still proves with it
        got = P.affine(*c_.prove(pk, *abc, w, w[1], w[2], scalars_mont=False))
        assert np.array_equal(got, inst.expected(abc, w, P.fr_int(w[1]), P.fr_int(w[2])))
    finally:
        pk.close()
        other.close()
