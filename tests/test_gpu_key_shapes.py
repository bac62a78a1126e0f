"""GPU parity on key-shaped bases (tests/key_shapes.py): identity-heavy queries, repeated and opposite points, one point
n times, P / -P alternations, doubling chains and a mix of them in a real key's proportions -- through the plain MSM,
the resident (table) MSM, thinned tables and whole proofs, bit-exact against the oracle in affine form and against a
closed form that needs no Pippenger wherever one exists.

`gen_bases` rows are distinct, unrelated and never the identity, so the group law's other branches -- P + P, P + (-P),
an identity operand, in the accumulation kernels, the in-workgroup tree, finalize, stitch, giant and fold, the row and
top kernels and the Horner tail -- are reached by such bases only by accident.  Here they are reached on purpose: with
`same` scalars both members of a pair land in the same bucket of every window, with `sparse_live` they are alone there
(the accumulator's second addition IS the doubling or the cancellation), with one point n times every segment partial,
tree node and giant slice is a multiple of one point.  test_key_shapes.py asserts on the host which bucket contents and
which finalize / giant / merged-launch regime each case below reaches; the cases themselves live in key_shapes.py.

The order of a bucket's entries comes from atomics: a wrong sum may show in one run and not in the next."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import corc
from gpu_util import ctx
import key_shapes as ks
import witness_shapes as ws

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _threads():
    import bench
    return bench.cpu_threads()


def _mul(curve, group):
    return lambda sc, base: ctx().fixed_base_mul(curve, group, sc, base=base)


@functools.lru_cache(maxsize=4)
def _rows(curve, group, n):
    seed = ks.SEEDS["rows"] + group
    b = ctx().gen_bases(curve, group, seed, n) if n >= 1 << 12 else corc.gen_points(curve, group, seed, n)
    b.setflags(write=False)
    return b


def _bases(shape, curve, group, n):
    bases, live = ks.make_bases(shape, curve, group, _rows(curve, group, n), ks.SEEDS["rows"], _mul(curve, group))
    for i in (0, 1, n // 2, n - 1):
        assert corc.on_curve(curve, group, bases[i:i + 1]) or not bases[i].any()
    return bases, live


def _msm(curve, group, bases, sc):
    return corc.msm(curve, group, bases, sc, threads=_threads())


def _pair_equal(sc):
    m = len(sc) // 2
    return np.array_equal(sc[0:2 * m:2], sc[1:2 * m:2])


def _closed_form(shape, curve, group, bases, live, sc):
    """The result without a Pippenger over the shaped bases, or None where the shape has no closed form."""
    n = len(sc)
    m = n // 2
    last = corc.point_mul(curve, group, bases[n - 1:n], ws.to_ints(sc[n - 1:n])[0]) if n % 2 else None
    if shape in ("pairs", "opposites") and _pair_equal(sc):
        out = np.zeros((1, bases.shape[1]), dtype=np.uint64)
        if shape == "pairs":
            half = _msm(curve, group, bases[0:2 * m:2], sc[0:2 * m:2])
            out = corc.point_add(curve, group, half, half)
        return out if last is None else corc.point_add(curve, group, out, last)
    if shape.startswith("identity_"):
        return _msm(curve, group, bases[live], sc[live])
    if shape == "chain":
        return corc.point_mul(curve, group, bases[:1], ks.chain_scalar(curve, sc))
    if shape == "all_equal":
        return corc.point_mul(curve, group, bases[:1], ks.sum_mod_r(curve, sc))
    if shape == "alternating":
        v = ws.to_ints(sc)
        return corc.point_mul(curve, group, bases[:1], (sum(v[0::2]) - sum(v[1::2])) % ks.modulus(curve))
    return None


def _check(shape, curve, group, bases, live, sc, got, oracle=True, label=None):
    got = np.asarray(got).reshape(1, -1)
    if oracle:
        assert np.array_equal(got, _msm(curve, group, bases, sc)), ("oracle", label)
    closed = _closed_form(shape, curve, group, bases, live, sc)
    assert closed is not None or oracle
    if closed is not None:
        assert np.array_equal(got, closed), ("closed form", label)
    if shape == "opposites" and _pair_equal(sc) and len(sc) % 2 == 0:
        assert not got.any()


# ---- (a) plain dg16_msm ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,group,n,shape", ks.PLAIN)
def test_plain_msm_on_key_shapes(curve, group, n, shape):
    """2^10 (the direct sort) and 2^14 + 37 (the partitioned sort), with and without the subgroup flag on the cofactor
    groups.  pairs / opposites: `same` scalars at 2^10 (every bucket holds whole pairs), `sparse_live` at 2^14 + 37 (a pair
    alone in a bucket of every window); the identity shapes, real_key and chain with dense scalars."""
    bases, live = _bases(shape, curve, group, n)
    for sub in ks.subgroup_flags(curve, group):
        kind, sc = ks.plain_scalars(curve, group, n, shape, sub)
        got = corc.jac_to_affine(curve, group, ctx().msm(curve, group, bases, sc, in_subgroup=sub))
        _check(shape, curve, group, bases, live, sc, got, label=(curve, group, n, shape, kind, sub))


@pytest.mark.parametrize("curve,group,n,shape,kind", ks.ONE_POINT)
def test_plain_msm_on_one_point(curve, group, n, shape, kind):
    """One point n times, or P, -P, P, ..: every segment partial, tree node, giant slice and fold operand is a multiple of
    ONE point or the identity, at every level -- n P / the identity for `ones`.  BN254 G1 at 2^12 with random scalars is
    the group test_all_equal_points_at_a_size_with_giant_buckets lacks (the tree and the stitch kernel); 2^20 (stitch giants,
    slices of more than 512 partials) is checked against the closed form alone."""
    p = _rows(curve, group, 1 << 10)[:1]
    bases = ks.all_equal(p, n) if shape == "all_equal" else ks.alternating(curve, group, p, n)
    sc = ks.scalars_of(kind, curve, n, ks.SEEDS["plain"])
    for sub in (ks.subgroup_flags(curve, group) if n <= 1 << 16 else (True,)):
        got = corc.jac_to_affine(curve, group, ctx().msm(curve, group, bases, sc, in_subgroup=sub))
        _check(shape, curve, group, bases, None, sc, got, oracle=n <= 1 << 16, label=(curve, group, n, shape, kind, sub))
        if kind == "ones":
            want = corc.point_mul(curve, group, p, n) if shape == "all_equal" else np.zeros_like(p)
            assert np.array_equal(got, want)


# ---- (b) resident MSM (dg16_bases_upload + dg16_msm_resident) ----------------------------------------------------------
@pytest.mark.parametrize("curve,group,n,shape", ks.RESIDENT)
def test_resident_msm_on_key_shapes(curve, group, n, shape):
    """One upload per base shape (msm_table_kernel doubles identities, copies and chain points into every table row), several
    scalar vectors per upload.  In a chain's table row j of P_i is P_(i + c j): the same affine point sits there many times."""
    c = ctx()
    bases, live = _bases(shape, curve, group, n)
    g = ks.table_geometry(curve, n)
    hb = c.bases_upload(curve, group, bases)
    try:
        assert hb.info()["window_bits"] == g["c"]
        for kind in ks.resident_scalar_kinds(shape):
            sc = ks.resident_scalars(curve, n, kind, g)
            got = c.msm_resident(hb, sc, affine=True)
            _check(shape, curve, group, bases, live, sc, got, label=(curve, group, n, shape, kind))
    finally:
        hb.close()


@pytest.mark.parametrize("curve,group,n,rows,shape,kinds", ks.THINNED)
def test_resident_msm_on_key_shapes_under_a_table_budget(curve, group, n, rows, shape, kinds):
    """A thinned table (stride > 1): several bucket sets and the Horner tail.  With dense scalars every set is live; with
    `bits` only the first is, and the tail's doublings and additions run on the identity (test_key_shapes.py)."""
    import dg16_amd
    bases, live = _bases(shape, curve, group, n)
    c = dg16_amd.Context(0)
    hb = None
    try:
        hb = c.bases_upload(curve, group, bases)
        full = hb.info()
        hb.close()
        nwin = ws.nwin_of(full["window_bits"], ws.SCALAR_BITS[curve])
        stride = ks.thinned_stride(curve, n, rows)
        c.set_table_budget(bases.nbytes * rows)
        hb = c.bases_upload(curve, group, bases)
        info = hb.info()
        kept = (nwin + stride - 1) // stride
        assert info["window_bits"] == full["window_bits"] and info["table_bytes"] < full["table_bytes"]
        assert abs(info["table_bytes"] / full["table_bytes"] - kept / nwin) < 0.5 / nwin
        g = ks.table_geometry(curve, n, stride)
        for kind in kinds:
            sc = ks.scalars_of(kind, curve, n, ks.SEEDS["budget"], ks.sparse_live_k(g, 2))
            got = c.msm_resident(hb, sc, affine=True)
            _check(shape, curve, group, bases, live, sc, got, label=(curve, group, n, shape, kind))
    finally:
        if hb is not None:
            hb.close()
        c.close()


@pytest.mark.parametrize("curve,group,n,count", ks.ALIAS)
def test_resident_msm_row_aliasing_on_a_chain(curve, group, n, count):
    """Chain bases, k[i] = d 2^(c j) and k[i + c j] = d, everything else zero: table row j of P_i and row 0 of P_(i + c j)
    are the same affine point and enter the same bucket d -- a doubling inside the accumulation.  The twin's 2^c - d
    (digits -d, +1) cancels there instead."""
    c = ctx()
    bases, _ = _bases("chain", curve, group, n)
    hb = c.bases_upload(curve, group, bases)
    try:
        wb = hb.info()["window_bits"]
        assert wb == ws.window_bits(n, True, ws.SCALAR_BITS[curve])
        tr = ks.alias_triples(curve, n, wb, count, ks.SEEDS["alias"])
        for twin in (False, True):
            sc = ks.alias_scalars(curve, n, wb, tr, twin)
            got = c.msm_resident(hb, sc, affine=True).reshape(1, -1)
            nz = sc.any(axis=1)
            assert np.array_equal(got, corc.msm(curve, group, bases[nz], sc[nz], algo=1)), twin
            assert np.array_equal(got, corc.point_mul(curve, group, bases[:1], ks.alias_closed_form(curve, wb, tr, twin))), twin
    finally:
        hb.close()


# ---- (c) whole proofs against bench.oracle_prove --------------------------------------------------------------------------
def _put(t, arr):
    import torch
    t.copy_(torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).to(t.device))


def _pk_of(c, wl, **kw):
    return c.pk_create(wl.curve, wl.nv, wl.ni, wl.m, wl.aq.data_ptr(), wl.b1q.data_ptr(), wl.b2q.data_ptr(),
                       wl.hq.data_ptr(), wl.lq.data_ptr(), wl.fixed.data_ptr(), device_ptrs=True, **kw)


def _rekey(c, wl, key):
    """The five queries of `wl` rewritten in place on the device with rows of key shape `key`; the resident key re-created
    as Workload.__init__ creates it.  bench.oracle_prove reads the same tensors."""
    import torch
    import bench
    l1, l2 = bench.FQ_BYTES[wl.curve] // 4, bench.FQ_BYTES[wl.curve] // 2
    ts = {"a": (wl.aq, l1), "b1": (wl.b1q, l1), "b2": (wl.b2q, l2), "h": (wl.hq, l1), "l": (wl.lq, l1)}
    q = {k: bench.to_host_u64(t, l).copy() for k, (t, l) in ts.items()}
    new = ks.key_queries(key, wl.curve, q, ks.SEEDS["proof"],
                         mul=lambda g, s, b: c.fixed_base_mul(wl.curve, g, s, base=b))
    for k, (t, _) in ts.items():
        assert new[k].shape == q[k].shape
        _put(t, new[k])
    torch.cuda.synchronize()
    old, wl.pk = wl.pk, None                     # (a caller's `finally` must not close the old key a second time)
    old.close()
    wl.pk = _pk_of(c, wl, shard=wl.rank, n_shards=wl.world, h_cyclic=wl.h_sharded)
    return new


def _set_witness(wl, w_rest):
    import torch
    wl.w[1:] = torch.from_numpy(np.ascontiguousarray(w_rest).view(np.int64)).to(wl.dev)
    torch.cuda.synchronize()


def _prove_and_check(c, wl, label, rs=None):
    import bench
    gp = bench.prove_once(c, wl, rs)
    if rs is None:
        (A, B, C), _ = bench.oracle_prove(wl, _threads())
    else:
        r, s = ws.to_ints(rs)
        (A, B, C), _ = bench.oracle_prove(wl, _threads(), r=r, s=s)
    gA, gB, gC = bench.gpu_proof_affine(wl.curve, gp)
    assert np.array_equal(A, gA) and np.array_equal(B, gB) and np.array_equal(C, gC), label
    assert A.any() and B.any() and C.any(), label


def _proof_case(curve, log_m, shape, key, budget):
    import torch
    import bench
    import dg16_amd
    c = dg16_amd.Context(0) if budget else ctx()
    wl = bench.Workload(c, torch.device("cuda", 0), log_m, 0, 1, seed=120 + log_m, curve=curve, **shape)
    try:
        if budget:
            full = wl.pk.info()["table_bytes"]
            c.set_table_budget(int(full * budget))
        _rekey(c, wl, key)
        if budget:
            info = wl.pk.info()
            assert info["table_stride"] > 1 and info["table_bytes"] < full, info
        for i, kind in enumerate(ks.PROOF_WITNESSES):
            _set_witness(wl, ks.proof_witness(curve, wl.nv, kind, i))
            _prove_and_check(c, wl, (curve, log_m, key, kind))
        if (curve, log_m, key) in ks.RS_ZERO_CASES:
            _prove_and_check(c, wl, (curve, log_m, key, "r = s = 0"), rs=np.zeros((2, 4), dtype=np.uint64))
    finally:
        if wl.pk is not None:
            wl.pk.close()
        if budget:
            c.close()


@pytest.mark.parametrize("curve,log_m,shape,key,budget", ks.PROOFS)
def test_proof_on_key_shapes(curve, log_m, shape, key, budget):
    """real: b1q and b2q the identity on the same 70 % of the wires, aq on 30 %, 5 % of lq copies; chain: all five queries
    doubling chains (local_dummy_crs); degenerate: every query one repeated point, b2q alternating P, -P.  Dense and bits
    witnesses; r = s = 0 too for one case per curve.  All of these run the merged A / B1 / L launch, the thinned key at any
    stride (test_key_shapes.py): 2^16 wires are still under the 2^22 entries from which the prover launches separately."""
    _proof_case(curve, log_m, shape, key, budget)


_CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import test_gpu_key_shapes as t
t._proof_case(%(curve)r, %(log_m)d, {}, %(key)r, None)
print("ok")
"""


def test_proof_on_a_real_key_with_separate_launches():
    """DG16_ABL_MERGED=0 (read once per process: a child process): A, B1 and L as three accumulation launches with their own
    reductions, on the real key at 2^16 -- by itself the prover separates them only past 2^17 wires."""
    curve, log_m, key = ks.PROOF_SEPARATE
    env = dict(os.environ)
    env["DG16_ABL_MERGED"] = "0"
    out = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT, "curve": curve, "log_m": log_m, "key": key}],
                         capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


def test_two_shard_proof_on_a_real_key():
    """groth16_msms per shard + groth16_assemble: each shard's slice of the real key has its own runs of identities."""
    import torch
    import bench
    curve, log_m, key, world = ks.SHARDED
    c = ctx()
    dev = torch.device("cuda", 0)
    wl = bench.Workload(c, dev, log_m, 0, 1, seed=140, curve=curve)
    keys = []
    try:
        _rekey(c, wl, key)
        _set_witness(wl, ks.proof_witness(curve, wl.nv, "bits", 7))
        keys = [_pk_of(c, wl, shard=k, n_shards=world) for k in range(world)]
        wl.qap()
        c.sync(0)
        recs = []
        for k in keys:
            rec = torch.empty(c.results_bytes(curve), dtype=torch.uint8, device=dev)
            c.groth16_msms_dev(k, wl.a.data_ptr(), wl.b.data_ptr(), wl.c.data_ptr(), wl.w.data_ptr(), wl.rs, rec.data_ptr(),
                               scalars_mont=False)
            for ch in range(3):
                c.sync(ch)
            recs.append(rec)
        gathered = torch.cat(recs)
        proof = torch.empty(wl.proof_bytes(), dtype=torch.uint8, device=dev)
        c.groth16_assemble_dev(keys[0], gathered.data_ptr(), world, wl.rs, proof.data_ptr(), scalars_mont=False)
        c.sync(0)
        (A, B, C), _ = bench.oracle_prove(wl, _threads())
        gA, gB, gC = bench.gpu_proof_affine(curve, proof.cpu().numpy())
        assert np.array_equal(A, gA) and np.array_equal(B, gB) and np.array_equal(C, gC)
        assert A.any() and B.any() and C.any()
    finally:
        for k in keys:
            k.close()
        if wl.pk is not None:
            wl.pk.close()


@pytest.mark.parametrize("log_m,key", ks.PROOFS_377)
def test_proof_on_key_shapes_bls12_377(log_m, key):
    """The resident BLS12-377 prover on a real and a chain key (the reference's own curve and its benchmark's CRS shape)."""
    import prover377_cases as P
    c = ctx()
    inst = P.Instance(c, log_m, seed=57)
    names = {"a": "a_query", "b1": "b_g1_query", "b2": "b_g2_query", "h": "h_query", "l": "l_query"}
    new = ks.key_queries(key, P.CURVE, {k: inst.key[v] for k, v in names.items()}, ks.SEEDS["proof"],
                         mul=lambda g, s, b: c.fixed_base_mul(P.CURVE, g, s, base=b))
    for k, v in names.items():
        inst.key[v] = new[k]
    pk = inst.pk(c)
    try:
        cases = [(kind, P.rand_fr(inst.rng, 2)) for kind in ks.PROOF_WITNESSES]
        if (P.CURVE, log_m, key) in ks.RS_ZERO_CASES:
            cases.append(("dense", np.zeros((2, 4), dtype=np.uint64)))
        for i, (kind, rs) in enumerate(cases):
            w = np.zeros((inst.nv, 4), dtype=np.uint64)
            w[0, 0] = 1
            w[1:] = ks.proof_witness(P.CURVE, inst.nv, kind, i)
            abc = inst.abc(w)
            got = P.affine(*c.prove(pk, *abc, w, rs[0], rs[1], scalars_mont=False))
            assert np.array_equal(got, inst.expected(abc, w, P.fr_int(rs[0]), P.fr_int(rs[1]))), (log_m, key, kind)
    finally:
        pk.close()
