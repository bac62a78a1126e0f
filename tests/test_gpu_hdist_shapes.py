"""GPU parity of the sharded transforms of csrc/ntt.hip (dg16_ntt_dist_stage, dg16_h_poly_dist_stage) on every shard
shape -- what tests/test_gpu_hdist.py's seven + ten random points do not reach.  All N ranks are played by this process
on one context; the all-to-all is a tensor transpose (test_gpu_hdist.all_to_all).

Every comparison is np.array_equal on the raw limbs against the C oracle (corc.ntt, corc.h_poly) or against Python
integers (oracle/pyref/hdist.py and poly.py through tests/hdist_cases.py): bit-exact, nothing skipped or filtered.

  a. shape sweep on random data: N in (2, 4, 8) x log_M in {lg, lg + 1, 5, 9, 10, 11, 12, 17} (S = 1 and 2; one-pass
     plans of length 1 .. 5, 9 and 10; the two-pass plans (5,6), (6,6), (8,9); pieces below, equal to and above a tile),
     three fields up to 12, two at 17; on BN254 with two ranks also log_M = 20 ((10,10), transform only) and 21
     ((7,7,7): three passes with 2^20-element pieces).  Transform forward and inverse and the h-polynomial at every
     point, every rank compared.
  b. structured values: the 29 families of tests/ntt_cases.py through the sharded transform (a rank's cyclic subsample
     of a constant / geometric / alternating vector is again one: exact multiples of p at the piece stores), the six
     prover-shaped input families through the sharded h-polynomial.
  c. the stage contract: the send buffers after the h-polynomial's stages 0 and 1 and after the transform's stage 0
     against integers, in the layouts include/dg16.h documents, for every domain up to 2^8.
  d. DG16_NTT_TABLE_MIN_LOG=0 (the one-table twiddles, in production from a per-rank size of 2^21) with piece loads and
     stores, in child processes.
  e. sharded and unsharded calls alternating on one context (workspace slots 8 and 12, the twiddle cache).
  f. dg16_ntt_dist_stage's argument checks.

Not covered: per-rank sizes of 2^22 and above (log_M >= 22; config 5 at 2^24 over eight ranks is 2^21 per rank, the
largest per-rank plan here) -- left uncovered rather than approximated by a property test.  dg16_ntt_dist / dg16_h_poly_dist / dg16_groth16_prove_dist through a communicator with more than one
rank in one process are not driven either (tests/test_gpu_two_rank.py runs them across processes).
"""

import ctypes
import os
import random
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from oracle import corc
from oracle.pyref.fields import FR
from gpu_util import ctx
import hdist_cases as HC
import ntt_cases as NC
from test_gpu_hdist import DEV, all_to_all, dev_t, sharded_h
from test_gpu_ntt_structured import _h_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host(t, rows):
    return t.cpu().numpy().view(np.uint64).reshape(rows, 4)


def sharded_ntt(c, curve, x, n_ranks, inverse):
    """All ranks in this process.  x: host array (m x 4, Montgomery), the global input.  Returns (send, out): [rank] ->
    host array after stage 0 (the send buffer) and after stage 1."""
    M = x.shape[0] // n_ranks
    log_n = x.shape[0].bit_length() - 1
    send = []
    for r in range(n_ranks):
        src = dev_t(x[r::n_ranks])
        dst = torch.empty(M * 4, dtype=torch.int64, device=DEV)
        c.ntt_dist_stage_dev(curve, log_n, r, n_ranks, inverse, 0, src.data_ptr(), dst.data_ptr())
        c.sync(0)
        send.append(dst)
    recv = all_to_all(send)
    torch.cuda.synchronize()
    out = []
    for r in range(n_ranks):
        o = torch.empty(M * 4, dtype=torch.int64, device=DEV)
        c.ntt_dist_stage_dev(curve, log_n, r, n_ranks, inverse, 1, recv[r].data_ptr(), o.data_ptr())
        c.sync(0)
        out.append(host(o, M))
    return [host(t, M) for t in send], out


def sharded_h_stages(c, curve, a, b, cc, n_ranks):
    """sharded_h of test_gpu_hdist.py, keeping every send buffer: returns (send0, send1, out), [rank] -> host array."""
    m = a.shape[0]
    log_m = m.bit_length() - 1
    M = m // n_ranks
    rows = [[dev_t(v[r::n_ranks]) for v in (a, b, cc)] for r in range(n_ranks)]
    bufs = []
    for stage in range(3):
        dst = [torch.empty((3 if stage < 2 else 1) * M * 4, dtype=torch.int64, device=DEV) for _ in range(n_ranks)]
        for r in range(n_ranks):
            ins = [t.data_ptr() for t in rows[r]] if stage == 0 else [recv[r].data_ptr()]
            c.h_poly_dist_stage_dev(curve, log_m, r, n_ranks, stage, ins, dst[r].data_ptr())
        c.sync(0)
        bufs.append(dst)
        if stage < 2:
            recv = all_to_all(dst)
            torch.cuda.synchronize()
    return [[host(t, t.numel() // 4) for t in b_] for b_ in bufs]


def assert_ntt_ranks(got, X, n_ranks, what):
    M = X.shape[0] // n_ranks
    for r in range(n_ranks):
        assert np.array_equal(got[r], X[HC.ntt_out_index(n_ranks, M, r)]), (what, "rank %d" % r)


def assert_h_ranks(got, ref, n_ranks, what):
    for r in range(n_ranks):
        assert np.array_equal(got[r], ref[r::n_ranks]), (what, "rank %d" % r)


# ---- a. shape sweep on random data ------------------------------------------------------------------------------------
def _sweep_point(curve, n_ranks, log_M, with_ntt=True, with_h=True):
    log_n = log_M + HC.lg(n_ranks)
    m = 1 << log_n
    c = ctx()
    if with_ntt:
        x = corc.rand_field(curve, "fr", 700 + 37 * n_ranks + log_n, m)
        for inverse in (False, True):
            _, got = sharded_ntt(c, curve, x, n_ranks, inverse)
            assert_ntt_ranks(got, corc.ntt(curve, x, inverse=inverse), n_ranks, "inverse" if inverse else "forward")
    if with_h:
        a, b, cc = (corc.rand_field(curve, "fr", 710 + 41 * n_ranks + log_n + i, m) for i in range(3))
        assert_h_ranks(sharded_h(c, curve, a, b, cc, n_ranks), corc.h_poly(curve, a, b, cc), n_ranks, "h")


@pytest.mark.parametrize("curve,n_ranks,log_M", HC.sweep())
def test_shape_sweep_on_random_data(curve, n_ranks, log_M):
    """Per-rank plan and piece size of every point: hdist_cases.describe (the table is in the CHANGELOG)."""
    _sweep_point(curve, n_ranks, log_M)


@pytest.mark.parametrize("curve,n_ranks,log_M,what", [(c_, n, k, w) for c_, n, k, with_h in HC.EXTRA
                                                      for w in ("transform", "h") if w == "transform" or with_h])
def test_shape_sweep_largest_plans(curve, n_ranks, log_M, what):
    """(10,10) with 2^19-element pieces (the transform) and the three-pass plan (7,7,7) with 2^20-element pieces: the
    smallest shape at which three passes meet piece loads and stores.  The transform and the h-polynomial are separate
    cases (the oracle's h-polynomial at 2^22 is the whole cost of its case)."""
    _sweep_point(curve, n_ranks, log_M, with_ntt=what == "transform", with_h=what == "h")
    torch.cuda.empty_cache()


# ---- b. structured values ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", HC.ALL)
@pytest.mark.parametrize("n_ranks,log_n", HC.structured_shapes())
def test_structured_values_through_the_sharded_transform(curve, n_ranks, log_n):
    F = FR[curve]
    n = 1 << log_n
    M = n // n_ranks
    c = ctx()
    arrs = NC.arrays(F, n)
    assert len(arrs) == 29
    for a in arrs:
        for inverse in (False, True):
            what = (a.name, "inverse" if inverse else "forward")
            _, got = sharded_ntt(c, curve, a.x, n_ranks, inverse)
            assert_ntt_ranks(got, corc.ntt(curve, a.x, inverse=inverse), n_ranks, what)
            sp = a.inv if inverse else a.fwd
            if sp is None:
                continue
            # one non-zero output of the global transform: exactly one rank holds exactly one non-zero row, where the
            # layout out[k1 S + j] = X[M k1 + rank S + j] puts it, with the closed-form value
            nz = [(r, int(i)) for r in range(n_ranks) for i in np.flatnonzero(got[r].any(axis=1))]
            if sp.value == 0:
                assert nz == [], (what, nz[:8])
                continue
            assert nz == [HC.locate_ntt(n_ranks, M, sp.pos)], (what, sp.pos, nz[:8])
            assert np.array_equal(got[nz[0][0]][nz[0][1]], NC.enc(F, [sp.value])[0]), what


@pytest.mark.parametrize("curve", HC.ALL)
@pytest.mark.parametrize("n_ranks,log_m", HC.structured_shapes())
def test_structured_inputs_through_the_sharded_h_polynomial(curve, n_ranks, log_m):
    F = FR[curve]
    m = 1 << log_m
    c = ctx()
    xi = NC.enc(F, [F.root_of_unity(2 * m)])
    fams = _h_inputs(curve, log_m)
    assert len(fams) == 6
    for name, a, b, c_, _ in fams:
        got = sharded_h(c, curve, a, b, c_, n_ranks)
        assert_h_ranks(got, corc.h_poly(curve, a, b, c_), n_ranks, name)
        if name in ("zero", "ones"):
            assert not any(g.any() for g in got), name                   # a b - c vanishes identically
        if name.startswith(("b = 0", "a = zero")):
            # a b = 0 on the coset: minus c's evaluations on the shifted domain, sliced per rank
            shifted = corc.ntt(curve, corc.ntt(curve, c_, inverse=True), coset=xi)
            assert_h_ranks(got, corc.field_op(curve, "fr", "neg", shifted), n_ranks, name)


# ---- c. the stage contract --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", HC.ALL)
@pytest.mark.parametrize("n_ranks,log_m", HC.contract_shapes())
def test_send_buffers_of_every_stage_equal_the_integers(curve, n_ranks, log_m):
    """include/dg16.h: the h-polynomial's send buffers are [peer][vector][S], the transform's is natural order = N
    pieces of S.  Callers that run the exchange themselves (parallel.py, the Rust shim) rely on it; a stage that is
    wrong in a way a later stage undoes must not pass."""
    F = FR[curve]
    m = 1 << log_m
    c = ctx()
    rng = random.Random(97 * m + n_ranks)
    data = [("random", [[rng.randrange(F.p) for _ in range(m)] for _ in range(3)]), ("ones", [[1] * m] * 3)]
    for name, (a, b, cc) in data:
        send0, send1, out = HC.h_stages(a, b, cc, F, n_ranks)
        g0, g1, g2 = sharded_h_stages(c, curve, NC.enc(F, a), NC.enc(F, b), NC.enc(F, cc), n_ranks)
        for r in range(n_ranks):
            assert np.array_equal(g0[r], NC.enc(F, send0[r])), (name, "stage 0", "rank %d" % r)
            assert np.array_equal(g1[r], NC.enc(F, send1[r])), (name, "stage 1", "rank %d" % r)
            assert np.array_equal(g2[r], NC.enc(F, out[r])), (name, "stage 2", "rank %d" % r)
        for inverse in (False, True):
            send, res = sharded_ntt(c, curve, NC.enc(F, a), n_ranks, inverse)
            exp_send, exp_out = HC.ntt_send(a, F, n_ranks, inverse), HC.ntt_out(a, F, n_ranks, inverse)
            for r in range(n_ranks):
                assert np.array_equal(send[r], NC.enc(F, exp_send[r])), (name, "transform stage 0", inverse, "rank %d" % r)
                assert np.array_equal(res[r], NC.enc(F, exp_out[r])), (name, "transform stage 1", inverse, "rank %d" % r)


# ---- d. one-table twiddles with pieces --------------------------------------------------------------------------------
# full_twiddle_min_log() reads DG16_NTT_TABLE_MIN_LOG once per process: the setting runs in fresh pythons
_ONE_TABLE_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
from oracle import corc
from oracle.pyref.fields import FR
import ntt_cases as NC
import dg16_amd
from test_gpu_hdist import sharded_h
from test_gpu_hdist_shapes import sharded_ntt, assert_ntt_ranks, assert_h_ranks
curve, n_ranks, logs = %(curve)r, %(n_ranks)r, %(logs)r
F = FR[curve]
c = dg16_amd.Context(0)
for log_M in logs:
    m = n_ranks << log_M
    rnd = [corc.rand_field(curve, "fr", 800 + log_M + 5 * n_ranks + i, m) for i in range(3)]
    wit = [NC.witness_arr(F, m, seed=9 + i) for i in range(2)]
    wit.append(corc.field_op(curve, "fr", "mul", wit[0], wit[1]))
    for name, (a, b, c_) in (("random", rnd), ("witness-shaped", wit)):
        for inverse in (False, True):
            _, got = sharded_ntt(c, curve, a, n_ranks, inverse)
            assert_ntt_ranks(got, corc.ntt(curve, a, inverse=inverse), n_ranks, (log_M, name, inverse))
        assert_h_ranks(sharded_h(c, curve, a, b, c_, n_ranks), corc.h_poly(curve, a, b, c_), n_ranks, (log_M, name))
print("ok")
"""
# one passing child on the MI355X host, measured: 2.9 s (BN254, N = 2), 4.8 s (BN254, N = 8), 3.2 s (BLS12-381, N = 2),
# 5.1 s (BLS12-381, N = 8), start of the interpreter included; the limit is ten times the slowest, the convention of
# the stream-order tests
CHILD_MEASURED_S = 5.1
CHILD_LIMIT_S = 10 * CHILD_MEASURED_S


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_one_table_twiddles_with_piece_loads_and_stores(curve):
    """DG16_NTT_TABLE_MIN_LOG=0: tw_full in the per-rank plans (5,6), (6,6) and (8,9) together with dst pieces (stage 0
    of both entry points, inverse: the table carries 1 / M) and src pieces (the h-polynomial's stage 2).  The default
    builds these tables from a per-rank size of 2^21 only.  One child after another; the first failure ends the test."""
    for n_ranks in (2, 8):
        e = dict(os.environ, DG16_NTT_TABLE_MIN_LOG="0")
        src = _ONE_TABLE_CHILD % {"root": ROOT, "curve": curve, "n_ranks": n_ranks, "logs": [11, 12, 17]}
        t0 = time.perf_counter()
        out = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, timeout=CHILD_LIMIT_S, env=e)
        print("one-table child %s N = %d: %.1f s" % (curve, n_ranks, time.perf_counter() - t0))
        assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (curve, n_ranks, out.stdout[-2000:] + out.stderr[-4000:])


# ---- e. one context, interleaved --------------------------------------------------------------------------------------
def test_sharded_and_unsharded_calls_interleaved_on_one_context():
    """Workspace slot 8 (scratch of every transform), slot 12 (dg16_h_poly's vectors, stage 2's vectors) and the twiddle
    cache are shared by dg16_ntt, dg16_h_poly and the stages: a sequence that alternates them at different sizes, the
    first call repeated at the end."""
    c = ctx()

    def abc(curve, log_m, seed):
        return [corc.rand_field(curve, "fr", seed + i, 1 << log_m) for i in range(3)]

    v1 = abc("bn254", 12, 900)
    first = c.h_poly("bn254", *v1)
    assert np.array_equal(first, corc.h_poly("bn254", *v1))
    v2 = abc("bn254", 14, 910)
    assert_h_ranks(sharded_h(c, "bn254", *v2, 4), corc.h_poly("bn254", *v2), 4, "h stages N = 4, 2^14")
    x3 = corc.rand_field("bls12_381", "fr", 920, 1 << 13)
    assert np.array_equal(c.ntt("bls12_381", x3, inverse=True), corc.ntt("bls12_381", x3, inverse=True))
    x4 = corc.rand_field("bn254", "fr", 930, 1 << 9)
    for inverse in (False, True):
        _, got = sharded_ntt(c, "bn254", x4, 8, inverse)
        assert_ntt_ranks(got, corc.ntt("bn254", x4, inverse=inverse), 8, ("transform stages N = 8, 2^9", inverse))
    v5 = abc("bn254", 6, 940)
    assert_h_ranks(sharded_h(c, "bn254", *v5, 2), corc.h_poly("bn254", *v5), 2, "h stages N = 2, 2^6")
    again = c.h_poly("bn254", *v1)
    assert np.array_equal(again, first)


# ---- f. argument checks of dg16_ntt_dist_stage ------------------------------------------------------------------------
def test_sharded_ntt_argument_checks():
    """Every refused call returns the status csrc/capi.hip and csrc/ntt.hip give it (DG16_ERR_BAD_ARG = 3,
    DG16_ERR_UNSUPPORTED = 7) and launches nothing: the output buffer keeps its fill.  A valid call on the same context
    follows each."""
    import dg16_amd
    from dg16_amd.lib import CURVES, F_DEVICE_PTRS
    c = ctx()
    log_n, n_ranks = 8, 4
    M = (1 << log_n) // n_ranks
    x = corc.rand_field("bn254", "fr", 950, 1 << log_n)
    X = corc.ntt("bn254", x)
    fill = 0x5A5A5A5A5A5A5A5A
    src = dev_t(x[0::n_ranks])
    bad = [(dict(n_ranks=3), 3), (dict(n_ranks=16, log_n=10), 7), (dict(log_n=3), 3), (dict(rank=4), 3), (dict(rank=9), 3),
           (dict(stage=2), 3), (dict(stage=-1), 3)]
    for kw, code in bad:
        a = dict(log_n=log_n, rank=0, n_ranks=n_ranks, stage=0)
        a.update(kw)
        dst = torch.full((M * 4,), fill, dtype=torch.int64, device=DEV)
        with pytest.raises(dg16_amd.Dg16Error) as ei:
            c.ntt_dist_stage_dev("bn254", a["log_n"], a["rank"], a["n_ranks"], False, a["stage"], src.data_ptr(), dst.data_ptr())
        c.sync(0)
        assert ei.value.code == code, (kw, ei.value.code)
        assert bool((dst == fill).all()), kw
        _, got = sharded_ntt(c, "bn254", x, n_ranks, False)
        assert_ntt_ranks(got, X, n_ranks, ("after", kw))
    # host pointers (no DG16_F_DEVICE_PTRS): refused before anything is read
    hin = np.ascontiguousarray(x[0::n_ranks])
    hout = np.full((M, 4), fill, dtype=np.uint64)
    vp = lambda arr: ctypes.c_void_p(arr.ctypes.data)      # noqa: E731
    for flags in (0, 1):
        assert flags & F_DEVICE_PTRS == 0
        rc = c.L.dg16_ntt_dist_stage(c.h, CURVES["bn254"], log_n, 0, n_ranks, 0, 0, vp(hin), vp(hout), flags, 0)
        assert rc == 3, (flags, rc)
        assert (hout == fill).all()
    # null operands
    dst = torch.full((M * 4,), fill, dtype=torch.int64, device=DEV)
    for i_ptr, o_ptr in ((None, ctypes.c_void_p(dst.data_ptr())), (ctypes.c_void_p(src.data_ptr()), None)):
        assert c.L.dg16_ntt_dist_stage(c.h, CURVES["bn254"], log_n, 0, n_ranks, 0, 0, i_ptr, o_ptr, F_DEVICE_PTRS, 0) == 3
    c.sync(0)
    assert bool((dst == fill).all())
    _, got = sharded_ntt(c, "bn254", x, n_ranks, False)
    assert_ntt_ranks(got, X, n_ranks, "after the refused calls")
