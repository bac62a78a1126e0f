"""GPU: "each channel owns a HIP stream and a workspace; calls on different channels may run concurrently from different
host threads" (include/dg16.h).  (a) the same call on channels 0, 1, 2 gives the same bytes and the oracle's value, before
and after a proof has left its buffers in the workspaces of channels 1 and 2; (b) three host threads, one per channel, run
a fixed seeded mix of calls -- with NTT and h-polynomial sizes the process has not used before, so the threads race to
create the same twiddle set and the same coset set -- and a fourth thread proves meanwhile; (c) two contexts on one
device, one thread each.  Every result is compared with values the oracle computed before the threads started.

(b) and (c) run in ONE child process (this file as a script): a deadlock ends the child, not the suite.  The child times
the single-threaded mix first and gives every threaded phase ten times that (printed); the parent's own limit is only
the ceiling above it."""

import os
import random
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVE = "bn254"
ROUNDS, ROUNDS_SHORT = 40, 10
# NTT / h-polynomial sizes (log2).  TIMING: the single-threaded timing run; the others are each used for the first time
# by the phase named, all threads reaching a size's first round together (a barrier), so its tables are created in a race.
# The timing run takes the sizes the phases leave over, up to one above their largest: its rounds move 17 K elements on
# average, the prover phase's 16 K and the thread phase's 3 K, so the limit is measured on a mix no lighter than theirs.
LOGS_TIMING = [8, 10, 12, 16]
LOGS_THREADS = [7, 9, 11, 13, 5, 6, 14, 4]
LOGS_PROVER_PHASE = [3, 15]
LOGS_TWO_CONTEXTS = [7, 9, 10, 12]
H_LIBSNARK_MAX_LOG = 9          # the Python model of the Libsnark quotient is quadratic; the other h runs at the size itself


# ---- (a) channel parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_every_channel_gives_the_oracles_bytes_before_and_after_a_proof():
    import torch
    import bench
    import dg16_amd
    from dg16_amd import verify
    import stream_cases as SC
    from oracle import corc
    ctx = dg16_amd.Context(0)
    dev = torch.device("cuda", 0)
    keep = []
    try:
        n = (1 << 10) + 37
        bases, sc = corc.gen_points(CURVE, 1, 301, n), corc.rand_field(CURVE, "fr", 302, n, mont=False)
        want_msm = corc.msm(CURVE, 1, bases, sc)
        hb = ctx.bases_upload(CURVE, 1, bases)
        keep.append(hb)
        x = corc.rand_field(CURVE, "fr", 303, 1 << 10)
        want_ntt = corc.ntt(CURVE, x)
        a, b, c = (corc.rand_field(CURVE, "fr", 304 + i, 1 << 10) for i in range(3))
        want_h = corc.h_poly(CURVE, a, b, c)
        v = SC.verify_material(CURVE)
        pvk = verify.PreparedVerifyingKey(ctx, CURVE, *v["vk"])
        keep.append(pvk)
        pts, ks = corc.gen_points(CURVE, 1, 307, 65), corc.rand_field(CURVE, "fr", 308, 65, mont=False)
        want_mul = np.concatenate([corc.point_mul(CURVE, 1, pts[i:i + 1], k) for i, k in enumerate(corc.arr_to_ints(ks))])

        def all_channels(when):
            for ch in range(3):
                what = "channel %d, %s the proof: " % (ch, when)
                assert np.array_equal(ctx.msm(CURVE, 1, bases, sc, affine=True, channel=ch), want_msm), what + "msm"
                assert np.array_equal(ctx.msm_resident(hb, sc, affine=True, channel=ch), want_msm), what + "msm_resident"
                assert np.array_equal(ctx.ntt(CURVE, x, channel=ch), want_ntt), what + "ntt"
                assert np.array_equal(ctx.h_poly(CURVE, a, b, c, channel=ch), want_h), what + "h_poly"
                assert np.array_equal(pvk.verify_batch(v["x"], v["mixed"], channel=ch), v["verdict"].astype(bool)), \
                    what + "verify_batch"
                assert np.array_equal(ctx.points_mul(CURVE, 1, pts, ks, channel=ch), want_mul), what + "points_mul"

        all_channels("before")
        wl = bench.Workload(ctx, dev, 10, 0, 1, seed=43, curve=CURVE)
        keep.append(wl.pk)
        got = bench.gpu_proof_affine(CURVE, bench.prove_once(ctx, wl))
        for name, g, w in zip("ABC", got, bench.oracle_prove(wl, bench.cpu_threads())[0]):
            assert np.array_equal(g, w), "the proof between the two rounds: %s" % name
        all_channels("after")
    finally:
        for h in keep:
            h.close()
        ctx.close()


# ---- (b), (c): the child ----------------------------------------------------------------------------------------------------------
class Mix:
    """The calls of one thread (seeded by `tid`) with the oracle's results, all made before any thread starts."""

    def __init__(self, tid, logs, table_bases):
        from oracle import corc
        self.tid, self.logs = tid, logs
        s = 1000 * (tid + 1)
        self.msm = []
        for j, n in enumerate((1 << 10, 1 << 14)):
            bases, sc = corc.gen_points(CURVE, 1, s + j, n), corc.rand_field(CURVE, "fr", s + 10 + j, n, mont=False)
            self.msm.append((bases, sc, corc.msm(CURVE, 1, bases, sc)))
        self.ntt = {}
        self.h = {}
        for lg in logs:
            x = corc.rand_field(CURVE, "fr", s + 20 + lg, 1 << lg)
            self.ntt[lg] = (x, corc.ntt(CURVE, x), corc.ntt(CURVE, x, inverse=True))
            abc = [corc.rand_field(CURVE, "fr", s + 40 + 3 * lg + i, 1 << lg) for i in range(3)]
            self.h[lg] = (abc, corc.h_poly(CURVE, *abc), self._libsnark(min(lg, H_LIBSNARK_MAX_LOG), s + lg))
        fa, fb = corc.rand_field(CURVE, "fr", s + 90, 5000), corc.rand_field(CURVE, "fr", s + 91, 5000)
        self.field = (fa, fb, corc.field_op(CURVE, "fr", "mul", fa, fb))
        rsc = corc.rand_field(CURVE, "fr", s + 92, table_bases.shape[0], mont=False)
        self.resident = (rsc, corc.msm(CURVE, 1, table_bases, rsc))

    @staticmethod
    def _libsnark(lg, seed):
        import test_libsnark_model as M
        from oracle import corc
        from oracle.pyref.fields import FR
        from oracle.pyref.poly import Domain
        F = FR[CURVE]
        m = 1 << lg
        rng = random.Random(seed)
        a = [rng.randrange(F.p) for _ in range(m)]
        b = [rng.randrange(F.p) for _ in range(m)]
        c = [x * y % F.p for x, y in zip(a, b)]
        enc = lambda v: corc.field_op(CURVE, "fr", "to_mont", corc.ints_to_arr(v, 4))     # noqa: E731
        return [enc(a), enc(b), enc(c)], enc(M.libsnark_h(a, b, c, Domain(F, m)))

    def run(self, ctx, channel, table, rounds, barrier=None, limit=None):
        """`rounds` rounds of the mix in a seeded order.  Round r < len(logs) is the first use of size logs[r]: there every
        thread runs the calls of the new size first and in the same order, released together before the first transform
        (the twiddle set) and again before the first h-polynomial (the coset set); the rest of the round is shuffled."""
        rng = random.Random(77 + self.tid)
        done = 0
        sized = ["ntt", "intt", "h_circom", "h_libsnark"]
        for r in range(rounds):
            lg = self.logs[r % len(self.logs)]
            first = r < len(self.logs)
            ops = ["msm0", "msm1", "field", "resident"] + ([] if first else sized)
            rng.shuffle(ops)
            if first:
                ops = sized + ops
            for op in ops:
                if first and barrier is not None and op in ("ntt", "h_circom"):
                    barrier.wait(timeout=limit)
                if op in ("msm0", "msm1"):
                    bases, sc, want = self.msm[int(op[3])]
                    got = ctx.msm(CURVE, 1, bases, sc, affine=True, channel=channel)
                elif op == "ntt":
                    got, want = ctx.ntt(CURVE, self.ntt[lg][0], channel=channel), self.ntt[lg][1]
                elif op == "intt":
                    got, want = ctx.ntt(CURVE, self.ntt[lg][0], inverse=True, channel=channel), self.ntt[lg][2]
                elif op == "field":
                    got, want = ctx.field_op(CURVE, "fr", "mul", self.field[0], self.field[1], channel=channel), self.field[2]
                elif op == "resident":
                    got, want = ctx.msm_resident(table, self.resident[0], affine=True, channel=channel), self.resident[1]
                elif op == "h_circom":
                    got, want = ctx.h_poly(CURVE, *self.h[lg][0], channel=channel), self.h[lg][1]
                else:
                    abc, want = self.h[lg][2]
                    got = ctx.h_poly(CURVE, *abc, channel=channel, reduction="libsnark")
                if not np.array_equal(got, want):
                    raise AssertionError("thread %d, channel %d, round %d: %s differs from the oracle's (size 2^%d)"
                                         % (self.tid, channel, r, op, lg))
                done += 1
        return done


def _threads(name, jobs, limit):
    """Runs the jobs, one host thread each; a thread that is still alive after `limit` seconds ends the process."""
    errs, counts = [], []

    def wrap(fn):
        def go():
            try:
                counts.append(fn())
            except BaseException as e:       # noqa: BLE001 -- reported below, with the phase's name
                errs.append("%s: %r" % (name, e))
        return go

    ths = [threading.Thread(target=wrap(fn), daemon=True) for fn in jobs]
    t0 = time.monotonic()
    for t in ths:
        t.start()
    for t in ths:
        t.join(max(0.0, limit - (time.monotonic() - t0)))
    if any(t.is_alive() for t in ths):
        print("PHASE %s: DEADLOCK or stall: a thread is still running after %.1f s" % (name, limit), flush=True)
        os._exit(3)
    took = time.monotonic() - t0
    if errs:
        print("PHASE %s: FAILED: %s" % (name, "; ".join(errs)), flush=True)
    else:
        print("PHASE %s: ok, %d calls checked against the oracle in %.2f s" % (name, sum(counts), took), flush=True)
    return not errs


def child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import bench
    import dg16_amd
    from oracle import corc
    ctx = dg16_amd.Context(0)
    dev = torch.device("cuda", 0)
    table_bases = corc.gen_points(CURVE, 1, 600, 1 << 10)
    table = ctx.bases_upload(CURVE, 1, table_bases)
    timing = Mix(9, LOGS_TIMING, table_bases)
    mixes = [Mix(t, LOGS_THREADS, table_bases) for t in range(3)]
    mixes_p = [Mix(3 + t, LOGS_PROVER_PHASE, table_bases) for t in range(3)]
    mixes_c = [Mix(6 + t, LOGS_TWO_CONTEXTS, table_bases) for t in range(2)]
    wl = bench.Workload(ctx, dev, 10, 0, 1, seed=44, curve=CURVE)
    want_proof = bench.oracle_prove(wl, bench.cpu_threads())[0]
    timing.run(ctx, 0, table, len(LOGS_TIMING))                          # warm: workspaces of channel 0, every timing size
    t0 = time.monotonic()
    timing.run(ctx, 0, table, ROUNDS)
    single = time.monotonic() - t0
    limit = 10.0 * single
    print("single-threaded mix of %d rounds: %.2f s; limit of every threaded phase: %.1f s" % (ROUNDS, single, limit), flush=True)
    ok = True

    # (b) three host threads, one per channel
    barrier = threading.Barrier(3)
    ok &= _threads("three threads", [lambda t=t: mixes[t].run(ctx, t, table, ROUNDS, barrier, limit) for t in range(3)], limit)

    # (b), fourth phase: a prover thread (all three channels, taken in the order 0, 1, 2) beside three single-channel threads
    def prover():
        for i in range(5):
            got = bench.gpu_proof_affine(CURVE, bench.prove_once(ctx, wl))
            for nm, g, w in zip("ABC", got, want_proof):
                if not np.array_equal(g, w):
                    raise AssertionError("proof %d beside the single-channel threads: %s differs from the oracle's" % (i, nm))
        return 5

    barrier4 = threading.Barrier(3)
    ok &= _threads("prover beside three threads",
                   [lambda t=t: mixes_p[t].run(ctx, t, table, ROUNDS_SHORT, barrier4, limit) for t in range(3)] + [prover],
                   limit)

    # (c) two contexts on one device, a thread each
    others = [dg16_amd.Context(0) for _ in range(2)]
    tables = [o.bases_upload(CURVE, 1, table_bases) for o in others]
    barrier2 = threading.Barrier(2)
    ok &= _threads("two contexts",
                   [lambda t=t: mixes_c[t].run(others[t], t, tables[t], ROUNDS_SHORT, barrier2, limit) for t in range(2)],
                   limit)
    for tb in tables + [table]:
        tb.close()
    wl.pk.close()
    for o in others + [ctx]:
        o.close()
    print("CHILD DONE" if ok else "CHILD FAILED", flush=True)
    return 0 if ok else 1


_child = {}


def child_output():
    if "out" not in _child:
        _child["out"] = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True,
                                       timeout=600, cwd=ROOT)
        print(_child["out"].stdout)
    return _child["out"]


@pytest.mark.gpu
def test_three_threads_one_per_channel_and_a_prover_beside_them():
    out = child_output()
    text = out.stdout + out.stderr
    assert "single-threaded mix of" in text, text
    assert "PHASE three threads: ok" in text, text
    assert "PHASE prover beside three threads: ok" in text, text
    assert out.returncode == 0 and "CHILD DONE" in text, text


@pytest.mark.gpu
def test_two_contexts_on_one_device_a_thread_each():
    out = child_output()
    text = out.stdout + out.stderr
    assert "PHASE two contexts: ok" in text, text


if __name__ == "__main__":
    sys.exit(child())
