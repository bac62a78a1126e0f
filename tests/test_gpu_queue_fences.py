"""A queue of proofs without the end-of-proof join (DG16_F_OVERLAP_TAIL, prover_impl.h: "A queue of proofs").

In the queued form channel 0's stream no longer waits for the last proof's side streams: the next proof's R1CS x witness
and h-polynomial start right behind H's accumulation, and every buffer the side streams may still touch (r_s, the shared
digit sort, the bucket buffers of B and B1, the results record) is fenced at its first reuse.  The hazards are
write-after-read, so consecutive proofs here differ in EVERY input that lands in those buffers -- the assignment
(including an all-equal one: every scalar in one bucket per window, the giant-bucket path) and r, s (including
r = s = 0) -- and every queued proof is compared with the C oracle's proof of the same instance, never with another
GPU run."""

import random

import numpy as np
import pytest

from oracle import corc
from gpu_util import ctx

pytestmark = pytest.mark.gpu

CASES = [("bn254", 12), ("bn254", 16), ("bn254", 20), ("bls12_381", 16)]
K = 6
SEED_A, SEED_B = 31, 32

_oracle_cache = {}


def _instances(wl, dev, curve):
    """K assignments and K (r, s), all different: 1 = the all-equal assignment, 2 = r = s = 0."""
    import torch
    import bench
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000 + wl.log_m)
    rng = random.Random(7 * wl.log_m + len(curve))
    R = bench.FR_MOD[curve]
    ws, rss = [], []
    for k in range(K):
        w = bench.rand_fr(wl.nv, dev, gen, curve)
        if k == 1:
            w[:] = w[1].clone()
        w[0] = 0
        w[0, 0] = 1
        ws.append(w)
        r, s = (0, 0) if k == 2 else (rng.randrange(1, R), rng.randrange(1, R))
        rss.append((r, s, corc.ints_to_arr([r, s], 4)))
    return ws, rss


def _oracle(wl, seed, k, w, r, s):
    """The oracle's proof (A, B, C affine) of key `seed`, instance k; made once per session."""
    import bench
    key = (wl.curve, wl.log_m, seed, k)
    if key not in _oracle_cache:
        wl.w = w
        _oracle_cache[key] = bench.oracle_prove(wl, bench.cpu_threads(), r, s)[0]
    return _oracle_cache[key]


def _check(curve, out, want, what):
    import bench
    got = bench.gpu_proof_affine(curve, out.cpu().numpy())
    for name, g, e in zip("ABC", got, want):
        assert np.array_equal(g, e), "%s: %s differs from the oracle's" % (what, name)


def _queue(c, wls, ws, rss, outs, between=None):
    """K proofs back to back, proof k with key k mod len(wls); nothing on the host waits."""
    for k in range(K):
        wl = wls[k % len(wls)]
        wl.w = ws[k]
        wl.qap()
        c.prove_dev(wl.pk, wl.a.data_ptr(), wl.b.data_ptr(), wl.c.data_ptr(), wl.w.data_ptr(), rss[k][2],
                    outs[k].data_ptr(), scalars_mont=False, overlap_tail=True)
        if between is not None:
            between(k)
    for ch in range(3):
        c.sync(ch)


@pytest.mark.parametrize("curve,log_m", CASES)
def test_queued_proofs_equal_the_oracle(curve, log_m):
    import torch
    import bench
    c = ctx()
    dev = torch.device("cuda", 0)
    wl = bench.Workload(c, dev, log_m, 0, 1, seed=SEED_A, curve=curve)
    ws, rss = _instances(wl, dev, curve)
    outs = [torch.zeros(wl.proof_bytes(), dtype=torch.uint8, device=dev) for _ in range(K)]
    torch.cuda.synchronize()
    _queue(c, [wl], ws, rss, outs)
    for k in range(K):
        _check(curve, outs[k], _oracle(wl, SEED_A, k, ws[k], rss[k][0], rss[k][1]), "queued proof %d" % k)
    wl.pk.close()


@pytest.mark.parametrize("curve,log_m", CASES)
def test_queued_proofs_of_two_alternating_keys(curve, log_m):
    """Two resident keys of the same shape take turns on one context: the bucket buffers, the sort and the record are the
    context's, so key B's proof reuses what key A's side streams still read."""
    import torch
    import bench
    c = ctx()
    dev = torch.device("cuda", 0)
    wls = [bench.Workload(c, dev, log_m, 0, 1, seed=sd, curve=curve) for sd in (SEED_A, SEED_B)]
    ws, rss = _instances(wls[0], dev, curve)
    outs = [torch.zeros(wls[0].proof_bytes(), dtype=torch.uint8, device=dev) for _ in range(K)]
    torch.cuda.synchronize()
    _queue(c, wls, ws, rss, outs)
    for k in range(K):
        want = _oracle(wls[k % 2], (SEED_A, SEED_B)[k % 2], k, ws[k], rss[k][0], rss[k][1])
        _check(curve, outs[k], want, "queued proof %d (key %s)" % (k, "AB"[k % 2]))
    for wl in wls:
        wl.pk.close()


@pytest.mark.parametrize("curve,log_m", CASES)
def test_other_entry_points_between_queued_proofs(curve, log_m):
    """An MSM on channel 1 and an NTT on channel 0 between the proofs of the queue: both reuse workspace of their channel
    and order themselves behind the whole last proof in Call() (ctx.h); the proofs, the MSMs and the NTTs must all be the
    oracle's."""
    import torch
    import bench
    c = ctx()
    dev = torch.device("cuda", 0)
    wl = bench.Workload(c, dev, log_m, 0, 1, seed=SEED_A, curve=curve)
    ws, rss = _instances(wl, dev, curve)
    outs = [torch.zeros(wl.proof_bytes(), dtype=torch.uint8, device=dev) for _ in range(K)]
    fqb = bench.FQ_BYTES[curve]
    n_msm, log_ntt = 1 << 12, 12
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)
    bases = torch.empty(n_msm * 2 * fqb, dtype=torch.uint8, device=dev)
    c.gen_bases_dev(curve, 1, 78, n_msm, bases.data_ptr())
    c.sync(0)
    scs = [bench.rand_fr(n_msm, dev, gen, curve) for _ in range(K)]
    msm_outs = [torch.zeros(3 * fqb, dtype=torch.uint8, device=dev) for _ in range(K)]
    xs = [corc.rand_field(curve, "fr", 40 + k, 1 << log_ntt) for k in range(K)]
    ntt_bufs = [torch.from_numpy(x.view(np.int64).copy()).to(dev) for x in xs]
    torch.cuda.synchronize()

    def between(k):
        c.msm_dev(curve, 1, bases.data_ptr(), scs[k].data_ptr(), n_msm, msm_outs[k].data_ptr(), channel=1)
        c.ntt_dev(curve, ntt_bufs[k].data_ptr(), log_ntt, inverse=bool(k & 1), channel=0)

    _queue(c, [wl], ws, rss, outs, between)
    bases_h = bench.to_host_u64(bases, fqb // 4)
    nl = fqb // 8
    for k in range(K):
        _check(curve, outs[k], _oracle(wl, SEED_A, k, ws[k], rss[k][0], rss[k][1]), "queued proof %d" % k)
        want = corc.msm(curve, 1, bases_h, bench.to_host_u64(scs[k], 4))
        got = corc.jac_to_affine(curve, 1, msm_outs[k].cpu().numpy().view(np.uint64)[:3 * nl])
        assert np.array_equal(got, want), "the MSM behind queued proof %d" % k
        assert np.array_equal(ntt_bufs[k].cpu().numpy().view(np.uint64).reshape(-1, 4),
                              corc.ntt(curve, xs[k], inverse=bool(k & 1))), "the NTT behind queued proof %d" % k
    wl.pk.close()
