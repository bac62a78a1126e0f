"""Helpers of tests/test_gpu_prover_bls12_377.py: BLS12-377 instances for the resident prover, and the proof they must
give -- assembled from the C oracle (corc.qap, corc.h_poly, corc.msm, corc.point_mul, corc.point_add) over the same key
arrays, never from the library.  bench.Workload knows two curves, so the instances are built here.

Planner thresholds of this curve (csrc/msm_geom.h; 253-bit scalars, 254 digit bits), at or under 2^14 points:
  * msm_window_bits: a table of fewer than 2^13 points (n <= 6144: "nearest power of two" below 2^13) takes the window
    log2(n) + 1, from there to 2^16 points 15 bits (15 and 16 leave the same 14-bit top window);
  * msm_partition_plan: the digit sort takes the LDS-partitioned passes from nwin * n >= 2^18 entries, i.e. with the
    17 windows of c = 15 from n = 15 421 points; below that the direct atomic path.
The others lie above 2^14: 16-bit windows past 2^16 points, the three separate A / B1 / L launches past rows * n = 2^22
entries, longer accumulation segments past nwin * n = 2^22."""

import numpy as np

from oracle import corc
from oracle.pyref.fields import FQ, FR

CURVE = "bls12_377"
F, Fq = FR[CURVE], FQ[CURVE]
NL = Fq.limbs64                       # 64-bit limbs of a base-field element
FR_TOP = F.p >> 192                   # top 64-bit limb of the scalar modulus
WINDOW_15_FROM = 6145                 # points: msm_window_bits
PARTITIONED_FROM = 15421              # points, at c = 15 (17 windows): msm_partition_plan


def fr_int(limbs):
    return int(sum(int(x) << (64 * i) for i, x in enumerate(limbs)))


def fr_arr(vals):
    return corc.ints_to_arr([v % F.p for v in vals], 4)


def rand_fr(rng, n):
    """Uniform limbs with the top limb below the modulus': canonical scalars (and valid Montgomery forms)."""
    out = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    out[:, 3] = rng.integers(0, FR_TOP, size=n, dtype=np.uint64)
    return out


def affine(A, B, C):
    """Jacobian (A, B, C) -> one array of the three affine points, converted by the oracle."""
    return np.concatenate([np.asarray(corc.jac_to_affine(CURVE, g, P)).reshape(-1) for g, P in ((1, A), (2, B), (1, C))])


def affine_of_bytes(proof):
    j = np.ascontiguousarray(proof).view(np.uint64).reshape(-1)
    return affine(j[:3 * NL], j[3 * NL:9 * NL], j[9 * NL:])


def scalars_times_generators(sa, sb, sc):
    return np.concatenate([np.asarray(corc.point_mul(CURVE, g, corc.generator(CURVE, g), k)).reshape(-1)
                           for g, k in ((1, sa), (2, sb), (1, sc))])


def oracle_proof(key, ni, a, b, c, w, r, s):
    """prove.rs:21-136 with the oracle's arithmetic.  key: a_query, b_g1_query, b_g2_query, h_query, l_query as uint64
    [points][limbs] and fixed_points = alpha_g1 | beta_g1 | delta_g1 | beta_g2 | delta_g2 (flat); a, b, c Montgomery, w
    canonical."""
    add = lambda g, P, Q: corc.point_add(CURVE, g, P, Q)            # noqa: E731
    mul = lambda g, P, k: corc.point_mul(CURVE, g, P, k % F.p)      # noqa: E731
    msm = lambda g, bases, sc: corc.msm(CURVE, g, bases, sc)        # noqa: E731
    f = np.asarray(key["fixed_points"]).reshape(-1)
    alpha, beta1, delta1 = (f[2 * NL * i:2 * NL * (i + 1)].reshape(1, -1) for i in range(3))
    beta2, delta2 = (f[6 * NL + 4 * NL * i:6 * NL + 4 * NL * (i + 1)].reshape(1, -1) for i in range(2))
    h = corc.field_op(CURVE, "fr", "from_mont", corc.h_poly(CURVE, a, b, c))
    aq, b1q, b2q = key["a_query"], key["b_g1_query"], key["b_g2_query"]
    A = add(1, add(1, msm(1, aq[1:], w[1:]), aq[0:1]), add(1, alpha, mul(1, delta1, r)))
    B1 = add(1, add(1, msm(1, b1q[1:], w[1:]), b1q[0:1]), add(1, beta1, mul(1, delta1, s)))
    B = add(2, add(2, msm(2, b2q[1:], w[1:]), b2q[0:1]), add(2, beta2, mul(2, delta2, s)))
    C = add(1, msm(1, key["l_query"], w[ni:]), msm(1, key["h_query"], h))
    C = add(1, add(1, C, mul(1, A, s)), add(1, mul(1, B1, r), mul(1, delta1, -(r * s))))
    return np.concatenate([np.asarray(P).reshape(-1) for P in (A, B, C)])


class Instance:
    """A synthetic key (random points of the subgroups, as PackedProvingKeyShare::rand makes one) and a synthetic R1CS with
    three non-zeros per row of A and B over nv wires: what the prover computes does not depend on the system being
    satisfied (qap.rs:44-91 sets c = a o b).  Everything on the host; keys are made resident by the caller."""

    def __init__(self, ctx, log_m, nv=None, ni=2, seed=31):
        self.log_m, self.m, self.ni = log_m, 1 << log_m, ni
        self.nv = self.m if nv is None else nv
        self.nc = self.m - ni
        m, nv, nc = self.m, self.nv, self.nc
        gen = lambda g, s, n: ctx.gen_bases(CURVE, g, 100 * seed + s, n)      # noqa: E731
        self.key = dict(a_query=gen(1, 1, nv), b_g1_query=gen(1, 2, nv), b_g2_query=gen(2, 3, nv), h_query=gen(1, 4, m),
                        l_query=gen(1, 5, nv - ni),
                        fixed_points=np.concatenate([gen(1, 6, 3).reshape(-1), gen(2, 7, 2).reshape(-1)]))
        rng = np.random.default_rng([seed, log_m, nv])
        ptr = (np.arange(nc + 1, dtype=np.uint64) * 3).astype(np.uint32)
        self.csr_a = (ptr, rng.integers(0, nv, 3 * nc).astype(np.uint32), rand_fr(rng, 3 * nc))
        self.csr_b = (ptr, rng.integers(0, nv, 3 * nc).astype(np.uint32), rand_fr(rng, 3 * nc))
        self.rng = rng

    def dense_witness(self):
        w = rand_fr(self.rng, self.nv)
        w[0] = (1, 0, 0, 0)
        return w

    def abc(self, w):
        """The oracle's a, b, c (Montgomery) of the canonical assignment w."""
        return corc.qap(CURVE, self.nc, self.ni, self.m, self.csr_a, self.csr_b, corc.field_op(CURVE, "fr", "to_mont", w))

    def pk(self, ctx, **kw):
        k = self.key
        return ctx.pk_create(CURVE, self.nv, self.ni, self.m, k["a_query"], k["b_g1_query"], k["b_g2_query"], k["h_query"],
                             k["l_query"], k["fixed_points"], **kw)

    def expected(self, abc, w, r, s):
        return oracle_proof(self.key, self.ni, abc[0], abc[1], abc[2], w, r, s)


def arrays_of_bigint_key(pk):
    """The oracle's big-integer key (oracle.pyref.groth16.setup) as the arrays dg16_pk_create takes."""
    from test_gpu_prover import enc_g1, enc_g2
    fixed = np.concatenate([enc_g1(Fq, [pk["alpha_g1"], pk["beta_g1"], pk["delta_g1"]]).reshape(-1),
                            enc_g2(Fq, [pk["beta_g2"], pk["delta_g2"]]).reshape(-1)])
    return (enc_g1(Fq, pk["a_query"]), enc_g1(Fq, pk["b_g1_query"]), enc_g2(Fq, pk["b_g2_query"]),
            enc_g1(Fq, pk["h_query"]), enc_g1(Fq, pk["l_query"]), fixed)


def queue_case(ctx):
    """Three witnesses and the first again through one context with DG16_F_OVERLAP_TAIL and device pointers at m = 2^12, a
    BN254 proof (bench.Workload) in the middle: the persistent events and the workspace slots are shared across curves.
    Every queued proof must equal the proof of the same inputs made one at a time (affine points: the queued form reduces
    H's buckets with another kernel shape), and the first one-at-a-time proof the oracle's.  Raises AssertionError."""
    import torch
    import bench
    dev = torch.device("cuda", 0)
    inst = Instance(ctx, 12, seed=88)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).to(dev)      # noqa: E731
    ws_ = [inst.dense_witness() for _ in range(3)]
    ws_[1][1:inst.nv // 2, 1:] = 0                 # half of the second witness: 64-bit values
    order = [0, 1, None, 2, 0]                     # None: the BN254 proof
    wl = bench.Workload(ctx, dev, 12, seed=31, curve="bn254")
    pk = inst.pk(ctx)
    try:
        jobs = []
        for i, k in enumerate(order):
            if k is None:
                wl.qap()
                ctx.sync(0)
                jobs.append((wl.pk, wl.w, [wl.a, wl.b, wl.c], wl.rs, wl.proof_bytes()))
                continue
            abc = inst.abc(ws_[k])
            rs = rand_fr(np.random.default_rng([88, k]), 2)
            jobs.append((pk, up(ws_[k]), [up(v) for v in abc], rs, 12 * 8 * NL))
            if i == 0:
                first = (abc, ws_[k], rs)

        def run(overlap):
            outs = [torch.zeros(nb, dtype=torch.uint8, device=dev) for *_, nb in jobs]
            torch.cuda.synchronize()
            for (key, wd, abc, rs, _), out in zip(jobs, outs):
                ctx.prove_dev(key, abc[0].data_ptr(), abc[1].data_ptr(), abc[2].data_ptr(), wd.data_ptr(), rs,
                              out.data_ptr(), scalars_mont=False, overlap_tail=overlap)
                if not overlap:
                    for ch in range(3):
                        ctx.sync(ch)
            for ch in range(3):
                ctx.sync(ch)
            res = []
            for k, out in zip(order, outs):
                o = out.cpu().numpy()
                res.append(np.concatenate([np.asarray(x).reshape(-1) for x in bench.gpu_proof_affine("bn254", o)])
                           if k is None else affine_of_bytes(o))
            return res

        one_at_a_time = run(False)
        queued = run(True)
        again = run(True)
        for i, (x, y, z) in enumerate(zip(one_at_a_time, queued, again)):
            assert x.any() and np.array_equal(x, y) and np.array_equal(x, z), "queued proof %d" % i
        assert np.array_equal(one_at_a_time[0], one_at_a_time[4])
        assert not np.array_equal(one_at_a_time[0], one_at_a_time[1])
        abc, w, rs = first
        assert np.array_equal(one_at_a_time[0], inst.expected(abc, w, fr_int(rs[0]), fr_int(rs[1])))
    finally:
        pk.close()
        wl.pk.close()

