#!/usr/bin/env python3
"""Times the aggregate verifier (dg16_groth16_verify_aggregate: one verdict per batch) against the batch verifier
(dg16_groth16_verify_batch: one verdict per proof) on the SAME inputs, in ONE process, the two calls interleaved so that
they share the clock state:

  both curves x n_proofs in {1, 1024, 65536, 262144} at n_public = 1, and n_proofs = 1024 at n_public = 40; device
  pointers; the whole call between the HIP events the library records on the channel's stream (dg16_last_kernel_ms);
  median of 3 after a warm-up of each call.

    python3 tools/verify_aggregate_timing.py [--out profiles/verify_aggregate_timing.json]

The key and the proof are made from trapdoor scalars with the fixed-base kernels (tools/verify_timing.py does the same
for n_public = 1): A = a G1, B = b G2, C = ((a b - alpha beta - gamma (u_0 + sum_j x_j u_j)) / delta) G1.  Every timed
batch is checked to be accepted by both calls, and a batch with one input changed to be rejected by the aggregate call
and at that index only by the batch call.
"""

import argparse
import ctypes
import json
import os
import random
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

R = {"bn254": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
     "bls12_381": 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001}
GRID = ((1, 1), (1024, 1), (65536, 1), (262144, 1), (1024, 40))     # (n_proofs, n_public)


def _scalars(vals):
    return np.stack([np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint64) for v in vals])


def instance(ctx, curve, n_public, seed=7):
    """(vk arrays, public input row [n_public][4], proof row)."""
    r = R[curve]
    rng = random.Random(seed + n_public)
    al, be, ga, de, a, b = (rng.randrange(1, r) for _ in range(6))
    u = [rng.randrange(1, r) for _ in range(n_public + 1)]
    x = [rng.randrange(r) for _ in range(n_public)]
    acc = (u[0] + sum(xi * ui for xi, ui in zip(x, u[1:]))) % r
    c = (a * b - al * be - ga * acc) * pow(de, r - 2, r) % r
    g1 = ctx.fixed_base_mul(curve, 1, _scalars([al, a, c] + u))
    g2 = ctx.fixed_base_mul(curve, 2, _scalars([be, ga, de, b]))
    vk = (g1[0], g2[0], g2[1], g2[2], g1[3:])
    return vk, _scalars(x) if n_public else np.zeros((0, 4), dtype=np.uint64), np.concatenate([g1[1], g2[3], g1[2]])


def coefficients(n, seed=11):
    """n nonzero 128-bit coefficients, n x 2 uint64 (seeded: a timing run needs no secrecy)."""
    c = np.random.default_rng(seed).integers(0, 1 << 63, size=(n, 2), dtype=np.uint64, endpoint=False)
    c[:, 0] |= np.uint64(1)
    return c


def time_point(ctx, pvk, pub, proof, n, reps=3):
    """(aggregate ms, batch ms), each the median of `reps` calls taken alternately."""
    import torch
    dev = torch.device("cuda", ctx.device)
    up = lambda arr: torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to(dev)     # noqa: E731
    n_public = pub.shape[0]
    xs = up(np.repeat(pub[None, :, :], n, axis=0).reshape(n, -1)) if n_public else torch.zeros(1, dtype=torch.int64,
                                                                                               device=dev)
    prs = up(np.repeat(proof[None, :], n, axis=0))
    rho = up(coefficients(n))
    torch.cuda.synchronize()
    agg = lambda x: pvk.verify_aggregate(x, prs, coeffs=rho, device=True, n_proofs=n)        # noqa: E731
    bat = lambda x: pvk.verify_batch(x, prs, device=True, n_proofs=n)                        # noqa: E731
    assert agg(xs) is True and bat(xs).all()                                                 # warm-up of both
    if n_public:
        bad_at = n // 2
        xs_bad = xs.clone()
        xs_bad[bad_at, 0] ^= 1
        want = np.ones(n, dtype=bool)
        want[bad_at] = False
        assert agg(xs_bad) is False and np.array_equal(bat(xs_bad), want)
    ms_a, ms_b = [], []
    for _ in range(reps):
        assert agg(xs) is True
        ms_a.append(ctx.last_kernel_ms(0, 0))
        assert bat(xs).all()
        ms_b.append(ctx.last_kernel_ms(0, 0))
    return statistics.median(ms_a), statistics.median(ms_b)


def measure(ctx, grid=GRID, curves=("bn254", "bls12_381")):
    from dg16_amd import verify
    res = {}
    for curve in curves:
        keys = {}
        points = []
        for n, n_public in grid:
            if n_public not in keys:
                vk, pub, proof = instance(ctx, curve, n_public)
                keys[n_public] = (verify.PreparedVerifyingKey(ctx, curve, *vk), pub, proof)
            pvk, pub, proof = keys[n_public]
            a, b = time_point(ctx, pvk, pub, proof, n)
            points.append({"n_proofs": n, "n_public": n_public, "aggregate_ms": a, "batch_ms": b, "ratio": a / b})
        for pvk, _, _ in keys.values():
            pvk.close()
        res[curve] = {"points": points}
    return res


def table(res):
    lines = ["| curve | n_proofs | n_public | aggregate ms | batch ms | aggregate / batch |", "|---|---|---|---|---|---|"]
    for curve, out in res.items():
        for p in out["points"]:
            lines.append("| %s | %d | %d | %.2f | %.2f | %.3f |" % (curve, p["n_proofs"], p["n_public"],
                                                                  p["aggregate_ms"], p["batch_ms"], p["ratio"]))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_aggregate_timing.json"))
    args = ap.parse_args()
    import dg16_amd
    ctx = dg16_amd.Context(0)
    res = measure(ctx)
    name = ctypes.create_string_buffer(128)
    cus = ctypes.c_int(0)
    ctx.L.dg16_device_info(ctx.h, name, 128, ctypes.byref(cus))
    res["device"] = {"name": name.value.decode(), "compute_units": cus.value}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(table({k: v for k, v in res.items() if k != "device"}))


if __name__ == "__main__":
    main()
