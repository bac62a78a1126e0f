#!/usr/bin/env python3
"""Times the batch verifier (dg16_groth16_verify_batch) next to what it is measured against, in ONE process:

  verify_batch   device pointers, n_public = 1, n_proofs in {1, 64, 1024, 16384}, both curves: the whole call between
                 the HIP events the library records on the channel's stream (dg16_last_kernel_ms), median of 3 after a
                 warm-up
  host_verify    the host verifier dg16_groth16_verify on BN254, single thread, mean of 10 calls
  prove_queued   dg16_groth16_prove at the headline size (2^20) per curve, proofs enqueued back to back on one context

    python3 tools/verify_timing.py [--out profiles/verify_timing.json] [--log-m 20]

The key and the proof are made from trapdoor scalars with the fixed-base kernels (A = a G1, B = b G2,
C = ((a b - alpha beta - gamma (u0 + x u1)) / delta) G1 satisfies the equation by construction); every timed batch is
checked to be accepted, and a batch with one input changed to be rejected at that index only.
"""

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

R = {"bn254": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
     "bls12_381": 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001}
SIZES = (1, 64, 1024, 16384)


def _scalars(vals):
    return np.stack([np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint64) for v in vals])


def instance(ctx, curve, seed=7):
    """(vk arrays, public input row, proof row) with n_public = 1."""
    import random
    r = R[curve]
    rng = random.Random(seed)
    al, be, ga, de, a, b, u0, u1, x = (rng.randrange(1, r) for _ in range(9))
    c = (a * b - al * be - ga * (u0 + x * u1)) * pow(de, r - 2, r) % r
    g1 = ctx.fixed_base_mul(curve, 1, _scalars([al, u0, u1, a, c]))
    g2 = ctx.fixed_base_mul(curve, 2, _scalars([be, ga, de, b]))
    vk = (g1[0], g2[0], g2[1], g2[2], g1[1:3])
    return vk, _scalars([x]), np.concatenate([g1[3], g2[3], g1[4]])


def time_verify(ctx, pvk, pub, proof, n, reps=3):
    import torch
    dev = torch.device("cuda", ctx.device)
    up = lambda arr: torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to(dev)     # noqa: E731
    xs = up(np.repeat(pub, n, axis=0))
    bad_at = n // 2
    xs_bad = xs.clone()
    xs_bad[bad_at, 0] ^= 1
    prs = up(np.repeat(proof[None, :], n, axis=0))
    torch.cuda.synchronize()
    want = np.ones(n, dtype=bool)
    assert np.array_equal(pvk.verify_batch(xs, prs, device=True, n_proofs=n), want)           # warm-up
    want[bad_at] = False
    assert np.array_equal(pvk.verify_batch(xs_bad, prs, device=True, n_proofs=n), want)
    ms = []
    for _ in range(reps):
        assert pvk.verify_batch(xs, prs, device=True, n_proofs=n).all()
        ms.append(ctx.last_kernel_ms(0, 0))
    return statistics.median(ms)


def time_host_verify(vk, pub, proof, calls):
    from dg16_amd import verify
    assert verify.verify_proof(*vk, pub, proof)
    t0 = time.perf_counter()
    for _ in range(calls):
        verify.verify_proof(*vk, pub, proof)
    return (time.perf_counter() - t0) / calls


def time_prove_queued(ctx, curve, log_m, steps=8):
    import torch
    import bench
    dev = torch.device("cuda", ctx.device)
    wl = bench.Workload(ctx, dev, log_m, 0, 1, seed=21, curve=curve)
    proofs = torch.empty((steps, wl.proof_bytes()), dtype=torch.uint8, device=dev)

    def queue(k):
        for i in range(k):
            wl.qap()
            ctx.prove_dev(wl.pk, wl.a.data_ptr(), wl.b.data_ptr(), wl.c.data_ptr(), wl.w.data_ptr(), wl.rs,
                          proofs[i].data_ptr(), scalars_mont=False)
        for ch in range(3):
            ctx.sync(ch)

    queue(2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    queue(steps)
    dt = (time.perf_counter() - t0) / steps
    wl.pk.close()
    del wl
    torch.cuda.empty_cache()
    return dt


def measure(ctx, sizes=SIZES, prover_log_m=20, host_calls=10):
    from dg16_amd import verify
    res = {}
    for curve in ("bn254", "bls12_381"):
        vk, pub, proof = instance(ctx, curve)
        pvk = verify.PreparedVerifyingKey(ctx, curve, *vk)
        out = {"verify_batch": {}}
        for n in sizes:
            ms = time_verify(ctx, pvk, pub, proof, n)
            out["verify_batch"][str(n)] = {"ms": ms, "proofs_per_s": n / (ms * 1e-3)}
        pvk.close()
        if curve == "bn254":
            s = time_host_verify(vk, pub, proof, host_calls)
            out["host_verify"] = {"ms": s * 1e3, "proofs_per_s": 1.0 / s, "calls": host_calls, "threads": 1}
        s = time_prove_queued(ctx, curve, prover_log_m)
        out["prove_queued"] = {"log_m": prover_log_m, "ms": s * 1e3, "proofs_per_s": 1.0 / s}
        res[curve] = out
    return res


def table(res):
    lines = ["| curve | n_proofs | batch ms | verified / s | prover / s (2^%d) | host verifier / s (1 thread) |" %
             res["bn254"]["prove_queued"]["log_m"], "|---|---|---|---|---|---|"]
    for curve, out in res.items():
        host = "%.1f" % out["host_verify"]["proofs_per_s"] if "host_verify" in out else "-"
        for n, v in out["verify_batch"].items():
            lines.append("| %s | %s | %.2f | %.0f | %.1f | %s |" % (curve, n, v["ms"], v["proofs_per_s"],
                                                                   out["prove_queued"]["proofs_per_s"], host))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_timing.json"))
    ap.add_argument("--log-m", type=int, default=20)
    args = ap.parse_args()
    import dg16_amd
    ctx = dg16_amd.Context(0)
    res = measure(ctx, prover_log_m=args.log_m)
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
