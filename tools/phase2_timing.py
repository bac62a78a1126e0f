#!/usr/bin/env python3
"""Times phase 2 of the key ceremony: the one-scalar point multiplication (dg16_points_scale) against the call it
replaces for that job, dg16_points_mul with the scalar replicated, and the two calls built on it.

  scale        n in {2^16, 2^20} for the six groups, in_subgroup 0 and 1: dg16_points_scale and dg16_points_mul on the
               SAME host points, alternating in one process.  Both calls take host arrays here (dg16_points_scale takes
               nothing else), so both figures include their copies; in brackets the time between the HIP events the
               library records around the kernels of the call (dg16_last_kernel_ms, which = 1).
  key          dg16_groth16_contribute and dg16_groth16_verify_contribution on BN254 and BLS12-381 for the arrays of a
               2^16- and a 2^20-constraint system (num_vars = 2^k + 1, one input, domain 2^k).  The points are
               dg16_gen_bases output -- neither call's cost depends on which subgroup points a key holds -- and `after`
               is `before` through dg16_groth16_contribute, so the verifier runs all its stages and accepts.

A synchronised host clock around the synchronous calls; median of 3 after one warm-up call.  Every step is a child
process under its own time limit, and the first failure stops the run:

    python3 tools/phase2_timing.py [--out profiles/phase2_timing.json]
"""

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GROUPS = (("bn254", 1), ("bn254", 2), ("bls12_381", 1), ("bls12_381", 2), ("bls12_377", 1), ("bls12_377", 2))
SIZES = (1 << 16, 1 << 20)
KEY_CURVES = ("bn254", "bls12_381")
KEY_LOGS = (16, 20)
SCALAR = 0x0a3c5e7f1b2d4c6e8f9a0b1c2d3e4f5a6b7c8d9e0f1a2b3c4d5e6f708192a3b4      # below r on all three curves
STEP_LIMIT_S = {"scale": 300, "key": 420}


def _timed(ctx, call, which):
    t0 = time.perf_counter()
    call()
    t1 = time.perf_counter()
    return 1e3 * (t1 - t0), ctx.last_kernel_ms(0, which)


def step_scale(ctx, curve, group):
    out = []
    for n in SIZES:
        pts = ctx.gen_bases(curve, group, 17, n)
        ks = np.ascontiguousarray(np.tile(np.frombuffer(SCALAR.to_bytes(32, "little"), dtype=np.uint64), (n, 1)))
        res = np.zeros_like(pts)
        row = {"n": n}
        for flag in (False, True):
            scale = lambda: ctx.points_scale(curve, group, pts, SCALAR, in_subgroup=flag, out=res)      # noqa: E731
            mul = lambda: ctx.points_mul(curve, group, pts, ks, in_subgroup=flag)                       # noqa: E731
            ref = mul()                                                                                 # warm-up
            scale()
            assert np.array_equal(res, ref), "dg16_points_scale differs from dg16_points_mul"
            del ref
            ts, tm = [], []
            for _ in range(3):
                ts.append(_timed(ctx, scale, 1))
                tm.append(_timed(ctx, mul, 1))
            tag = "subgroup" if flag else "plain"
            row[tag] = {"scale_ms": statistics.median(t[0] for t in ts), "scale_kernels_ms": statistics.median(t[1] for t in ts),
                        "mul_ms": statistics.median(t[0] for t in tm), "mul_kernels_ms": statistics.median(t[1] for t in tm)}
        out.append(row)
        del pts, ks, res
    return out


def step_key(ctx, curve, log_n):
    from dg16_amd.verify import random_coefficients
    n = 1 << log_n
    nv, ni = n + 1, 1
    g1 = lambda seed, count: ctx.gen_bases(curve, 1, seed, count)      # noqa: E731
    fixed = np.concatenate([g1(31, 3).reshape(-1), ctx.gen_bases(curve, 2, 32, 2).reshape(-1)])
    before = [g1(33, nv), g1(34, nv), ctx.gen_bases(curve, 2, 35, nv), g1(36, n), g1(37, nv - ni), fixed,
              ctx.gen_bases(curve, 2, 38, 1), g1(39, ni)]
    delta = SCALAR
    contribute = lambda: ctx.groth16_contribute(curve, before[4], before[3], fixed, delta)      # noqa: E731
    l, h, f = contribute()                                                                     # warm-up
    t_c = [_timed(ctx, contribute, 0)[0] for _ in range(3)]
    after = list(before)
    after[3], after[4], after[5] = h, l, f
    coeffs = random_coefficients(n)
    verify = lambda: ctx.groth16_verify_contribution(curve, ni, nv, n, before, after, coeffs)   # noqa: E731
    assert verify() == (0, 0, 0, 0), "the contributed key was rejected"
    t_v = [_timed(ctx, verify, 0)[0] for _ in range(3)]
    return {"log_n": log_n, "points_scaled": 2 * n + 2, "contribute_ms": statistics.median(t_c),
            "verify_contribution_ms": statistics.median(t_v)}


def run_step(name):
    import dg16_amd
    ctx = dg16_amd.Context(0)
    kind, _, arg = name.partition(":")
    if kind == "scale":
        curve, group = arg.rsplit("_g", 1)
        res = step_scale(ctx, curve, int(group))
    elif kind == "key":
        curve, log_n = arg.rsplit("_", 1)
        res = step_key(ctx, curve, int(log_n))
    else:
        name_buf = ctypes.create_string_buffer(128)
        cus = ctypes.c_int(0)
        ctx.L.dg16_device_info(ctx.h, name_buf, 128, ctypes.byref(cus))
        res = {"name": name_buf.value.decode(), "compute_units": cus.value}
    print("RESULT " + json.dumps(res))


def table(res):
    lines = ["| group | n | in_subgroup | `dg16_points_scale` ms (kernels) | `dg16_points_mul` ms (kernels) | ratio (kernels) |",
             "|---|---|---|---|---|---|"]
    for key, rows in res.get("scale", {}).items():
        for p in rows:
            for tag in ("plain", "subgroup"):
                t = p[tag]
                lines.append("| %s | 2^%d | %d | %.2f (%.2f) | %.2f (%.2f) | %.2f (%.2f) |" % (
                    key, p["n"].bit_length() - 1, tag == "subgroup", t["scale_ms"], t["scale_kernels_ms"], t["mul_ms"],
                    t["mul_kernels_ms"], t["scale_ms"] / t["mul_ms"], t["scale_kernels_ms"] / t["mul_kernels_ms"]))
    lines += ["", "| curve | constraints | `contribute` ms | `verify_contribution` ms |", "|---|---|---|---|"]
    for key, p in res.get("key", {}).items():
        lines.append("| %s | 2^%d | %.1f | %.1f |" % (key.rsplit("_", 1)[0], p["log_n"], p["contribute_ms"],
                                                     p["verify_contribution_ms"]))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phase2_timing.json"))
    ap.add_argument("--step", help="(internal) run one step in this process")
    args = ap.parse_args()
    if args.step:
        run_step(args.step)
        return
    steps = ["device"] + ["scale:%s_g%d" % g for g in GROUPS] + ["key:%s_%d" % (c, k) for c in KEY_CURVES for k in KEY_LOGS]
    res = {"scale": {}, "key": {}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for step in steps:
        limit = STEP_LIMIT_S.get(step.partition(":")[0], 60)
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], capture_output=True, text=True,
                               timeout=limit)
        except subprocess.TimeoutExpired:
            print("step %s exceeded %d s: stopping" % (step, limit), flush=True)
            sys.exit(124)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print("step %s failed (status %d): stopping\n%s\n%s" % (step, p.returncode, p.stdout[-2000:], p.stderr[-4000:]),
                  flush=True)
            sys.exit(1)
        val = json.loads(line[-1][7:])
        kind, _, arg = step.partition(":")
        if arg:
            res[kind][arg] = val
        else:
            res[kind] = val
        print("step %s done" % step, flush=True)
        with open(args.out + ".partial", "w") as f:
            json.dump(res, f)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    os.remove(args.out + ".partial")
    print(table(res))


if __name__ == "__main__":
    main()
