#!/usr/bin/env python3
"""Times phase 1 of the key ceremony: a contribution to a powers-of-tau transcript (dg16_srs_contribute) and its
verification (dg16_srs_verify_contribution), beside the path a user had before them.

  series       BN254 G1, 2^14 points: dg16_points_mul_series against dg16_points_mul on scalars prepared beforehand, the
               two alternating five times in one process -- the workload and the figures (ratio of the medians, max / min
               of dg16_points_mul's repeats) of the timing assertion in tests/test_gpu_points_series.py.
  phase1       m in {2^16, 2^20} on BN254 and BLS12-381, the transcript of a known trapdoor (powers_from_trapdoor):
                 contribute_ms            keygen.contribute_powers with a key, host arrays in and out
                 verify_ms                keygen.verify_powers_contribution (accepts)
                 by_hand_scalars_ms       the 5m - 1 scalars c t^j mod r made in a Python loop and packed
                 by_hand_points_mul_ms    four dg16_points_mul calls on them (tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1)
               and the four arrays of the two paths are compared byte for byte.

A synchronised host clock around the synchronous calls, copies included; median of 3 after one warm-up call (the
Python loop is timed once).  NOT timed: the kernels apart from their copies.  Every step is a child process under its
own time limit, and the first failure stops the run:

    python3 tools/phase1_timing.py [--out profiles/phase1_timing.json]
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

CURVES = ("bn254", "bls12_381")
LOGS = (16, 20)
# below r on all three curves
SECRETS = {"before": (0x0a3c5e7f1b2d4c6e8f9a0b1c2d3e4f5a6b7c8d9e0f1a2b3c4d5e6f708192a3b4,
                      0x0123456789abcdef0fedcba9876543210123456789abcdef0fedcba987654321,
                      0x0b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfe),
           "mine": (0x09e3779b97f4a7c15f39cc0605cedc8341082276bf3a27251f86c6ea9b5c1d2e,
                    0x0243f6a8885a308d313198a2e03707344a4093822299f31d0082efa98ec4e6c8,
                    0x0452821e638d01377be5466cf34e90c6cc0ac29b7c97c50dd3f84d5b5b547091)}
BLINDS = (0x05a827999fcef32422e7ecd6a1d6f3c1b0d9e8f7a6b5c4d3e2f1a0b9c8d7e6f5, 0x06ed9eba1fcef32422e7ecd6a1d6f3c1b0d9e8f7a6b5c4d3e2f1a0b9c8d7e6f5,
          0x08f1bbcdcfcef32422e7ecd6a1d6f3c1b0d9e8f7a6b5c4d3e2f1a0b9c8d7e6f5)
STEP_LIMIT_S = {"series": 120, "phase1": 560}


def _ms(call):
    t0 = time.perf_counter()
    out = call()
    return 1e3 * (time.perf_counter() - t0), out


def _pack(vals):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def step_series(ctx):
    from dg16_amd.keygen import FR_MODULUS
    curve, group, n = "bn254", 1, 1 << 14
    r = FR_MODULUS[curve]
    first, ratio = SECRETS["mine"][1] % r, SECRETS["mine"][0] % r
    pts = ctx.gen_bases(curve, group, 5, n)
    ks, v = [], first
    for _ in range(n):
        ks.append(v)
        v = v * ratio % r
    ks = _pack(ks)
    ref = ctx.points_mul(curve, group, pts, ks, in_subgroup=True)
    assert np.array_equal(ctx.points_mul_series(curve, group, pts, first, ratio, in_subgroup=True), ref)
    ts, tm = [], []
    for _ in range(5):
        ts.append(_ms(lambda: ctx.points_mul_series(curve, group, pts, first, ratio, in_subgroup=True))[0])
        tm.append(_ms(lambda: ctx.points_mul(curve, group, pts, ks, in_subgroup=True))[0])
    return {"n": n, "series_ms": statistics.median(ts), "points_mul_ms": statistics.median(tm),
            "ratio": statistics.median(ts) / statistics.median(tm), "points_mul_spread": max(tm) / min(tm)}


def step_phase1(ctx, curve, log_m):
    from dg16_amd import keygen
    r = keygen.FR_MODULUS[curve]
    m = 1 << log_m
    a0, b0, t0 = (x % r for x in SECRETS["before"])
    a, b, t = (x % r for x in SECRETS["mine"])
    before = keygen.powers_from_trapdoor(ctx, curve, log_m, a0, b0, t0)
    sp = ctx.gen_bases(curve, 2, 77, 3)
    contribute = lambda: keygen.contribute_powers(ctx, curve, log_m, before, t, a, b, blinds=[x % r for x in BLINDS],   # noqa: E731
                                                  challenge=sp)
    after, key = contribute()                                                              # warm-up
    t_c = [_ms(contribute)[0] for _ in range(3)]
    verify = lambda: keygen.verify_powers_contribution(ctx, curve, log_m, before, after, key, sp)      # noqa: E731
    assert verify().accepted, "the contribution was rejected"
    t_v = [_ms(verify)[0] for _ in range(3)]

    def scalars():
        pw, v = [], 1
        for _ in range(2 * m - 1):
            pw.append(v)
            v = v * t % r
        return (_pack(pw), _pack(pw[:m]), _pack([a * x % r for x in pw[:m]]), _pack([b * x % r for x in pw[:m]]))

    t_s, ks = _ms(scalars)
    by_hand = lambda: [ctx.points_mul(curve, g, p, k, in_subgroup=True)                    # noqa: E731
                       for g, p, k in zip((1, 2, 1, 1), before[:4], ks)]
    hand = by_hand()                                                                       # warm-up
    for name, x, y in zip(("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1"), after, hand):
        assert np.array_equal(x, y), "%s differs between the two paths" % name
    t_h = [_ms(by_hand)[0] for _ in range(3)]
    return {"log_m": log_m, "points": 5 * m, "contribute_ms": statistics.median(t_c), "verify_ms": statistics.median(t_v),
            "by_hand_scalars_ms": t_s, "by_hand_points_mul_ms": statistics.median(t_h)}


def run_step(name):
    import dg16_amd
    ctx = dg16_amd.Context(0)
    kind, _, arg = name.partition(":")
    if kind == "series":
        res = step_series(ctx)
    elif kind == "phase1":
        curve, log_m = arg.rsplit("_", 1)
        res = step_phase1(ctx, curve, int(log_m))
    else:
        name_buf = ctypes.create_string_buffer(128)
        cus = ctypes.c_int(0)
        ctx.L.dg16_device_info(ctx.h, name_buf, 128, ctypes.byref(cus))
        res = {"name": name_buf.value.decode(), "compute_units": cus.value}
    print("RESULT " + json.dumps(res))


def table(res):
    s = res.get("series", {})
    lines = []
    if s:
        lines += ["series, BN254 G1, 2^14: %.3f ms against %.3f ms, ratio %.3f, spread of dg16_points_mul %.3f"
                  % (s["series_ms"], s["points_mul_ms"], s["ratio"], s["points_mul_spread"]), ""]
    lines += ["| curve | m | `contribute_powers` ms | `verify_powers_contribution` ms | by hand: Python scalars ms | "
              "by hand: four `dg16_points_mul` ms |", "|---|---|---|---|---|---|"]
    for key, p in res.get("phase1", {}).items():
        lines.append("| %s | 2^%d | %.1f | %.1f | %.0f | %.1f |" % (key.rsplit("_", 1)[0], p["log_m"], p["contribute_ms"],
                                                                   p["verify_ms"], p["by_hand_scalars_ms"],
                                                                   p["by_hand_points_mul_ms"]))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phase1_timing.json"))
    ap.add_argument("--step", help="(internal) run one step in this process")
    args = ap.parse_args()
    if args.step:
        run_step(args.step)
        return
    steps = ["device", "series"] + ["phase1:%s_%d" % (c, k) for c in CURVES for k in LOGS]
    res = {"phase1": {}}
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
