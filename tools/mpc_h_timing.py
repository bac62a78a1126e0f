#!/usr/bin/env python3
"""Times dg16_ext_wit_h with and without DG16_F_H_ODD at the reference's size, m = 2^15, with the 4 l parties as contexts
(host threads) of one process on one GPU.

  cases        BN254 and BLS12-377; l = 2 unflagged and flagged, alternating in one visit, three runs each after one
               warm-up of each; l = 4 and l = 8 flagged (the unflagged call refuses those l), three runs after a warm-up.
  clock        a host clock around the synchronous call on the king (party 0), who leaves last: six transform rounds,
               the gather, the king's step, the scatter, host copies included.  The king's step is the only part that
               differs between the two calls: three unpack launches, h_odd_kernel and a pack launch (7 m n field products,
               a 6 m element buffer) against one h_king_kernel launch (4 m n, no buffer).
  yardstick    the unflagged call at l = 2, whose kernels the flag does not touch: the flagged median should lie within
               that call's own max - min of three runs of the unflagged median, or below it.  Recorded either way.
  checked      at l = 2 the two calls' outputs are compared byte for byte on every party.

Every (curve, l) is a child process under its own time limit, and the first failure stops the run:

    python3 tools/mpc_h_timing.py [--out profiles/mpc_h_timing.json]
"""

import argparse
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

CURVES = ("bn254", "bls12_377")
LS = (2, 4, 8)
LOG_M = 15
RUNS = 3
STEP_LIMIT_S = 240


def step(curve, l, log_m):
    import dg16_amd
    from dg16_amd import dist as D
    n, m = 4 * l, 1 << log_m
    ctxs = [dg16_amd.Context(0) for _ in range(n)]
    pps = [D.PackedSharingParams(c, curve, l) for c in ctxs]
    net = D.LocalTestNet(n)
    rng = np.random.default_rng(1000 * l + log_m)
    # any Montgomery words below the modulus are shares: the top limb stays under 2^60, both moduli exceed 2^252
    shares = rng.integers(0, 1 << 63, size=(n, 3, m // l, 4), dtype=np.uint64)
    shares[..., 3] >>= np.uint64(4)

    def call(odd):
        def party(i, h):
            t0 = time.perf_counter()
            out = D.ext_wit_h(ctxs[i], pps[i], h, shares[i, 0], shares[i, 1], shares[i, 2], log_m, odd=odd)
            return 1e3 * (time.perf_counter() - t0), out
        res = net.simulate_network_round(party)
        return res[0][0], [r[1] for r in res]

    res = {"curve": curve, "l": l, "parties": n, "log_m": log_m}
    _, out_odd = call(True)                                                          # warm-ups
    kinds = [True]
    if l == 2:
        _, out_ref = call(False)
        res["flagged_equals_unflagged"] = all(np.array_equal(a, b) for a, b in zip(out_odd, out_ref))
        assert res["flagged_equals_unflagged"], "DG16_F_H_ODD differs from the unflagged call at l = 2"
        kinds = [False, True]
    times = {k: [] for k in kinds}
    for _ in range(RUNS):
        for k in kinds:
            times[k].append(call(k)[0])
    for k in kinds:
        name = "flagged" if k else "unflagged"
        res[name + "_ms"] = times[k]
        res[name + "_median_ms"] = statistics.median(times[k])
        print("  %s l=%d %s: %s ms" % (curve, l, name, ", ".join("%.2f" % t for t in times[k])), file=sys.stderr, flush=True)
    if l == 2:
        spread = max(times[False]) - min(times[False])
        diff = res["flagged_median_ms"] - res["unflagged_median_ms"]
        res["unflagged_spread_ms"] = spread
        res["flagged_minus_unflagged_ms"] = diff
        res["within_yardstick"] = bool(diff <= spread)
    net.close()
    return res


def table(res):
    lines = ["| curve | l | parties | unflagged ms (3 runs) | flagged ms (3 runs) | flagged - unflagged, medians | unflagged max - min | within |",
             "|---|---|---|---|---|---|---|---|"]
    fmt = lambda ts: ", ".join("%.2f" % t for t in ts)       # noqa: E731
    for r in res["cases"].values():
        if r["l"] == 2:
            lines.append("| %s | 2 | 8 | %s | %s | %+.2f | %.2f | %s |" % (
                r["curve"], fmt(r["unflagged_ms"]), fmt(r["flagged_ms"]), r["flagged_minus_unflagged_ms"],
                r["unflagged_spread_ms"], "yes" if r["within_yardstick"] else "no"))
        else:
            lines.append("| %s | %d | %d | refused | %s | | | |" % (r["curve"], r["l"], r["parties"], fmt(r["flagged_ms"])))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc_h_timing.json"))
    ap.add_argument("--step", help="(internal) run one case in this process: curve:l:log_m")
    args = ap.parse_args()
    if args.step:
        curve, l, log_m = args.step.split(":")
        print("RESULT " + json.dumps(step(curve, int(l), int(log_m))))
        return
    res = {"log_m": LOG_M, "runs": RUNS, "clock": "host clock around the synchronous call on the king, ms", "cases": {}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for curve in CURVES:
        for l in LS:
            name = "%s:%d:%d" % (curve, l, LOG_M)
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], stdout=subprocess.PIPE,
                                   text=True, timeout=STEP_LIMIT_S)
            except subprocess.TimeoutExpired:
                print("case %s exceeded %d s: stopping" % (name, STEP_LIMIT_S), flush=True)
                sys.exit(124)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print("case %s failed (status %d): stopping\n%s" % (name, p.returncode, p.stdout[-2000:]), flush=True)
                sys.exit(1)
            res["cases"]["%s_l%d" % (curve, l)] = json.loads(line[-1][7:])
            print("case %s done" % name, flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(table(res))


if __name__ == "__main__":
    main()
