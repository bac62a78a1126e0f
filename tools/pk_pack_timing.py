#!/usr/bin/env python3
"""Times the packing of a proving key into party shares: dg16_pk_pack / dg16_pss_pack_points (csrc/pss_pack.h) against
the five dg16_pss_apply_exp calls groth16_mpc.pack_from_arkworks_proving_key makes.

  keys         wire counts 2^16 and 2^20 (num_vars = 2^k + 1, one input, domain 2^k: every query packs 2^k points);
               BN254 at l = 2 and l = 8, BLS12-381 at l = 2.  The points are dg16_gen_bases output -- neither path's
               cost depends on which subgroup points a key holds.
  method       per query array (s, u, w, h, v) dg16_pss_pack_points and dg16_pss_apply_exp alternate on the SAME host
               points in one process, each timed by a host clock around the synchronous call (copies included on both
               sides), median of 3 after one warm-up of each; then the whole key: one dg16_pk_pack against the sum of
               the old path's five medians.  The new call is timed with in_subgroup = 0 and 1 (the old path has no
               such argument).  Outputs are compared byte for byte at every timed size.
  counted      beside each time, the group operations per output by the header's count: old l x (254 doublings + 127
               additions); new (top position + 1/4) doublings + (31 / 4 + l x bits / 8) additions at width 7, bits = 254
               on the DIM 2 split, 255 plain, 264 on the DIM 4 split.

Every key is a child process under its own time limit, and the first failure stops the run:

    python3 tools/pk_pack_timing.py [--out profiles/pk_pack_timing.json]
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

KEYS = (("bn254", 2), ("bn254", 8), ("bls12_381", 2))
LOGS = (16, 20)
STEP_LIMIT_S = {16: 180, 20: 600}
WIDTH = 7
QUERIES = (("s", 1, "a_query[1..]"), ("u", 1, "h_query"), ("w", 1, "l_query"), ("h", 1, "b_g1_query[1..]"),
           ("v", 2, "b_g2_query[1..]"))


def counted(curve, group, l, in_subgroup):
    """group operations per output (doublings, additions) of both paths, by the header's count"""
    split = (curve, group) == ("bn254", 1) or in_subgroup
    dim = 1 if not split else 4 if (curve != "bn254" and group == 2) else 2
    top, bits = {1: (254, 255), 2: (126, 254), 4: (65, 264)}[dim]
    new = (top + 0.25, ((1 << (WIDTH - 2)) - 1) / 4 + l * bits / (WIDTH + 1))
    return {"parts": dim, "new_doublings": new[0], "new_additions": round(new[1], 2), "old_doublings": 254 * l,
            "old_additions": 127 * l, "ratio": round(sum(new) / (381 * l), 3)}


def _ms(call):
    t0 = time.perf_counter()
    call()
    return 1e3 * (time.perf_counter() - t0)


def step(curve, l, log_n):
    import dg16_amd
    from dg16_amd import dist as D
    from dg16_amd.lib import PkShares, _ptr
    ctx = dg16_amd.Context(0)
    pp = D.PackedSharingParams(ctx, curve, l)
    L, n = ctx.L, 1 << log_n
    chunks = n // l
    res = {"log_n": log_n, "l": l, "points_per_query": n, "outputs_per_query": chunks * pp.n, "queries": {}}
    pts, new_out = {}, {}
    old_total = 0.0
    for seed, (name, group, what) in enumerate(QUERIES):
        p = ctx.gen_bases(curve, group, 50 + seed, n + (what.endswith("[1..]")))      # element 0 is dropped by [1..]
        body = p[1:] if what.endswith("[1..]") else p
        nl = p.shape[1]
        out_new = np.zeros((pp.n, chunks, nl), dtype=np.uint64)
        out_old = np.zeros((chunks, pp.n, nl), dtype=np.uint64)
        new = lambda f: ctx._chk(L.dg16_pss_pack_points(ctx.h, pp.h, group, _ptr(body), n, _ptr(out_new), f))      # noqa: E731
        old = lambda: ctx._chk(L.dg16_pss_apply_exp(ctx.h, pp.h, group, 0, _ptr(body), chunks, _ptr(out_old), 0, 0))  # noqa: E731
        old()                                                                                   # warm-ups
        new(1)
        assert np.array_equal(out_new, out_old.transpose(1, 0, 2)), "in_subgroup result differs from dg16_pss_apply_exp"
        new(0)
        assert np.array_equal(out_new, out_old.transpose(1, 0, 2)), "dg16_pss_pack_points differs from dg16_pss_apply_exp"
        t_new, t_sub, t_old = [], [], []
        for _ in range(3):
            t_new.append(_ms(lambda: new(0)))
            t_old.append(_ms(old))
            t_sub.append(_ms(lambda: new(1)))
        m_new, m_sub, m_old = (statistics.median(t) for t in (t_new, t_sub, t_old))
        old_total += m_old
        res["queries"][name] = {"array": what, "group": group, "new_ms": m_new, "new_in_subgroup_ms": m_sub,
                                "old_ms": m_old, "ratio": m_new / m_old, "ratio_in_subgroup": m_sub / m_old,
                                "counted": counted(curve, group, l, False),
                                "counted_in_subgroup": counted(curve, group, l, True)}
        print("  %s %s 2^%d l=%d: new %.1f ms (in_subgroup %.1f), old %.1f ms" % (curve, name, log_n, l, m_new, m_sub,
                                                                                   m_old), file=sys.stderr, flush=True)
        pts[name], new_out[name] = p, out_new.copy()
        del out_old
    # the whole key in one call
    outs = {k: np.zeros_like(v) for k, v in new_out.items()}
    ks = PkShares(**{k: _ptr(v).value for k, v in outs.items()})
    nv = n + 1
    whole = lambda f: ctx._chk(L.dg16_pk_pack(ctx.h, pp.h, nv, 1, n, _ptr(pts["s"]), _ptr(pts["h"]), _ptr(pts["v"]),   # noqa: E731
                                              _ptr(pts["u"]), _ptr(pts["w"]), ctypes.byref(ks), f))
    whole(0)
    assert all(np.array_equal(outs[k], new_out[k]) for k in outs), "dg16_pk_pack differs from the five packings"
    t0 = statistics.median(_ms(lambda: whole(0)) for _ in range(3))
    t1 = statistics.median(_ms(lambda: whole(1)) for _ in range(3))
    res["whole_key"] = {"pk_pack_ms": t0, "pk_pack_in_subgroup_ms": t1, "old_five_calls_ms": old_total,
                        "ratio": t0 / old_total, "ratio_in_subgroup": t1 / old_total}
    return res


def table(res):
    lines = ["| curve | l | wires | query | new ms | new ms, in_subgroup | old ms | ratio | ratio, in_subgroup | counted ratio (plain / split) |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for key, r in res["keys"].items():
        curve = key.rsplit("_l", 1)[0]
        for name, q in r["queries"].items():
            lines.append("| %s | %d | 2^%d | %s (%s) | %.1f | %.1f | %.1f | %.3f | %.3f | %.3f / %.3f |" % (
                curve, r["l"], r["log_n"], name, q["array"], q["new_ms"], q["new_in_subgroup_ms"], q["old_ms"], q["ratio"],
                q["ratio_in_subgroup"], q["counted"]["ratio"], q["counted_in_subgroup"]["ratio"]))
        w = r["whole_key"]
        lines.append("| %s | %d | 2^%d | whole key | %.1f | %.1f | %.1f | %.3f | %.3f | |" % (
            curve, r["l"], r["log_n"], w["pk_pack_ms"], w["pk_pack_in_subgroup_ms"], w["old_five_calls_ms"], w["ratio"],
            w["ratio_in_subgroup"]))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pk_pack_timing.json"))
    ap.add_argument("--step", help="(internal) run one key in this process: curve:l:log_n")
    args = ap.parse_args()
    if args.step:
        curve, l, log_n = args.step.split(":")
        print("RESULT " + json.dumps(step(curve, int(l), int(log_n))))
        return
    res = {"width": WIDTH, "keys": {}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for log_n in LOGS:
        for curve, l in KEYS:
            name = "%s:%d:%d" % (curve, l, log_n)
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], stdout=subprocess.PIPE,
                                   text=True, timeout=STEP_LIMIT_S[log_n])
            except subprocess.TimeoutExpired:
                print("key %s exceeded %d s: stopping" % (name, STEP_LIMIT_S[log_n]), flush=True)
                sys.exit(124)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print("key %s failed (status %d): stopping\n%s" % (name, p.returncode, p.stdout[-2000:]), flush=True)
                sys.exit(1)
            res["keys"]["%s_l%d_2^%d" % (curve, l, log_n)] = json.loads(line[-1][7:])
            print("key %s done" % name, flush=True)
            with open(args.out + ".partial", "w") as f:
                json.dump(res, f)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    os.remove(args.out + ".partial")
    print(table(res))


if __name__ == "__main__":
    main()
