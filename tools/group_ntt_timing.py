"""Times dg16_group_ntt and dg16_srs_prepare next to dg16_points_mul for exactly the number of products the transform's
budget names, on the same group in the same run: the butterflies add two additions and a share of a batched inversion to
each product and every stage a few launches, so a transform should stay within 15 % of that figure.

    python tools/group_ntt_timing.py [--logs 16 20] [--reps 2] [--limit 600] [--out profiles/group_ntt_timing.json]

  ntt   forward dg16_group_ntt of 2^k points (BN254 G1 and G2, BLS12-381 G1), host arrays as the call takes them, against
        dg16_points_mul with DG16_F_BASES_IN_SUBGROUP on (n / 2) k - (n - 1) products (device pointers: no transfer in
        that figure, so the ratio charges the transform its copies as well)
  srs   dg16_srs_prepare for m = 2^k (BN254, circom h basis) against its budget: four G1 passes and one G2 pass of
        (m / 2) k - (m - 1) + m products each

The parent never touches the GPU: each case runs in a child process of its own under `timeout -k 10 <limit>`, and the
first child that fails ends the run with its status.  Wall clock around the synchronous calls (one warm-up, the median
of --reps).  Prints a markdown table (the one in DESIGN.md 2.6.2) and writes the JSON."""

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NTT_GROUPS = (("bn254", 1), ("bn254", 2), ("bls12_381", 1))
SRS_CURVE = "bn254"


def budget(log_n, inverse=False):
    n = 1 << log_n
    return (n // 2) * log_n - (n - 1) + (n if inverse else 0)


def median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts)


def points_mul_ms(ctx, dev, curve, group, products, reps, calls=1):
    """`calls` dg16_points_mul calls of `products` products each, subgroup flag set, device pointers"""
    import numpy as np
    import torch
    import bench
    gen = torch.Generator(device=dev)
    gen.manual_seed(products % 1000003)
    base = torch.from_numpy(ctx.gen_bases(curve, group, 3, 1 << 12).view(np.int64)).to(dev)
    pts = base.repeat((products + base.shape[0] - 1) // base.shape[0], 1)[:products].contiguous()
    sc = bench.rand_fr(products, dev, gen, curve)
    out = torch.empty_like(pts)
    torch.cuda.synchronize()

    def run():
        for _ in range(calls):
            ctx.points_mul(curve, group, pts, sc, in_subgroup=True, device=True, n=products, out=out)
        ctx.sync(0)

    return median_ms(run, reps)


def child(case, reps, out_path):
    import torch
    import dg16_amd
    from dg16_amd import keygen

    ctx = dg16_amd.Context(0)
    dev = torch.device("cuda", 0)
    kind, curve, group, log_n = case.split(":")
    group, log_n = int(group), int(log_n)
    name, cus = ctx.device_info()
    res = dict(case=case, kind=kind, curve=curve, log_n=log_n, device=name, compute_units=cus, reps=reps)
    if kind == "ntt":
        x = ctx.gen_bases(curve, group, 7, 1 << log_n)
        res.update(group=group, products=budget(log_n))
        res["group_ntt_ms"] = median_ms(lambda: ctx.group_ntt(curve, group, x), reps)
        res["points_mul_ms"] = points_mul_ms(ctx, dev, curve, group, budget(log_n), reps)
    else:
        powers = keygen.powers_from_trapdoor(ctx, curve, log_n, 0x1234567, 0x7654321, 0xABCDEF01 + 5 * log_n)
        per_pass = budget(log_n, inverse=True)
        res.update(products_g1=4 * per_pass, products_g2=per_pass)
        res["srs_prepare_ms"] = median_ms(lambda: ctx.srs_prepare(curve, log_n, *powers), reps)
        res["points_mul_g1_ms"] = points_mul_ms(ctx, dev, curve, 1, per_pass, reps, calls=4)
        res["points_mul_g2_ms"] = points_mul_ms(ctx, dev, curve, 2, per_pass, reps)
        res["points_mul_ms"] = res["points_mul_g1_ms"] + res["points_mul_g2_ms"]
    res["ratio"] = res["group_ntt_ms" if kind == "ntt" else "srs_prepare_ms"] / res["points_mul_ms"]
    with open(out_path, "w") as f:
        json.dump(res, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--limit", type=int, default=600, help="seconds per child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_ntt_timing.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-out", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps, a.child_out)
        return 0
    cases = ["ntt:%s:%d:%d" % (c, g, k) for k in a.logs for c, g in NTT_GROUPS]
    cases += ["srs:%s:1:%d" % (SRS_CURVE, k) for k in a.logs]
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, case in enumerate(cases):
            part = os.path.join(tmp, "%d.json" % i)
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", case,
                   "--child-out", part, "--reps", str(a.reps)]
            rc = subprocess.call(cmd)
            if rc != 0:
                print("case %s ended with status %d: stopping" % (case, rc), file=sys.stderr)
                return rc
            with open(part) as f:
                rows.append(json.load(f))
            print("%s: ratio %.2f" % (case, rows[-1]["ratio"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(cases=rows), f, indent=1)
    print("| call | group | log2 n | ms | products | dg16_points_mul ms | ratio |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        if r["kind"] == "ntt":
            print("| dg16_group_ntt | %s G%d | %d | %.1f | %d | %.1f | %.2f |"
                  % (r["curve"], r["group"], r["log_n"], r["group_ntt_ms"], r["products"], r["points_mul_ms"], r["ratio"]))
        else:
            print("| dg16_srs_prepare | %s | %d | %.1f | %d G1 + %d G2 | %.1f | %.2f |"
                  % (r["curve"], r["log_n"], r["srs_prepare_ms"], r["products_g1"], r["products_g2"], r["points_mul_ms"],
                     r["ratio"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
