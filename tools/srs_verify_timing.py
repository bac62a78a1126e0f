"""Times dg16_points_check and dg16_srs_verify next to what the library offered before them, in the same run.

    python tools/srs_verify_timing.py [--log-n 20] [--logs 16 20] [--reps 2] [--limit 600] [--out profiles/srs_verify_timing.json]

  check   dg16_points_check(subgroup = 1) of 2^log_n subgroup points (BN254 G2, BLS12-381 G1 and G2; host arrays, as the
          call takes them, so its copies are in the figure) against dg16_points_mul of the same points by full-width
          scalars without the subgroup flag -- what r P costs through the general kernel -- on device pointers (no
          transfer in that figure).  Next to the wall clock of both, the time between the events around the kernels
          (dg16_last_kernel_ms).
  srs     dg16_srs_verify for m = 2^k on BN254 against dg16_srs_prepare of the same size, and against its own parts, each
          through the public call that does the same work: membership (dg16_points_check of the five arrays), the eight
          sums (dg16_msm with 128-bit scalars and the subgroup flag, host arrays), the host pairings (dg16_srs_verify at
          log_m = 1, where everything else is nine points).

The parent never touches the GPU: each case runs in a child process of its own under `timeout -k 10 <limit>`, and the
first child that fails ends the run with its status.  Wall clock around the synchronous calls (one warm-up, the median
of --reps).  Prints the markdown tables of DESIGN.md 2.6.3 and writes the JSON."""

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

CHECK_GROUPS = (("bn254", 2), ("bls12_381", 1), ("bls12_381", 2))
SRS_CURVE = "bn254"


def median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts)


def coefficients(n, seed):
    import random
    import numpy as np
    rng = random.Random(seed)
    raw = b"".join(rng.randrange(1, 1 << 128).to_bytes(16, "little") for _ in range(n))
    return np.frombuffer(raw, dtype=np.uint64).reshape(n, 2).copy()


def child(case, reps, out_path):
    import numpy as np
    import torch
    import dg16_amd
    from dg16_amd import keygen
    import bench

    ctx = dg16_amd.Context(0)
    dev = torch.device("cuda", 0)
    kind, curve, group, log_n = case.split(":")
    group, log_n = int(group), int(log_n)
    name, cus = ctx.device_info()
    res = dict(case=case, kind=kind, curve=curve, log_n=log_n, device=name, compute_units=cus, reps=reps)
    if kind == "check":
        n = 1 << log_n
        pts = ctx.gen_bases(curve, group, 7, n)
        verdict = []
        res["check_ms"] = median_ms(lambda: verdict.append(ctx.points_check(curve, group, pts)), reps)
        res["check_kernels_ms"] = ctx.last_kernel_ms(0, 1)
        if any(v != (0, n) for v in verdict):
            print("subgroup points were reported bad: %r" % (verdict[-1],), file=sys.stderr)
            sys.exit(3)
        gen = torch.Generator(device=dev)
        gen.manual_seed(log_n)
        d_pts = torch.from_numpy(pts.view(np.int64)).to(dev)
        d_sc = bench.rand_fr(n, dev, gen, curve)
        d_out = torch.empty_like(d_pts)
        torch.cuda.synchronize()

        def mul():
            ctx.points_mul(curve, group, d_pts, d_sc, device=True, n=n, out=d_out)
            ctx.sync(0)

        res["points_mul_ms"] = median_ms(mul, reps)
        res["points_mul_kernels_ms"] = ctx.last_kernel_ms(0, 1)
        res.update(group=group, ratio=res["check_ms"] / res["points_mul_ms"],
                   ratio_kernels=res["check_kernels_ms"] / res["points_mul_kernels_ms"])
    else:
        m = 1 << log_n
        powers = keygen.powers_from_trapdoor(ctx, curve, log_n, 0x1234567, 0x7654321, 0xABCDEF01 + 5 * log_n)
        rho = coefficients(2 * m - 2, log_n)
        reports = []
        res["srs_verify_ms"] = median_ms(lambda: reports.append(ctx.srs_verify(curve, log_n, *powers, rho)), reps)
        if any(r != (0, 0, 0, 0) for r in reports):
            print("the transcript was rejected: %r" % (reports[-1],), file=sys.stderr)
            sys.exit(3)
        res["srs_prepare_ms"] = median_ms(lambda: ctx.srs_prepare(curve, log_n, *powers), reps)
        groups = (1, 2, 1, 1, 2)
        res["membership_ms"] = median_ms(lambda: [ctx.points_check(curve, g, a) for g, a in zip(groups, powers)], reps)
        wide = np.zeros((2 * m - 2, 4), dtype=np.uint64)
        wide[:, :2] = rho

        def sums():
            for arr, g, terms in ((powers[0], 1, 2 * m - 2), (powers[2], 1, m - 1), (powers[3], 1, m - 1),
                                  (powers[1], 2, m - 1)):
                for shift in (0, 1):
                    ctx.msm(curve, g, arr[shift:shift + terms], wide[:terms], affine=True, in_subgroup=True)

        res["sums_ms"] = median_ms(sums, reps)
        small = keygen.powers_from_trapdoor(ctx, curve, 1, 0x1234567, 0x7654321, 0xABCDEF01)
        res["pairings_ms"] = median_ms(lambda: ctx.srs_verify(curve, 1, *small, rho[:2]), reps)
        res["parts_ms"] = res["membership_ms"] + res["sums_ms"] + res["pairings_ms"]
        res.update(ratio=res["srs_verify_ms"] / res["srs_prepare_ms"], ratio_parts=res["srs_verify_ms"] / res["parts_ms"])
    with open(out_path, "w") as f:
        json.dump(res, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20, help="points of the membership cases")
    ap.add_argument("--logs", type=int, nargs="*", default=[16, 20], help="log2 m of the transcript cases")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--limit", type=int, default=600, help="seconds per child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "srs_verify_timing.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-out", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps, a.child_out)
        return 0
    cases = ["check:%s:%d:%d" % (c, g, a.log_n) for c, g in CHECK_GROUPS]
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
    print("| group | log2 n | dg16_points_check ms (kernels) | dg16_points_mul ms (kernels) | ratio (kernels) |")
    print("|---|---|---|---|---|")
    for r in rows:
        if r["kind"] == "check":
            print("| %s G%d | %d | %.1f (%.1f) | %.1f (%.1f) | %.2f (%.2f) |"
                  % (r["curve"], r["group"], r["log_n"], r["check_ms"], r["check_kernels_ms"], r["points_mul_ms"],
                     r["points_mul_kernels_ms"], r["ratio"], r["ratio_kernels"]))
    print()
    print("| curve | log2 m | dg16_srs_verify ms | dg16_srs_prepare ms | ratio | membership ms | sums ms | pairings ms |"
          " verify / parts |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        if r["kind"] == "srs":
            print("| %s | %d | %.1f | %.1f | %.2f | %.1f | %.1f | %.1f | %.2f |"
                  % (r["curve"], r["log_n"], r["srs_verify_ms"], r["srs_prepare_ms"], r["ratio"], r["membership_ms"],
                     r["sums_ms"], r["pairings_ms"], r["ratio_parts"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
