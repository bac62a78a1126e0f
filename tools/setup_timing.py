"""Times key generation on one GPU, one process: dg16_fixed_base_mul (G1, G2) at n = 2^10 .. 2^22 per curve next to
dg16_msm over fresh bases at the same n (the yardstick: the same number of mixed additions per point, plus a bucket
reduction the fixed-base path does not have, minus its table build and affine conversion), and the whole
dg16_groth16_setup at m = 2^15 and 2^20 split per stage.  HIP events on the library's stream (dg16_last_kernel_ms,
which = 0: the whole call), one warm-up and the median of `--reps` repetitions per figure.

    python tools/setup_timing.py [--curves bn254,bls12_381,bls12_377] [--max-log 22] [--out profiles/setup_timing.json]

Prints a markdown table (the one in DESIGN.md) and writes the JSON."""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np          # noqa: E402
import torch                # noqa: E402

import dg16_amd             # noqa: E402
from dg16_amd import keygen  # noqa: E402
import bench                # noqa: E402


def median_ms(ctx, fn, reps, channel=0):
    fn()
    ctx.sync(channel)
    out = []
    for _ in range(reps):
        fn()
        ctx.sync(channel)
        out.append(ctx.last_kernel_ms(channel, 0))
    return statistics.median(out)


def rand_fr(curve, n, dev, gen):
    top = keygen.FR_MODULUS[curve] >> 192
    lo = torch.randint(-2**63, 2**63 - 1, (n, 3), dtype=torch.int64, device=dev, generator=gen)
    hi = torch.randint(0, top, (n, 1), dtype=torch.int64, device=dev, generator=gen)
    return torch.cat([lo, hi], dim=1).contiguous()


def time_kernels(ctx, curve, dev, max_log, reps):
    fqb = 32 if curve == "bn254" else 48
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    rows = []
    for group in (1, 2):
        pb = 2 * fqb * group
        for log_n in range(10, max_log + 1, 2):
            n = 1 << log_n
            sc = rand_fr(curve, n, dev, gen)
            bases = torch.empty(n * pb, dtype=torch.uint8, device=dev)
            out = torch.empty(n * pb, dtype=torch.uint8, device=dev)
            res = torch.empty(3 * pb // 2, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            ctx.gen_bases_dev(curve, group, 5 + log_n, n, bases.data_ptr())
            ctx.sync(0)
            fb = median_ms(ctx, lambda: ctx.fixed_base_mul_dev(curve, group, sc.data_ptr(), n, out.data_ptr()), reps)
            fb_core = ctx.last_kernel_ms(0, 1)        # multiply + affine kernels of the last repetition (no table build)
            msm = median_ms(ctx, lambda: ctx.msm_dev(curve, group, bases.data_ptr(), sc.data_ptr(), n, res.data_ptr(),
                                                     in_subgroup=True), reps)
            rows.append(dict(curve=curve, group=group, log_n=log_n, window_bits=ctx.L.dg16_fixed_base_window_bits(n),
                             fixed_base_ms=fb, fixed_base_points_ms=fb_core, msm_ms=msm, ratio=fb / msm))
            del sc, bases, out, res
            torch.cuda.empty_cache()
    return rows


def time_setup(ctx, curve, dev, log_m, reps):
    """Synthetic system: 3 non-zeros per row of A and B over all wires, one per row of C; num_vars = m."""
    m, ni = 1 << log_m, 2
    nc, nv = m - ni, m
    gen = torch.Generator(device=dev)
    gen.manual_seed(log_m)
    ptr3 = (torch.arange(nc + 1, dtype=torch.int64, device=dev) * 3).to(torch.int32)
    ptr1 = torch.arange(nc + 1, dtype=torch.int32, device=dev)
    col = lambda k: torch.randint(0, nv, (k,), dtype=torch.int32, device=dev, generator=gen)      # noqa: E731
    system = dict(num_constraints=nc, num_inputs=ni, num_vars=nv, a=(ptr3, col(3 * nc), rand_fr(curve, 3 * nc, dev, gen)),
                  b=(ptr3, col(3 * nc), rand_fr(curve, 3 * nc, dev, gen)), c=(ptr1, col(nc), rand_fr(curve, nc, dev, gen)))
    torch.cuda.synchronize()
    keygen.generate_parameters(ctx, curve, system)       # warm-up (twiddles, workspaces)
    whole = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p = keygen.generate_parameters(ctx, curve, system)
        whole.append(1e3 * (time.perf_counter() - t0))
        del p
    # the point stage alone, call by call, on scalars of the same count
    fqb = 32 if curve == "bn254" else 48
    sc = rand_fr(curve, m, dev, gen)
    out = torch.empty(m * 4 * fqb, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g1 = median_ms(ctx, lambda: ctx.fixed_base_mul_dev(curve, 1, sc.data_ptr(), m, out.data_ptr(), scalars_mont=True), reps)
    g2 = median_ms(ctx, lambda: ctx.fixed_base_mul_dev(curve, 2, sc.data_ptr(), nv, out.data_ptr(), scalars_mont=True), reps)
    total = statistics.median(whole)
    # a, b1, h: m points each, l: m - ni, gamma_abc + fixed: a handful  ->  ~4 G1 calls of m points; b2: one G2 call
    return dict(curve=curve, log_m=log_m, setup_ms=total, g1_ms=4 * g1, g2_ms=g2, scalars_ms=max(total - 4 * g1 - g2, 0.0),
                note="g1 = 4 x one m-point G1 call, g2 = one num_vars-point G2 call, timed separately; scalars = rest "
                     "(powers, two inverse NTTs, three transposes, column gather, temporary allocations, host sync)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="bn254,bls12_381,bls12_377")
    ap.add_argument("--max-log", type=int, default=22)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--setup-logs", default="15,20")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "setup_timing.json"))
    a = ap.parse_args()
    ctx = dg16_amd.Context(0)
    dev = torch.device("cuda", 0)
    name, cus = ctx.device_info()
    res = dict(device=name, compute_units=cus, reps=a.reps, kernels=[], setup=[])
    for curve in a.curves.split(","):
        res["kernels"] += time_kernels(ctx, curve, dev, a.max_log, a.reps)
        for log_m in [int(x) for x in a.setup_logs.split(",") if x]:
            res["setup"].append(time_setup(ctx, curve, dev, log_m, a.reps))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("| curve | group | log2 n | c | fixed_base_mul ms | of which points ms | dg16_msm ms | ratio |")
    print("|---|---|---|---|---|---|---|---|")
    for r in res["kernels"]:
        print("| %s | G%d | %d | %d | %.3f | %.3f | %.3f | %.2f |" % (r["curve"], r["group"], r["log_n"], r["window_bits"],
                                                                  r["fixed_base_ms"], r["fixed_base_points_ms"],
                                                                  r["msm_ms"], r["ratio"]))
    print()
    print("| curve | log2 m | dg16_groth16_setup ms | scalars | G1 points | G2 points |")
    print("|---|---|---|---|---|---|")
    for r in res["setup"]:
        print("| %s | %d | %.1f | %.1f | %.1f | %.1f |" % (r["curve"], r["log_m"], r["setup_ms"], r["scalars_ms"], r["g1_ms"],
                                                       r["g2_ms"]))


if __name__ == "__main__":
    main()
