"""Times a BLS12-377 Groth16 proof over a resident key on one GPU, at m = 2^15 (the size of the reference's
groth16/examples/local_groth_bench.rs) and m = 2^20, three ways over the same arrays:

    one_at_a_time   dg16_groth16_prove, the host waiting for each proof
    queued          a queue of proofs with DG16_F_OVERLAP_TAIL, time per proof
    msm_calls       dg16_h_poly and five dg16_msm calls over the plain query arrays -- the only way to a proof of this
                    curve before the resident prover had it; the host-side additions that finish such a proof are NOT
                    in the figure.  This step uses nothing of the resident prover and runs unchanged on older commits.

The key is random points of the subgroups and a, b, c, w are random field elements: the prover's work does not depend on
the system being satisfied.  Each step is a fresh child process with a time limit of its own; the first step that fails
or runs out of time ends the run.

    python tools/prover377_timing.py [--sizes 15 20] [--reps 5] [--out profiles/prover377_timing.json]

Prints a markdown table (the one in DESIGN.md section 2.8.1) and writes the JSON, with the box's calibration line."""

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CURVE = "bls12_377"
FR_TOP = 0x12AB655E9A2CA556        # top 64-bit limb of the scalar modulus
FQ_BYTES = 48
WAYS = ("msm_calls", "one_at_a_time", "queued")
LIMIT_S = {"calibration": 120, "msm_calls": 240, "one_at_a_time": 240, "queued": 240}


def rand_fr(torch, n, dev, gen):
    """Uniform limbs with the top limb below the modulus': canonical scalars (and valid Montgomery forms)."""
    lo = torch.randint(-2**63, 2**63 - 1, (n, 3), dtype=torch.int64, device=dev, generator=gen)
    hi = torch.randint(0, FR_TOP, (n, 1), dtype=torch.int64, device=dev, generator=gen)
    return torch.cat([lo, hi], dim=1).contiguous()


def step(name, log_m, reps):
    import numpy as np
    import torch
    import dg16_amd
    import bench
    if name == "calibration":
        return bench.calibrate(0)
    ctx = dg16_amd.Context(0)
    dev = torch.device("cuda", 0)
    m, ni = 1 << log_m, 2
    nv = m
    g1b, g2b = 2 * FQ_BYTES, 4 * FQ_BYTES

    def bases(group, cnt, seed):
        t = torch.empty(cnt * g1b * group, dtype=torch.uint8, device=dev)
        ctx.gen_bases_dev(CURVE, group, 3700 + seed, cnt, t.data_ptr())
        return t

    aq, b1q, b2q, hq, lq = bases(1, nv, 1), bases(1, nv, 2), bases(2, nv, 3), bases(1, m, 4), bases(1, nv - ni, 5)
    f1, f2 = bases(1, 3, 6), bases(2, 2, 7)
    ctx.sync(0)
    fixed = torch.cat([f1, f2])
    gen = torch.Generator(device=dev)
    gen.manual_seed(log_m)
    a, b, c = (rand_fr(torch, m, dev, gen) for _ in range(3))
    w = rand_fr(torch, nv, dev, gen)
    w[0] = 0
    w[0, 0] = 1
    rs = np.array([[0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB, 0x0123456789ABCDEF],
                   [0xD6E8FEB86659FD93, 0xCA5A826395121157, 0xC2B2AE3D27D4EB4F, 0x0FEDCBA987654321]], dtype=np.uint64)
    torch.cuda.synchronize()
    n = max(reps, 3) * 4

    def timed(one, sync):
        for _ in range(2):
            one()
        sync()
        t0 = time.perf_counter()
        for _ in range(n):
            one()
        sync()
        return 1e3 * (time.perf_counter() - t0) / n

    if name == "msm_calls":
        h = torch.empty((m, 4), dtype=torch.int64, device=dev)
        res = [torch.empty(3 * FQ_BYTES * g, dtype=torch.uint8, device=dev) for g in (1, 1, 2, 1, 1)]
        torch.cuda.synchronize()

        def one():
            ctx.h_poly_dev(CURVE, a.data_ptr(), b.data_ptr(), c.data_ptr(), log_m, h.data_ptr())
            w1 = w.data_ptr() + 32
            ctx.msm_dev(CURVE, 1, aq.data_ptr() + g1b, w1, nv - 1, res[0].data_ptr(), in_subgroup=True)
            ctx.msm_dev(CURVE, 1, b1q.data_ptr() + g1b, w1, nv - 1, res[1].data_ptr(), in_subgroup=True)
            ctx.msm_dev(CURVE, 2, b2q.data_ptr() + g2b, w1, nv - 1, res[2].data_ptr(), in_subgroup=True)
            ctx.msm_dev(CURVE, 1, lq.data_ptr(), w.data_ptr() + 32 * ni, nv - ni, res[3].data_ptr(), in_subgroup=True)
            ctx.msm_dev(CURVE, 1, hq.data_ptr(), h.data_ptr(), m, res[4].data_ptr(), scalars_mont=True, in_subgroup=True)
            ctx.sync(0)          # the host adds the points next: it has to wait for them

        return dict(ms_per_proof=timed(one, lambda: ctx.sync(0)), proofs=n)

    t0 = time.perf_counter()
    pk = ctx.pk_create(CURVE, nv, ni, m, aq.data_ptr(), b1q.data_ptr(), b2q.data_ptr(), hq.data_ptr(), lq.data_ptr(),
                       fixed.data_ptr(), device_ptrs=True)
    pk_s = time.perf_counter() - t0
    info = pk.info()
    proof = torch.empty(12 * FQ_BYTES, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    overlap = name == "queued"

    def sync_all():
        for ch in range(3):
            ctx.sync(ch)

    def one():
        ctx.prove_dev(pk, a.data_ptr(), b.data_ptr(), c.data_ptr(), w.data_ptr(), rs, proof.data_ptr(), scalars_mont=False,
                      overlap_tail=overlap)
        if not overlap:
            sync_all()

    out = dict(ms_per_proof=timed(one, sync_all), proofs=n, pk_create_s=pk_s, c_ab=info["c_ab"], c_h=info["c_h"],
               table_bytes=info["table_bytes"])
    pk.close()
    return out


def run_step(name, log_m, reps):
    limit = LIMIT_S[name]
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--sizes", str(log_m), "--reps",
                            str(reps)], capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        print("step %s (2^%d) ran out of its %d s: stopping" % (name, log_m, limit), file=sys.stderr)
        return None
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        print("step %s (2^%d) failed (exit %d): stopping\n%s" % (name, log_m, r.returncode, r.stderr[-2000:]), file=sys.stderr)
        return None
    print("step %s (2^%d): %s" % (name, log_m, line[-1][7:]), file=sys.stderr, flush=True)
    return json.loads(line[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[15, 20])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ways", nargs="+", default=list(WAYS), choices=WAYS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prover377_timing.json"))
    ap.add_argument("--step", default=None, help="(internal) run one step in this process and print its JSON")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step(a.step, a.sizes[0], a.reps)))
        return 0
    res = dict(curve=CURVE, reps=a.reps, sizes={})
    res["calibration"] = run_step("calibration", a.sizes[0], a.reps)
    if res["calibration"] is None:
        return 1
    for log_m in a.sizes:
        row = res["sizes"][str(log_m)] = {}
        for way in a.ways:
            row[way] = run_step(way, log_m, a.reps)
            if row[way] is None:
                return 1
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("| %s, ms per proof | %s |" % (CURVE, " | ".join("m = 2^%d" % k for k in a.sizes)))
    print("|---|%s" % ("---|" * len(a.sizes)))
    for way in a.ways:
        print("| %s | %s |" % (way, " | ".join("%.3f" % res["sizes"][str(k)][way]["ms_per_proof"] for k in a.sizes)))
    if "msm_calls" in a.ways:
        for way in a.ways:
            if way != "msm_calls":
                print("| msm_calls / %s | %s |" % (way, " | ".join(
                    "%.2f" % (res["sizes"][str(k)]["msm_calls"]["ms_per_proof"] / res["sizes"][str(k)][way]["ms_per_proof"])
                    for k in a.sizes)))
    print("calibration: %s" % json.dumps(res["calibration"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
