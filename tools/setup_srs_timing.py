"""Times dg16_groth16_setup_srs (the key in the exponent, from a structured reference string) next to dg16_groth16_setup
(the key from a trapdoor) for the same system in the same run: BN254, 2^log_m - 2 constraints with the bench workload's
matrix shape (3 non-zeros per row of A and of B, uniform over all wires; one per row of C; num_vars = 2^log_m) -- once
with every coefficient +-1, as in a circom circuit, and once with full-width coefficients.  The reference string comes
from keygen.srs_from_trapdoor under the trapdoor (alpha, beta, 1, 1, tau) the other call gets, so the two keys are
compared as well.

    python tools/setup_srs_timing.py [--log-m 20] [--reps 3] [--limit 900] [--out profiles/setup_srs_timing.json]

The parent never touches the GPU: each case runs in a child process of its own under `timeout -k 10 <limit>`, and the
first child that fails ends the run with its status.  Wall clock around the synchronous calls on device pointers (one
warm-up, the median of --reps); next to the times, the share of terms that skipped the multiplication and the terms per
summation path.  Prints a markdown table (the one in DESIGN.md) and writes the JSON."""

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

CASES = ("pm1", "full")
CURVE = "bn254"


def child(case, log_m, reps, out_path, in_subgroup):
    import numpy as np
    import torch
    import dg16_amd
    from dg16_amd import keygen
    import bench

    ctx = dg16_amd.Context(0)
    dev = torch.device("cuda", 0)
    r = keygen.FR_MODULUS[CURVE]
    m, ni = 1 << log_m, 2
    nc, nv = m - ni, m
    gen = torch.Generator(device=dev)
    gen.manual_seed(log_m)

    def coeffs(n):
        if case == "full":
            return bench.rand_fr(n, dev, gen, CURVE)
        # +-1 in Montgomery form, a coin per entry
        R = (1 << 256) % r
        pm = torch.from_numpy(keygen._ints_to_arr([R, r - R]).view(np.int64)).to(dev)
        return pm[torch.randint(0, 2, (n,), device=dev, generator=gen)].contiguous()

    ptr3 = (torch.arange(nc + 1, dtype=torch.int64, device=dev) * 3).to(torch.int32)
    ptr1 = torch.arange(nc + 1, dtype=torch.int32, device=dev)
    col = lambda k: torch.randint(0, nv, (k,), dtype=torch.int32, device=dev, generator=gen)      # noqa: E731
    mats = [(ptr3, col(3 * nc), coeffs(3 * nc)), (ptr3, col(3 * nc), coeffs(3 * nc)), (ptr1, col(nc), coeffs(nc))]
    td = (0x1234567 + 2 * log_m, 0x7654321 + 3 * log_m, 1, 1, 0xABCDEF01 + 5 * log_m)
    t0 = time.perf_counter()
    srs = keygen.srs_from_trapdoor(ctx, CURVE, log_m, td[0], td[1], td[4])
    srs_s = time.perf_counter() - t0
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)      # noqa: E731
    tabs = [up(getattr(srs, n)) for n in keygen.Srs.ARRAYS]
    g1b, g2b = 64, 128
    sizes = (nv * g1b, nv * g1b, nv * g2b, m * g1b, (nv - ni) * g1b, 3 * g1b + 2 * g2b, g2b, ni * g1b)
    outs = [[torch.empty(s, dtype=torch.uint8, device=dev) for s in sizes] for _ in range(2)]
    tdarr = keygen._trapdoor_array(CURVE, td)
    torch.cuda.synchronize()
    ctx.sync(0)
    mp = [[t.data_ptr() for t in mt] for mt in mats]

    def run_trapdoor():
        ctx.groth16_setup(CURVE, nc, ni, nv, log_m, *mp, tdarr, [t.data_ptr() for t in outs[0]], device_ptrs=True)

    def run_srs():
        ctx.groth16_setup_srs(CURVE, nc, ni, nv, log_m, *mp, [t.data_ptr() for t in tabs] + [srs.fixed],
                              [t.data_ptr() for t in outs[1]], device_ptrs=True, in_subgroup=in_subgroup)

    def median_ms(fn):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(ts)

    t_td = median_ms(run_trapdoor)
    t_srs = median_ms(run_srs)
    torch.cuda.synchronize()
    equal = all(bool(torch.equal(a, b)) for a, b in zip(outs[0], outs[1]))
    # terms per path of each of the four outputs (the rule of dg16_setup_srs_limits on the column counts) and the share
    # of terms whose coefficient is 0, 1 or r - 1
    import ctypes
    wf, mf = ctypes.c_uint(), ctypes.c_uint()
    ctx.L.dg16_setup_srs_limits(ctypes.byref(wf), ctypes.byref(mf))
    cnt = [torch.bincount(mt[1].long(), minlength=nv) for mt in mats]
    inst = torch.zeros(nv, dtype=torch.long, device=dev)
    inst[:ni] = 1
    seg = {"a_query": cnt[0] + inst, "b_g1_query": cnt[1], "b_g2_query": cnt[1], "K": cnt[0] + cnt[1] + cnt[2] + inst}
    paths = {}
    for name, ln in seg.items():
        lane = int(ln[(ln > 0) & (ln < wf.value)].sum())
        wave = int(ln[(ln >= wf.value) & (ln < mf.value)].sum())
        msm = int(ln[ln >= mf.value].sum())
        paths[name] = dict(lane=lane, wave=wave, msm=msm)
    terms = sum(sum(p.values()) for p in paths.values())
    trivial_per_matrix = [n if case == "pm1" else 0 for n in (3 * nc, 3 * nc, nc)]      # by construction of coeffs()
    trivial = 2 * trivial_per_matrix[0] + 3 * trivial_per_matrix[1] + trivial_per_matrix[2] + 2 * ni
    name, cus = ctx.device_info()
    res = dict(case=case, curve=CURVE, log_m=log_m, num_constraints=nc, num_vars=nv, device=name, compute_units=cus,
               reps=reps, in_subgroup=in_subgroup, setup_ms=t_td, setup_srs_ms=t_srs, ratio=t_srs / t_td, terms=terms,
               terms_without_multiplication=trivial, share_without_multiplication=trivial / terms, terms_per_path=paths,
               wave_from=wf.value, msm_from=mf.value, keys_equal=equal, srs_from_trapdoor_s=srs_s)
    with open(out_path, "w") as f:
        json.dump(res, f)
    if not equal:
        print("the two keys differ", file=sys.stderr)
        sys.exit(3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-m", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=900, help="seconds per child process")
    ap.add_argument("--in-subgroup", action="store_true", help="pass DG16_F_BASES_IN_SUBGROUP (the endomorphism split)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "setup_srs_timing.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-out", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.log_m, a.reps, a.child_out, a.in_subgroup)
        return 0
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for case in CASES:
            part = os.path.join(tmp, case + ".json")
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", case,
                   "--child-out", part, "--log-m", str(a.log_m), "--reps", str(a.reps)]
            if a.in_subgroup:
                cmd.append("--in-subgroup")
            rc = subprocess.call(cmd)
            if rc != 0:
                print("case %s ended with status %d: stopping" % (case, rc), file=sys.stderr)
                return rc
            with open(part) as f:
                rows.append(json.load(f))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(cases=rows), f, indent=1)
    print("| coefficients | log2 m | dg16_groth16_setup ms | dg16_groth16_setup_srs ms | ratio | terms | without multiplication |"
          " lane / wave / MSM terms |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        lane = sum(p["lane"] for p in r["terms_per_path"].values())
        wave = sum(p["wave"] for p in r["terms_per_path"].values())
        msm = sum(p["msm"] for p in r["terms_per_path"].values())
        print("| %s | %d | %.1f | %.1f | %.1f | %d | %.1f %% | %d / %d / %d |"
              % ("+-1" if r["case"] == "pm1" else "full-width", r["log_m"], r["setup_ms"], r["setup_srs_ms"], r["ratio"],
                 r["terms"], 100 * r["share_without_multiplication"], lane, wave, msm))
    return 0


if __name__ == "__main__":
    sys.exit(main())
