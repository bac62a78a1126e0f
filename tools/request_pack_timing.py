#!/usr/bin/env python3
"""Times the packing of one proof request into party shares: dg16_request_pack (csrc/pss_scalars.h) against the numpy
composition it replaces (groth16_mpc.qap_pss + two pack_from_witness: bit reversal and re-striding on the host,
dg16_pss_apply, a slice per party on the host).

  request      m = 2^20 on BN254 (num_vars = m, 3 inputs), l = 2 and l = 8, without and with a seed.  The values are
               random field elements -- neither path's cost depends on them.
  whole call   host clock around the synchronous call, copies included on both sides, median of 3 after one warm-up of
               each; the two paths alternate in one process.  The plain result is compared byte for byte with the
               composition's at the timed size.
  kernel       the packing kernel of one vector alone, by the library's events (dg16_last_kernel_ms, which = 1: the
               kernel of the call's LAST slice; a vector of 2^20 is two equal slices at the default setting, so a
               vector's kernel time is that figure times the slice count): a DFFT vector of m values plain and with
               uploaded blinds (dg16_pss_pack_scalars), and the last vector of a seeded request (blinds made in the
               kernel).  Beside it the bytes the kernels move -- m values in, 4 m shares out, m blinds in for the
               uploaded form -- and the share of the HBM roof (8 TB/s) that is.
  host copies  what is left of the whole call after five kernels: uploads, the strided copies out and their waits.

Every step is a child process under its own time limit, and the first failure stops the run:

    python3 tools/request_pack_timing.py [--out profiles/request_pack_timing.json]
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

CURVE = "bn254"
LOG_M = 20
LS = (2, 8)
STEP_LIMIT_S = 420
HBM_ROOF_GBS = 8000.0
SEED = bytes(range(32))


def _ms(call):
    t0 = time.perf_counter()
    out = call()
    return 1e3 * (time.perf_counter() - t0), out


def _random_fr(rng, n):
    """n field elements below 2^253 (so below r), as Montgomery-form words for all the two paths care"""
    a = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 61) - 1)
    return a


def step(l, log_m):
    import dg16_amd
    from dg16_amd import dist as D
    from dg16_amd import groth16_mpc as M
    ctx = dg16_amd.Context(0)
    pp = D.PackedSharingParams(ctx, CURVE, l)
    m = 1 << log_m
    num_vars, num_inputs = m, 3
    rng = np.random.default_rng(20 + l)
    a, b, c, w = (_random_fr(rng, n) for n in (m, m, m, num_vars))

    def old():
        return M.qap_pss(pp, a, b, c), M.pack_from_witness(pp, w[1:]), M.pack_from_witness(pp, w[num_inputs:])

    new = lambda seed: M.pack_request(pp, a, b, c, w, num_inputs, seed=seed)      # noqa: E731
    want, got = old(), new(None)                                                   # warm-ups
    for i in range(pp.n):
        assert all(np.array_equal(got[i][0][k], want[0][i][k]) for k in range(3)), "a, b, c differ from qap_pss"
        assert np.array_equal(got[i][1], want[1][i]) and np.array_equal(got[i][2], want[2][i]), "witness shares differ"
    del want, got
    new(SEED)
    t_old, t_plain, t_seed = [], [], []
    for _ in range(3):
        t_plain.append(_ms(lambda: new(None))[0])
        t_old.append(_ms(old)[0])
        t_seed.append(_ms(lambda: new(SEED))[0])
    m_old, m_plain, m_seed = (statistics.median(t) for t in (t_old, t_plain, t_seed))
    print("  l=%d 2^%d: request_pack %.1f ms plain, %.1f ms seeded; numpy composition %.1f ms"
          % (l, log_m, m_plain, m_seed, m_old), file=sys.stderr, flush=True)

    # one vector's kernels alone: the last slice's, times the slices (pss_scalars.h: slice_chunks at 2^21 outputs)
    per = max(64, (1 << 21) // pp.n // 64 * 64)
    slices = -(-(m // l) // per)
    blinds = _random_fr(rng, m)
    kern = {}
    for name, call in (("plain", lambda: pp.pack_scalars(a, D.PACK_DFFT)),
                       ("uploaded_blinds", lambda: pp.pack_scalars(a, D.PACK_DFFT, blinds)),
                       ("seeded", lambda: new(SEED))):
        ms = []
        for _ in range(4):
            call()
            ms.append(ctx.last_kernel_ms(0, 1))
        k_ms = statistics.median(ms[1:]) * slices
        moved = 32 * (m + pp.n * (m // l) + (m if name == "uploaded_blinds" else 0))
        kern[name] = {"kernel_ms": k_ms, "slices": slices, "bytes_moved": moved, "gb_per_s": moved / k_ms / 1e6,
                      "hbm_roof_share": moved / k_ms / 1e6 / HBM_ROOF_GBS}
    out_bytes = 32 * pp.n * (3 * (m // l) + -(-(num_vars - 1) // l) + -(-(num_vars - num_inputs) // l))
    return {"curve": CURVE, "l": l, "log_m": log_m, "num_vars": num_vars, "num_inputs": num_inputs,
            "bytes_in": 32 * (3 * m + num_vars), "bytes_out": out_bytes,
            "request_pack_ms": m_plain, "request_pack_seeded_ms": m_seed, "numpy_composition_ms": m_old,
            "ratio": m_plain / m_old, "ratio_seeded": m_seed / m_old, "seeded_over_plain": m_seed / m_plain,
            "kernel": kern,
            "host_copy_share": 1 - 5 * kern["plain"]["kernel_ms"] / m_plain,
            "host_copy_share_seeded": 1 - 5 * kern["seeded"]["kernel_ms"] / m_seed}


def table(res):
    lines = ["| l | request_pack ms | seeded ms | numpy composition ms | ratio | ratio, seeded | kernel ms per vector (plain / "
             "uploaded blinds / seeded) | HBM roof share (plain) | host-copy share (plain / seeded) |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in res["steps"].values():
        k = r["kernel"]
        lines.append("| %d | %.1f | %.1f | %.1f | %.3f | %.3f | %.3f / %.3f / %.3f | %.3f | %.3f / %.3f |" % (
            r["l"], r["request_pack_ms"], r["request_pack_seeded_ms"], r["numpy_composition_ms"], r["ratio"],
            r["ratio_seeded"], k["plain"]["kernel_ms"], k["uploaded_blinds"]["kernel_ms"], k["seeded"]["kernel_ms"],
            k["plain"]["hbm_roof_share"], r["host_copy_share"], r["host_copy_share_seeded"]))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "request_pack_timing.json"))
    ap.add_argument("--log-m", type=int, default=LOG_M)
    ap.add_argument("--step", help="(internal) run one step in this process: l:log_m")
    args = ap.parse_args()
    if args.step:
        l, log_m = args.step.split(":")
        print("RESULT " + json.dumps(step(int(l), int(log_m))))
        return
    res = {"hbm_roof_gb_per_s": HBM_ROOF_GBS, "steps": {}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for l in LS:
        name = "%d:%d" % (l, args.log_m)
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], stdout=subprocess.PIPE,
                               text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print("step %s exceeded %d s: stopping" % (name, STEP_LIMIT_S), flush=True)
            sys.exit(124)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print("step %s failed (status %d): stopping\n%s" % (name, p.returncode, p.stdout[-2000:]), flush=True)
            sys.exit(1)
        res["steps"]["%s_l%d_2^%d" % (CURVE, l, args.log_m)] = json.loads(line[-1][7:])
        print("step %s done" % name, flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(table(res))


if __name__ == "__main__":
    main()
