#!/usr/bin/env python3
"""Times the batched point multiplication (dg16_points_mul) and proof re-randomization (dg16_groth16_rerandomize), and
beside every figure a call that bounds it from one side, taken in the SAME process:

  points_mul    n in {2^10, 2^16, 2^20} for BN254 G1 / G2, BLS12-381 G1 / G2 and BLS12-377 G1, with and without
                DG16_F_BASES_IN_SUBGROUP; beside it dg16_fixed_base_mul at the same n and group (no doublings: a floor
                for what a product can cost)
  rerandomize   n_proofs in {1, 1 024, 65 536} on BN254 and BLS12-381; beside it dg16_groth16_verify_batch at the same
                n_proofs (re-randomizing should be a small fraction of verifying).  The re-randomized family is checked to
                be accepted by the batch verifier.
  dbl_add       ec.h's per-lane double-and-add scalar_mul (what the verifier's kernels use today) wrapped in a throwaway
                kernel that this tool compiles for itself -- it is not part of the library -- at n = 2^16 per group

Device pointers; the whole call between the HIP events the library records on the channel's stream
(dg16_last_kernel_ms), torch events around the throwaway kernel; median of 3 after one warm-up call.  Points come from
dg16_gen_bases on the device; the proof family is one valid proof (made from trapdoor scalars, as
tools/verify_aggregate_timing.py does) re-randomized on the device under n different (r1, r2).

Every step is a child process under its own time limit, and the first failure stops the run:

    python3 tools/points_mul_timing.py [--out profiles/points_mul_timing.json] [--cache-dir DIR]
"""

import argparse
import ctypes
import hashlib
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

R = {"bn254": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
     "bls12_381": 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001}
GROUPS = (("bn254", 1), ("bn254", 2), ("bls12_381", 1), ("bls12_381", 2), ("bls12_377", 1))
SIZES = (1 << 10, 1 << 16, 1 << 20)
PROOFS = (1, 1024, 65536)
FQ64 = {"bn254": 4, "bls12_381": 6, "bls12_377": 6}
CURVE_ID = {"bn254": 0, "bls12_381": 1, "bls12_377": 2}
STEP_LIMIT_S = {"points_mul": 240, "rerandomize": 240, "dbl_add": 300}

DBL_ADD_SRC = r"""
// throwaway: ec.h's per-lane double-and-add, one product per lane, XYZZ out (no conversion to affine)
#include "types.h"
using namespace dg16;
template <class F>
__global__ void __launch_bounds__(64) dbl_add_kernel(const Affine<F>* p, const uint32_t* k, size_t n, XYZZ<F>* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = scalar_mul<F, 8>(XYZZ<F>::from_affine(p[i]), k + 8 * i);
}
template <class F>
static void go(const void* p, const void* k, size_t n, void* out, hipStream_t s) {
  hipLaunchKernelGGL(dbl_add_kernel<F>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, (const Affine<F>*)p,
                     (const uint32_t*)k, n, (XYZZ<F>*)out);
}
extern "C" int dbl_add_launch(int gid, const void* p, const void* k, size_t n, void* out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  switch (gid) {
    case 0: go<CurveTypes<0>::Fq>(p, k, n, out, s); break;
    case 1: go<CurveTypes<0>::Fq2>(p, k, n, out, s); break;
    case 2: go<CurveTypes<1>::Fq>(p, k, n, out, s); break;
    case 3: go<CurveTypes<1>::Fq2>(p, k, n, out, s); break;
    case 4: go<CurveTypes<2>::Fq>(p, k, n, out, s); break;
    default: return 1;
  }
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
"""


def _scalars(vals):
    return np.stack([np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint64) for v in vals])


def random_scalars(n, seed):
    """n x 4 uint64 below 2^252: canonical on all three curves."""
    k = np.random.default_rng(seed).integers(0, 1 << 63, size=(n, 4), dtype=np.uint64, endpoint=False)
    k[:, 3] &= np.uint64((1 << 60) - 1)
    return k


def _median_ms(ctx, call, reps=3):
    call()                                   # warm-up (workspace growth, code load)
    ctx.sync(0)
    ms = []
    for _ in range(reps):
        call()
        ctx.sync(0)
        ms.append(ctx.last_kernel_ms(0, 0))
    return statistics.median(ms)


def step_points_mul(ctx, curve, group):
    import torch
    dev = torch.device("cuda", ctx.device)
    words = FQ64[curve] * 2 * group
    out = []
    for n in SIZES:
        pts = torch.zeros(n * words, dtype=torch.int64, device=dev)
        res = torch.zeros_like(pts)
        ks = torch.from_numpy(random_scalars(n, 5).view(np.int64)).to(dev)
        torch.cuda.synchronize()
        ctx.gen_bases_dev(curve, group, 17, n, pts.data_ptr())
        ctx.sync(0)
        row = {"n": n}
        for flag in (False, True):
            ms = _median_ms(ctx, lambda: ctx.points_mul(curve, group, pts, ks, in_subgroup=flag, device=True, out=res, n=n))
            row["subgroup_ms" if flag else "plain_ms"] = ms
        row["fixed_base_ms"] = _median_ms(ctx, lambda: ctx.fixed_base_mul_dev(curve, group, ks.data_ptr(), n,
                                                                               res.data_ptr()))
        row["plain_us_per_product"] = 1e3 * row["plain_ms"] / n
        row["subgroup_us_per_product"] = 1e3 * row["subgroup_ms"] / n
        out.append(row)
        del pts, res, ks
    return out


def instance(ctx, curve, seed=7):
    """(vk arrays, public input row [1][4], proof row): a valid proof from trapdoor scalars, n_public = 1."""
    r = R[curve]
    rng = random.Random(seed)
    al, be, ga, de, a, b = (rng.randrange(1, r) for _ in range(6))
    u = [rng.randrange(1, r) for _ in range(2)]
    x = [rng.randrange(r)]
    acc = (u[0] + x[0] * u[1]) % r
    c = (a * b - al * be - ga * acc) * pow(de, r - 2, r) % r
    g1 = ctx.fixed_base_mul(curve, 1, _scalars([al, a, c] + u))
    g2 = ctx.fixed_base_mul(curve, 2, _scalars([be, ga, de, b]))
    vk = (g1[0], g2[0], g2[1], g2[2], g1[3:])
    return vk, _scalars(x), np.concatenate([g1[1], g2[3], g1[2]])


def step_rerandomize(ctx, curve):
    import torch
    from dg16_amd import verify
    dev = torch.device("cuda", ctx.device)
    up = lambda arr: torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to(dev)     # noqa: E731
    vk, pub, proof = instance(ctx, curve)
    pvk = verify.PreparedVerifyingKey(ctx, curve, *vk)
    out = []
    for n in PROOFS:
        rng = np.random.default_rng(23)
        rs = rng.integers(0, 1 << 63, size=(n, 2, 4), dtype=np.uint64, endpoint=False)
        rs[:, :, 3] &= np.uint64((1 << 60) - 1)
        rs[:, :, 0] |= np.uint64(1)                                # nonzero, below 2^252 < r
        family = up(np.repeat(proof[None, :], n, axis=0))
        d_rs, d_rs2 = up(rs), up(rs[::-1])
        res = torch.zeros_like(family)
        xs = up(np.repeat(pub[None, :, :], n, axis=0).reshape(n, -1))
        torch.cuda.synchronize()
        pvk.rerandomize(family, d_rs, device=True, n_proofs=n)                      # the family, in place
        ctx.sync(0)
        ms = _median_ms(ctx, lambda: pvk.rerandomize(family, d_rs2, device=True, n_proofs=n, out=res))
        assert pvk.verify_batch(xs, res, device=True, n_proofs=n).all(), "a re-randomized proof was rejected"
        ms_v = []
        for _ in range(3):
            assert pvk.verify_batch(xs, family, device=True, n_proofs=n).all()
            ms_v.append(ctx.last_kernel_ms(0, 0))
        out.append({"n_proofs": n, "rerandomize_ms": ms, "verify_batch_ms": statistics.median(ms_v),
                    "ratio": ms / statistics.median(ms_v)})
    pvk.close()
    return out


def build_dbl_add(cache_dir):
    csrc = os.path.join(ROOT, "distributed-groth16_amd", "csrc")
    tag = hashlib.sha256(DBL_ADD_SRC.encode()).hexdigest()[:12]
    so = os.path.join(cache_dir, "dbl_add_%s.so" % tag)
    if not os.path.exists(so):
        os.makedirs(cache_dir, exist_ok=True)
        src = os.path.join(cache_dir, "dbl_add_%s.hip" % tag)
        with open(src, "w") as f:
            f.write(DBL_ADD_SRC)
        subprocess.check_call(["/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc",
                               "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-I", csrc, src, "-o", so])
    return so


def step_dbl_add(ctx, cache_dir):
    import torch
    dev = torch.device("cuda", ctx.device)
    L = ctypes.CDLL(build_dbl_add(cache_dir))
    vp = ctypes.c_void_p
    L.dbl_add_launch.argtypes = [ctypes.c_int, vp, vp, ctypes.c_size_t, vp, vp]
    n = 1 << 16
    out = []
    for gid, (curve, group) in enumerate(GROUPS):
        words = FQ64[curve] * 2 * group
        pts = torch.zeros(n * words, dtype=torch.int64, device=dev)
        acc = torch.zeros(2 * n * words, dtype=torch.int64, device=dev)
        res = torch.zeros_like(pts)
        ks = torch.from_numpy(random_scalars(n, 5).view(np.int64)).to(dev)
        torch.cuda.synchronize()
        ctx.gen_bases_dev(curve, group, 17, n, pts.data_ptr())
        ctx.sync(0)
        stream = torch.cuda.current_stream(dev)
        ms = []
        for rep in range(4):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            rc = L.dbl_add_launch(gid if gid < 4 else 4, pts.data_ptr(), ks.data_ptr(), n, acc.data_ptr(),
                                  ctypes.c_void_p(stream.cuda_stream))
            e1.record(stream)
            assert rc == 0
            torch.cuda.synchronize()
            if rep:
                ms.append(e0.elapsed_time(e1))
        pm = _median_ms(ctx, lambda: ctx.points_mul(curve, group, pts, ks, device=True, out=res, n=n))
        out.append({"curve": curve, "group": group, "n": n, "dbl_add_ms": statistics.median(ms), "points_mul_plain_ms": pm})
    return out


def run_step(name, cache_dir):
    import dg16_amd
    ctx = dg16_amd.Context(0)
    kind, _, arg = name.partition(":")
    if kind == "points_mul":
        curve, group = arg.rsplit("_g", 1)
        res = step_points_mul(ctx, curve, int(group))
    elif kind == "rerandomize":
        res = step_rerandomize(ctx, arg)
    elif kind == "dbl_add":
        res = step_dbl_add(ctx, cache_dir)
    else:
        name_buf = ctypes.create_string_buffer(128)
        cus = ctypes.c_int(0)
        ctx.L.dg16_device_info(ctx.h, name_buf, 128, ctypes.byref(cus))
        res = {"name": name_buf.value.decode(), "compute_units": cus.value}
    print("RESULT " + json.dumps(res))


def table(res):
    lines = ["| group | n | plain ms | us / product | subgroup ms | us / product | fixed-base ms |", "|---|---|---|---|---|---|---|"]
    for key, rows in res.get("points_mul", {}).items():
        for p in rows:
            lines.append("| %s | %d | %.2f | %.3f | %.2f | %.3f | %.2f |" % (
                key, p["n"], p["plain_ms"], p["plain_us_per_product"], p["subgroup_ms"], p["subgroup_us_per_product"],
                p["fixed_base_ms"]))
    lines += ["", "| curve | n_proofs | rerandomize ms | verify_batch ms | ratio |", "|---|---|---|---|---|"]
    for curve, rows in res.get("rerandomize", {}).items():
        for p in rows:
            lines.append("| %s | %d | %.2f | %.2f | %.3f |" % (curve, p["n_proofs"], p["rerandomize_ms"],
                                                              p["verify_batch_ms"], p["ratio"]))
    lines += ["", "| group | n | double-and-add ms | points_mul (plain) ms |", "|---|---|---|---|"]
    for p in res.get("dbl_add", []):
        lines.append("| %s g%d | %d | %.2f | %.2f |" % (p["curve"], p["group"], p["n"], p["dbl_add_ms"],
                                                       p["points_mul_plain_ms"]))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_mul_timing.json"))
    ap.add_argument("--cache-dir", default=os.path.join(tempfile.gettempdir(), "dg16_points_mul_timing"),
                    help="where the throwaway double-and-add kernel is compiled (reused when present)")
    ap.add_argument("--step", help="(internal) run one step in this process")
    args = ap.parse_args()
    if args.step:
        run_step(args.step, args.cache_dir)
        return
    steps = ["device"] + ["points_mul:%s_g%d" % g for g in GROUPS] + ["rerandomize:bn254", "rerandomize:bls12_381",
                                                                      "dbl_add"]
    res = {"points_mul": {}, "rerandomize": {}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for step in steps:
        limit = STEP_LIMIT_S.get(step.partition(":")[0], 60)
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--cache-dir", args.cache_dir],
                               capture_output=True, text=True, timeout=limit)
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
