"""Times the Libsnark QAP reduction next to the circom one on one GPU at m = 2^log_m (default 2^20, BN254):

    h_poly   dg16_h_poly without and with DG16_F_QAP_LIBSNARK (six transforms + one pointwise pass | seven + one)
    qap      dg16_qap | dg16_qap_r1cs with the violation count (two matrices | three and one more product per row)
    queue    a queue of proofs with DG16_F_OVERLAP_TAIL under each reduction (dg16_qap / dg16_qap_r1cs + dg16_groth16_prove
             per proof, setup with the matching h_query), time per proof

The expectation is the circom figure of the SAME run.  Each step is a fresh child process with a time limit of its own;
the first step that fails or runs out of time ends the run.

    python tools/libsnark_timing.py [--log-m 20] [--reps 5] [--out profiles/libsnark_timing.json]

Prints a markdown table (the one in DESIGN.md section 2.8) and writes the JSON, with the box's calibration line."""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = (("calibration", 120), ("h_poly", 180), ("qap", 180), ("queue", 420))
CURVE = "bn254"


def satisfied_instance(ctx, dev, log_m, seed):
    """3 non-zeros per row of A and B over the free wires, constraint i's output wire has the C row [(1, out_i)] and the
    value <A_i, w> <B_i, w> (taken from dg16_qap's c_out).  Montgomery form throughout.  -> system, w."""
    import numpy as np
    import torch
    import bench
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    m, ni = 1 << log_m, 2
    nc = m - ni
    free = min(1 << 16, max(m // 4, 4))
    nv = free + nc
    ptr3 = (torch.arange(nc + 1, dtype=torch.int64, device=dev) * 3).to(torch.int32)
    a_col = torch.randint(0, free, (3 * nc,), dtype=torch.int32, device=dev, generator=gen)
    b_col = torch.randint(0, free, (3 * nc,), dtype=torch.int32, device=dev, generator=gen)
    a_val, b_val = bench.rand_fr(3 * nc, dev, gen, CURVE), bench.rand_fr(3 * nc, dev, gen, CURVE)
    ptr1 = torch.arange(nc + 1, dtype=torch.int32, device=dev)
    c_col = (torch.arange(nc, dtype=torch.int64, device=dev) + free).to(torch.int32)
    one = np.array([[1, 0, 0, 0]], dtype=np.uint64)
    one = torch.from_numpy(ctx.field_op(CURVE, "fr", "to_mont", one).view(np.int64)).to(dev)
    c_val = one.repeat(nc, 1).contiguous()
    w = torch.zeros((nv, 4), dtype=torch.int64, device=dev)
    w[:free] = bench.rand_fr(free, dev, gen, CURVE)
    w[0] = one[0]
    abc = [torch.empty((m, 4), dtype=torch.int64, device=dev) for _ in range(3)]
    torch.cuda.synchronize()
    ctx.qap_dev(CURVE, nc, ni, nv, log_m, ptr3.data_ptr(), a_col.data_ptr(), a_val.data_ptr(), ptr3.data_ptr(),
                b_col.data_ptr(), b_val.data_ptr(), w.data_ptr(), *[t.data_ptr() for t in abc])
    ctx.sync(0)
    w[free:] = abc[2][:nc]
    torch.cuda.synchronize()
    system = dict(num_constraints=nc, num_inputs=ni, num_vars=nv, a=(ptr3, a_col, a_val), b=(ptr3, b_col, b_val),
                  c=(ptr1, c_col, c_val))
    return system, w


def median_ms(ctx, fn, reps):
    fn()
    ctx.sync(0)
    out = []
    for _ in range(reps):
        fn()
        ctx.sync(0)
        out.append(ctx.last_kernel_ms(0, 0))
    return statistics.median(out)


def step(name, log_m, reps):
    import torch
    import dg16_amd
    import bench
    if name == "calibration":
        return bench.calibrate(0)
    ctx = dg16_amd.Context(0)
    dev = torch.device("cuda", 0)
    m = 1 << log_m
    system, w = satisfied_instance(ctx, dev, log_m, seed=log_m)
    nc, ni, nv = system["num_constraints"], system["num_inputs"], system["num_vars"]
    mats = [t.data_ptr() for k in "abc" for t in system[k]]
    abc = [torch.empty((m, 4), dtype=torch.int64, device=dev) for _ in range(3)]
    viol = torch.zeros(2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def qap_circom():
        ctx.qap_dev(CURVE, nc, ni, nv, log_m, *mats[:6], w.data_ptr(), *[t.data_ptr() for t in abc])

    def qap_r1cs():
        ctx.qap_r1cs_dev(CURVE, nc, ni, nv, log_m, mats, w.data_ptr(), *[t.data_ptr() for t in abc],
                         violations_ptr=viol.data_ptr())

    if name == "qap":
        res = dict(dg16_qap_ms=median_ms(ctx, qap_circom, reps), dg16_qap_r1cs_ms=median_ms(ctx, qap_r1cs, reps))
        assert [int(x) for x in viol.cpu()] == [0, -1], "the timed witness satisfies the system"
        return res
    if name == "h_poly":
        qap_r1cs()
        ctx.sync(0)
        h = torch.empty((m, 4), dtype=torch.int64, device=dev)
        p = [t.data_ptr() for t in abc]
        return dict(circom_ms=median_ms(ctx, lambda: ctx.h_poly_dev(CURVE, *p, log_m, h.data_ptr()), reps),
                    libsnark_ms=median_ms(ctx, lambda: ctx.h_poly_dev(CURVE, *p, log_m, h.data_ptr(), reduction="libsnark"),
                                          reps))
    assert name == "queue"
    import numpy as np
    rs = np.array([[3, 0, 0, 0], [5, 0, 0, 0]], dtype=np.uint64)
    out = dict()
    for red, qap in (("circom", qap_circom), ("libsnark", qap_r1cs)):
        params = dg16_amd.generate_parameters(ctx, CURVE, system, reduction=red)
        pk = params.proving_key(ctx)
        del params
        torch.cuda.empty_cache()
        proof = torch.empty(12 * 32, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

        def one():
            qap()
            ctx.prove_dev(pk, abc[0].data_ptr(), abc[1].data_ptr(), abc[2].data_ptr(), w.data_ptr(), rs, proof.data_ptr(),
                          scalars_mont=True, overlap_tail=True, reduction=red)

        for _ in range(2):
            one()
        for ch in range(3):
            ctx.sync(ch)
        n = max(reps, 3) * 4
        t0 = time.perf_counter()
        for _ in range(n):
            one()
        for ch in (0, 2):
            ctx.sync(ch)
        out["%s_ms_per_proof" % red] = 1e3 * (time.perf_counter() - t0) / n
        pk.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-m", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "libsnark_timing.json"))
    ap.add_argument("--step", default=None, help="(internal) run one step in this process and print its JSON")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step(a.step, a.log_m, a.reps)))
        return 0
    res = dict(curve=CURVE, log_m=a.log_m, reps=a.reps)
    for name, limit in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--log-m", str(a.log_m), "--reps",
                                str(a.reps)], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print("step %s ran out of its %d s: stopping" % (name, limit), file=sys.stderr)
            return 1
        line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print("step %s failed (exit %d): stopping\n%s" % (name, r.returncode, r.stderr[-2000:]), file=sys.stderr)
            return 1
        res[name] = json.loads(line[-1][7:])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    h, q, u = res["h_poly"], res["qap"], res["queue"]
    print("| m = 2^%d, %s | circom | Libsnark | ratio |" % (a.log_m, CURVE))
    print("|---|---|---|---|")
    print("| dg16_h_poly ms | %.3f | %.3f | %.2f |" % (h["circom_ms"], h["libsnark_ms"], h["libsnark_ms"] / h["circom_ms"]))
    print("| dg16_qap / dg16_qap_r1cs ms | %.3f | %.3f | %.2f |" % (q["dg16_qap_ms"], q["dg16_qap_r1cs_ms"],
                                                                  q["dg16_qap_r1cs_ms"] / q["dg16_qap_ms"]))
    print("| queued proof ms | %.3f | %.3f | %.2f |" % (u["circom_ms_per_proof"], u["libsnark_ms_per_proof"],
                                                       u["libsnark_ms_per_proof"] / u["circom_ms_per_proof"]))
    print("calibration: %s" % json.dumps(res["calibration"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
