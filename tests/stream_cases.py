"""The stream-order contract of include/dg16.h ("device-pointer calls are stream-ordered on the channel's stream -- use
dg16_sync or the stream you installed with dg16_set_stream"), as test cases: shared by tests/test_gpu_stream_order.py and
tests/test_stream_table.py.  No test functions here.

The delayed producer.  On a caller-owned stream S, installed on the channel with dg16_set_stream, a sleep kernel runs and
then a device-to-device copy puts the REAL input into the buffer the call reads.  Until then the buffer holds a DECOY: a
different but valid input of the same shape (reduced field elements, points of the subgroup, the same CSR structure), so a
call that reads too early computes the decoy's answer and never indexes out of range.  Index arrays (row_ptr, col) and
HOST-pointer arguments are never delayed.

The consumer.  Right after the call, with no dg16_sync, the output is copied to a snapshot on the stream the contract
orders it on and then overwritten on that stream; only the snapshot is compared, with the oracle, after one final
synchronisation.  A call that left its output on a stream that is not joined back shows the pattern or the overwrite.

Every expected value comes from the C oracle (oracle.corc) or from Python integers (oracle.pyref, the model of
tests/test_libsnark_model.py); the decoy's answer is computed only for the control (`Env.find_stream`)."""

import ctypes
import random
import time

import numpy as np

from oracle import corc

F_MONT, F_DEV, F_AFFINE, F_SUBGROUP, F_LIBSNARK = 1, 2, 4, 64, 128
BEFORE, AFTER = 0xA5, 0x5A          # fill of an output before the call / the consumer's overwrite after the snapshot
MIN_DELAY_MS = 25.0
CONTROL_N = 4096
U64_MAX = 2 ** 64 - 1

# Pointers that stay HOST pointers with DG16_F_DEVICE_PTRS (include/dg16.h): read before the call returns, never delayed.
HOST_POINTERS = ("r_s", "coset_offset", "base", "trapdoor", "generators", "srs->fixed")


def u8(x):
    return np.ascontiguousarray(x).view(np.uint8).reshape(-1)


def to_dev(x, dev):
    """numpy array or device tensor -> a flat uint8 tensor of its own on `dev`."""
    import torch
    if isinstance(x, np.ndarray):
        return torch.from_numpy(u8(x).copy()).to(dev)
    return x.contiguous().view(torch.uint8).reshape(-1).clone()


class Spec:
    """What one row's `make` returns.  inputs: name -> (real, decoy), delayed; static: name -> array, resident before the
    call (index arrays, undelayed operands); outputs: name -> byte count, or None when the name is an input that the call
    transforms in place; call(ctx, channel, p) with p[name] the device pointers; check(out) with out[name] the snapshot
    bytes; prepare(env, p) once, before the warm-up (resident handles: its result is p["handle"]); close(p)."""

    def __init__(self, inputs, outputs, call, check, static=None, prepare=None, close=None, out_channel=None):
        self.inputs, self.outputs, self.call, self.check = inputs, outputs, call, check
        self.static, self.prepare, self.close, self.out_channel = static or {}, prepare, close, out_channel


class Row:
    """One entry point (or a chain of them) that takes DG16_F_DEVICE_PTRS.  entries: the C functions it runs; channels:
    where the test installs the caller's stream and runs it -- (0, 1, 2) for the single-channel calls, (0,) for those that
    use all three or have no `channel` argument; host: which arguments are HOST pointers by contract."""

    def __init__(self, name, entries, channels, make, host=()):
        assert all(h in HOST_POINTERS for h in host)
        self.name, self.entries, self.channels, self.make, self.host = name, tuple(entries), tuple(channels), make, host
        self._spec = None

    def spec(self):
        if self._spec is None:
            self._spec = self.make()
        return self._spec


# ---- the harness -------------------------------------------------------------------------------------------------------
class Env:
    """A context of its own, the device, the caller's stream S found by the control, and the sleep calibration."""

    def __init__(self, ctx, dev):
        self.ctx, self.dev = ctx, dev
        self.S = None
        self.streams = []            # every candidate stays alive: a new stream then lands on another hardware queue
        self.ms_per_cycle = None
        self.bufs = {}               # row name -> device buffers
        self.control_verdict = None

    def calibrate(self, S, cycles=10_000_000):
        """Milliseconds per unit of torch.cuda._sleep on stream S, measured with two events."""
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(S):
            torch.cuda._sleep(1000)
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
        S.synchronize()
        return e0.elapsed_time(e1) / cycles

    def sleep(self, S, ms):
        """Enqueues a sleep of about `ms` milliseconds on S; returns (e0, e1), events around it."""
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(S):
            e0.record()
            torch.cuda._sleep(max(int(ms / self.ms_per_cycle), 1))
            e1.record()
        return e0, e1

    def find_stream(self):
        """The control: a delay can tell something only if the library's OWN stream is not held up by the sleeping
        caller stream (they may share a hardware queue).  One field_op of CONTROL_N elements runs with the library left on
        its own stream while a candidate S sleeps in front of the copy of the real operand: it must return the DECOY's
        product.  Up to 8 candidates; the first for which this holds becomes S.  This is the only place where a stale read
        is expected, and it reads valid data."""
        import torch
        curve, n, ctx, dev = "bn254", CONTROL_N, self.ctx, self.dev
        a1, a0, b = (corc.rand_field(curve, "fr", s, n) for s in (901, 902, 903))
        want_real, want_decoy = corc.field_op(curve, "fr", "mul", a1, b), corc.field_op(curve, "fr", "mul", a0, b)
        assert not np.array_equal(want_real, want_decoy)
        real, decoy, bt = to_dev(a1, dev), to_dev(a0, dev), to_dev(b, dev)
        buf, out = decoy.clone(), torch.empty_like(decoy)
        torch.cuda.synchronize()
        ctx.field_op_dev(curve, "fr", 2, buf.data_ptr(), bt.data_ptr(), out.data_ptr(), n)     # warm
        ctx.sync(0)
        tried = []
        for i in range(8):
            S = torch.cuda.Stream(device=dev)
            self.streams.append(S)
            per = self.calibrate(S)
            self.ms_per_cycle = per
            buf.copy_(decoy)
            out.fill_(BEFORE)
            torch.cuda.synchronize()
            e0, e1 = self.sleep(S, MIN_DELAY_MS)
            with torch.cuda.stream(S):
                buf.copy_(real, non_blocking=True)
            ctx.field_op_dev(curve, "fr", 2, buf.data_ptr(), bt.data_ptr(), out.data_ptr(), n)  # on the library's stream
            ctx.sync(0)
            got = out.cpu().numpy().view(np.uint64).reshape(-1, 4)
            S.synchronize()
            slept = e0.elapsed_time(e1)
            if np.array_equal(got, want_decoy):
                self.S = S
                self.control_verdict = ("control: candidate %d of 8: the library's own stream ran under a %.1f ms sleep of "
                                        "the caller's stream and read the decoy (%.3g ms per sleep unit)" % (i, slept, per))
                print(self.control_verdict)
                return S
            assert np.array_equal(got, want_real), "the control's field_op returned neither the decoy's nor the real product"
            tried.append("candidate %d: held up (slept %.1f ms)" % (i, slept))
        raise AssertionError("the control found no caller stream whose sleep leaves the library's own stream running: "
                             "no delay on this machine can show a misordered read (%s)" % "; ".join(tried))

    def buffers(self, row):
        """Device buffers of a row, made once: the real and decoy inputs, the buffers the call reads, outputs, snapshots."""
        import torch
        if row.name in self.bufs:
            return self.bufs[row.name]
        sp, dev = row.spec(), self.dev
        b = dict(real={}, decoy={}, buf={}, out={}, snap={}, p={})
        for name, (real, decoy) in sp.inputs.items():
            b["real"][name], b["decoy"][name] = to_dev(real, dev), to_dev(decoy, dev)
            assert b["real"][name].numel() == b["decoy"][name].numel(), name
            assert not torch.equal(b["real"][name], b["decoy"][name]), "%s: the decoy equals the real input" % name
            b["buf"][name] = b["real"][name].clone()
            b["p"][name] = b["buf"][name].data_ptr()
        for name, arr in sp.static.items():
            b["buf"]["static:" + name] = to_dev(arr, dev)
            b["p"][name] = b["buf"]["static:" + name].data_ptr()
        for name, nbytes in sp.outputs.items():
            b["out"][name] = b["buf"][name] if nbytes is None else torch.empty(nbytes, dtype=torch.uint8, device=dev)
            b["snap"][name] = torch.empty_like(b["out"][name])
            b["p"][name] = b["out"][name].data_ptr()
        torch.cuda.synchronize()
        if sp.prepare is not None:
            b["p"]["handle"] = sp.prepare(self, b["p"])
        self.bufs[row.name] = b
        return b

    def close(self):
        for name, b in self.bufs.items():
            sp = ROWS_BY_NAME[name].spec()
            if sp.close is not None:
                sp.close(b["p"])
        self.bufs = {}


def run_delayed(env, row, channel=0, out_stream=None):
    """Warm-up, measured warm call, then: decoy in place, sleep + copy of the real input on S, the call, snapshot and
    overwrite on the output's stream, one final synchronisation, oracle check.  out_stream: a second caller stream
    installed on the row's out_channel (the overlapped proof's tail)."""
    import torch
    ctx, S, sp = env.ctx, env.S, row.spec()
    b = env.buffers(row)
    out_ch = channel if sp.out_channel is None else sp.out_channel
    So = S if out_ch == channel else out_stream
    ctx.set_stream(channel, S.cuda_stream)
    if out_ch != channel:
        ctx.set_stream(out_ch, So.cuda_stream)
    try:
        def load(which):
            for name in sp.inputs:
                b["buf"][name].copy_(b[which][name], non_blocking=True)

        def drain():
            S.synchronize()
            if So is not S:
                So.synchronize()

        with torch.cuda.stream(S):
            load("real")
        sp.call(ctx, channel, b["p"])            # warm-up: workspaces grow, twiddle sets are built (both synchronise)
        drain()
        with torch.cuda.stream(S):
            load("real")
        S.synchronize()
        t0 = time.perf_counter()
        sp.call(ctx, channel, b["p"])
        drain()
        warm_ms = (time.perf_counter() - t0) * 1e3
        delay_ms = max(MIN_DELAY_MS, 10.0 * warm_ms)
        load("decoy")
        for name, nbytes in sp.outputs.items():
            if nbytes is not None:
                b["out"][name].fill_(BEFORE)
            b["snap"][name].fill_(BEFORE)
        torch.cuda.synchronize()
        e0, e1 = env.sleep(S, delay_ms)
        with torch.cuda.stream(S):
            load("real")
        t0 = time.perf_counter()
        sp.call(ctx, channel, b["p"])
        host_ms = (time.perf_counter() - t0) * 1e3
        with torch.cuda.stream(So):
            for name in sp.outputs:
                b["snap"][name].copy_(b["out"][name], non_blocking=True)
                b["out"][name].fill_(AFTER)
        drain()
        print("%s on channel %d: warmed call %.2f ms, delay asked %.1f ms, slept %.1f ms, the call held the host %.1f ms"
              % (row.name, channel, warm_ms, delay_ms, e0.elapsed_time(e1), host_ms))
        sp.check({name: b["snap"][name].cpu().numpy() for name in sp.outputs})
    finally:
        ctx.set_stream(channel, None)
        if out_ch != channel:
            ctx.set_stream(out_ch, None)


# ---- helpers of the rows -------------------------------------------------------------------------------------------------
CURVE = "bn254"


def fr(seed, n, curve=CURVE, mont=True):
    return corc.rand_field(curve, "fr", seed, n, mont=mont)


def as_u64(x, cols):
    return np.ascontiguousarray(x).view(np.uint64).reshape(-1, cols)


def same(got, want, what):
    assert np.array_equal(u8(got), u8(want)), "%s differs from the oracle's" % what


def jac_affine(curve, group, out):
    return corc.jac_to_affine(curve, group, np.ascontiguousarray(out).view(np.uint64))


def points_as_ints(curve, arr):
    """G1 affine Montgomery array -> [(x, y)] Python integers."""
    nl = corc.limbs_of(curve, "fq")
    flat = corc.field_op(curve, "fq", "from_mont", np.ascontiguousarray(arr).reshape(-1, nl))
    v = corc.arr_to_ints(flat)
    return [(v[2 * i], v[2 * i + 1]) for i in range(len(v) // 2)]


# ---- rows: field arithmetic, NTT, h-polynomial ---------------------------------------------------------------------------
def make_field_op():
    n = 5000
    a1, a0, b1, b0 = (fr(s, n) for s in (11, 12, 13, 14))
    want = corc.field_op(CURVE, "fr", "mul", a1, b1)
    return Spec(dict(a=(a1, a0), b=(b1, b0)), dict(out=32 * n),
                lambda ctx, ch, p: ctx.field_op_dev(CURVE, "fr", 2, p["a"], p["b"], p["out"], n, channel=ch),
                lambda out: same(out["out"], want, "a * b"))


def make_ntt(inverse, coset):
    def make():
        log_n = 10
        x1, x0 = fr(21, 1 << log_n), fr(22, 1 << log_n)
        g = fr(23, 1) if coset else None
        want = corc.ntt(CURVE, x1, inverse=inverse, coset=g)
        return Spec(dict(data=(x1, x0)), dict(data=None),
                    lambda ctx, ch, p: ctx.ntt_dev(CURVE, p["data"], log_n, inverse=inverse, coset=g, channel=ch),
                    lambda out: same(out["data"], want, "the transform"))
    return make


def make_h_poly(reduction):
    def make():
        log_m = 10
        m = 1 << log_m
        if reduction == "circom":
            ins = {k: (fr(30 + i, m), fr(40 + i, m)) for i, k in enumerate("abc")}
            want = corc.h_poly(CURVE, *(ins[k][0] for k in "abc"))
        else:
            import test_libsnark_model as M
            from oracle.pyref.fields import FR
            from oracle.pyref.poly import Domain
            F = FR[CURVE]
            rng = random.Random(5)
            enc = lambda v: corc.field_op(CURVE, "fr", "to_mont", corc.ints_to_arr(v, 4))     # noqa: E731
            vecs = []
            for _ in range(2):        # c = a o b on every row: a satisfied system's vectors, for the decoy as well
                a = [rng.randrange(F.p) for _ in range(m)]
                bb = [rng.randrange(F.p) for _ in range(m)]
                vecs.append((a, bb, [x * y % F.p for x, y in zip(a, bb)]))
            want = enc(M.libsnark_h(*vecs[0], Domain(F, m)))
            ins = {k: (enc(vecs[0][i]), enc(vecs[1][i])) for i, k in enumerate("abc")}
        return Spec(ins, dict(out=32 * m),
                    lambda ctx, ch, p: ctx.h_poly_dev(CURVE, p["a"], p["b"], p["c"], log_m, p["out"], channel=ch,
                                                      reduction=reduction),
                    lambda out: same(out["out"], want, "h (%s)" % reduction))
    return make


# ---- rows: R1CS x witness ------------------------------------------------------------------------------------------------
def _synthetic_csr(log_m, seed, nnz=3):
    m = 1 << log_m
    nc, ni, nv = m - 2, 2, m
    rng = np.random.RandomState(seed)
    row_ptr = (np.arange(nc + 1, dtype=np.uint32) * nnz).astype(np.uint32)
    cols = [rng.randint(0, nv, nc * nnz).astype(np.uint32) for _ in range(2)]
    return m, nc, ni, nv, row_ptr, cols


def make_qap(rows):
    def make():
        log_m = 10
        m, nc, ni, nv, row_ptr, (a_col, b_col) = _synthetic_csr(log_m, 3)
        nz = a_col.shape[0]
        real = [fr(50, nz), fr(51, nz), fr(52, nv)]
        decoy = [fr(53, nz), fr(54, nz), fr(55, nv)]
        a, b, c = corc.qap(CURVE, nc, ni, m, (row_ptr, a_col, real[0]), (row_ptr, b_col, real[1]), real[2])
        start, stride = (1, 4) if rows else (0, 1)
        want = dict(a_out=a[start::stride], b_out=b[start::stride], c_out=c[start::stride])

        def call(ctx, ch, p):
            args = (CURVE, nc, ni, nv, log_m, p["row_ptr"], p["a_col"], p["a_val"], p["row_ptr"], p["b_col"], p["b_val"],
                    p["w"])
            outs = (p["a_out"], p["b_out"], p["c_out"])
            if rows:
                ctx.qap_rows_dev(*args, start, stride, *outs, scalars_mont=True, channel=ch)
            else:
                ctx.qap_dev(*args, *outs, scalars_mont=True, channel=ch)

        def check(out):
            for k in want:
                same(out[k], want[k], k)

        return Spec(dict(a_val=(real[0], decoy[0]), b_val=(real[1], decoy[1]), w=(real[2], decoy[2])),
                    {k: 32 * m // stride for k in want}, call, check,
                    static=dict(row_ptr=row_ptr, a_col=a_col, b_col=b_col))
    return make


def make_qap_r1cs():
    import test_libsnark_model as M
    from oracle.pyref.fields import FR
    F = FR[CURVE]
    log_m = 10
    m = 1 << log_m
    r1cs, w = M.instance(F, m, seed=61)
    a, b, c, dom = M.libsnark_abc(r1cs, w, F)
    assert dom.size == m
    enc = lambda v: corc.field_op(CURVE, "fr", "to_mont", corc.ints_to_arr([x % F.p for x in v], 4))     # noqa: E731
    nc, ni = r1cs["num_constraints"], r1cs["num_instance"]
    nv = ni + r1cs["num_witness"]
    static, ins = {}, {}
    for j, k in enumerate("abc"):
        rows = r1cs[k]
        static[k + "_ptr"] = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
        static[k + "_col"] = np.array([i for r in rows for _, i in r], dtype=np.uint32)
        coeff = enc([cf for r in rows for cf, _ in r])
        ins[k + "_val"] = (coeff, fr(62 + j, coeff.shape[0]))
    ins["w"] = (enc(w), fr(66, nv))
    want = dict(a_out=enc(a), b_out=enc(b), c_out=enc(c), viol=np.array([0, U64_MAX], dtype=np.uint64))

    def call(ctx, ch, p):
        ctx.qap_r1cs_dev(CURVE, nc, ni, nv, log_m, [p[k + s] for k in "abc" for s in ("_ptr", "_col", "_val")], p["w"],
                         p["a_out"], p["b_out"], p["c_out"], violations_ptr=p["viol"], scalars_mont=True, channel=ch)

    def check(out):
        for k in want:
            same(out[k], want[k], k)

    return Spec(ins, dict(a_out=32 * m, b_out=32 * m, c_out=32 * m, viol=16), call, check, static=static)


# ---- rows: MSM, resident bases, point arithmetic ---------------------------------------------------------------------------
def make_msm(curve, group, n, in_subgroup):
    def make():
        bases, bases0 = corc.gen_points(curve, group, 70 + n, n), corc.gen_points(curve, group, 71 + n, n)
        sc, sc0 = fr(72, n, curve, mont=False), fr(73, n, curve, mont=False)
        want = corc.msm(curve, group, bases, sc)
        jac = 3 * corc.limbs_of(curve, "fq") * 8 * group
        return Spec(dict(bases=(bases, bases0), scalars=(sc, sc0)), dict(out=jac),
                    lambda ctx, ch, p: ctx.msm_dev(curve, group, p["bases"], p["scalars"], n, p["out"], channel=ch,
                                                   in_subgroup=in_subgroup),
                    lambda out: same(jac_affine(curve, group, out["out"]), want, "the MSM"))
    return make


def make_bases_upload():
    """dg16_bases_upload reads its bases on channel 0's stream and is synchronous; the MSM over the new table follows."""
    n = 1 << 10
    bases, bases0 = corc.gen_points(CURVE, 1, 80, n), corc.gen_points(CURVE, 1, 81, n)
    sc, sc0 = fr(82, n, mont=False), fr(83, n, mont=False)
    want = corc.msm(CURVE, 1, bases, sc)
    handles = []

    def call(ctx, ch, p):
        handles.append(ctx.bases_upload(CURVE, 1, p["bases"], n=n, device_ptrs=True))     # freed at the end: a free synchronises
        ctx.msm_resident_dev(handles[-1], p["scalars"], n, p["out"], channel=ch)

    def close(p):
        while handles:
            handles.pop().close()

    return Spec(dict(bases=(bases, bases0), scalars=(sc, sc0)), dict(out=96), call,
                lambda out: same(jac_affine(CURVE, 1, out["out"]), want, "the MSM over the uploaded table"), close=close)


def make_msm_resident():
    n = 1 << 10
    bases = corc.gen_points(CURVE, 1, 84, n)
    sc, sc0 = fr(85, n, mont=False), fr(86, n, mont=False)
    want = corc.msm(CURVE, 1, bases, sc)
    return Spec(dict(scalars=(sc, sc0)), dict(out=96),
                lambda ctx, ch, p: ctx.msm_resident_dev(p["handle"], p["scalars"], n, p["out"], channel=ch),
                lambda out: same(jac_affine(CURVE, 1, out["out"]), want, "the resident MSM"),
                prepare=lambda env, p: env.ctx.bases_upload(CURVE, 1, bases), close=lambda p: p["handle"].close())


def make_gen_bases():
    n, seed = 1000, 91
    want = corc.gen_points(CURVE, 1, seed, n)
    return Spec({}, dict(out=64 * n), lambda ctx, ch, p: ctx.gen_bases_dev(CURVE, 1, seed, n, p["out"], channel=ch),
                lambda out: same(out["out"], want, "the generated bases"))


def make_to_affine():
    n = 65
    mul = lambda a, b: corc.field_op(CURVE, "fq", "mul", a, b)     # noqa: E731

    def jacobian(seed):      # (x l^2, y l^3, l) for a random l per point
        pts = corc.gen_points(CURVE, 1, seed, n)
        lam = corc.rand_field(CURVE, "fq", seed + 1, n)
        lam2 = mul(lam, lam)
        return pts, np.concatenate([mul(pts[:, :4], lam2), mul(pts[:, 4:], mul(lam2, lam)), lam], axis=1)

    want, jac = jacobian(100)
    _, jac0 = jacobian(102)
    assert np.array_equal(corc.jac_to_affine(CURVE, 1, jac[0]), want[0:1])
    return Spec(dict(jac=(jac, jac0)), dict(out=64 * n),
                lambda ctx, ch, p: ctx._chk(ctx.L.dg16_to_affine(ctx.h, 0, 1, p["jac"], p["out"], n, F_DEV, ch)),
                lambda out: same(out["out"], want, "the affine points"))


def make_fixed_base_mul():
    n = 65
    sc, sc0 = fr(110, n, mont=False), fr(111, n, mont=False)
    base = corc.point_mul(CURVE, 1, corc.generator(CURVE, 1), 0x1234567)          # HOST pointer by contract
    want = np.concatenate([corc.point_mul(CURVE, 1, base, k) for k in corc.arr_to_ints(sc)])
    return Spec(dict(scalars=(sc, sc0)), dict(out=64 * n),
                lambda ctx, ch, p: ctx.fixed_base_mul_dev(CURVE, 1, p["scalars"], n, p["out"], base=base, channel=ch),
                lambda out: same(out["out"], want, "scalars[i] * base"))


def make_points_mul():
    n = 65
    pts, pts0 = corc.gen_points(CURVE, 1, 120, n), corc.gen_points(CURVE, 1, 121, n)
    sc, sc0 = fr(122, n, mont=False), fr(123, n, mont=False)
    want = np.concatenate([corc.point_mul(CURVE, 1, pts[i:i + 1], k) for i, k in enumerate(corc.arr_to_ints(sc))])
    return Spec(dict(points=(pts, pts0), scalars=(sc, sc0)), dict(out=64 * n),
                lambda ctx, ch, p: ctx.points_mul(CURVE, 1, p["points"], p["scalars"], device=True, channel=ch, out=p["out"],
                                                  n=n),
                lambda out: same(out["out"], want, "scalars[i] * points[i]"))


def make_points_codec(decompress):
    def make():
        import codec_cases as CC
        n = 65
        pts, pts0 = corc.gen_points(CURVE, 1, 130, n), corc.gen_points(CURVE, 1, 131, n)
        raw, raw0 = (np.frombuffer(b"".join(CC.encode(CURVE, 1, P) for P in points_as_ints(CURVE, a)), dtype=np.uint8)
                     for a in (pts, pts0))
        if decompress:
            return Spec(dict(raw=(raw, raw0)), dict(out=64 * n),
                        lambda ctx, ch, p: ctx.points_decompress_dev(CURVE, 1, p["raw"], n, p["out"], channel=ch),
                        lambda out: same(out["out"], pts, "the decompressed points"))
        return Spec(dict(points=(pts, pts0)), dict(out=32 * n),
                    lambda ctx, ch, p: ctx.points_compress_dev(CURVE, 1, p["points"], n, p["out"], channel=ch),
                    lambda out: same(out["out"], raw, "the compressed points"))
    return make


def make_wire_fr(decode):
    def make():
        n = 1000
        wire = lambda mont: np.concatenate([np.array([n], dtype=np.uint64).view(np.uint8),            # noqa: E731
                                            u8(corc.field_op(CURVE, "fr", "from_mont", mont))])
        x, x0 = fr(140, n), fr(141, n)
        nbytes = 8 + 32 * n
        if decode:
            n_out = ctypes.c_size_t()
            return Spec(dict(raw=(wire(x), wire(x0))), dict(out=32 * n),
                        lambda ctx, ch, p: ctx._chk(ctx.L.dg16_wire_fr_decode(ctx.h, 0, p["raw"], nbytes, p["out"],
                                                                              ctypes.byref(n_out), F_DEV, ch)),
                        lambda out: same(out["out"], x, "the decoded elements"))
        return Spec(dict(mont=(x, x0)), dict(out=nbytes),
                    lambda ctx, ch, p: ctx._chk(ctx.L.dg16_wire_fr_encode(ctx.h, 0, p["mont"], n, p["out"], F_DEV, ch)),
                    lambda out: same(out["out"], wire(x), "the wire bytes"))
    return make


# ---- rows: verification ----------------------------------------------------------------------------------------------------
_verify_material = {}


def verify_material(curve):
    """One oracle key, 65 proofs (two distinct oracle proofs, alternating) and the same batch with A of proofs 3, 17 and 64
    exchanged for the other proof's: a point of the subgroup, so only the equation rejects them.  The verdicts are those
    of the oracle's verifier (oracle.pyref.pairing.groth16_verify, about a second a proof: hence two proofs, and four
    distinct ones to verify)."""
    if curve not in _verify_material:
        import verify_cases as VC
        from oracle.pyref import pairing as PR
        r1cs, w, pk = VC.oracle_key(curve, 7)
        base = [VC.oracle_proof(curve, pk, r1cs, w, 20 + j) for j in range(2)]
        n = 65
        good = [base[i % 2] for i in range(n)]
        mixed = list(good)
        for i in (3, 17, 64):
            mixed[i] = (good[i - 1][0], good[i][1], good[i][2])
            assert mixed[i][0] != good[i][0]
        vk, pub, seen = VC.vk_of(pk), w[1:3], {}
        for pr in mixed:
            if pr not in seen:
                seen[pr] = PR.groth16_verify(curve, vk, pub, pr)
        verdict = np.array([seen[pr] for pr in mixed], dtype=np.uint8)
        assert len(seen) == 4 and [i for i in range(n) if not verdict[i]] == [3, 17, 64]
        _verify_material[curve] = dict(pk=pk, vk=VC.pack_vk(curve, VC.vk_of(pk)), good=VC.pack_proofs(curve, good),
                                       mixed=VC.pack_proofs(curve, mixed), verdict=verdict, base=base,
                                       x=VC.scalars(curve, [w[1:3]] * n), x0=VC.scalars(curve, [[w[2], w[1]]] * n), n=n)
    return _verify_material[curve]


def _pvk(curve):
    def prepare(env, p):
        from dg16_amd import verify
        return verify.PreparedVerifyingKey(env.ctx, curve, *verify_material(curve)["vk"])
    return prepare


def make_verify_batch(curve):
    def make():
        v = verify_material(curve)
        n = v["n"]
        # the decoy: 65 valid proofs and swapped public inputs.  Early-read proofs with the real inputs: 1 everywhere; early-read
        # inputs: 0 everywhere -- neither is the expected mix of 62 accepted and 3 rejected
        return Spec(dict(proofs=(v["mixed"], v["good"]), inputs=(v["x"], v["x0"])), dict(verdict=n),
                    lambda ctx, ch, p: ctx._chk(ctx.L.dg16_groth16_verify_batch(ctx.h, p["handle"].h, p["inputs"], 2,
                                                                                p["proofs"], n, F_DEV, p["verdict"], ch)),
                    lambda out: same(out["verdict"], v["verdict"], "the verdicts"),
                    prepare=_pvk(curve), close=lambda p: p["handle"].close())
    return make


def make_verify_aggregate():
    v = verify_material(CURVE)
    n = v["n"]
    rng = random.Random(150)
    co, co0 = (np.array([[rng.getrandbits(64) | 1, rng.getrandbits(64)] for _ in range(n)], dtype=np.uint64)
               for _ in range(2))
    # any non-zero coefficients accept 65 valid proofs, so other random ones would not show an early read of `coeffs`: the
    # decoy holds a zero coefficient, a legal input whose verdict is accepted = 0 (include/dg16.h)
    co0[n // 2] = 0
    return Spec(dict(proofs=(v["good"], v["mixed"]), inputs=(v["x"], v["x0"]), coeffs=(co, co0)), dict(accepted=1),
                lambda ctx, ch, p: ctx._chk(ctx.L.dg16_groth16_verify_aggregate(ctx.h, p["handle"].h, p["inputs"], 2,
                                                                                p["proofs"], n, p["coeffs"], F_DEV,
                                                                                p["accepted"], ch)),
                lambda out: same(out["accepted"], np.array([1], dtype=np.uint8), "the aggregate verdict"),
                prepare=_pvk(CURVE), close=lambda p: p["handle"].close())


def make_rerandomize():
    import points_mul_cases as PM
    import verify_cases as VC
    from oracle.pyref.fields import FR
    v = verify_material(CURVE)
    n, F = v["n"], FR[CURVE]
    rng = random.Random(160)
    rs2 = [(rng.randrange(1, F.p), rng.randrange(1, F.p)) for _ in range(2)]
    exp2 = [PM.oracle_rerandomize(CURVE, v["base"][j], v["pk"]["delta_g2"], *rs2[j]) for j in range(2)]
    want = VC.pack_proofs(CURVE, [exp2[i % 2] for i in range(n)])
    rs = np.stack([PM.scalars_arr(CURVE, list(rs2[i % 2])) for i in range(n)])
    rs0 = np.stack([PM.scalars_arr(CURVE, list(rs2[(i + 1) % 2])) for i in range(n)])
    return Spec(dict(proofs=(v["good"], v["mixed"]), r1_r2=(rs, rs0)), dict(out=v["good"].nbytes),
                lambda ctx, ch, p: ctx._chk(ctx.L.dg16_groth16_rerandomize(ctx.h, p["handle"].h, p["proofs"], n, p["r1_r2"],
                                                                           F_DEV, p["out"], ch)),
                lambda out: same(out["out"], want, "the re-randomized proofs"),
                prepare=_pvk(CURVE), close=lambda p: p["handle"].close())


# ---- rows: packed secret sharing on one context (a dg16_pss handle, no net) ------------------------------------------------
PSS_L = 2


def _pss(env, p):
    from dg16_amd import dist
    return dist.PackedSharingParams(env.ctx, CURVE, PSS_L)


def _pack_matrix(F):
    """M[r][c] of the oracle's pack_from_public at PSS_L, canonical: the images of the unit vectors."""
    from oracle.pyref.pss import PackedSharingParams as RefPSS
    ref = RefPSS(F, PSS_L)
    images = [ref.pack_from_public([int(i == c) for i in range(PSS_L)]) for c in range(PSS_L)]
    return [list(row) for row in zip(*images)]


def make_pss_apply():
    """pack_from_public of 300 vectors of l secrets (more than one block): reduced field elements, the decoy as well."""
    from oracle.pyref.fields import FR
    from oracle.pyref.pss import PackedSharingParams as RefPSS
    F, count = FR[CURVE], 300
    ref = RefPSS(F, PSS_L)
    rng = random.Random(170)
    enc = lambda v: corc.field_op(CURVE, "fr", "to_mont", corc.ints_to_arr(v, 4))     # noqa: E731
    secrets = [[rng.randrange(F.p) for _ in range(PSS_L)] for _ in range(count)]
    want = enc([s for row in secrets for s in ref.pack_from_public(row)])
    x, x0 = enc([s for row in secrets for s in row]), fr(171, count * PSS_L)
    return Spec(dict(secrets=(x, x0)), dict(out=32 * count * 4 * PSS_L),
                lambda ctx, ch, p: ctx._chk(ctx.L.dg16_pss_apply(ctx.h, p["handle"].h, 0, p["secrets"], count, p["out"],
                                                                 F_DEV, ch)),
                lambda out: same(out["out"], want, "the packed shares"),
                prepare=_pss, close=lambda p: p["handle"].close())


def make_pss_apply_exp():
    """packexp_from_public of 33 vectors of l points of the subgroup (one of them the identity): 264 outputs, the
    lane-per-output kernel.  Expected: the oracle's pack matrix applied with the C oracle's MSM."""
    from oracle.pyref.fields import FR
    count, n = 33, 4 * PSS_L
    M = [corc.ints_to_arr(row, 4) for row in _pack_matrix(FR[CURVE])]
    pts, pts0 = corc.gen_points(CURVE, 1, 180, count * PSS_L), corc.gen_points(CURVE, 1, 181, count * PSS_L)
    pts[1] = 0
    P = pts.reshape(count, PSS_L, -1)
    want = np.stack([np.concatenate([corc.msm(CURVE, 1, Pe, sc, threads=1) for sc in M]) for Pe in P])
    return Spec(dict(points=(pts, pts0)), dict(out=64 * count * n),
                lambda ctx, ch, p: ctx._chk(ctx.L.dg16_pss_apply_exp(ctx.h, p["handle"].h, 1, 0, p["points"], count,
                                                                     p["out"], F_DEV, ch)),
                lambda out: same(out["out"], want, "the shares packed in the exponent"),
                prepare=_pss, close=lambda p: p["handle"].close())


# ---- rows: the prover ------------------------------------------------------------------------------------------------------
class ProverCase:
    """A bench.Workload at log_m = 10 on the test's context, a second (decoy) witness with its a, b, c, and the oracle's
    proof of the real instance (bench.oracle_prove).  Made on first use; needs the GPU."""

    _made = {}

    def __init__(self, env, curve, seed=41):
        import torch
        import bench
        self.curve = curve
        wl = self.wl = bench.Workload(env.ctx, env.dev, 10, 0, 1, seed=seed, curve=curve)
        gen = torch.Generator(device=env.dev)
        gen.manual_seed(seed + 1)
        self.real = dict(a=wl.a.clone(), b=wl.b.clone(), c=wl.c.clone(), w=wl.w.clone())
        w0 = bench.rand_fr(wl.nv, env.dev, gen, curve)
        w0[0] = 0
        w0[0, 0] = 1
        torch.cuda.synchronize()
        wl.w = w0
        wl.qap()
        env.ctx.sync(0)
        self.decoy = dict(a=wl.a.clone(), b=wl.b.clone(), c=wl.c.clone(), w=w0)
        wl.w = self.real["w"]
        assert not torch.equal(self.real["w"], w0), "the decoy witness equals the real one"
        torch.cuda.synchronize()
        self.want = bench.oracle_prove(wl, bench.cpu_threads())[0]

    @classmethod
    def get(cls, env, curve):
        key = (id(env), curve)
        if key not in cls._made:
            cls._made[key] = cls(env, curve)
        return cls._made[key]

    def check(self, proof_bytes, what):
        import bench
        got = bench.gpu_proof_affine(self.curve, np.ascontiguousarray(proof_bytes))
        for name, g, e in zip("ABC", got, self.want):
            assert np.array_equal(g, e), "%s: %s differs from the oracle's" % (what, name)


class ProverRow(Row):
    """prove_dev, or groth16_msms_dev (split=True) / h_poly_dev and groth16_msms_h_dev (split="h") followed by
    groth16_assemble_dev: the Spec needs the environment (a resident key)."""

    def __init__(self, name, entries, curve, split=False, overlap=False):
        super().__init__(name, entries, (0,), None, host=("r_s",))
        self.curve, self.split, self.overlap = curve, split, overlap
        self.env = None

    def bind(self, env):
        if self.env is not env:
            self.env, self._spec = env, None
        return self

    def spec(self):
        if self._spec is None:
            pc = ProverCase.get(self.env, self.curve)
            wl = pc.wl
            outs = dict(proof=wl.proof_bytes())
            if self.split:
                outs["record"] = self.env.ctx.results_bytes(self.curve)
            if self.split == "h":
                outs["h"] = 32 * wl.m

            def call(ctx, ch, p):
                if self.split == "h":       # the h-polynomial on its own, then the half of a proof that starts from h
                    ctx.h_poly_dev(self.curve, p["a"], p["b"], p["c"], wl.log_m, p["h"], channel=ch)
                    ctx.groth16_msms_h_dev(wl.pk, p["h"], p["w"], wl.rs, p["record"], scalars_mont=False)
                    ctx.groth16_assemble_dev(wl.pk, p["record"], 1, wl.rs, p["proof"], scalars_mont=False)
                elif self.split:
                    ctx.groth16_msms_dev(wl.pk, p["a"], p["b"], p["c"], p["w"], wl.rs, p["record"], scalars_mont=False)
                    ctx.groth16_assemble_dev(wl.pk, p["record"], 1, wl.rs, p["proof"], scalars_mont=False)
                else:
                    ctx.prove_dev(wl.pk, p["a"], p["b"], p["c"], p["w"], wl.rs, p["proof"], scalars_mont=False,
                                  overlap_tail=self.overlap)

            self._spec = Spec({k: (pc.real[k], pc.decoy[k]) for k in "abcw"}, outs, call,
                              lambda out: pc.check(out["proof"], self.name), out_channel=2 if self.overlap else None)
        return self._spec


ALL3, CH0 = (0, 1, 2), (0,)
ROWS = [
    Row("field_op", ["dg16_field_op"], ALL3, make_field_op),
    Row("ntt", ["dg16_ntt"], ALL3, make_ntt(False, False)),
    Row("ntt_inverse_coset", ["dg16_ntt"], ALL3, make_ntt(True, True), host=("coset_offset",)),
    Row("h_poly_circom", ["dg16_h_poly"], ALL3, make_h_poly("circom")),
    Row("h_poly_libsnark", ["dg16_h_poly"], ALL3, make_h_poly("libsnark")),
    Row("qap", ["dg16_qap"], ALL3, make_qap(False)),
    Row("qap_rows", ["dg16_qap_rows"], ALL3, make_qap(True)),
    Row("qap_r1cs", ["dg16_qap_r1cs"], ALL3, make_qap_r1cs),
    Row("msm_g1_2e10", ["dg16_msm"], ALL3, make_msm("bn254", 1, 1 << 10, False)),
    Row("msm_g1_2e10_in_subgroup", ["dg16_msm"], ALL3, make_msm("bn254", 1, 1 << 10, True)),
    Row("msm_g1_partitioned_sort", ["dg16_msm"], ALL3, make_msm("bn254", 1, (1 << 14) + 37, False)),
    Row("msm_g1_partitioned_sort_in_subgroup", ["dg16_msm"], ALL3, make_msm("bn254", 1, (1 << 14) + 37, True)),
    Row("msm_g2_bls12_381", ["dg16_msm"], ALL3, make_msm("bls12_381", 2, 1 << 10, False)),
    Row("msm_g2_bls12_381_in_subgroup", ["dg16_msm"], ALL3, make_msm("bls12_381", 2, 1 << 10, True)),
    Row("msm_resident", ["dg16_msm_resident"], ALL3, make_msm_resident),
    Row("bases_upload", ["dg16_bases_upload", "dg16_msm_resident"], CH0, make_bases_upload),
    Row("gen_bases", ["dg16_gen_bases"], ALL3, make_gen_bases),
    Row("to_affine", ["dg16_to_affine"], ALL3, make_to_affine),
    Row("fixed_base_mul", ["dg16_fixed_base_mul"], ALL3, make_fixed_base_mul, host=("base",)),
    Row("points_mul", ["dg16_points_mul"], ALL3, make_points_mul),
    Row("points_compress", ["dg16_points_compress"], ALL3, make_points_codec(False)),
    Row("points_decompress", ["dg16_points_decompress"], ALL3, make_points_codec(True)),
    Row("wire_fr_encode", ["dg16_wire_fr_encode"], ALL3, make_wire_fr(False)),
    Row("wire_fr_decode", ["dg16_wire_fr_decode"], ALL3, make_wire_fr(True)),
    Row("verify_batch", ["dg16_groth16_verify_batch"], ALL3, make_verify_batch("bn254")),
    Row("verify_batch_bls12_381", ["dg16_groth16_verify_batch"], ALL3, make_verify_batch("bls12_381")),
    Row("verify_aggregate", ["dg16_groth16_verify_aggregate"], ALL3, make_verify_aggregate),
    Row("rerandomize", ["dg16_groth16_rerandomize"], ALL3, make_rerandomize),
    Row("pss_apply", ["dg16_pss_apply"], ALL3, make_pss_apply),
    Row("pss_apply_exp", ["dg16_pss_apply_exp"], ALL3, make_pss_apply_exp),
    ProverRow("msms_then_assemble", ["dg16_groth16_msms", "dg16_groth16_assemble"], "bn254", split=True),
    ProverRow("h_poly_then_msms_h", ["dg16_h_poly", "dg16_groth16_msms_h", "dg16_groth16_assemble"], "bn254", split="h"),
    ProverRow("prove", ["dg16_groth16_prove"], "bn254"),
    ProverRow("prove_bls12_381", ["dg16_groth16_prove"], "bls12_381"),
    ProverRow("prove_overlap_tail", ["dg16_groth16_prove"], "bn254", overlap=True),
]
ROWS_BY_NAME = {r.name: r for r in ROWS}

# Entry points without a `channel` argument: synchronous, ordered behind the work enqueued on channel 0's stream.  They
# are tested one by one in tests/test_gpu_stream_order.py (section "entry points without a channel"), not through ROWS.
NO_CHANNEL = {
    "dg16_pk_create": "test_pk_create_is_ordered_behind_channel_0",
    "dg16_pk_create_shard": "test_pk_create_is_ordered_behind_channel_0",
    "dg16_vk_create": "test_vk_create_is_ordered_behind_channel_0",
    "dg16_groth16_setup": "test_setups_are_ordered_behind_channel_0",
    "dg16_groth16_setup_srs": "test_setups_are_ordered_behind_channel_0",
}

# Entry points that take DG16_F_DEVICE_PTRS and have NO ordering test here, each with the reason.
EXCEPTIONS = {
    "dg16_ntt_dist": "needs a dg16_comm; run at world size 1 by tests/test_gpu_hdist.py",
    "dg16_h_poly_dist": "needs a dg16_comm; run at world size 1 by tests/test_gpu_hdist.py",
    "dg16_groth16_prove_dist": "needs a dg16_comm; run at world size 1 by tests/test_gpu_hdist.py",
    "dg16_ntt_dist_stage": "a local stage of dg16_ntt_dist, meaningful between the caller's exchanges only; "
                           "tests/test_gpu_hdist.py",
    "dg16_h_poly_dist_stage": "a local stage of dg16_h_poly_dist, meaningful between the caller's exchanges only; "
                              "tests/test_gpu_hdist.py",
    "dg16_d_fft": "needs a dg16_net (blocking collectives between parties); tests/test_gpu_dist.py",
    "dg16_d_msm": "needs a dg16_net; tests/test_gpu_dist.py",
    "dg16_d_msm_resident": "needs a dg16_net; tests/test_gpu_dist.py",
    "dg16_deg_red": "needs a dg16_net; tests/test_gpu_dist.py",
    "dg16_d_pp": "needs a dg16_net; tests/test_gpu_dist.py",
    "dg16_ext_wit_h": "needs a dg16_net; tests/test_gpu_dist.py",
    "dg16_prove_a": "needs a dg16_net; tests/test_gpu_dist.py",
    "dg16_prove_b": "needs a dg16_net; tests/test_gpu_dist.py",
    "dg16_prove_c": "needs a dg16_net and drives all three channels from its own threads; tests/test_gpu_dist.py",
}


def covered_entry_points():
    out = set(NO_CHANNEL)
    for r in ROWS:
        out.update(r.entries)
    return out
