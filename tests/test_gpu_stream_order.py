"""GPU: WHEN the library reads and writes device memory (include/dg16.h, "Conventions": device-pointer calls are
stream-ordered on the channel's stream -- dg16_sync or the stream installed with dg16_set_stream).  Every case puts a
delayed producer in front of a call and a consumer right behind it on a caller-owned stream (tests/stream_cases.py says
how and why the misordered outcome is always a valid computation); every expected value is the oracle's.  Run with -s to
see the control's verdict and the measured delays.  No graph capture of any of these streams."""

import random
import time

import numpy as np
import pytest

import stream_cases as SC
from oracle import corc

pytestmark = pytest.mark.gpu

CURVE = "bn254"


@pytest.fixture(scope="module")
def env():
    """A context of its own (not gpu_util.ctx(): streams are installed on its channels), closed at the end."""
    import torch
    import dg16_amd
    ctx = dg16_amd.Context(0)
    e = SC.Env(ctx, torch.device("cuda", 0))
    e.control_error = None
    try:
        try:
            e.find_stream()
        except AssertionError as err:      # reported by every test (a failure, not a skip and not a fixture error)
            e.control_error = str(err)
        yield e
    finally:
        for ch in range(3):
            ctx.set_stream(ch, None)
        torch.cuda.synchronize()
        e.close()
        for pc in list(SC.ProverCase._made.values()):
            pc.wl.pk.close()
        SC.ProverCase._made.clear()
        ctx.close()


def ready(env):
    assert env.control_error is None, env.control_error
    return env


def test_control_a_sleeping_caller_stream_leaves_the_library_stream_running(env):
    ready(env)
    assert env.S is not None and env.ms_per_cycle > 0
    print(env.control_verdict)


# ---- a. producer and consumer on an installed stream ------------------------------------------------------------------------
CASES = [(r.name, ch) for r in SC.ROWS for ch in r.channels]


@pytest.mark.parametrize("name,channel", CASES, ids=["%s-ch%d" % c for c in CASES])
def test_call_is_ordered_on_the_installed_stream(env, name, channel):
    import torch
    row = SC.ROWS_BY_NAME[name]
    if isinstance(row, SC.ProverRow):
        row.bind(ready(env))
    out_stream = None
    if name == "prove_overlap_tail":        # dg16.h: proof_out is complete on CHANNEL 2's stream -- a second caller stream
        out_stream = torch.cuda.Stream(device=env.dev)
    SC.run_delayed(ready(env), row, channel, out_stream=out_stream)


# ---- b. the prover: delayed witness -> qap_dev -> prove_dev -> snapshot, no host call in between ----------------------------
def _rs(curve, seed):
    import bench
    rng = random.Random(seed)
    R = bench.FR_MOD[curve]
    r, s = rng.randrange(1, R), rng.randrange(1, R)
    return r, s, corc.ints_to_arr([r, s], 4)


_chain_oracle = {}


def _chain_want(pc, k):
    """The oracle's proof of the real instance under the k-th (r, s); made once."""
    import bench
    if k not in _chain_oracle:
        r, s, _ = _rs(pc.curve, 700 + k)
        _chain_oracle[k] = bench.oracle_prove(pc.wl, bench.cpu_threads(), r, s)[0]
    return _chain_oracle[k]


@pytest.mark.parametrize("form,n_proofs", [("plain", 1), ("overlap_tail", 1), ("overlap_tail_queue", 3)])
def test_prover_chain_behind_a_delayed_witness(env, form, n_proofs):
    import torch
    import bench
    ctx, S, dev = ready(env).ctx, env.S, env.dev
    pc = SC.ProverCase.get(env, CURVE)
    wl = pc.wl
    overlap = form != "plain"
    So = torch.cuda.Stream(device=dev) if overlap else S
    rss = [_rs(CURVE, 700 + k)[2] for k in range(n_proofs)]
    wbuf = pc.real["w"].clone()
    assert not torch.equal(pc.real["w"], pc.decoy["w"])
    outs = [torch.empty(wl.proof_bytes(), dtype=torch.uint8, device=dev) for _ in range(n_proofs)]
    snaps = [torch.empty_like(o) for o in outs]
    torch.cuda.synchronize()

    def chain(delay_ms):
        ev = env.sleep(S, delay_ms) if delay_ms else None
        with torch.cuda.stream(S):
            wbuf.copy_(pc.real["w"], non_blocking=True)
        for k in range(n_proofs):
            ctx.qap_dev(CURVE, wl.nc, wl.ni, wl.nv, wl.log_m, wl.row_ptr.data_ptr(), wl.a_col.data_ptr(),
                        wl.a_val.data_ptr(), wl.row_ptr.data_ptr(), wl.b_col.data_ptr(), wl.b_val.data_ptr(),
                        wbuf.data_ptr(), wl.a.data_ptr(), wl.b.data_ptr(), wl.c.data_ptr(), scalars_mont=False)
            ctx.prove_dev(wl.pk, wl.a.data_ptr(), wl.b.data_ptr(), wl.c.data_ptr(), wbuf.data_ptr(), rss[k],
                          outs[k].data_ptr(), scalars_mont=False, overlap_tail=overlap)
            with torch.cuda.stream(So):
                snaps[k].copy_(outs[k], non_blocking=True)
                outs[k].fill_(SC.AFTER)
        S.synchronize()
        So.synchronize()
        return ev

    ctx.set_stream(0, S.cuda_stream)         # only channel 0 has a caller stream (and channel 2 for the overlapped tail)
    if overlap:
        ctx.set_stream(2, So.cuda_stream)
    try:
        chain(0)                             # warm-up
        t0 = time.perf_counter()
        chain(0)
        warm_ms = (time.perf_counter() - t0) * 1e3
        delay_ms = max(SC.MIN_DELAY_MS, 10.0 * warm_ms)
        wbuf.copy_(pc.decoy["w"])
        for o, sn in zip(outs, snaps):
            o.fill_(SC.BEFORE)
            sn.fill_(SC.BEFORE)
        torch.cuda.synchronize()
        e0, e1 = chain(delay_ms)
        print("prover chain (%s): warmed %.2f ms, delay asked %.1f ms, slept %.1f ms" % (form, warm_ms, delay_ms,
                                                                                       e0.elapsed_time(e1)))
        for k in range(n_proofs):
            got = bench.gpu_proof_affine(CURVE, snaps[k].cpu().numpy())
            for nm, g, w in zip("ABC", got, _chain_want(pc, k)):
                assert np.array_equal(g, w), "%s, proof %d: %s differs from the oracle's" % (form, k, nm)
    finally:
        ctx.set_stream(0, None)
        ctx.set_stream(2, None)
        for ch in range(3):
            ctx.sync(ch)


# ---- c. entry points without a channel: synchronous, ordered behind channel 0's stream --------------------------------------
def _warmed_ms(call):
    """Wall time of one call that has run before with the same shapes (these calls are synchronous), real inputs in place."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def _delayed_inputs(env, bufs, reals, warm_ms):
    """bufs hold decoys; on S: a sleep of max(MIN_DELAY_MS, 10 x the warmed call), then the real inputs.  Returns the delay
    asked for and the sleep's events."""
    import torch
    torch.cuda.synchronize()
    delay_ms = max(SC.MIN_DELAY_MS, 10.0 * warm_ms)
    ev = (delay_ms,) + env.sleep(env.S, delay_ms)
    with torch.cuda.stream(env.S):
        for b, r in zip(bufs, reals):
            b.copy_(r, non_blocking=True)
    return ev


@pytest.mark.parametrize("n_shards", [1, 2])
def test_pk_create_is_ordered_behind_channel_0(env, n_shards):
    """The key made from queries that a producer on channel 0's stream is still writing must be the key of the REAL queries:
    a proof under it equals the oracle's.  n_shards = 2: shard 0 is made behind the delay, shard 1 from settled inputs, and
    the two records are assembled."""
    import torch
    import bench
    ctx, S, dev = ready(env).ctx, env.S, env.dev
    pc = SC.ProverCase.get(env, CURVE)
    wl = pc.wl
    reals = [wl.aq, wl.b1q, wl.b2q, wl.hq, wl.lq, wl.fixed]
    fqb = bench.FQ_BYTES[CURVE]
    decoys = []
    for i, (group, cnt) in enumerate([(1, wl.nv), (1, wl.nv), (2, wl.nv), (1, wl.m), (1, wl.nv - wl.ni)]):
        t = torch.empty(cnt * 2 * fqb * group, dtype=torch.uint8, device=dev)
        ctx.gen_bases_dev(CURVE, group, 9000 + i, cnt, t.data_ptr())        # other points of the subgroup
        decoys.append(t)
    f1, f2 = (torch.empty(n * 2 * fqb * g, dtype=torch.uint8, device=dev) for g, n in ((1, 3), (2, 2)))
    ctx.gen_bases_dev(CURVE, 1, 9006, 3, f1.data_ptr())
    ctx.gen_bases_dev(CURVE, 2, 9007, 2, f2.data_ptr())
    ctx.sync(0)
    decoys.append(torch.cat([f1, f2]))
    for d, r in zip(decoys, reals):
        assert d.numel() == r.numel() and not torch.equal(d, r.view(torch.uint8).reshape(-1))
    bufs = [r.clone() for r in reals]
    torch.cuda.synchronize()

    def create(shard):
        return ctx.pk_create(CURVE, wl.nv, wl.ni, wl.m, *[b.data_ptr() for b in bufs], device_ptrs=True, shard=shard,
                             n_shards=n_shards)

    ctx.set_stream(0, S.cuda_stream)
    keys = []
    try:
        create(0).close()                    # warm-up, same shapes
        warm_ms = _warmed_ms(lambda: keys.append(create(0)))
        keys.pop().close()
        for b, d in zip(bufs, decoys):
            b.copy_(d.view(b.dtype).reshape(b.shape))
        delay_ms, e0, e1 = _delayed_inputs(env, bufs, reals, warm_ms)
        t0 = time.perf_counter()
        keys.append(create(0))
        held = (time.perf_counter() - t0) * 1e3
        with torch.cuda.stream(S):           # complete on return: the inputs may change right away
            for b, d in zip(bufs, decoys):
                b.copy_(d.view(b.dtype).reshape(b.shape), non_blocking=True)
        S.synchronize()
        print("pk_create (%d shard(s)): warmed call %.2f ms, delay asked %.1f ms, slept %.1f ms, the call held the host %.1f ms"
              % (n_shards, warm_ms, delay_ms, e0.elapsed_time(e1), held))
        ctx.set_stream(0, None)
        for b, r in zip(bufs, reals):
            b.copy_(r)
        torch.cuda.synchronize()
        for k in range(1, n_shards):
            keys.append(create(k))
        rb = ctx.results_bytes(CURVE)
        recs = torch.zeros(n_shards * rb, dtype=torch.uint8, device=dev)
        proof = torch.zeros(wl.proof_bytes(), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        a, b_, c, w = (pc.real[k].data_ptr() for k in "abcw")
        for k, key in enumerate(keys):
            ctx.groth16_msms_dev(key, a, b_, c, w, wl.rs, recs.data_ptr() + k * rb, scalars_mont=False)
        ctx.groth16_assemble_dev(keys[0], recs.data_ptr(), n_shards, wl.rs, proof.data_ptr(), scalars_mont=False)
        for ch in range(3):
            ctx.sync(ch)
        pc.check(proof.cpu().numpy(), "the proof under the key made behind the delay")
    finally:
        ctx.set_stream(0, None)
        for key in keys:
            key.close()


def test_vk_create_is_ordered_behind_channel_0(env):
    """dg16_vk_create on device pointers that channel 0's stream is still writing: the handle must be the REAL key's -- it
    accepts the oracle's valid proofs and rejects the three whose A was exchanged."""
    import ctypes
    import torch
    import verify_cases as VC
    ctx, S, dev = ready(env).ctx, env.S, env.dev
    v = SC.verify_material(CURVE)
    _, _, pk0 = VC.oracle_key(CURVE, 8)
    real = [SC.to_dev(x, dev) for x in v["vk"]]
    decoy = [SC.to_dev(x, dev) for x in VC.pack_vk(CURVE, VC.vk_of(pk0))]
    assert all(r.numel() == d.numel() and not torch.equal(r, d) for r, d in zip(real, decoy))
    bufs = [r.clone() for r in real]
    n_ic = v["vk"][4].shape[0]
    L = ctx.L

    def create():
        h = ctypes.c_void_p()
        ctx._chk(L.dg16_vk_create(ctx.h, 0, *[b.data_ptr() for b in bufs], n_ic, SC.F_DEV, ctypes.byref(h)))
        return h

    ctx.set_stream(0, S.cuda_stream)
    h = None
    try:
        L.dg16_vk_destroy(create())          # warm-up
        made = []
        warm_ms = _warmed_ms(lambda: made.append(create()))
        L.dg16_vk_destroy(made.pop())
        for b, d in zip(bufs, decoy):
            b.copy_(d)
        delay_ms, e0, e1 = _delayed_inputs(env, bufs, real, warm_ms)
        h = create()
        with torch.cuda.stream(S):
            for b, d in zip(bufs, decoy):
                b.copy_(d, non_blocking=True)
        S.synchronize()
        print("vk_create: warmed call %.2f ms, delay asked %.1f ms, slept %.1f ms" % (warm_ms, delay_ms, e0.elapsed_time(e1)))
        ctx.set_stream(0, None)
        p = lambda a: np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)       # noqa: E731
        for proofs, want in ((v["good"], np.ones(v["n"], dtype=np.uint8)), (v["mixed"], v["verdict"])):
            verdict = np.full(v["n"], SC.BEFORE, dtype=np.uint8)
            x, pr = np.ascontiguousarray(v["x"]), np.ascontiguousarray(proofs)
            ctx._chk(L.dg16_groth16_verify_batch(ctx.h, h, p(x), 2, p(pr), v["n"], 0, p(verdict), 0))
            assert np.array_equal(verdict, want)
    finally:
        ctx.set_stream(0, None)
        if h is not None:
            L.dg16_vk_destroy(h)


SETUP_NAMES = ("a_query", "b_g1_query", "b_g2_query", "h_query", "l_query", "fixed_points", "gamma_g2", "gamma_abc_g1")


def _setup_case(env):
    """dg16_groth16_setup on BN254 at log_m = 10 under a general trapdoor.  Expected: the oracle's query scalars
    (oracle.pyref.groth16.setup_scalars, Python integers) times the generators by the C oracle."""
    from oracle.pyref.fields import FR
    from oracle.pyref import groth16 as G
    import test_libsnark_model as M
    from test_gpu_setup import csr_of
    curve, log_m = CURVE, 10
    F = FR[curve]
    r1cs, _ = M.instance(F, 1 << log_m, seed=46)
    rng = random.Random(47)
    td = tuple(rng.randrange(2, F.p) for _ in range(5))
    alpha, beta, gamma, delta, _ = td
    sc = G.setup_scalars(r1cs, F, td)
    assert sc["m"] == 1 << log_m and len(sc["h"]) == 1 << log_m
    g = {grp: corc.generator(curve, grp) for grp in (1, 2)}
    mul = lambda grp, xs: np.concatenate([corc.point_mul(curve, grp, g[grp], x) for x in xs])      # noqa: E731
    want = dict(a_query=mul(1, sc["a"]), b_g1_query=mul(1, sc["b"]), b_g2_query=mul(2, sc["b"]), h_query=mul(1, sc["h"]),
                l_query=mul(1, sc["l"]), fixed_points=np.concatenate([SC.u8(mul(1, [alpha, beta, delta])),
                                                                      SC.u8(mul(2, [beta, delta]))]),
                gamma_g2=mul(2, [gamma]), gamma_abc_g1=mul(1, sc["gamma_abc"]))
    csr = [csr_of(F, r1cs[k]) for k in "abc"]
    real = [mat[2] for mat in csr]
    decoy = [SC.fr(480 + j, mat[2].shape[0], curve) for j, mat in enumerate(csr)]
    nc, ni = r1cs["num_constraints"], r1cs["num_instance"]

    def call(mats, srs_ptrs, outs):
        env.ctx.groth16_setup(curve, nc, ni, ni + r1cs["num_witness"], log_m, *mats, corc.ints_to_arr(list(td), 4), outs,
                              device_ptrs=True)

    return csr, real, decoy, want, call


def _setup_srs_case(env):
    """dg16_groth16_setup_srs on the column-shapes system of tests/test_gpu_setup_srs.py (BLS12-381, log_m = 13): wires
    whose segments are added by a lane, by a wave and by the MSM, with the expected key that file takes from the oracle.
    The decoy: other reduced coefficients and four other tables of points of the subgroup."""
    from oracle.pyref.fields import FR
    from test_gpu_setup import csr_of
    from test_gpu_setup_srs import shapes
    sh = shapes()
    curve, m = sh["curve"], sh["m"]
    F = FR[curve]
    csr = [csr_of(F, sh["r1cs"][k]) for k in "abc"]
    real = [mat[2] for mat in csr]
    decoy = [SC.fr(490 + j, mat[2].shape[0], curve) for j, mat in enumerate(csr)]
    t = sh["tabs"]
    real += [t[k] for k in ("lag_g1", "lag_g2", "alpha_lag_g1", "beta_lag_g1", "h_g1")]
    other = [env.ctx.fixed_base_mul(curve, grp, SC.fr(495 + j, m, curve, mont=False))
             for j, grp in enumerate((1, 2, 1, 1))]
    decoy += other + [np.ascontiguousarray(other[2][::-1])]

    def call(mats, srs_ptrs, outs):
        env.ctx.groth16_setup_srs(curve, sh["nc"], sh["ni"], sh["nv"], sh["log_m"], *mats, srs_ptrs + [t["fixed"]], outs,
                                  device_ptrs=True)                                  # srs->fixed: HOST by contract

    return csr, real, decoy, sh["exp"], call


@pytest.mark.parametrize("which", ["setup", "setup_srs"])
def test_setups_are_ordered_behind_channel_0(env, which):
    """dg16_groth16_setup / dg16_groth16_setup_srs with coefficient values (and, for the latter, the reference string's
    point arrays) that channel 0's stream is still writing: the key is the oracle's key of the REAL inputs, complete on
    return.  row_ptr and col are never delayed: a stale index array could index out of range."""
    import torch
    ctx, S, dev = ready(env).ctx, env.S, env.dev
    csr, real, decoy, want, call_with = (_setup_case if which == "setup" else _setup_srs_case)(env)
    idx = [[SC.to_dev(x, dev) for x in mat[:2]] for mat in csr]
    real, decoy = [SC.to_dev(x, dev) for x in real], [SC.to_dev(x, dev) for x in decoy]
    assert all(r.numel() == d.numel() and not torch.equal(r, d) for r, d in zip(real, decoy))
    bufs = [r.clone() for r in real]
    want = {n: SC.u8(want[n]) for n in SETUP_NAMES}
    outs = [torch.empty(max(want[n].nbytes, 16), dtype=torch.uint8, device=dev) for n in SETUP_NAMES]
    torch.cuda.synchronize()
    mats = [(idx[j][0].data_ptr(), idx[j][1].data_ptr(), bufs[j].data_ptr()) for j in range(3)]

    def call():
        call_with(mats, [b.data_ptr() for b in bufs[3:]], [o.data_ptr() for o in outs])

    ctx.set_stream(0, S.cuda_stream)
    try:
        call()                               # warm-up
        warm_ms = _warmed_ms(call)
        for b, d in zip(bufs, decoy):
            b.copy_(d)
        for o in outs:
            o.fill_(SC.BEFORE)
        delay_ms, e0, e1 = _delayed_inputs(env, bufs, real, warm_ms)
        call()
        got = [o.cpu().numpy() for o in outs]          # complete on return: read without any synchronisation of S
        S.synchronize()
        print("%s: warmed call %.2f ms, delay asked %.1f ms, slept %.1f ms" % (which, warm_ms, delay_ms, e0.elapsed_time(e1)))
        for n, g in zip(SETUP_NAMES, got):
            assert np.array_equal(g[:want[n].nbytes], want[n]), "%s: %s differs from the oracle's key" % (which, n)
    finally:
        ctx.set_stream(0, None)


# ---- d. dg16_set_stream itself -----------------------------------------------------------------------------------------------
def _field_op_case(env, seed):
    n = SC.CONTROL_N
    a, b = SC.fr(seed, n), SC.fr(seed + 1, n)
    return n, SC.to_dev(a, env.dev), SC.to_dev(b, env.dev), corc.field_op(CURVE, "fr", "mul", a, b)


def test_set_stream_refuses_a_bad_channel_and_the_context_still_works(env):
    import torch
    ctx = ready(env).ctx
    for ch in (-1, 3):
        assert ctx.L.dg16_set_stream(ctx.h, ch, env.S.cuda_stream) == 3          # DG16_ERR_BAD_ARG
        assert ctx.L.dg16_last_error(ctx.h).decode().strip() != ""
    n, a, b, want = _field_op_case(env, 500)
    out = torch.zeros_like(a)
    torch.cuda.synchronize()
    ctx.field_op_dev(CURVE, "fr", 2, a.data_ptr(), b.data_ptr(), out.data_ptr(), n)
    ctx.sync(0)
    SC.same(out.cpu().numpy(), want, "a * b after the refused calls")


def test_null_restores_the_librarys_own_stream(env):
    """After set_stream(ch, NULL) a call is NOT held up by the sleeping caller stream: it completes (dg16_sync returns, with
    the oracle's product) while the sleep that was enqueued before it is still running."""
    import torch
    ctx, S = ready(env).ctx, env.S
    n, a, b, want = _field_op_case(env, 510)
    out = torch.zeros_like(a)
    torch.cuda.synchronize()
    ctx.set_stream(0, S.cuda_stream)
    try:
        ctx.field_op_dev(CURVE, "fr", 2, a.data_ptr(), b.data_ptr(), out.data_ptr(), n)      # warm, on S
        S.synchronize()
    finally:
        ctx.set_stream(0, None)
    out.fill_(SC.BEFORE)
    torch.cuda.synchronize()
    e0, e1 = env.sleep(S, 8 * SC.MIN_DELAY_MS)
    ctx.field_op_dev(CURVE, "fr", 2, a.data_ptr(), b.data_ptr(), out.data_ptr(), n)
    ctx.sync(0)
    still_sleeping = not e1.query()
    got = out.cpu().numpy()
    S.synchronize()
    print("restore: the caller stream slept %.1f ms; still sleeping when the call had completed: %s"
          % (e0.elapsed_time(e1), still_sleeping))
    SC.same(got, want, "a * b on the restored stream")
    assert still_sleeping, "the call on the restored stream waited for the caller's stream"


def test_sync_waits_for_the_installed_stream(env):
    ctx, S = ready(env).ctx, env.S
    ctx.set_stream(1, S.cuda_stream)
    try:
        e0, e1 = env.sleep(S, 4 * SC.MIN_DELAY_MS)
        assert not e1.query(), "the sleep was over before dg16_sync was called: nothing to wait for"
        ctx.sync(1)
        assert e1.query(), "dg16_sync returned before the installed stream had drained"
    finally:
        ctx.set_stream(1, None)
        S.synchronize()


def test_last_kernel_ms_on_an_installed_stream(env):
    import torch
    ctx, S = ready(env).ctx, env.S
    n = 1 << 10
    bases, sc = SC.to_dev(corc.gen_points(CURVE, 1, 520, n), env.dev), SC.to_dev(SC.fr(521, n, mont=False), env.dev)
    out = torch.zeros(96, dtype=torch.uint8, device=env.dev)
    torch.cuda.synchronize()
    for ch in range(3):
        ctx.set_stream(ch, S.cuda_stream)
        try:
            ctx.msm_dev(CURVE, 1, bases.data_ptr(), sc.data_ptr(), n, out.data_ptr(), channel=ch)
            S.synchronize()
            assert ctx.last_kernel_ms(ch, 0) > 0.0, "the whole-call events were not recorded on the installed stream"
        finally:
            ctx.set_stream(ch, None)


def test_installing_a_stream_under_a_pending_tail_keeps_the_next_call_behind_it(env):
    """An overlapped proof's tail is still running on channel 2 when a caller stream is installed on channel 0: the next
    call there (dg16_to_affine of the proof's A) must still see the finished proof.  proof_out holds another valid proof
    (other r, s) until the tail writes it, so a call that ran ahead converts that one's A.  Nothing here can hold the tail
    back (it runs on the library's own stream, a few milliseconds at log 10): once it has finished, the case passes
    whatever the library does.  It prints whether the caller's stream was still busy when the one-point conversion had
    been enqueued, which is what a pending tail looks like from outside."""
    import torch
    ctx, S, dev = ready(env).ctx, env.S, env.dev
    pc = SC.ProverCase.get(env, CURVE)
    wl = pc.wl
    other = torch.zeros(wl.proof_bytes(), dtype=torch.uint8, device=dev)
    proof = torch.zeros_like(other)
    aff = torch.zeros(64, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    args = [pc.real[k].data_ptr() for k in "abcw"]
    ctx.prove_dev(wl.pk, *args, _rs(CURVE, 530)[2], other.data_ptr(), scalars_mont=False)
    for ch in range(3):
        ctx.sync(ch)
    assert not np.array_equal(corc.jac_to_affine(CURVE, 1, other.cpu().numpy().view(np.uint64)[:12]), pc.want[0])
    proof.copy_(other)
    torch.cuda.synchronize()
    try:
        ctx.prove_dev(wl.pk, *args, wl.rs, proof.data_ptr(), scalars_mont=False, overlap_tail=True)
        ctx.set_stream(0, S.cuda_stream)
        ctx._chk(ctx.L.dg16_to_affine(ctx.h, 0, 1, proof.data_ptr(), aff.data_ptr(), 1, SC.F_DEV, 0))
        busy = not S.query()
        S.synchronize()
        print("pending tail: the caller's stream still had work when dg16_to_affine returned: %s" % busy)
        got = aff.cpu().numpy()
    finally:
        ctx.set_stream(0, None)
        for ch in range(3):
            ctx.sync(ch)
    SC.same(got, pc.want[0], "A of the overlapped proof, converted on the newly installed stream")
    pc.check(proof.cpu().numpy(), "the overlapped proof")
