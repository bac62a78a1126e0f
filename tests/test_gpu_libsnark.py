"""The Libsnark QAP reduction on the GPU (DG16_F_QAP_LIBSNARK, dg16_qap_r1cs) against the big-int model of
tests/test_libsnark_model.py and the oracle's point arithmetic -- never against the code under test."""

import random

import numpy as np
import pytest

from oracle import corc
from oracle.pyref.fields import FQ, FR
from oracle.pyref import groth16 as G
from gpu_util import ctx
from test_gpu_prover import enc_fr
from test_gpu_setup import csr_of, system_of
import test_libsnark_model as M

pytestmark = pytest.mark.gpu

PROVER_CURVES = ["bn254", "bls12_381"]
ALL = ["bn254", "bls12_381", "bls12_377"]
U64_MAX = 2**64 - 1


def dec_fr(F, arr):
    rinv = F.inv(F.R)
    return [x * rinv % F.p for x in corc.arr_to_ints(np.asarray(arr).reshape(-1, 4))]


def instance(F, log_m, seed, below=False):
    """A satisfied system on the size-2^log_m domain: num_constraints + num_inputs exactly m, or (below) m / 2 + 1 -- the
    smallest count that still selects this domain, so almost half the rows are padding."""
    m = 1 << log_m
    return M.instance(F, m, seed, slack=(m // 2 - 1) if below else 0)


def qap_r1cs(curve, r1cs, w, **kw):
    F = FR[curve]
    return ctx().qap_r1cs(curve, r1cs["num_constraints"], r1cs["num_instance"], csr_of(F, r1cs["a"]), csr_of(F, r1cs["b"]),
                          csr_of(F, r1cs["c"]), enc_fr(F, w), **kw)


def violated_rows(r1cs, w, p):
    return [i for i, (ra, rb, rc) in enumerate(zip(r1cs["a"], r1cs["b"], r1cs["c"]))
            if G.evaluate_constraint(ra, w, p) * G.evaluate_constraint(rb, w, p) % p != G.evaluate_constraint(rc, w, p)]


# ---- dg16_qap_r1cs: values -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", PROVER_CURVES)
@pytest.mark.parametrize("log_m", [3, 6, 10])
@pytest.mark.parametrize("below", [False, True])
def test_qap_r1cs_values(curve, log_m, below):
    F = FR[curve]
    r1cs, w = instance(F, log_m, seed=log_m, below=below)
    a, b, c, dom = M.libsnark_abc(r1cs, w, F)
    assert dom.size == 1 << log_m
    ga, gb, gc, viol = qap_r1cs(curve, r1cs, w)
    assert np.array_equal(ga, enc_fr(F, a)) and np.array_equal(gb, enc_fr(F, b)) and np.array_equal(gc, enc_fr(F, c))
    assert viol == (0, None)
    # the strided form: rows 1 + 4 j, written densely
    sa, sb, sc, sviol = qap_r1cs(curve, r1cs, w, row_start=1, row_stride=4)
    assert np.array_equal(sa, enc_fr(F, a[1::4])) and np.array_equal(sb, enc_fr(F, b[1::4]))
    assert np.array_equal(sc, enc_fr(F, c[1::4])) and sviol == (0, None)


def test_qap_r1cs_c_comes_from_the_matrix():
    """c is C w, not a o b: with a C matrix that does not match, c differs from dg16_qap's and the rows are reported."""
    curve, F = "bn254", FR["bn254"]
    r1cs, w = instance(F, 4, seed=2)
    r1cs = dict(r1cs, c=[[((cf + 1) % F.p, j) for cf, j in row] for row in r1cs["c"]])
    a, b, c, _ = M.libsnark_abc(r1cs, w, F)
    _, _, gc, viol = qap_r1cs(curve, r1cs, w)
    assert np.array_equal(gc, enc_fr(F, c))
    bad = violated_rows(r1cs, w, F.p)
    assert bad and viol == (len(bad), bad[0])


# ---- dg16_qap_r1cs: violations ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", PROVER_CURVES)
def test_violations_count_and_first_row(curve):
    F = FR[curve]
    p = F.p
    r1cs, w = instance(F, 10, seed=11, below=True)         # 511 constraints: two workgroups, padding rows
    nc = r1cs["num_constraints"]
    assert qap_r1cs(curve, r1cs, w)[3] == (0, None)
    # the last constraint's output wire: only the last row is violated
    w_last = list(w)
    w_last[-1] = (w_last[-1] + 1) % p
    assert violated_rows(r1cs, w_last, p) == [nc - 1]
    assert qap_r1cs(curve, r1cs, w_last)[3] == (1, nc - 1)
    # row 0's output wire
    out0 = r1cs["c"][0][0][1]
    w_first = list(w)
    w_first[out0] = (w_first[out0] + 1) % p
    bad = violated_rows(r1cs, w_first, p)
    assert bad[0] == 0
    assert qap_r1cs(curve, r1cs, w_first)[3] == (len(bad), 0)
    # a free wire many rows read: many rows, several workgroups
    w_many = list(w)
    w_many[2] = (w_many[2] + 1) % p
    bad = violated_rows(r1cs, w_many, p)
    assert len(bad) > 1
    assert qap_r1cs(curve, r1cs, w_many)[3] == (len(bad), bad[0])
    # one C coefficient perturbed
    k = nc // 2
    r2 = dict(r1cs, c=[list(row) for row in r1cs["c"]])
    r2["c"][k] = [((r2["c"][k][0][0] + 1) % p, r2["c"][k][0][1])]
    assert violated_rows(r2, w, p) == [k]
    assert qap_r1cs(curve, r2, w)[3] == (1, k)
    # the strided form counts the rows it evaluates and names the row of the system, not the slot
    got = qap_r1cs(curve, r1cs, w_many, row_start=1, row_stride=4)[3]
    sub = [i for i in bad if i % 4 == 1]
    assert got == (len(sub), sub[0] if sub else None)


def test_violations_raw_words_on_device_pointers():
    """The device-pointer form writes (0, UINT64_MAX) for a satisfied witness, stream-ordered, valid after sync."""
    import torch
    curve, F = "bn254", FR["bn254"]
    dev = torch.device("cuda", 0)
    r1cs, w = instance(F, 6, seed=5)
    nc, ni, nv = r1cs["num_constraints"], r1cs["num_instance"], len(w)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)      # noqa: E731
    mats = [up(x) for k in "abc" for x in csr_of(F, r1cs[k])]
    wd = up(enc_fr(F, w))
    out = [torch.empty(64 * 32, dtype=torch.uint8, device=dev) for _ in range(3)]
    viol = torch.full((2,), 7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx().qap_r1cs_dev(curve, nc, ni, nv, 6, [t.data_ptr() for t in mats], wd.data_ptr(), *[t.data_ptr() for t in out],
                       violations_ptr=viol.data_ptr())
    ctx().sync(0)
    assert [int(x) & U64_MAX for x in viol.cpu().numpy()] == [0, U64_MAX]
    a, b, c, _ = M.libsnark_abc(r1cs, w, F)
    assert np.array_equal(out[2].cpu().numpy().view(np.uint64).reshape(-1, 4), enc_fr(F, c))
    # violations = NULL is legal
    ctx().qap_r1cs_dev(curve, nc, ni, nv, 6, [t.data_ptr() for t in mats], wd.data_ptr(), *[t.data_ptr() for t in out])
    ctx().sync(0)


def test_check_witness_on_the_circom_fixture():
    """The 10 000-constraint circom R1CS with its real witness (solved as tests/test_r1cs_reader.py does)."""
    from dg16_amd.r1cs import R1CS, check_witness
    from test_r1cs_reader import FIX, witness_for_complex_circuit
    p = FR["bn254"].p
    r = R1CS.from_file(FIX)
    w = witness_for_complex_circuit(r, p)
    assert check_witness(ctx(), "bn254", r, w) == (0, None)
    w[5000] = (w[5000] + 1) % p
    rows = dict(a=r.rows(0), b=r.rows(1), c=r.rows(2))
    bad = violated_rows(rows, w, p)
    assert bad
    assert check_witness(ctx(), "bn254", r, w) == (len(bad), bad[0])


# ---- dg16_h_poly with the flag ---------------------------------------------------------------------------------------
# ntt.hip plans: one pass up to 2^10, two up to 2^20, three above.  1, 3, 8, 12: a single butterfly, sub-tile, one LDS
# tile, multi-pass; 10 | 11 and 20 | 21 are the two plan boundaries the seven transforms cross.
@pytest.mark.parametrize("curve", ALL)
@pytest.mark.parametrize("log_m", [1, 3, 8, 10, 11, 12])
def test_h_poly_libsnark_equals_the_model(curve, log_m):
    F = FR[curve]
    m = 1 << log_m
    rng = random.Random(log_m)
    # any a, b with c = a o b on every row is a satisfied system's evaluation vectors (the check needs no R1CS)
    a = [rng.randrange(F.p) for _ in range(m)]
    b = [rng.randrange(F.p) for _ in range(m)]
    c = [x * y % F.p for x, y in zip(a, b)]
    from oracle.pyref.poly import Domain
    h = M.libsnark_h(a, b, c, Domain(F, m))
    assert h[m - 1] == 0
    A, B, C = enc_fr(F, a), enc_fr(F, b), enc_fr(F, c)
    keep = [x.copy() for x in (A, B, C)]
    got = ctx().h_poly(curve, A, B, C, reduction="libsnark")
    assert np.array_equal(got, enc_fr(F, h))
    assert all(np.array_equal(x, y) for x, y in zip((A, B, C), keep))
    # without the flag the call is the circom witness map, as before
    assert np.array_equal(ctx().h_poly(curve, A, B, C), corc.h_poly(curve, A, B, C))


@pytest.mark.parametrize("curve", PROVER_CURVES)
@pytest.mark.parametrize("log_m", [3, 12])
def test_h_poly_libsnark_out_aliases_a(curve, log_m):
    import torch
    F = FR[curve]
    m = 1 << log_m
    dev = torch.device("cuda", 0)
    rng = random.Random(log_m + 40)
    a = [rng.randrange(F.p) for _ in range(m)]
    b = [rng.randrange(F.p) for _ in range(m)]
    c = [x * y % F.p for x, y in zip(a, b)]
    from oracle.pyref.poly import Domain
    h = enc_fr(F, M.libsnark_h(a, b, c, Domain(F, m)))
    up = lambda x: torch.from_numpy(enc_fr(F, x).view(np.int64)).to(dev)      # noqa: E731
    da, db, dc = up(a), up(b), up(c)
    kb, kc = db.clone(), dc.clone()
    torch.cuda.synchronize()
    ctx().h_poly_dev(curve, da.data_ptr(), db.data_ptr(), dc.data_ptr(), log_m, da.data_ptr(), reduction="libsnark")
    ctx().sync(0)
    assert np.array_equal(da.cpu().numpy().view(np.uint64), h)
    assert torch.equal(db, kb) and torch.equal(dc, kc)


def _device_abc(curve, log_m, seed):
    """Random Montgomery a, b on the device and c = a o b by dg16_field_op (not the code under test)."""
    import torch
    from bench import rand_fr
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    m = 1 << log_m
    a, b = rand_fr(m, dev, gen, curve), rand_fr(m, dev, gen, curve)
    c = torch.empty_like(a)
    torch.cuda.synchronize()
    ctx().field_op_dev(curve, "fr", 2, a.data_ptr(), b.data_ptr(), c.data_ptr(), m)
    ctx().sync(0)
    return a, b, c


@pytest.mark.parametrize("curve", PROVER_CURVES)
def test_h_poly_libsnark_quotient_identity_2e16(curve):
    """m = 2^16, where the big-int model is slow: h(x) (x^m - 1) == A(x) B(x) - C(x) at a random x, A, B, C by the
    barycentric formula from the domain values (one batch inversion), h by Horner; and the top coefficient is zero."""
    import torch
    F = FR[curve]
    p, log_m = F.p, 16
    m = 1 << log_m
    a, b, c = _device_abc(curve, log_m, seed=16)
    h = torch.empty_like(a)
    ctx().h_poly_dev(curve, a.data_ptr(), b.data_ptr(), c.data_ptr(), log_m, h.data_ptr(), reduction="libsnark")
    ctx().sync(0)
    av, bv, cv, hv = (dec_fr(F, t.cpu().numpy().view(np.uint64)) for t in (a, b, c, h))
    assert hv[m - 1] == 0
    from oracle.pyref.poly import Domain
    dom = Domain(F, m)
    x = random.Random(16).randrange(2, p)
    assert pow(x, m, p) != 1
    # 1 / (x - w^i) for all i by one inversion
    den, wi = [], 1
    for _ in range(m):
        den.append((x - wi) % p)
        wi = wi * dom.group_gen % p
    pre, acc = [], 1
    for d in den:
        pre.append(acc)
        acc = acc * d % p
    inv = F.inv(acc)
    sa = sb = sc = 0
    wis = [1] * m
    for i in range(1, m):
        wis[i] = wis[i - 1] * dom.group_gen % p
    for i in range(m - 1, -1, -1):
        di = inv * pre[i] % p
        inv = inv * den[i] % p
        t = wis[i] * di % p
        sa, sb, sc = (sa + av[i] * t) % p, (sb + bv[i] * t) % p, (sc + cv[i] * t) % p
    k = (pow(x, m, p) - 1) * dom.size_inv % p
    Ax, Bx, Cx = sa * k % p, sb * k % p, sc * k % p
    assert M.horner(hv, x, p) * (pow(x, m, p) - 1) % p == (Ax * Bx - Cx) % p


@pytest.mark.parametrize("log_m", [20, 21])
def test_h_poly_libsnark_on_the_odd_coset_at_the_three_pass_boundary(log_m):
    """2^20 | 2^21: the last two-pass and the first three-pass plan (and, from 2^21, the passes' one-table twiddles), where
    Python big ints are too slow even for one barycentric evaluation.  The identity is checked on ALL points of the odd
    coset xi H, xi = w_2m, instead: h Z = A B - C there reads h(xi w^i) (xi^m - 1) = -2 h(xi w^i) = circom_h[i], with
    h(xi w^i) from dg16_ntt with the coset offset and circom_h from dg16_h_poly without the flag -- both compared with
    the oracle bit for bit in tests/test_gpu_ntt.py.  All values are canonical, so the comparison is exact."""
    import torch
    curve = "bn254"
    F = FR[curve]
    m = 1 << log_m
    a, b, c = _device_abc(curve, log_m, seed=log_m)
    h, hc = torch.empty_like(a), torch.empty_like(a)
    ctx().h_poly_dev(curve, a.data_ptr(), b.data_ptr(), c.data_ptr(), log_m, h.data_ptr(), reduction="libsnark")
    ctx().h_poly_dev(curve, a.data_ptr(), b.data_ptr(), c.data_ptr(), log_m, hc.data_ptr())
    ctx().sync(0)
    assert not bool(h[m - 1].any())                      # the top coefficient
    xi = enc_fr(F, [F.root_of_unity(2 * m)])
    ctx().ntt_dev(curve, h.data_ptr(), log_m, coset=xi)
    ctx().field_op_dev(curve, "fr", 0, h.data_ptr(), h.data_ptr(), h.data_ptr(), m)        # 2 h
    ctx().field_op_dev(curve, "fr", 7, h.data_ptr(), None, h.data_ptr(), m)                # -2 h
    ctx().sync(0)
    assert torch.equal(h, hc)


# ---- setup with the flag ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", ALL)
@pytest.mark.parametrize("log_m", [3, 7])
def test_setup_libsnark_h_query(curve, log_m):
    import dg16_amd
    F = FR[curve]
    m = 1 << log_m
    r1cs, _ = instance(F, log_m, seed=log_m + 1, below=(log_m == 7))
    rng = random.Random(log_m)
    td = tuple(rng.randrange(2, F.p) for _ in range(5))
    sc = M.libsnark_setup_scalars(r1cs, F, td)
    circom = dg16_amd.generate_parameters(ctx(), curve, system_of(F, r1cs), trapdoor=td)
    params = dg16_amd.generate_parameters(ctx(), curve, system_of(F, r1cs), trapdoor=td, reduction="libsnark")
    assert params.domain_size == m
    hq = params.host("h_query")
    assert hq.shape[0] == m and not hq[m - 1].any()
    gen = corc.generator(curve, 1)
    exp = np.stack([np.asarray(corc.point_mul(curve, 1, gen, s)).reshape(-1) for s in sc["h"][:m - 1]])
    assert np.array_equal(hq[:m - 1], exp)
    assert not np.array_equal(hq, circom.host("h_query"))
    for name in dg16_amd.Parameters.NAMES:
        if name != "h_query":
            assert np.array_equal(params.host(name), circom.host(name)), name


# ---- end to end ------------------------------------------------------------------------------------------------------
def _affine_proof(curve, A, B, C):
    return np.concatenate([np.asarray(corc.jac_to_affine(curve, 1, A)).reshape(-1),
                           np.asarray(corc.jac_to_affine(curve, 2, B)).reshape(-1),
                           np.asarray(corc.jac_to_affine(curve, 1, C)).reshape(-1)])


@pytest.mark.parametrize("curve", PROVER_CURVES)
@pytest.mark.parametrize("log_m", [6, 10])
def test_setup_prove_verify_end_to_end(curve, log_m):
    import dg16_amd
    F = FR[curve]
    p = F.p
    r1cs, w = instance(F, log_m, seed=3 * log_m, below=(log_m == 10))
    ni = r1cs["num_instance"]
    rng = random.Random(log_m)
    td = tuple(rng.randrange(2, p) for _ in range(5))
    r, s = rng.randrange(1, p), rng.randrange(1, p)
    sc = M.libsnark_setup_scalars(r1cs, F, td)
    params = dg16_amd.generate_parameters(ctx(), curve, system_of(F, r1cs), trapdoor=td, reduction="libsnark")
    dpk = params.proving_key(ctx())
    pvk = dg16_amd.PreparedVerifyingKey.from_parameters(ctx(), params)
    pub = corc.ints_to_arr([x % p for x in w[1:ni]], 4)
    try:
        a, b, c, viol = qap_r1cs(curve, r1cs, w)
        assert viol == (0, None)
        proof = _affine_proof(curve, *ctx().prove(dpk, a, b, c, enc_fr(F, w), enc_fr(F, [r]), enc_fr(F, [s]),
                                                  reduction="libsnark"))
        # the model's proof: its discrete logs times the generators
        ma, mb, mc, dom = M.libsnark_abc(r1cs, w, F)
        sa, sb, scc = M.libsnark_proof_scalars(r1cs, F, td, sc, r, s, w, M.libsnark_h(ma, mb, mc, dom))
        assert G.verify_in_exponent(r1cs, F, td, sc, (sa, sb, scc), w)
        exp = np.concatenate([np.asarray(corc.point_mul(curve, g, corc.generator(curve, g), k)).reshape(-1)
                              for g, k in ((1, sa), (2, sb), (1, scc))])
        assert np.array_equal(proof, exp)
        assert list(pvk.verify_batch(pub, proof)) == [True]
        # the same witness without the prove flag against the Libsnark key: the flag selects something
        circom = _affine_proof(curve, *ctx().prove(dpk, a, b, c, enc_fr(F, w), enc_fr(F, [r]), enc_fr(F, [s])))
        assert list(pvk.verify_batch(pub, circom)) == [False]
        # an unsatisfying witness: reported, and its proof rejected
        w_bad = list(w)
        w_bad[-1] = (w_bad[-1] + 1) % p
        a2, b2, c2, viol = qap_r1cs(curve, r1cs, w_bad)
        assert viol == (1, r1cs["num_constraints"] - 1)
        bad = _affine_proof(curve, *ctx().prove(dpk, a2, b2, c2, enc_fr(F, w_bad), enc_fr(F, [r]), enc_fr(F, [s]),
                                                reduction="libsnark"))
        assert list(pvk.verify_batch(pub, bad)) == [False]
    finally:
        dpk.close()
        pvk.close()


# ---- a queue of proofs -----------------------------------------------------------------------------------------------
def test_queue_of_libsnark_proofs_with_overlap_tail():
    """Three witnesses through one context with DG16_F_OVERLAP_TAIL, a circom proof on another key between them: every
    proof is bit-equal to the proof of the same inputs made one at a time (tests/test_gpu_queue_fences.py has the rule).
    Proofs are compared as affine points, converted by the oracle: the queued form reduces H's buckets with another
    kernel shape than the one-at-a-time form, so the Jacobian representatives of the same point may differ."""
    import torch
    import dg16_amd
    curve, log_m = "bn254", 10
    F = FR[curve]
    p = F.p
    dev = torch.device("cuda", 0)
    r1cs, w0 = instance(F, log_m, seed=77)
    nc, ni, nv, m = r1cs["num_constraints"], r1cs["num_instance"], len(w0), 1 << log_m
    rng = random.Random(77)
    td = tuple(rng.randrange(2, p) for _ in range(5))
    lib_params = dg16_amd.generate_parameters(ctx(), curve, system_of(F, r1cs), trapdoor=td, reduction="libsnark")
    cir_params = dg16_amd.generate_parameters(ctx(), curve, system_of(F, r1cs), trapdoor=td[::-1])
    lib_pk, cir_pk = lib_params.proving_key(ctx()), cir_params.proving_key(ctx())
    # three witnesses (the two perturbed ones do not satisfy the system: the pipeline runs all the same)
    ws = [list(w0), list(w0), list(w0)]
    ws[1][3] = (ws[1][3] + 1) % p
    ws[2][-1] = (ws[2][-1] + 5) % p
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)      # noqa: E731
    mats = [up(x) for k in "abc" for x in csr_of(F, r1cs[k])]
    jobs = []                     # (key, reduction, w, a, b, c, rs)
    for i, w in enumerate([ws[0], ws[1], None, ws[2]]):
        libsnark = w is not None
        w = ws[0] if w is None else w
        wd = up(enc_fr(F, w))
        abc = [torch.empty(m * 32, dtype=torch.uint8, device=dev) for _ in range(3)]
        torch.cuda.synchronize()
        if libsnark:
            ctx().qap_r1cs_dev(curve, nc, ni, nv, log_m, [t.data_ptr() for t in mats], wd.data_ptr(),
                               *[t.data_ptr() for t in abc])
        else:
            ctx().qap_dev(curve, nc, ni, nv, log_m, *[t.data_ptr() for t in mats[:6]], wd.data_ptr(),
                          *[t.data_ptr() for t in abc])
        ctx().sync(0)
        rs = enc_fr(F, [rng.randrange(1, p), rng.randrange(1, p)])
        jobs.append((lib_pk if libsnark else cir_pk, "libsnark" if libsnark else "circom", wd, abc, rs))

    def run(overlap):
        outs = [torch.zeros(12 * 32, dtype=torch.uint8, device=dev) for _ in jobs]
        torch.cuda.synchronize()
        for (pk, red, wd, abc, rs), out in zip(jobs, outs):
            ctx().prove_dev(pk, abc[0].data_ptr(), abc[1].data_ptr(), abc[2].data_ptr(), wd.data_ptr(), rs,
                            out.data_ptr(), overlap_tail=overlap, reduction=red)
            if not overlap:
                for ch in range(3):
                    ctx().sync(ch)
        for ch in range(3):
            ctx().sync(ch)
        return [_affine_proof(curve, *np.split(o.cpu().numpy().view(np.uint64), [12, 36])) for o in outs]

    try:
        one_at_a_time = run(False)
        queued = run(True)
        again = run(True)
        for i, (x, y, z) in enumerate(zip(one_at_a_time, queued, again)):
            assert x.any() and np.array_equal(x, y) and np.array_equal(x, z), i
        assert not np.array_equal(one_at_a_time[0], one_at_a_time[1])
    finally:
        lib_pk.close()
        cir_pk.close()


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_sharded_entry_points_refuse_the_flag():
    import ctypes
    import torch
    import dg16_amd
    from dg16_amd import lib
    curve, log_m = "bn254", 4
    F = FR[curve]
    dev = torch.device("cuda", 0)
    c_ = ctx()
    r1cs, w = instance(F, log_m, seed=9)
    params = dg16_amd.generate_parameters(c_, curve, system_of(F, r1cs), trapdoor=(3, 5, 7, 11, 13), reduction="libsnark")
    pk = params.proving_key(c_)
    m = 1 << log_m
    buf = [torch.zeros(m * 32, dtype=torch.uint8, device=dev) for _ in range(5)]
    wd = torch.zeros(len(w) * 32, dtype=torch.uint8, device=dev)
    rs = enc_fr(F, [1, 2])
    res = torch.zeros(4096, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    vp = ctypes.c_void_p
    P = lambda t: vp(t.data_ptr())          # noqa: E731
    flags = lib.F_DEVICE_PTRS | lib.F_SCALARS_MONT | lib.F_QAP_LIBSNARK
    rsp = rs.ctypes.data_as(vp)
    ins = (vp * 3)(buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr())
    L = c_.L
    calls = {
        "dg16_groth16_msms": lambda: L.dg16_groth16_msms(c_.h, pk.h, P(buf[0]), P(buf[1]), P(buf[2]), P(wd), rsp, flags, P(res)),
        "dg16_groth16_msms_h": lambda: L.dg16_groth16_msms_h(c_.h, pk.h, P(buf[3]), P(wd), rsp, flags, P(res)),
        "dg16_groth16_prove_dist": lambda: L.dg16_groth16_prove_dist(c_.h, pk.h, None, P(buf[0]), P(buf[1]), P(buf[2]), P(wd),
                                                                     rsp, flags, P(res)),
        "dg16_h_poly_dist": lambda: L.dg16_h_poly_dist(c_.h, 0, None, P(buf[0]), P(buf[1]), P(buf[2]), log_m, P(buf[4]),
                                                       flags, 0),
        "dg16_h_poly_dist_stage": lambda: L.dg16_h_poly_dist_stage(c_.h, 0, log_m, 0, 2, 0, ins, P(buf[4]), flags, 0),
    }
    try:
        for name, call in calls.items():
            assert call() == 7, name                                   # DG16_ERR_UNSUPPORTED
            assert b"LIBSNARK" in L.dg16_last_error(c_.h), name
        for ch in range(3):
            c_.sync(ch)
    finally:
        pk.close()
    with pytest.raises(ValueError):
        c_.h_poly(curve, rs, rs, rs, reduction="bellman")
