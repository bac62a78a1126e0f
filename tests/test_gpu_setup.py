"""dg16_groth16_setup / keygen.generate_parameters on the GPU against the CPU oracle (oracle.pyref.groth16.setup,
corc.point_mul) and the pairing verifier -- never against the code under test."""

import random
import time

import numpy as np
import pytest

from oracle import corc
from oracle.pyref.fields import FQ, FR
from oracle.pyref.curves import CURVES
from oracle.pyref import groth16 as G
from gpu_util import ctx
from test_gpu_prover import enc_fr, enc_g1, enc_g2, dec_g1, dec_g2

pytestmark = pytest.mark.gpu

ALL = ["bn254", "bls12_381", "bls12_377"]


def csr_of(F, rows):
    ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    col = np.array([i for r in rows for _, i in r], dtype=np.uint32)
    coeff = enc_fr(F, [c for r in rows for c, _ in r]).reshape(-1, 4)
    return ptr, col, coeff


def system_of(F, r1cs):
    return dict(num_constraints=r1cs["num_constraints"], num_inputs=r1cs["num_instance"],
                num_vars=r1cs["num_instance"] + r1cs["num_witness"], a=csr_of(F, r1cs["a"]), b=csr_of(F, r1cs["b"]),
                c=csr_of(F, r1cs["c"]))


def expected_arrays(curve, pk):
    Fq = FQ[curve]
    fixed = np.concatenate([enc_g1(Fq, [pk["alpha_g1"], pk["beta_g1"], pk["delta_g1"]]).reshape(-1),
                            enc_g2(Fq, [pk["beta_g2"], pk["delta_g2"]]).reshape(-1)])
    return dict(a_query=enc_g1(Fq, pk["a_query"]), b_g1_query=enc_g1(Fq, pk["b_g1_query"]),
                b_g2_query=enc_g2(Fq, pk["b_g2_query"]), h_query=enc_g1(Fq, pk["h_query"]),
                l_query=enc_g1(Fq, pk["l_query"]), fixed_points=fixed.reshape(-1, Fq.limbs64),
                gamma_g2=enc_g2(Fq, [pk["gamma_g2"]]), gamma_abc_g1=enc_g1(Fq, pk["gamma_abc_g1"]))


@pytest.mark.parametrize("curve", ALL)
@pytest.mark.parametrize("nc,ni,nw", [(17, 2, 9), (100, 3, 120), (255, 1, 300)])
def test_key_equals_the_oracles_small(curve, nc, ni, nw):
    import dg16_amd
    F = FR[curve]
    r1cs, _ = G.synthetic_r1cs(F, num_constraints=nc, num_instance=ni, num_witness=nw, seed=nc)
    rng = random.Random(nc)
    td = tuple(rng.randrange(1, F.p) for _ in range(5))
    pk, sc = G.setup(curve, r1cs, td)
    if nw > nc:       # wires that appear in no row of A or B: their query points are the identity
        assert sum(1 for P in pk["a_query"] if P is None) > 0 and sum(1 for P in pk["b_g2_query"] if P is None) > 0
    params = dg16_amd.generate_parameters(ctx(), curve, system_of(F, r1cs), trapdoor=td)
    assert params.domain_size == sc["m"]
    for name, exp in expected_arrays(curve, pk).items():
        assert np.array_equal(params.host(name), exp), (curve, name)


def test_key_with_other_generators():
    import dg16_amd
    curve = "bn254"
    F, Fq = FR[curve], FQ[curve]
    g1, g2 = CURVES[curve, "g1"], CURVES[curve, "g2"]
    r1cs, _ = G.synthetic_r1cs(F, num_constraints=20, num_instance=2, num_witness=25, seed=4)
    td = tuple(random.Random(6).randrange(1, F.p) for _ in range(5))
    sc = G.setup_scalars(r1cs, F, td)
    P1, P2 = g1.mul(g1.gen, 5), g2.mul(g2.gen, 11)
    params = dg16_amd.generate_parameters(ctx(), curve, system_of(F, r1cs), trapdoor=td,
                                          generators=(enc_g1(Fq, [P1]), enc_g2(Fq, [P2])))
    alpha, beta, gamma, delta, _ = td
    assert np.array_equal(params.host("a_query"), enc_g1(Fq, [g1.mul(P1, s) for s in sc["a"]]))
    assert np.array_equal(params.host("b_g2_query"), enc_g2(Fq, [g2.mul(P2, s) for s in sc["b"]]))
    assert np.array_equal(params.host("h_query"), enc_g1(Fq, [g1.mul(P1, s) for s in sc["h"]]))
    assert np.array_equal(params.host("l_query"), enc_g1(Fq, [g1.mul(P1, s) for s in sc["l"]]))
    assert np.array_equal(params.host("gamma_abc_g1"), enc_g1(Fq, [g1.mul(P1, s) for s in sc["gamma_abc"]]))
    assert np.array_equal(params.host("gamma_g2"), enc_g2(Fq, [g2.mul(P2, gamma)]))
    fixed = np.concatenate([enc_g1(Fq, [g1.mul(P1, alpha), g1.mul(P1, beta), g1.mul(P1, delta)]).reshape(-1),
                            enc_g2(Fq, [g2.mul(P2, beta), g2.mul(P2, delta)]).reshape(-1)])
    assert np.array_equal(params.host("fixed_points").reshape(-1), fixed)


@pytest.mark.parametrize("curve", ALL)
def test_proof_from_gpu_key_in_the_exponent(curve):
    """nc ~ 2^13: GPU key -> resident key -> proof with drawn r, s == proof_scalars_from_trapdoor * G (three
    corc.point_mul): one equation per proof element that every query point enters.  (BLS12-377, for which the resident
    prover is not built, proves through dg16_msm / dg16_h_poly: _prove_with_msms.)"""
    import dg16_amd
    F = FR[curve]
    nc, ni, nw = 8000, 3, 8100
    r1cs, w = G.synthetic_r1cs(F, num_constraints=nc, num_instance=ni, num_witness=nw, seed=21)
    rng = random.Random(22)
    td = tuple(rng.randrange(1, F.p) for _ in range(5))
    sc = G.setup_scalars(r1cs, F, td)
    params = dg16_amd.generate_parameters(ctx(), curve, system_of(F, r1cs), trapdoor=td)
    a, b, c, dom = G.qap(r1cs, w, F)
    assert dom.size == params.domain_size == 8192
    r, s = rng.randrange(1, F.p), rng.randrange(1, F.p)
    if curve == "bls12_377":
        A, B, C = _prove_with_msms(curve, params, a, b, c, w, r, s)
    else:
        dpk = params.proving_key(ctx())
        A, B, C = ctx().prove(dpk, enc_fr(F, a), enc_fr(F, b), enc_fr(F, c), enc_fr(F, w), enc_fr(F, [r]), enc_fr(F, [s]))
        dpk.close()
        A, B, C = corc.jac_to_affine(curve, 1, A), corc.jac_to_affine(curve, 2, B), corc.jac_to_affine(curve, 1, C)
    sa, sb, scc = G.proof_scalars_from_trapdoor(r1cs, F, td, sc, r, s, w)
    assert G.verify_in_exponent(r1cs, F, td, sc, (sa, sb, scc), w)
    assert np.array_equal(A, corc.point_mul(curve, 1, corc.generator(curve, 1), sa))
    assert np.array_equal(B, corc.point_mul(curve, 2, corc.generator(curve, 2), sb))
    assert np.array_equal(C, corc.point_mul(curve, 1, corc.generator(curve, 1), scc))


def _prove_with_msms(curve, params, a, b, c, w, r, s):
    """The proof over the GPU key for a curve the resident prover is not built for (dg16_pk_create: BN254 and
    BLS12-381): the five MSMs through dg16_msm and the h-polynomial through dg16_h_poly, the A / B / C assembly of
    groth16/src/prove.rs:21-136 with the oracle's point arithmetic.  Every query point enters, as in dg16_groth16_prove."""
    F = FR[curve]
    ni = params.num_inputs
    fq = FQ[curve].limbs64
    add = lambda g, P, Q: corc.point_add(curve, g, P, Q)            # noqa: E731
    mul = lambda g, P, k: corc.point_mul(curve, g, P, k % F.p)      # noqa: E731
    wv = enc_fr(F, w)
    msm = lambda g, name, sc: ctx().msm(curve, g, params.host(name), sc, scalars_mont=True, affine=True)   # noqa: E731
    f = params.host("fixed_points").reshape(-1)
    alpha_g1, beta_g1, delta_g1 = (f[2 * fq * i:2 * fq * (i + 1)].reshape(1, -1) for i in range(3))
    beta_g2, delta_g2 = (f[6 * fq + 4 * fq * i:6 * fq + 4 * fq * (i + 1)].reshape(1, -1) for i in range(2))
    h = ctx().h_poly(curve, enc_fr(F, a), enc_fr(F, b), enc_fr(F, c))
    A = add(1, add(1, alpha_g1, msm(1, "a_query", wv)), mul(1, delta_g1, r))
    B1 = add(1, add(1, beta_g1, msm(1, "b_g1_query", wv)), mul(1, delta_g1, s))
    B = add(2, add(2, beta_g2, msm(2, "b_g2_query", wv)), mul(2, delta_g2, s))
    C = add(1, msm(1, "l_query", wv[ni:]), msm(1, "h_query", h))
    C = add(1, add(1, C, mul(1, A, s)), add(1, mul(1, B1, r), mul(1, delta_g1, -(r * s))))
    return A, B, C


def _satisfied_instance(log_m, seed):
    """A satisfied BN254 instance with m = 2^log_m built on the GPU: rows of A and B have 3 random non-zeros over the
    first F wires (instance + free witness), constraint i's output wire F + i has C row [(1, F + i)] and the value
    <A_i, w> <B_i, w> taken from dg16_qap's own c_out.  Everything in Montgomery form."""
    import torch
    from bench import rand_fr as bench_rand_fr
    curve = "bn254"
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    m, ni = 1 << log_m, 2
    nc = m - ni
    free = min(1 << 16, m // 4)
    nv = free + nc

    def rand_fr(n):      # uniform limbs with the top limb below the modulus': a valid (Montgomery) element
        return bench_rand_fr(n, dev, gen, curve)

    row_ptr = (torch.arange(nc + 1, dtype=torch.int64, device=dev) * 3).to(torch.int32)
    a_col = torch.randint(0, free, (3 * nc,), dtype=torch.int32, device=dev, generator=gen)
    b_col = torch.randint(0, free, (3 * nc,), dtype=torch.int32, device=dev, generator=gen)
    a_val, b_val = rand_fr(3 * nc), rand_fr(3 * nc)
    c_ptr = torch.arange(nc + 1, dtype=torch.int32, device=dev)
    c_col = (torch.arange(nc, dtype=torch.int64, device=dev) + free).to(torch.int32)
    one = torch.from_numpy(enc_fr(FR[curve], [1]).view(np.int64)).to(dev)
    c_val = one.repeat(nc, 1).contiguous()
    w = torch.zeros((nv, 4), dtype=torch.int64, device=dev)
    w[:free] = rand_fr(free)
    w[0] = one[0]
    abc = [torch.empty((m, 4), dtype=torch.int64, device=dev) for _ in range(3)]
    torch.cuda.synchronize()

    def qap():
        ctx().qap_dev(curve, nc, ni, nv, log_m, row_ptr.data_ptr(), a_col.data_ptr(), a_val.data_ptr(),
                      row_ptr.data_ptr(), b_col.data_ptr(), b_val.data_ptr(), w.data_ptr(), abc[0].data_ptr(),
                      abc[1].data_ptr(), abc[2].data_ptr(), scalars_mont=True)
        ctx().sync(0)

    qap()
    w[free:] = abc[2][:nc]              # output wires: <A_i, w> <B_i, w>
    torch.cuda.synchronize()
    qap()
    system = dict(num_constraints=nc, num_inputs=ni, num_vars=nv, a=(row_ptr, a_col, a_val),
                  b=(row_ptr, b_col, b_val), c=(c_ptr, c_col, c_val))
    return system, w, abc


def _prove_affine(params, w, abc, rs):
    import torch
    pk = params.proving_key(ctx())
    proof = torch.empty(12 * 32, dtype=torch.uint8, device=w.device)
    torch.cuda.synchronize()
    ctx().prove_dev(pk, abc[0].data_ptr(), abc[1].data_ptr(), abc[2].data_ptr(), w.data_ptr(), rs, proof.data_ptr())
    for ch in range(3):
        ctx().sync(ch)
    j = proof.cpu().numpy().view(np.uint64)
    pk.close()
    return np.concatenate([ctx().to_affine("bn254", 1, j[:12]).reshape(-1), ctx().to_affine("bn254", 2, j[12:36]).reshape(-1),
                           ctx().to_affine("bn254", 1, j[36:]).reshape(-1)])


@pytest.mark.parametrize("log_m", [12, 20])
def test_generated_key_proves_and_the_pairing_verifier_accepts(log_m):
    """Key generation, proof and pairing check at the headline size (m = 2^20) and, to tell a failure at size from a
    failure of the construction, at 2^12.  The verifier accepts the proof, rejects it for an incremented public input,
    and rejects a proof made with a key from a different tau.  Measured on an MI355X: the whole 2^20 case (two keys,
    two resident keys with their window tables, two proofs, three host pairing checks) takes 1.9 s of the 60 s budget,
    so the headline size is kept."""
    import torch
    import dg16_amd
    from dg16_amd import verify
    t0 = time.perf_counter()
    F = FR["bn254"]
    system, w, abc = _satisfied_instance(log_m, seed=log_m)
    rng = random.Random(log_m)
    td = tuple(rng.randrange(1, F.p) for _ in range(5))
    rs = enc_fr(F, [rng.randrange(1, F.p), rng.randrange(1, F.p)])
    params = dg16_amd.generate_parameters(ctx(), "bn254", system, trapdoor=td)
    t_key = time.perf_counter() - t0
    vk = params.verifying_key()
    proof = _prove_affine(params, w, abc, rs)
    del params
    torch.cuda.empty_cache()
    pub = ctx().field_op("bn254", "fr", "from_mont", w[1:2].cpu().numpy().view(np.uint64))
    assert verify.verify_proof(*vk, pub, proof)
    x = (int(corc.arr_to_ints(pub)[0]) + 1) % F.p
    assert not verify.verify_proof(*vk, corc.ints_to_arr([x], 4), proof)
    other = dg16_amd.generate_parameters(ctx(), "bn254", system, trapdoor=td[:4] + ((td[4] + 1) % F.p or 1,))
    assert np.array_equal(other.verifying_key()[0], vk[0])          # same alpha .. delta: only tau differs
    bad = _prove_affine(other, w, abc, rs)
    del other
    torch.cuda.empty_cache()
    assert not verify.verify_proof(*vk, pub, bad)
    total = time.perf_counter() - t0
    print("\nsetup+prove+verify m=2^%d: first key %.2f s, whole case (two keys, two proofs, three pairing checks) %.2f s"
          % (log_m, t_key, total))
    assert total < 60.0


def test_setup_argument_errors():
    import dg16_amd
    curve = "bn254"
    F = FR[curve]
    r1cs, w = G.synthetic_r1cs(F, num_constraints=28, num_instance=2, num_witness=40, seed=28)
    system = system_of(F, r1cs)
    c_ = ctx()
    good = (3, 5, 7, 11, 13)

    def call(td, log_m=5, null_out=None):
        td = corc.ints_to_arr(list(td), 4)
        outs = [np.zeros(n, dtype=np.uint64) for n in (42 * 8, 42 * 8, 42 * 16, 32 * 8, 40 * 8, 3 * 8 + 2 * 16, 16, 2 * 8)]
        if null_out is not None:
            outs[null_out] = None
        c_.groth16_setup(curve, 28, 2, 42, log_m, system["a"], system["b"], system["c"], td, outs)
        return outs

    for td in ((0, 5, 7, 11, 13), (3, 5, 0, 11, 13), (3, 5, 7, 11, 0), (3, 5, 7, 11, F.p), (3, 5, 7, 11, 1),
               (3, 5, 7, 11, F.p - 1)):       # zero, not below r, tau = 1 and tau = -1: tau^m = 1
        with pytest.raises(dg16_amd.Dg16Error) as e:
            call(td)
        assert e.value.code == 3
    with pytest.raises(dg16_amd.Dg16Error) as e:
        call(good, log_m=4)                   # 2^4 < 28 + 2
    assert e.value.code == 3
    for k in (0, 3, 5, 7):
        with pytest.raises(dg16_amd.Dg16Error) as e:
            call(good, null_out=k)
        assert e.value.code == 3
    # ... and the context generates and proves correctly afterwards
    pk, sc = G.setup(curve, r1cs, good)
    outs = call(good)
    assert np.array_equal(outs[0].reshape(-1, 8), enc_g1(FQ[curve], pk["a_query"]))
    dpk = c_.pk_create(curve, 42, 2, 32, *[o for o in outs[:6]])
    a, b, c, dom = G.qap(r1cs, w, F)
    A, B, C = c_.prove(dpk, enc_fr(F, a), enc_fr(F, b), enc_fr(F, c), enc_fr(F, w), enc_fr(F, [9]), enc_fr(F, [10]))
    eA, eB, eC = G.create_proof(curve, pk, 9, 10, r1cs, w)
    Fq = FQ[curve]
    assert (dec_g1(Fq, corc.jac_to_affine(curve, 1, A)), dec_g2(Fq, corc.jac_to_affine(curve, 2, B)),
            dec_g1(Fq, corc.jac_to_affine(curve, 1, C))) == (eA, eB, eC)
    dpk.close()


@pytest.mark.parametrize("group", [1, 2])
def test_fixed_base_is_windowed_ratio_to_msm_below_8(group):
    """n = 2^20, BN254: dg16_fixed_base_mul takes less than 8x dg16_msm over fresh bases at the same n (median of three
    timed repetitions each, same process).  A double-and-add chain per point would be above 20x."""
    import torch
    from bench import rand_fr
    curve, n = "bn254", 1 << 20
    dev = torch.device("cuda", 0)
    c_ = ctx()
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    sc = rand_fr(n, dev, gen, curve)
    pb = 64 * group
    bases = torch.empty(n * pb, dtype=torch.uint8, device=dev)
    out = torch.empty(n * pb, dtype=torch.uint8, device=dev)
    res = torch.empty(3 * pb // 2, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    c_.gen_bases_dev(curve, group, 77, n, bases.data_ptr())
    c_.sync(0)

    def timed(fn):
        ts = []
        for i in range(4):                      # one warm-up, three timed
            t0 = time.perf_counter()
            fn()
            c_.sync(0)
            ts.append(time.perf_counter() - t0)
        return sorted(ts[1:])[1]

    t_msm = timed(lambda: c_.msm_dev(curve, group, bases.data_ptr(), sc.data_ptr(), n, res.data_ptr(), in_subgroup=True))
    t_fb = timed(lambda: c_.fixed_base_mul_dev(curve, group, sc.data_ptr(), n, out.data_ptr()))
    print("\nBN254 G%d n=2^20: fixed_base_mul %.3f ms, msm %.3f ms, ratio %.2f" % (group, 1e3 * t_fb, 1e3 * t_msm, t_fb / t_msm))
    assert t_fb / t_msm < 8.0
