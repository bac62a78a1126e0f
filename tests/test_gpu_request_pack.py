"""GPU: dg16_fr_expand (Context.fr_expand), dg16_pss_pack_scalars (PackedSharingParams.pack_scalars,
pack_from_public_rand) and dg16_request_pack (groth16_mpc.pack_request): the shares of all parties of a scalar vector or
of a whole proof request, plain or blinded (csrc/pss_scalars.h).  Without blinds the contract is byte equality with the
numpy composition over dg16_pss_apply (groth16_mpc.qap_pss, pack_from_witness); with blinds the reference is the oracle's
pack_from_public_rand with the same randomness and hashlib's SHA-256 (tests/request_pack_cases.py).  Every comparison is
exact."""

import ctypes
import functools
import hashlib
import random

import numpy as np
import pytest

import dist_pool
import request_pack_cases as RC
from oracle import corc
from oracle.pyref import groth16 as G
from oracle.pyref.curves import CURVES
from oracle.pyref.fields import FQ, FR

pytestmark = pytest.mark.gpu

DG16_ERR_BAD_CURVE, DG16_ERR_BAD_ARG = 2, 3
CHUNKS, DFFT = RC.CHUNKS, RC.DFFT
SEED = hashlib.sha256(b"tests/test_gpu_request_pack.py").digest()
SEED2 = hashlib.sha256(b"another request").digest()


def pp_of(curve, l):
    return dist_pool.params(curve, l, parties=1)[0]


@functools.lru_cache(maxsize=None)
def values(curve, n, seed=0):
    """n random field elements: (ints, Montgomery words); shared and read-only"""
    rng = random.Random(0x7a1 + 31 * n + seed)
    ints = tuple(rng.randrange(FR[curve].p) for _ in range(n))
    words = RC.to_words(ints, curve, mont=True)
    words.setflags(write=False)
    return ints, words


def party_major(per_party):
    return np.stack([np.asarray(p) for p in per_party])


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ---- no blinds: the numpy composition over dg16_pss_apply -------------------------------------------------------------------
@pytest.mark.parametrize("l", RC.LS)
@pytest.mark.parametrize("curve", ["bn254", "bls12_377"])
def test_without_blinds_equals_qap_pss_and_pack_from_witness(curve, l):
    """DFFT: m = l (one chunk), 2 l, 64 and 2^12 (16 blocks at l = 1).  CHUNKS: witness lengths 1, l - 1, l + 1 (padding
    in the last chunk) and 1000.  n_values = 0 writes nothing."""
    from dg16_amd import groth16_mpc as M
    pp = pp_of(curve, l)
    for m in sorted({l, 2 * l, 64, 1 << 12}):
        v = [values(curve, m, s)[1] for s in range(3)]
        want = M.qap_pss(pp, *v)
        for k in range(3):
            got = pp.pack_scalars(v[k], DFFT)
            assert got.shape == (pp.n, m // l, 4)
            assert np.array_equal(got, party_major([want[i][k] for i in range(pp.n)])), (m, k)
    for n in sorted({1, l - 1, l + 1, 1000} - {0}):
        w = values(curve, n)[1]
        got = pp.pack_scalars(w, CHUNKS)
        assert got.shape == (pp.n, -(-n // l), 4)
        assert np.array_equal(got, party_major(M.pack_from_witness(pp, w))), n
    assert pp.pack_scalars(np.zeros((0, 4), dtype=np.uint64), CHUNKS).shape == (pp.n, 0, 4)
    assert pp.scalar_chunks(CHUNKS, 0) == 0


@pytest.mark.parametrize("l", RC.LS)
def test_a_plain_request_equals_the_three_host_compositions(l):
    from dg16_amd import groth16_mpc as M
    curve = "bn254"
    pp = pp_of(curve, l)
    m, num_vars, num_inputs = 64, 45, 3
    a, b, c = (values(curve, m, s)[1] for s in range(3))
    w = values(curve, num_vars, 9)[1]
    got = M.pack_request(pp, a, b, c, w, num_inputs)
    qs, a_sh, ax_sh = M.qap_pss(pp, a, b, c), M.pack_from_witness(pp, w[1:]), M.pack_from_witness(pp, w[num_inputs:])
    assert len(got) == pp.n
    for i in range(pp.n):
        assert all(np.array_equal(got[i][0][k], qs[i][k]) for k in range(3)), i
        assert np.array_equal(got[i][1], a_sh[i]) and np.array_equal(got[i][2], ax_sh[i]), i
    # num_vars == num_inputs: an empty ax vector; num_vars = 1: both witness vectors empty
    got = M.pack_request(pp, a, b, c, w[:3], 3)
    assert got[0][2].shape == (0, 4) and np.array_equal(got[1][1], M.pack_from_witness(pp, w[1:3])[1])
    got = M.pack_request(pp, a, b, c, w[:1], 1, seed=SEED)
    assert got[0][1].shape == (0, 4) and got[0][2].shape == (0, 4)


# ---- explicit blinds: the oracle's pack_from_public_rand -----------------------------------------------------------------------
@pytest.mark.parametrize("l", RC.LS)
@pytest.mark.parametrize("curve", ["bn254", "bls12_377"])
def test_explicit_blinds_equal_the_oracle(curve, l):
    """Four chunks of each layout (the CHUNKS vector one short of full, so its last chunk is padded), Montgomery and
    canonical form; pack_from_public_rand is the same call per packing."""
    pp = pp_of(curve, l)
    r = FR[curve].p
    rng = random.Random(0xb1 + l)
    for layout, n in ((DFFT, 4 * l), (CHUNKS, 4 * l - (1 if l > 1 else 0))):
        vals = list(values(curve, n, 5)[0])
        chunks = pp.scalar_chunks(layout, n)
        assert chunks == 4
        blinds = [[rng.randrange(r) for _ in range(l)] for _ in range(chunks)]
        blinds[1] = [0] * l                                  # one chunk packed as by pack_from_public
        blinds[2] = [r - 1] * l
        want = RC.oracle_shares(curve, l, layout, vals, blinds)
        flat = [x for row in blinds for x in row]
        for mont in (True, False):
            got = pp.pack_scalars(RC.to_words(vals, curve, mont), layout, RC.to_words(flat, curve, mont))
            assert [RC.to_ints(row, curve, mont) for row in got] == want, (layout, mont)
    secrets = [[rng.randrange(r) for _ in range(l)] for _ in range(3)]
    blinds = [[rng.randrange(r) for _ in range(l)] for _ in range(3)]
    got = pp.pack_from_public_rand(RC.to_words([x for s in secrets for x in s], curve, True),
                                   RC.to_words([x for s in blinds for x in s], curve, True))
    assert got.shape == (3, pp.n, 4)
    assert [RC.to_ints(g, curve, True) for g in got] == [RC.oracle_pack_rand(curve, l, s, b) for s, b in zip(secrets, blinds)]
    assert [RC.to_ints(u, curve, True) for u in pp.unpack(got)] == secrets


# ---- slices ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l", [2, 8])
def test_across_a_slice_boundary(l):
    """Slices of 64 chunks.  CHUNKS: 65 chunks (one slice and one chunk, the last one padded); DFFT: 128 chunks (two
    slices).  unpack(shares) gives the values back, the chunks at both ends and on both sides of the boundary equal the
    oracle's, the shares are linear in (values, blinds), and the seeded request equals the explicit-blind call when both
    run sliced."""
    from dg16_amd import groth16_mpc as M
    curve = "bn254"
    pp = pp_of(curve, l)
    r = FR[curve].p
    pp.ctx.set_points_mul_slice(64 * pp.n)
    try:
        for layout, n in ((CHUNKS, 65 * l - (l - 1)), (DFFT, 128 * l)):
            chunks = pp.scalar_chunks(layout, n)
            v1, v2 = list(values(curve, n, 1)[0]), list(values(curve, n, 2)[0])
            b1, b2 = list(values(curve, chunks * l, 3)[0]), list(values(curve, chunks * l, 4)[0])
            enc = lambda x: RC.to_words(x, curve, True)      # noqa: E731
            s1 = pp.pack_scalars(enc(v1), layout, enc(b1))
            s2 = pp.pack_scalars(enc(v2), layout, enc(b2))
            s12 = pp.pack_scalars(enc([(x + y) % r for x, y in zip(v1, v2)]), layout,
                                  enc([(x + y) % r for x, y in zip(b1, b2)]))
            i1, i2, i12 = ([RC.to_ints(row, curve, True) for row in s] for s in (s1, s2, s12))
            assert i12 == [[(x + y) % r for x, y in zip(p, q)] for p, q in zip(i1, i2)]
            src = RC.chunk_sources(layout, l, v1)
            for e in (0, 1, 62, 63, 64, chunks - 2, chunks - 1):
                sec = [v1[i] if i is not None else 0 for i in src[e]]
                assert [row[e] for row in i1] == RC.oracle_pack_rand(curve, l, sec, b1[e * l:(e + 1) * l]), (layout, e)
            un = pp.unpack(np.ascontiguousarray(s1.transpose(1, 0, 2)))           # [chunks][l]
            flat = RC.to_ints(un, curve, True)
            assert [flat[e * l + c] for e in range(chunks) for c in range(l) if src[e][c] is not None] == \
                [v1[i] for e in range(chunks) for i in src[e] if i is not None]
            assert all(flat[e * l + c] == 0 for e in range(chunks) for c in range(l) if src[e][c] is None)
        # the seeded request, sliced: m = 128 l, 65 chunks of witness
        m, num_vars = 128 * l, 65 * l + 1 - (l - 1)
        a = values(curve, m, 1)[1]
        w = values(curve, num_vars, 6)[1]
        got = M.pack_request(pp, a, a, a, w, 1, seed=SEED)
        for v, (vals, layout) in enumerate(((a, DFFT), (a, DFFT), (a, DFFT), (w[1:], CHUNKS), (w[1:], CHUNKS))):
            chunks = pp.scalar_chunks(layout, vals.shape[0])
            blinds = RC.to_words(RC.model_expand(curve, SEED, v, 0, chunks * l), curve, True)
            want = pp.pack_scalars(vals, layout, blinds)
            have = party_major([got[i][0][v] if v < 3 else got[i][v - 2] for i in range(pp.n)])
            assert np.array_equal(have, want), v
    finally:
        pp.ctx.set_points_mul_slice(0)


# ---- the expansion ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", list(RC.CURVES))
def test_fr_expand_equals_the_hashlib_model(curve):
    """n = 0, 1, 63, 64, 65 (around a wave), 1000 (four blocks); first around 2^32 and 2^63; several streams; both
    forms."""
    ctx = pp_of(curve, 1).ctx
    cases = [(0, 0, 0), (1, 0, 0), (63, 1, 2**32 - 30), (64, 4, 2**32 - 64), (65, 2**40 + 3, 2**63 - 32), (1000, 2, 0),
             (65, 2**64 - 1, 2**64 - 66)]
    for n, stream, first in cases:
        want = RC.model_expand(curve, SEED, stream, first, n)
        for mont in (False, True):
            got = ctx.fr_expand(curve, SEED, stream, first, n, mont=mont)
            assert got.shape == (n, 4)
            assert RC.to_ints(got, curve, mont) == want, (n, stream, first, mont)
            assert all(v < FR[curve].p for v in RC.to_ints(got))
    # a window of a stream is the stream: element 1000 - 1 of the long call, alone
    assert RC.to_ints(ctx.fr_expand(curve, SEED, 2, 999, 1)) == RC.model_expand(curve, SEED, 2, 999, 1)
    assert RC.to_ints(ctx.fr_expand(curve, SEED2, 2, 999, 1)) != RC.model_expand(curve, SEED, 2, 999, 1)


# ---- the request ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mont", [True, False])
@pytest.mark.parametrize("curve,l", [("bn254", 1), ("bls12_381", 2), ("bls12_377", 4), ("bn254", 8)])
def test_the_seed_path_equals_the_explicit_blind_path(curve, l, mont):
    """Blind (e, k) of output v is element e l + k of stream v, in the form of the inputs.  The same seed gives the same
    bytes; another seed other shares of the same values; equal a and b get different shares (the streams differ)."""
    from dg16_amd import groth16_mpc as M
    pp = pp_of(curve, l)
    m, num_vars, num_inputs = 64, 83, 3
    ints = [values(curve, m, 1)[0], values(curve, m, 1)[0], values(curve, m, 2)[0], values(curve, num_vars, 3)[0]]
    a, b, c, w = (RC.to_words(x, curve, mont) for x in ints)
    assert np.array_equal(a, b)
    got = M.pack_request(pp, a, b, c, w, num_inputs, seed=SEED, mont=mont)
    stacked = [party_major([got[i][0][v] if v < 3 else got[i][v - 2] for i in range(pp.n)]) for v in range(5)]
    jobs = ((a, DFFT), (b, DFFT), (c, DFFT), (w[1:], CHUNKS), (w[num_inputs:], CHUNKS))
    for v, (vals, layout) in enumerate(jobs):
        chunks = pp.scalar_chunks(layout, vals.shape[0])
        blinds = RC.to_words(RC.model_expand(curve, SEED, v, 0, chunks * l), curve, mont)
        assert np.array_equal(stacked[v], pp.pack_scalars(vals, layout, blinds)), v
    again = M.pack_request(pp, a, b, c, w, num_inputs, seed=SEED, mont=mont)
    other = M.pack_request(pp, a, b, c, w, num_inputs, seed=SEED2, mont=mont)
    plain = M.pack_request(pp, a, b, c, w, num_inputs, mont=mont)
    for i in range(pp.n):
        for x, y in zip(got[i][0] + got[i][1:], again[i][0] + again[i][1:]):
            assert np.array_equal(x, y)
    assert not np.array_equal(stacked[0], stacked[1])                   # a == b, streams 0 and 1
    for v in range(5):
        o = party_major([other[i][0][v] if v < 3 else other[i][v - 2] for i in range(pp.n)])
        p = party_major([plain[i][0][v] if v < 3 else plain[i][v - 2] for i in range(pp.n)])
        assert not np.array_equal(o, stacked[v]) and not np.array_equal(p, stacked[v])
        un = [pp.unpack(np.ascontiguousarray(s.transpose(1, 0, 2))) for s in (stacked[v], o, p)]
        assert np.array_equal(un[0], un[1]) and np.array_equal(un[0], un[2])


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def _prove(curve, l, nc, ni, nw, seed):
    """(pk, r1cs, w, the parties' outputs from the plain request, from the blinded one)"""
    from dg16_amd import groth16_mpc as M
    from test_gpu_prover import enc_g1, enc_g2
    F, Fq = FR[curve], FQ[curve]
    ctxs, pps, net, _ = dist_pool.parties(curve, l)
    r1cs, w = G.synthetic_r1cs(F, num_constraints=nc, num_instance=ni, num_witness=nw, seed=3)
    rng = random.Random(5)
    pk, _ = G.setup(curve, r1cs, tuple(rng.randrange(1, F.p) for _ in range(5)))
    a, b, c, dom = G.qap(r1cs, w, F)
    hpk = {k: enc_g1(Fq, pk[k]) for k in ("a_query", "b_g1_query", "h_query", "l_query")}
    hpk["b_g2_query"] = enc_g2(Fq, pk["b_g2_query"])
    crs = M.pack_proving_key(pps[0], hpk, in_subgroup=True)
    enc = lambda vals: RC.to_words(vals, curve, True)      # noqa: E731
    log_m = dom.size.bit_length() - 1
    out = []
    for sd in (None, seed):
        req = M.pack_request(pps[0], enc(a), enc(b), enc(c), enc(w), ni, seed=sd)
        out.append(net.simulate_network_round(
            lambda i, h: M.party_prove(ctxs[i], pps[i], h, crs[i], req[i][0], req[i][1], req[i][2], log_m)))
    plain_req = M.pack_request(pps[0], enc(a), enc(b), enc(c), enc(w), ni)
    blind_req = M.pack_request(pps[0], enc(a), enc(b), enc(c), enc(w), ni, seed=seed)
    assert not np.array_equal(plain_req[0][1], blind_req[0][1])          # the second run did start from other shares
    return pk, r1cs, w, log_m, out[0], out[1]


def test_end_to_end_proof_from_a_blinded_request():
    """BN254, l = 2, 8 parties, m = 2^5: party_prove from the blinded request gives the proof of the plain request, which
    is the single prover's (oracle.pyref.groth16.create_proof): unpack drops the blind slots, unpack2 reads the even
    points, the king repacks."""
    from test_gpu_prover import dec_g1, dec_g2
    curve = "bn254"
    Fq = FQ[curve]
    pk, r1cs, w, log_m, plain, blinded = _prove(curve, 2, 29, 2, 33, SEED)
    assert log_m == 5
    g1, g2 = CURVES[curve, "g1"], CURVES[curve, "g2"]
    proofs = []
    for res in (plain, blinded):
        pi_a, pi_b, pi_c = res[0]
        A = g1.add(dec_g1(Fq, corc.jac_to_affine(curve, 1, pi_a)), g1.add(pk["a_query"][0], pk["alpha_g1"]))
        B = g2.add(dec_g2(Fq, corc.jac_to_affine(curve, 2, pi_b)), g2.add(pk["b_g2_query"][0], pk["beta_g2"]))
        proofs.append((A, B, dec_g1(Fq, corc.jac_to_affine(curve, 1, pi_c))))
    assert proofs[0] == proofs[1] == G.create_proof(curve, pk, 0, 0, r1cs, w)


def test_blinded_and_plain_outputs_agree_at_l_1():
    """BLS12-377, l = 1 (t = 0, 4 parties): the outputs of party_prove from the blinded request equal those from the
    plain one, point for point.  (At l = 1 ext_wit_h mirrors the reference, which is not the single prover's witness
    map: include/dg16.h.)"""
    curve = "bls12_377"
    _, _, _, _, plain, blinded = _prove(curve, 1, 6, 2, 7, SEED2)
    for k in range(3):
        group = 2 if k == 1 else 1
        assert np.array_equal(corc.jac_to_affine(curve, group, plain[0][k]), corc.jac_to_affine(curve, group, blinded[0][k]))


# ---- hiding, on the device ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("party", [0, 3, 7])
def test_matching_blinds_make_one_partys_shares_equal(party):
    """l = 2 (t = 1): for two different inputs and any blinds of the first, a blind vector computed on the host gives
    party `party` byte-equal shares of the second -- what that party sees does not tell the inputs apart.  The other
    parties' shares differ."""
    curve, l = "bn254", 2
    pp = pp_of(curve, l)
    r = FR[curve].p
    n = 10 * l
    x1, x2 = list(values(curve, n, 1)[0]), list(values(curve, n, 2)[0])
    b1 = list(values(curve, n, 3)[0])
    # row `party` of the matrix from the oracle: the images of the unit vectors
    row = [RC.oracle_pack_rand(curve, l, [int(i == k) for k in range(l)], [int(i == l + k) for k in range(l)])[party]
           for i in range(2 * l)]
    assert row[l] != 0
    b2 = []
    for e in range(n // l):
        s = sum(row[c] * x1[e * l + c] + row[l + c] * b1[e * l + c] for c in range(l)) % r
        rest = sum(row[c] * x2[e * l + c] for c in range(l)) % r
        b2 += [(s - rest) * pow(row[l], -1, r) % r] + [0] * (l - 1)
    enc = lambda x: RC.to_words(x, curve, True)      # noqa: E731
    s1 = pp.pack_scalars(enc(x1), CHUNKS, enc(b1))
    s2 = pp.pack_scalars(enc(x2), CHUNKS, enc(b2))
    assert np.array_equal(s1[party], s2[party])
    assert all(not np.array_equal(s1[j], s2[j]) for j in range(pp.n) if j != party)
    unpacked = [RC.to_ints(pp.unpack(np.ascontiguousarray(s.transpose(1, 0, 2))), curve, True) for s in (s1, s2)]
    assert unpacked == [x1, x2]


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing_and_the_context_goes_on():
    import dg16_amd
    from dg16_amd import groth16_mpc as M
    from dg16_amd.lib import RequestShares
    curve, l = "bn254", 4
    ctxs = dist_pool.contexts(2)
    pp = pp_of(curve, l)
    other = dist_pool.params(curve, l, parties=2)[1]                      # a handle of another context
    ctx = pp.ctx
    assert ctx is ctxs[0] and other.ctx is ctxs[1]
    L = ctx.L
    vals = np.array(values(curve, 64)[1])
    sentinel = 0xA5A5A5A5A5A5A5A5
    out = np.full((pp.n, 64, 4), sentinel, dtype=np.uint64)
    blinds = np.array(values(curve, 64 * l, 1)[1])

    def scalars(p=pp, layout=CHUNKS, v=vp(vals), n=64, b=None, o=vp(out), c=ctx):
        return L.dg16_pss_pack_scalars(c.h if c else None, p.h if p else None, layout, v, n, b, o)

    bad = [scalars(c=None), scalars(p=None), scalars(p=other), scalars(layout=2), scalars(layout=-1), scalars(v=None),
           scalars(o=None), scalars(n=1 << 30), scalars(layout=DFFT, n=12), scalars(layout=DFFT, n=2),
           scalars(layout=DFFT, n=48, b=vp(blinds))]
    assert bad == [DG16_ERR_BAD_ARG] * len(bad)
    assert pp.scalar_chunks(DFFT, 12) == 0 and pp.scalar_chunks(DFFT, 2) == 0 and pp.scalar_chunks(7, 64) == 0

    outs = [np.full((pp.n, 64, 4), sentinel, dtype=np.uint64) for _ in range(5)]
    shares = RequestShares(*[o.ctypes.data for o in outs])
    w = np.array(values(curve, 40, 2)[1])
    seed = np.frombuffer(SEED, dtype=np.uint8).copy()

    def request(p=pp, log_m=6, a=vp(vals), w_=vp(w), nv=40, ni=3, sh=ctypes.byref(shares), c=ctx):
        return L.dg16_request_pack(c.h if c else None, p.h if p else None, log_m, a, vp(vals), vp(vals), w_, nv, ni,
                                   vp(seed), 1, sh)

    no_a = RequestShares(None, *[o.ctypes.data for o in outs[1:]])
    no_ax = RequestShares(*[o.ctypes.data for o in outs[:4]], None)
    bad = [request(c=None), request(p=None), request(p=other), request(log_m=30), request(log_m=1), request(a=None),
           request(w_=None), request(ni=0), request(ni=41), request(nv=0), request(nv=1 << 30), request(sh=None),
           request(sh=ctypes.byref(no_a)), request(sh=ctypes.byref(no_ax))]
    assert bad == [DG16_ERR_BAD_ARG] * len(bad)

    ex = np.full((8, 4), sentinel, dtype=np.uint64)

    def expand(curve_id=0, sd=vp(seed), first=0, n=8, o=vp(ex), c=ctx):
        return L.dg16_fr_expand(c.h if c else None, curve_id, sd, 0, first, n, 0, o)

    assert [expand(c=None), expand(sd=None), expand(o=None), expand(n=1 << 30), expand(first=2**64 - 4)] == \
        [DG16_ERR_BAD_ARG] * 5
    assert expand(curve_id=7) == DG16_ERR_BAD_CURVE and expand(first=2**64 - 9) == 0
    assert RC.to_ints(ex) == RC.model_expand(curve, SEED, 0, 2**64 - 9, 8)
    ex[:] = sentinel
    assert expand(n=0) == 0

    for arr in [out, ex] + outs:
        assert (arr == sentinel).all()
    with pytest.raises(dg16_amd.Dg16Error):
        pp.pack_scalars(vals[:12], DFFT)

    # the context goes on: a blinded packing equals the oracle's, and a proof of the single prover's size runs on it
    got = pp.pack_scalars(vals[:2 * l], DFFT, blinds[:2 * l])
    want = RC.oracle_shares(curve, l, DFFT, list(values(curve, 64)[0][:2 * l]),
                            [list(values(curve, 64 * l, 1)[0][e * l:(e + 1) * l]) for e in range(2)])
    assert [RC.to_ints(row, curve, True) for row in got] == want
    import bench
    import torch
    _, ok = bench.cpu_baseline_and_parity(ctx, torch.device("cuda", 0), 8)
    assert ok
