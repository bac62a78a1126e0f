"""The distributed primitives at EVERY packing factor dg16_pss_create accepts: l = 1, 2, 4, 8 (4, 8, 16, 32 parties).

tests/test_gpu_dist.py runs them at l = 2, where the king-side code of csrc/dist.hip takes one path only: one fft2
level, one swap of the ping-pong buffers, the wave-per-term combination in the exponent with 2 or 8 terms, a prefix
product of one partial or of exactly 16 full tiles, and PSS matrices small enough for one thread per entry.  Here:

  l = 1      zero fft2 levels (rotate_pad reads the unpacked vector itself); 1-term wave kernel
  l = 4, 8   2 / 3 fft2 levels (i_level > 1, even and odd numbers of swaps); d_msm's king step on the lane-per-output
             kernel (16 / 32 terms); 4-term wave kernel; 3 n l = 768 canonical matrix entries at l = 8
  d_pp       a partial last tile after full ones (kScanTile = 2048)
  ext_wit_h  l = 1 mirrors the reference; l = 4, 8 are refused (the reference panics), like m < l and a wrong net

Everything is bit-exact against oracle/pyref (pinned at these l by tests/test_dist_oracle_l.py) and the C oracle.  Sizes
are the smallest that reach the path: the restatement is pure Python."""

import random

import numpy as np
import pytest

import dist_pool
from oracle import corc
from oracle.pyref import dist as R, groth16 as G
from oracle.pyref.fields import FR
from oracle.pyref.poly import Domain
from oracle.pyref.pss import PackedSharingParams as RefPSS

pytestmark = pytest.mark.gpu

DG16_ERR_BAD_ARG, DG16_ERR_UNSUPPORTED = 3, 7


def enc(F, vals):
    return corc.ints_to_arr([F.to_mont(v) for v in vals], 4)


def dec(F, arr):
    return [F.from_mont(v) for v in corc.arr_to_ints(np.asarray(arr).reshape(-1, 4))]


def log2(l):
    return l.bit_length() - 1


def ref_map(ref, which):
    return (ref.pack_from_public, ref.unpack, ref.unpack2)[which]


# ---- PSS matrices on field elements (dg16_pss_apply; one context, no net) ----------------------------------------------
@pytest.mark.parametrize("l", [1, 2, 4, 8])
@pytest.mark.parametrize("curve", ["bn254", "bls12_381", "bls12_377"])
def test_pss_matrices(curve, l):
    F = FR[curve]
    pp = dist_pool.params(curve, l, parties=1)[0]
    ref = RefPSS(F, l)
    rng = random.Random(10 * l + len(curve))
    for which, fn in enumerate((pp.pack_from_public, pp.unpack, pp.unpack2)):
        cols = l if which == 0 else 4 * l
        vecs = [[int(i == j) for i in range(cols)] for j in range(cols)]          # one matrix column each
        vecs += [[0] * cols, [F.p - 1] * cols]
        vecs += [[rng.randrange(F.p) for _ in range(cols)] for _ in range(20)]
        got = fn(np.concatenate([enc(F, v) for v in vecs]))
        assert [dec(F, g) for g in got] == [ref_map(ref, which)(v) for v in vecs], which
    # share-wise products of two sharings unpack (unpack2) to the products of the secrets (pss.rs:200-241)
    a = [[rng.randrange(F.p) for _ in range(l)] for _ in range(20)]
    b = [[rng.randrange(F.p) for _ in range(l)] for _ in range(20)]
    prod = [[x * y % F.p for x, y in zip(ref.pack_from_public(s), ref.pack_from_public(o))] for s, o in zip(a, b)]
    got = pp.unpack2(np.concatenate([enc(F, p_) for p_ in prod]))
    assert [dec(F, g) for g in got] == [[x * y % F.p for x, y in zip(s, o)] for s, o in zip(a, b)]


# ---- the same matrices in the exponent (dg16_pss_apply_exp) ------------------------------------------------------------
EXP_CASES = [(c, 1, l) for c in ("bn254", "bls12_377") for l in (1, 2, 4, 8)] + [("bn254", 2, 2), ("bn254", 2, 8)]
_points = {}


def points(curve, group, count):
    """`count` points of the group with the identity (0, 0) at index 1; one generation per (curve, group)."""
    key = (curve, group)
    if key not in _points or len(_points[key]) < count:
        pts = corc.gen_points(curve, group, 31, max(count, 1100))
        pts[1] = 0
        pts.setflags(write=False)
        _points[key] = pts
    return _points[key][:count]


def exp_matrix(F, l, which):
    """M[r][c] of the oracle's pack / unpack / unpack2 map, canonical: the images of the unit vectors."""
    ref = RefPSS(F, l)
    cols = l if which == 0 else 4 * l
    images = [ref_map(ref, which)([int(i == c) for i in range(cols)]) for c in range(cols)]
    return [list(row) for row in zip(*images)]


def apply_in_exponent(curve, group, M, P):
    """out[e][r] = sum_c M[r][c] P[e][c] with the C oracle's MSM."""
    rows = [corc.ints_to_arr(row, 4) for row in M]
    return np.stack([np.concatenate([corc.msm(curve, group, Pe, sc, threads=1) for sc in rows]) for Pe in P])


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("curve,group,l", EXP_CASES)
def test_pss_matrices_in_the_exponent(curve, group, l, which):
    F = FR[curve]
    pp = dist_pool.params(curve, l, parties=1)[0]
    cols, rows = (l, 4 * l) if which == 0 else (4 * l, l)
    M = exp_matrix(F, l, which)
    fn = pp.packexp_from_public if which == 0 else (lambda g, x: pp.unpackexp(g, x, which == 2))
    # matvec_points (csrc/msm_group.hip) takes the wave-per-term kernel when count * rows <= 256 and cols <= 8, the
    # lane-per-output kernel otherwise: one count on each side of the switch
    for count in (2, 256 // rows + 1):
        assert (count * rows <= 256) == (count == 2)
        P = points(curve, group, count * cols).reshape(count, cols, -1)
        got = fn(group, P)
        assert np.array_equal(got, apply_in_exponent(curve, group, M, P)), count


@pytest.mark.parametrize("curve,group,l", EXP_CASES)
def test_unpackexp_of_packexp_is_the_identity(curve, group, l):
    # dmsm/mod.rs:127-145
    pp = dist_pool.params(curve, l, parties=1)[0]
    x = points(curve, group, 3 * l).reshape(3, l, -1)
    packed = pp.packexp_from_public(group, x)
    assert np.array_equal(pp.unpackexp(group, packed, False), x)
    assert np.array_equal(pp.unpackexp(group, packed, True), x)


# ---- d_fft / d_ifft -----------------------------------------------------------------------------------------------------
def dfft_log_ms(l):
    return sorted({max(1, log2(l)), log2(l) + 1, 6, 10})


DFFT_CASES = [(c, l, log_m) for c, l in (("bls12_377", 1), ("bls12_377", 4), ("bls12_377", 8), ("bn254", 4))
              for log_m in dfft_log_ms(l)]


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("curve,l,log_m", DFFT_CASES)
def test_d_fft_shares_bit_exact(curve, l, log_m, inverse):
    """log_m = log2 l: one element per party, no local level, every level on the king (fft2_level_kernel with
    i_level = log2 l .. 1).  l = 1: no king level at all."""
    F = FR[curve]
    ctxs, pps, net, D = dist_pool.parties(curve, l)
    ref = RefPSS(F, l)
    m = 1 << log_m
    dom = Domain(F, m)
    rng = random.Random(1000 * l + log_m)
    x = [rng.randrange(F.p) for _ in range(m)]
    shares = R.share_for_dfft(x, ref)
    fn = R.d_ifft if inverse else R.d_fft
    for rearrange, pad, degree2 in ((False, 1, False), (True, 2, False), (True, 1, False)):
        exp = fn(shares, rearrange, pad, degree2, dom, ref)
        got = net.simulate_network_round(
            lambda i, h: D.d_fft(ctxs[i], pps[i], h, enc(F, shares[i]), log_m, rearrange, pad, degree2, inverse=inverse))
        assert [dec(F, g) for g in got] == exp, (rearrange, pad)
        if not rearrange:       # the relation the reference asserts (dfft/mod.rs:373,458)
            vals = [v for row in pps[0].unpack(np.stack(got, axis=1)) for v in dec(F, row)]
            assert vals == (dom.ifft(x) if inverse else dom.fft(x))


@pytest.mark.parametrize("curve,l", [("bls12_377", 1), ("bls12_377", 4), ("bls12_377", 8), ("bn254", 4)])
def test_d_fft_degree2_on_share_products(curve, l):
    F = FR[curve]
    ctxs, pps, net, D = dist_pool.parties(curve, l)
    ref = RefPSS(F, l)
    log_m = log2(l) + 2
    m = 1 << log_m
    dom = Domain(F, m)
    rng = random.Random(l)
    x = [rng.randrange(F.p) for _ in range(m)]
    y = [rng.randrange(F.p) for _ in range(m)]
    sx, sy = R.share_for_dfft(x, ref), R.share_for_dfft(y, ref)
    prod = [[a * b % F.p for a, b in zip(px, py)] for px, py in zip(sx, sy)]     # degree-2(t + l) shares
    for inverse in (False, True):
        exp = (R.d_ifft if inverse else R.d_fft)(prod, False, 1, True, dom, ref)
        got = net.simulate_network_round(
            lambda i, h: D.d_fft(ctxs[i], pps[i], h, enc(F, prod[i]), log_m, False, 1, True, inverse=inverse))
        assert [dec(F, g) for g in got] == exp, inverse


# ---- d_msm / d_msm_resident ---------------------------------------------------------------------------------------------
DMSM_CASES = [(c, 1, l) for l in (1, 4, 8) for c in ("bn254", "bls12_377")] + [("bn254", 2, 4)]


def packed_msm_inputs(curve, group, l, pp, seed):
    F = FR[curve]
    M = 64
    pts = points(curve, group, M)                   # the identity among them
    packed_bases = pp.packexp_from_public(group, pts.reshape(M // l, l, -1))      # [M/l][n][..]
    rng = random.Random(seed)

    def scalars():
        sc = [rng.randrange(F.p) for _ in range(M)]
        clear = corc.msm(curve, group, pts, corc.ints_to_arr(sc, 4))
        return pp.pack_from_public(enc(F, sc).reshape(M // l, l, 4)), clear        # [M/l][n][4]
    return packed_bases, scalars


@pytest.mark.parametrize("curve,group,l", DMSM_CASES)
def test_d_msm_equals_clear_msm(curve, group, l):
    """The king combines n = 4 l shares in the exponent with v2sum: the wave kernel at 4 parties, the lane kernel at 16
    and 32 (more than 8 terms)."""
    ctxs, pps, net, D = dist_pool.parties(curve, l)
    packed_bases, scalars = packed_msm_inputs(curve, group, l, pps[0], 9 + l)
    packed_sc, clear = scalars()
    got = net.simulate_network_round(
        lambda i, h: D.d_msm(ctxs[i], pps[i], h, group, np.ascontiguousarray(packed_bases[:, i]),
                             np.ascontiguousarray(packed_sc[:, i]), in_subgroup=True))
    assert all(np.array_equal(corc.jac_to_affine(curve, group, g), clear) for g in got)


@pytest.mark.parametrize("curve,group,l", DMSM_CASES)
def test_d_msm_resident_equals_clear_msm(curve, group, l):
    ctxs, pps, net, D = dist_pool.parties(curve, l)
    packed_bases, scalars = packed_msm_inputs(curve, group, l, pps[0], 19 + l)
    resident = [c.bases_upload(curve, group, np.ascontiguousarray(packed_bases[:, i])) for i, c in enumerate(ctxs)]
    try:
        assert resident[0].info()["n"] == 64 // l
        for _ in range(2):
            packed_sc, clear = scalars()
            got = net.simulate_network_round(
                lambda i, h: D.d_msm_resident(ctxs[i], pps[i], h, resident[i], np.ascontiguousarray(packed_sc[:, i])))
            assert all(np.array_equal(corc.jac_to_affine(curve, group, g), clear) for g in got)
    finally:
        for r in resident:
            r.close()


# ---- deg_red / d_pp -----------------------------------------------------------------------------------------------------
def nonzero(F, seed, m):
    rng = random.Random(seed)
    return [rng.randrange(1, F.p) for _ in range(m)]


@pytest.mark.parametrize("l", [1, 4, 8])
def test_deg_red_and_d_pp(l):
    curve = "bls12_377"
    F = FR[curve]
    ctxs, pps, net, D = dist_pool.parties(curve, l)
    ref = RefPSS(F, l)
    m = 64
    ns = R.transpose(R.pack_vec(nonzero(F, 4 + l, m), ref))
    ds = R.transpose(R.pack_vec(nonzero(F, 40 + l, m), ref))
    got = net.simulate_network_round(lambda i, h: D.d_pp(ctxs[i], pps[i], h, enc(F, ns[i]), enc(F, ds[i])))
    assert [dec(F, g) for g in got] == R.d_pp(ns, ds, ref)
    prod = [[a * b % F.p for a, b in zip(p_, q_)] for p_, q_ in zip(ns, ds)]
    got = net.simulate_network_round(lambda i, h: D.deg_red(ctxs[i], pps[i], h, enc(F, prod[i])))
    assert [dec(F, g) for g in got] == R.deg_red(prod, ref)


SCAN_SIZES = {"2048": lambda l: 2048, "2048+l": lambda l: 2048 + l, "3*2048-l": lambda l: 3 * 2048 - l,
              "2*2048+3l": lambda l: 2 * 2048 + 3 * l}


@pytest.mark.parametrize("tiles", list(SCAN_SIZES))
@pytest.mark.parametrize("l", [2, 4])
def test_d_pp_across_scan_tiles(l, tiles):
    """The king's prefix product scans tiles of 2048: exactly one full tile, a full tile and a partial one of l, two full
    and one short of full by l, two full and a partial one of 3 l."""
    curve = "bls12_377"
    F = FR[curve]
    ctxs, pps, net, D = dist_pool.parties(curve, l)
    ref = RefPSS(F, l)
    m = SCAN_SIZES[tiles](l)
    assert m % l == 0
    num, den = nonzero(F, m, m), nonzero(F, m + 1, m)
    ns = R.transpose(R.pack_vec(num, ref))
    ds = R.transpose(R.pack_vec(den, ref))
    got = net.simulate_network_round(lambda i, h: D.d_pp(ctxs[i], pps[i], h, enc(F, ns[i]), enc(F, ds[i])))
    assert [dec(F, g) for g in got] == R.d_pp(ns, ds, ref)
    # ... which is the packed sharing of the running products of num / den
    vals = [v for row in pps[0].unpack(np.stack(got, axis=1)) for v in dec(F, row)]
    acc, exp = 1, []
    for a, b in zip(num, den):
        acc = acc * a % F.p * F.inv(b) % F.p
        exp.append(acc)
    assert vals == exp


# ---- ext_wit::h ---------------------------------------------------------------------------------------------------------
def abc(F, m, seed):
    rng = random.Random(seed)
    return tuple([rng.randrange(F.p) for _ in range(m)] for _ in range(3))


@pytest.mark.parametrize("log_m", [3, 7])
def test_ext_wit_h_mirrors_the_reference_at_l_1(log_m):
    """t = 0: the reference's swap is the identity and it keeps the first m of the 2m evaluations.  That is not the witness
    map (tests/test_dist_oracle_l.py), so only the shares are compared."""
    curve = "bn254"
    F = FR[curve]
    ctxs, pps, net, D = dist_pool.parties(curve, 1)
    ref = RefPSS(F, 1)
    m = 1 << log_m
    qs = G.qap_pss(*abc(F, m, log_m), ref)
    exp = G.ext_wit_h(qs, Domain(F, m), ref)
    got = net.simulate_network_round(
        lambda i, h: D.ext_wit_h(ctxs[i], pps[i], h, enc(F, qs[i][0]), enc(F, qs[i][1]), enc(F, qs[i][2]), log_m))
    assert [dec(F, g) for g in got] == exp


def ext_wit_h_codes(ctxs, pps, net, D, F, log_m, share_len):
    """Every party calls ext_wit_h; the status each one gets (0 = no error)."""
    import dg16_amd
    share = enc(F, [1] * share_len)

    def run(i, h):
        try:
            D.ext_wit_h(ctxs[i], pps[i], h, share, share, share, log_m)
        except dg16_amd.Dg16Error as e:
            return e.code
        return 0
    return net.simulate_network_round(run)


@pytest.mark.parametrize("l", [4, 8])
def test_ext_wit_h_refuses_l_above_2_on_every_party(l):
    """The reference indexes past its vector here and panics; the library answers DG16_ERR_UNSUPPORTED on every party
    before any collective, so nobody waits and the same net and contexts go on working."""
    curve = "bn254"
    F = FR[curve]
    ctxs, pps, net, D = dist_pool.parties(curve, l)
    log_m = 5
    assert ext_wit_h_codes(ctxs, pps, net, D, F, log_m, (1 << log_m) // l) == [DG16_ERR_UNSUPPORTED] * (4 * l)
    ref = RefPSS(F, l)
    x = [random.Random(l).randrange(F.p) for _ in range(1 << log_m)]
    shares = R.share_for_dfft(x, ref)
    got = net.simulate_network_round(
        lambda i, h: D.d_fft(ctxs[i], pps[i], h, enc(F, shares[i]), log_m, False, 1, False))
    assert [dec(F, g) for g in got] == R.d_fft(shares, False, 1, False, Domain(F, 1 << log_m), ref)


def test_ext_wit_h_bad_arguments():
    import dg16_amd
    curve = "bn254"
    F = FR[curve]
    # a domain smaller than the packing factor (m / l = 0), at a supported and at an unsupported l
    for l, log_m in ((2, 0), (4, 1), (8, 2)):
        ctxs, pps, net, D = dist_pool.parties(curve, l)
        assert ext_wit_h_codes(ctxs, pps, net, D, F, log_m, 1) == [DG16_ERR_BAD_ARG] * (4 * l)
    # a net of another party count than the parameters': 4 parties, l = 2
    ctxs, pps, net, D = dist_pool.parties(curve, 2)
    share = enc(F, [1] * 4)
    with pytest.raises(dg16_amd.Dg16Error) as e:
        D.ext_wit_h(ctxs[0], pps[0], dist_pool.net(4).party(0), share, share, share, 3)
    assert e.value.code == DG16_ERR_BAD_ARG
    # a domain no buffer could hold (the library shifts by log_m)
    with pytest.raises(dg16_amd.Dg16Error) as e:
        D.ext_wit_h(ctxs[0], pps[0], net.party(0), share, share, share, 48)
    assert e.value.code == DG16_ERR_BAD_ARG
