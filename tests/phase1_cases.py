"""Shared cases of the phase-1 tests (tests/test_gpu_points_series.py, tests/test_gpu_phase1.py): the special points of
the series tests, the scalars of a series made with Python's pow(), and the oracle's side of a contribution's key and
of the eight relations dg16_srs_verify_contribution decides.  Expected values come from Python big integers, from
dg16_points_mul / dg16_fixed_base_mul (merged code) and from the oracle only."""

import functools
import random

import numpy as np

import points_mul_cases as PM
from oracle import corc
from oracle.pyref import pairing as PR
from oracle.pyref.curves import CURVES
from oracle.pyref.fields import FQ, FR

# bits of dg16_srs_contribution_report::failed
AFTER, BAD_POINT, IDENTITY, BASE = 1, 2, 4, 8
KEY_TAU, KEY_ALPHA, KEY_BETA = 16, 32, 64
LINK_TAU_G1, LINK_TAU_G2, LINK_ALPHA, LINK_BETA, LINK_BETA_G2 = 128, 256, 512, 1024, 2048
PAIRING_BITS = (KEY_TAU, KEY_ALPHA, KEY_BETA, LINK_TAU_G1, LINK_TAU_G2, LINK_ALPHA, LINK_BETA, LINK_BETA_G2)

_points = {}


def _neg(curve, group, p):
    """-P of a packed affine point (the identity stays)"""
    Fq = FQ[curve]
    out = np.array(p, dtype=np.uint64, copy=True)
    if not out.any():
        return out
    half = out.size // 2
    ys = [Fq.from_mont(v) for v in corc.arr_to_ints(out[half:].reshape(-1, Fq.limbs64))]
    out[half:] = corc.ints_to_arr([Fq.to_mont((Fq.p - y) % Fq.p) for y in ys], Fq.limbs64).reshape(-1)
    return out


def special_points(curve, group, outside, n=257):
    """n subgroup points from the generator of tests/test_gpu_points_scale.py (the same seed per group): the identity at
    the first, the middle and the last index, P and -P adjacent (10, 11), one point four times (20..23); with `outside`
    a curve point outside the subgroup at 40."""
    key = (curve, group, outside, n)
    if key not in _points:
        pts = corc.gen_points(curve, group, 61 + PM.gid(curve, group), n)
        pts[0] = 0
        pts[n // 2] = 0
        pts[n - 1] = 0
        pts[11] = _neg(curve, group, pts[10])
        pts[21:24] = pts[20]
        if outside:
            pts[40] = PM.pack_point(curve, group, PM.outside_point(curve, group))
        _points[key] = pts
    return _points[key]


def series_ints(curve, first, ratio, start, n):
    """first * ratio^(start + i) mod r, i < n, by Python's pow()"""
    r = FR[curve].p
    out, v = [], first * pow(ratio, start, r) % r
    for _ in range(n):
        out.append(v)
        v = v * ratio % r
    return out


def series_scalars(curve, first, ratio, start, n):
    return corc.ints_to_arr(series_ints(curve, first, ratio, start, n), 4)


def series_params(curve, seed=0):
    rng = random.Random(0x91a5e + 7 * corc.CURVES[curve] + seed)
    r = FR[curve].p
    return rng.randrange(2, r), rng.randrange(2, r)


# ---- points as the oracle's tuples ------------------------------------------------------------------------------------
def dec(curve, group, words):
    Fq = FQ[curve]
    v = [Fq.from_mont(x) for x in corc.arr_to_ints(np.asarray(words, dtype=np.uint64).reshape(-1, Fq.limbs64))]
    if not any(v):
        return None
    return (v[0], v[1]) if group == 1 else ((v[0], v[1]), (v[2], v[3]))


def key_view(curve, key):
    """the words of a key -> [(g1_s, g1_sx, g2_spx)] for tau, alpha, beta, packed"""
    fq = FQ[curve].limbs64
    k = np.asarray(key, dtype=np.uint64).reshape(3, 8 * fq)
    return [(k[j, :2 * fq], k[j, 2 * fq:4 * fq], k[j, 4 * fq:]) for j in range(3)]


def oracle_key(curve, g, secrets, blinds, challenge):
    """s_x G | s_x x G | x SP_x per secret by the oracle's group law, packed like dg16_srs_contribute's key_out; g and the
    challenge points are packed affine points"""
    r = FR[curve].p
    c1, c2 = CURVES[curve, "g1"], CURVES[curve, "g2"]
    G = dec(curve, 1, g)
    out = []
    for x, s, sp in zip(secrets, blinds, challenge):
        out += [PM.pack_point(curve, 1, c1.mul(G, s)).reshape(-1), PM.pack_point(curve, 1, c1.mul(G, s * x % r)).reshape(-1),
                PM.pack_point(curve, 2, c2.mul(dec(curve, 2, sp), x)).reshape(-1)]
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def _relation_holds(curve, a, b, c, d):
    """R(a, b; c, d): e(a, d) = e(b, c), by oracle.pyref.pairing (memoised: tamperings share most relations)"""
    c1 = CURVES[curve, "g1"]
    return PR.pairing_product_is_one(curve, [(a, d), (c1.neg(b), c)])


def expected_pairing_bits(curve, before, after, key, challenge):
    """The eight pairing bits of the word, each relation evaluated by the oracle's pairing on the decoded points.
    before / after: five arrays each; every point involved must be a subgroup point and none the identity."""
    d1 = lambda w: dec(curve, 1, w)      # noqa: E731
    d2 = lambda w: dec(curve, 2, w)      # noqa: E731
    (kt, ka, kb) = [(d1(a), d1(b), d2(c)) for a, b, c in key_view(curve, key)]
    sp = [d2(w) for w in np.asarray(challenge, dtype=np.uint64).reshape(3, -1)]
    T1, T1n = d1(before[0][1]), d1(after[0][1])
    U1, U1n = d2(before[1][1]), d2(after[1][1])
    A0, A0n = d1(before[2][0]), d1(after[2][0])
    B0, B0n = d1(before[3][0]), d1(after[3][0])
    BG, BGn = d2(np.asarray(before[4]).reshape(-1)), d2(np.asarray(after[4]).reshape(-1))
    rel = {KEY_TAU: (kt[0], kt[1], sp[0], kt[2]), KEY_ALPHA: (ka[0], ka[1], sp[1], ka[2]),
           KEY_BETA: (kb[0], kb[1], sp[2], kb[2]),
           LINK_TAU_G1: (T1, T1n, sp[0], kt[2]), LINK_TAU_G2: (kt[0], kt[1], U1, U1n),
           LINK_ALPHA: (A0, A0n, sp[1], ka[2]), LINK_BETA: (B0, B0n, sp[2], kb[2]),
           LINK_BETA_G2: (kb[0], kb[1], BG, BGn)}
    word = 0
    for bit, args in rel.items():
        if not _relation_holds(curve, *args):
            word |= bit
    return word
