"""GPU: dg16_points_mul_series (Context.points_mul_series), out[i] = (first * ratio^(start + i)) P_i with the scalars
made on the device, all six groups.  The yardstick is dg16_points_mul on scalars made with Python's pow(): affine output
is canonical, so the two are compared byte for byte.  A few products per curve go against the oracle's group law."""

import ctypes
import time

import numpy as np
import pytest

import phase1_cases as P1
import points_mul_cases as PM
from oracle import corc
from oracle.pyref.fields import FR
from gpu_util import ctx
from test_gpu_srs_verify import context_still_proves

pytestmark = pytest.mark.gpu

SIZES = (1, 15, 16, 17, 63, 64, 65, 257)          # around the chunk of 16 exponents and the wave of 64 products
BIG_START = 2**32 + 5


def by_points_mul(curve, group, pts, first, ratio, start, in_subgroup):
    """merged code on Python-made scalars"""
    ks = P1.series_scalars(curve, first, ratio, start, len(pts))
    return ctx().points_mul(curve, group, pts, ks, in_subgroup=in_subgroup)


@pytest.mark.parametrize("in_subgroup", [False, True])
@pytest.mark.parametrize("curve,group", PM.GROUPS)
def test_series_against_points_mul(curve, group, in_subgroup):
    """Every n of SIZES (a prefix of one series, so one reference serves them all), then start = 2^32 + 5, then 130
    products in slices of 64 -- three slices, the last partial -- from start 0 and from start 2^63 - 70, where the
    exponents of the second slice pass 2^63.  On the plain path of a cofactor group the point at index 40 is outside
    the subgroup.  Identity inputs stay identities."""
    outside = (not in_subgroup) and (curve, group) in PM.COFACTOR_GROUPS
    pts = P1.special_points(curve, group, outside)
    first, ratio = P1.series_params(curve)
    c = ctx()
    exp = by_points_mul(curve, group, pts, first, ratio, 0, in_subgroup)
    assert exp[1].any() and (not outside or exp[40].any())
    for n in SIZES:
        got = c.points_mul_series(curve, group, pts[:n], first, ratio, in_subgroup=in_subgroup)
        assert got.shape == exp[:n].shape and np.array_equal(got, exp[:n]), n
    for i in (0, len(pts) // 2, len(pts) - 1):
        assert not exp[i].any()
    got = c.points_mul_series(curve, group, pts[:65], first, ratio, start=BIG_START, in_subgroup=in_subgroup)
    assert np.array_equal(got, by_points_mul(curve, group, pts[:65], first, ratio, BIG_START, in_subgroup))
    c.set_points_mul_slice(64)
    try:
        got = c.points_mul_series(curve, group, pts[:130], first, ratio, in_subgroup=in_subgroup)
        far = c.points_mul_series(curve, group, pts[:130], first, ratio, start=2**63 - 70, in_subgroup=in_subgroup)
    finally:
        c.set_points_mul_slice(0)
    assert np.array_equal(got, exp[:130])
    assert np.array_equal(far, by_points_mul(curve, group, pts[:130], first, ratio, 2**63 - 70, in_subgroup))


@pytest.mark.parametrize("curve,group", PM.GROUPS)
def test_ratio_one_ratio_zero_and_first_zero(curve, group):
    """ratio = 1 is dg16_points_scale(first) byte for byte; ratio = 0 leaves `first` at exponent 0 and identities
    elsewhere (from start 0) or identities everywhere (from start 1); first = 0 gives identities."""
    r = FR[curve].p
    pts = P1.special_points(curve, group, False)[:65]
    first, ratio = P1.series_params(curve, seed=1)
    c = ctx()
    for k in (first, 1, r - 1):
        assert np.array_equal(c.points_mul_series(curve, group, pts, k, 1, start=BIG_START, in_subgroup=True),
                              c.points_scale(curve, group, pts, k, in_subgroup=True)), hex(k)
    got = c.points_mul_series(curve, group, pts[1:], first, 0, in_subgroup=True)
    assert np.array_equal(got[0], c.points_scale(curve, group, pts[1:2], first, in_subgroup=True)[0])
    assert got[0].any() and not got[1:].any()
    assert not c.points_mul_series(curve, group, pts[1:], first, 0, start=1, in_subgroup=True).any()
    assert not c.points_mul_series(curve, group, pts, 0, ratio, in_subgroup=True).any()
    assert not c.points_mul_series(curve, group, pts, 0, 0, in_subgroup=False).any()


@pytest.mark.parametrize("curve,group", [("bn254", 1), ("bls12_381", 2), ("bls12_377", 1)])
def test_in_place(curve, group):
    pts = P1.special_points(curve, group, False)[:130]
    first, ratio = P1.series_params(curve, seed=2)
    exp = by_points_mul(curve, group, pts, first, ratio, 3, True)
    buf = pts.copy()
    c = ctx()
    c.set_points_mul_slice(64)
    try:
        assert c.points_mul_series(curve, group, buf, first, ratio, start=3, in_subgroup=True, out=buf) is buf
    finally:
        c.set_points_mul_slice(0)
    assert np.array_equal(buf, exp)


@pytest.mark.parametrize("curve", ["bn254", "bls12_381", "bls12_377"])
def test_against_the_oracles_group_law(curve):
    """Both groups, n = 20 (two chunks), start = 2^32 - 3 so that the exponents pass 2^32 inside the call: five
    products each against corc.point_mul."""
    r = FR[curve].p
    first, ratio = P1.series_params(curve, seed=3)
    start, n = 2**32 - 3, 20
    ks = P1.series_ints(curve, first, ratio, start, n)
    assert ks[5] == first * pow(ratio, 2**32 + 2, r) % r
    for group in (1, 2):
        pts = P1.special_points(curve, group, False)[:n]
        got = ctx().points_mul_series(curve, group, pts, first, ratio, start=start, in_subgroup=False)
        for i in (1, 2, 5, 16, 19):
            assert np.array_equal(got[i], corc.point_mul(curve, group, pts[i:i + 1], ks[i])[0]), (group, i)


def test_refusals_and_the_context_proves_afterwards():
    c_ = ctx()
    L, h = c_.L, c_.h
    r = FR["bn254"].p
    pts = np.ascontiguousarray(P1.special_points("bn254", 1, False)[:4])
    out = np.zeros_like(pts)
    word = lambda v: np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint64).copy()     # noqa: E731
    f, q = word(12345), word(678)
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)     # noqa: E731
    call = lambda curve, group, p, n, a, b, start, o: L.dg16_points_mul_series(   # noqa: E731
        h, curve, group, vp(p), n, vp(a), vp(b), start, vp(o), 1)
    assert call(0, 1, pts, 4, f, q, 0, out) == 0
    exp = out.copy()
    assert call(0, 1, None, 4, f, q, 0, out) == 3
    assert call(0, 1, pts, 4, None, q, 0, out) == 3
    assert call(0, 1, pts, 4, f, None, 0, out) == 3
    assert call(0, 1, pts, 4, f, q, 0, None) == 3
    assert call(0, 1, None, 0, None, None, 0, None) == 0           # n = 0
    assert call(0, 1, pts, 1 << 30, f, q, 0, out) == 3             # n >= 2^30
    assert call(0, 3, pts, 4, f, q, 0, out) == 3                   # group 3
    assert call(0, 0, pts, 4, f, q, 0, out) == 3
    assert call(3, 1, pts, 4, f, q, 0, out) == 2                   # curve 3
    for bad in (r, r + 1, (1 << 256) - 1):
        assert call(0, 1, pts, 4, word(bad), q, 0, out) == 3       # first, ratio not below r
        assert call(0, 1, pts, 4, f, word(bad), 0, out) == 3
    assert call(0, 1, pts, 4, f, q, 2**64 - 4, out) == 3           # start + n wraps
    assert call(0, 1, pts, 4, f, q, 2**64 - 5, out) == 0
    assert L.dg16_points_mul_series(None, 0, 1, vp(pts), 4, vp(f), vp(q), 0, vp(out), 1) == 3
    context_still_proves()
    assert np.array_equal(c_.points_mul_series("bn254", 1, pts, 12345, 678, in_subgroup=True), exp)
    assert np.array_equal(exp, by_points_mul("bn254", 1, pts, 12345, 678, 0, True))


def test_not_slower_than_points_mul_on_prepared_scalars():
    """BN254 G1, n = 2^14, in_subgroup = 1, host arrays in and out in both calls (each allocates its result); the scalars of dg16_points_mul are prepared outside
    the timed region.  The two calls alternate five times in one process after a warm-up and the medians are compared:
    the new call runs the same product kernel and skips the upload of the scalars, so it should not be slower.  The
    margin is the old path's own spread, max over min of its five repeats in this run."""
    curve, group, n = "bn254", 1, 1 << 14
    c = ctx()
    pts = c.gen_bases(curve, group, 5, n)
    first, ratio = P1.series_params(curve, seed=4)
    ks = np.ascontiguousarray(P1.series_scalars(curve, first, ratio, 0, n))
    exp = c.points_mul(curve, group, pts, ks, in_subgroup=True)                        # warm-up, and the expected value
    assert np.array_equal(c.points_mul_series(curve, group, pts, first, ratio, in_subgroup=True), exp)
    t_series, t_mul = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        c.points_mul_series(curve, group, pts, first, ratio, in_subgroup=True)
        t1 = time.perf_counter()
        c.points_mul(curve, group, pts, ks, in_subgroup=True)
        t2 = time.perf_counter()
        t_series.append(t1 - t0)
        t_mul.append(t2 - t1)
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    spread = max(t_mul) / min(t_mul)
    print("dg16_points_mul_series median %.3f ms, dg16_points_mul median %.3f ms: ratio %.3f, spread %.3f"
          % (1e3 * med(t_series), 1e3 * med(t_mul), med(t_series) / med(t_mul), spread))
    assert med(t_series) <= med(t_mul) * spread
