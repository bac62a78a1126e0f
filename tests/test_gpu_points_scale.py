"""GPU: dg16_points_scale (Context.points_scale), out[i] = k P_i for ONE scalar, all six groups.  The yardstick is
dg16_points_mul with the scalar replicated: affine output is canonical, so the two are compared byte for byte.  A handful
of products per group go against the oracle (`corc.point_mul`) as well.  The scalar list is the CPU test's
(tests/points_scale_cases.py)."""

import ctypes
import random
import time

import numpy as np
import pytest

import points_mul_cases as PM
import points_scale_cases as PS
from oracle import corc
from oracle.pyref.curves import CURVES
from oracle.pyref.fields import FR
from gpu_util import ctx
from test_gpu_points_mul import _neg
from test_gpu_srs_verify import context_still_proves

pytestmark = pytest.mark.gpu

W = 5          # points_scale.h's width (the CPU test reads it from the header; here it only picks 2^w - 1 and 2^w)
_points = {}


def special_points(curve, group, outside):
    """n = 65 subgroup points: the identity at the first, the middle and the last index, P and -P adjacent (10, 11), one
    point four times (20..23); with `outside` a curve point outside the subgroup at 40."""
    key = (curve, group, outside)
    if key not in _points:
        pts = corc.gen_points(curve, group, 61 + PM.gid(curve, group), 65)
        pts[0] = 0
        pts[32] = 0
        pts[64] = 0
        pts[11] = _neg(curve, group, pts[10])
        pts[21:24] = pts[20]
        if outside:
            pts[40] = PM.pack_point(curve, group, PM.outside_point(curve, group))
        _points[key] = pts
    return _points[key]


def replicated(curve, group, pts, k, in_subgroup):
    """the parent's code: dg16_points_mul with the scalar in every lane"""
    ks = np.ascontiguousarray(np.tile(corc.ints_to_arr([k], 4), (len(pts), 1)))
    return ctx().points_mul(curve, group, pts, ks, in_subgroup=in_subgroup)


@pytest.mark.parametrize("in_subgroup", [False, True])
@pytest.mark.parametrize("curve,group", PM.GROUPS)
def test_scalar_list_against_points_mul(curve, group, in_subgroup):
    """Every scalar of the list over the special points; on the plain path of a cofactor group one of them is outside the
    subgroup.  k = r gives identities on the subgroup points and r +- 1 give +-P."""
    r = FR[curve].p
    outside = (not in_subgroup) and (curve, group) in PM.COFACTOR_GROUPS
    pts = special_points(curve, group, outside)
    sub = [i for i in range(len(pts)) if not (outside and i == 40)]
    ks = PS.scalar_list(curve, W)
    # one dg16_points_mul call for the whole list: scalar j over the points, row-major
    many = np.ascontiguousarray(np.tile(pts, (len(ks), 1)))
    exp = ctx().points_mul(curve, group, many, np.repeat(corc.ints_to_arr(ks, 4), len(pts), axis=0),
                           in_subgroup=in_subgroup).reshape(len(ks), len(pts), -1)
    for j, k in enumerate(ks):
        got = ctx().points_scale(curve, group, pts, k, in_subgroup=in_subgroup)
        assert np.array_equal(got, exp[j]), hex(k)
        if k == r:
            assert not got[sub].any()
        if k == r + 1:
            assert np.array_equal(got[sub], pts[sub])
        if k == r - 1:
            assert np.array_equal(got[10], pts[11]) and np.array_equal(got[11], pts[10])
    # against the oracle: four scalars on three subgroup points
    for k in (ks[-1], ks[-40], r - 2, (1 << 255) - 1):
        got = ctx().points_scale(curve, group, pts, k, in_subgroup=in_subgroup)
        for i in (1, 20, 63):
            assert np.array_equal(got[i], corc.point_mul(curve, group, pts[i:i + 1], k)[0]), (hex(k), i)


@pytest.mark.parametrize("in_subgroup", [False, True])
@pytest.mark.parametrize("curve,group", PM.GROUPS)
def test_partial_waves_and_slices(curve, group, in_subgroup):
    """n in {0, 1, 63, 64, 65}, and 129 with the slice set to 64: two full slices and a ragged last one."""
    r = FR[curve].p
    base = special_points(curve, group, False)
    pts = np.ascontiguousarray(np.concatenate([base, base[::-1]])[:129])
    k = PS.random_scalars(curve)[3]
    exp = replicated(curve, group, pts, k, in_subgroup)
    for n in (0, 1, 63, 64, 65):
        got = ctx().points_scale(curve, group, pts[:n], k, in_subgroup=in_subgroup)
        assert got.shape == exp[:n].shape and np.array_equal(got, exp[:n]), n
    c = ctx()
    c.set_points_mul_slice(64)
    try:
        got = c.points_scale(curve, group, pts, k, in_subgroup=in_subgroup)
        assert np.array_equal(got, exp)
        got = c.points_scale(curve, group, pts, r - 1, in_subgroup=in_subgroup)
    finally:
        c.set_points_mul_slice(0)
    assert np.array_equal(got, replicated(curve, group, pts, r - 1, in_subgroup))


@pytest.mark.parametrize("curve,group,n", [("bn254", 1, 16383), ("bn254", 1, 16384), ("bn254", 1, 16385),
                                           ("bn254", 1, 32769), ("bls12_381", 2, 16385)])
def test_affine_tail_with_several_points_per_lane(curve, group, n):
    """The batched inversion behind every product call (fb_to_affine) gives lane t the points t, t + lanes, ..: one per
    lane up to n = 16383, two from 16384 on (8192 lanes, even; at 16385 the last of 8193 lanes has no second point),
    four at 32769 (8193 lanes, ragged).  Default slice, so one launch.  Input i G from dg16_fixed_base_mul with identities
    at 0, n - 1 and on either side of `lanes`; 5 P and then 5^-1 (5 P) must give the input back byte for byte, and eight
    seeded products equal the oracle's."""
    r = FR[curve].p
    per_lane = min(max(n >> 13, 1), 32)
    lanes = -(-n // per_lane)
    assert (per_lane, lanes) == {16383: (1, 16383), 16384: (2, 8192), 16385: (2, 8193), 32769: (4, 8193)}[n]
    c = ctx()
    pts = c.fixed_base_mul(curve, group, corc.ints_to_arr(list(range(n)), 4))
    holes = sorted({0, n - 1, lanes - 1, min(lanes, n - 1)})
    pts[holes] = 0
    out = c.points_scale(curve, group, pts, 5, in_subgroup=True)
    back = c.points_scale(curve, group, out, pow(5, r - 2, r), in_subgroup=True)
    assert np.array_equal(back, pts)
    assert np.flatnonzero(~out.any(axis=1)).tolist() == holes
    cv = CURVES[curve, "g%d" % group]
    for i in random.Random(n).sample(range(n), 8):
        exp = np.zeros_like(out[i]) if i in holes else PM.pack_point(curve, group, cv.mul(cv.gen, 5 * i))
        assert np.array_equal(out[i], exp), i


@pytest.mark.parametrize("curve,group", [("bn254", 1), ("bls12_381", 2), ("bls12_377", 1)])
def test_in_place(curve, group):
    pts = special_points(curve, group, False)
    k = PS.random_scalars(curve)[5]
    exp = replicated(curve, group, pts, k, True)
    buf = pts.copy()
    c = ctx()
    c.set_points_mul_slice(64)
    try:
        assert c.points_scale(curve, group, buf, k, in_subgroup=True, out=buf) is buf
    finally:
        c.set_points_mul_slice(0)
    assert np.array_equal(buf, exp)


def test_refusals_and_the_context_proves_afterwards():
    c_ = ctx()
    L, h = c_.L, c_.h
    pts = np.ascontiguousarray(special_points("bn254", 1, False)[:4])
    out = np.zeros_like(pts)
    k = np.frombuffer((12345).to_bytes(32, "little"), dtype=np.uint64).copy()
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)     # noqa: E731
    call = lambda curve, group, p, s, n, o: L.dg16_points_scale(h, curve, group, vp(p), vp(s), n, vp(o), 1)  # noqa: E731
    assert call(0, 1, pts, k, 4, out) == 0
    assert call(0, 1, None, k, 4, out) == 3
    assert call(0, 1, pts, None, 4, out) == 3
    assert call(0, 1, pts, k, 4, None) == 3
    assert call(0, 1, None, None, 0, None) == 0                 # n = 0
    assert call(0, 3, pts, k, 4, out) == 3                      # group 3
    assert call(0, 0, pts, k, 4, out) == 3
    assert call(3, 1, pts, k, 4, out) == 2                      # curve 3
    big = np.frombuffer((1 << 255).to_bytes(32, "little"), dtype=np.uint64).copy()
    assert call(0, 1, pts, big, 4, out) == 3                    # a scalar from 2^255 on
    assert L.dg16_points_scale(None, 0, 1, vp(pts), vp(k), 4, vp(out), 1) == 3
    context_still_proves()
    assert np.array_equal(c_.points_scale("bn254", 1, pts, 12345, in_subgroup=True), out)


def test_not_slower_than_points_mul_with_the_scalar_replicated():
    """BN254 G1, n = 2^16, in_subgroup = 1, host arrays in both calls: the two alternated five times in one process after
    a warm-up.  dg16_points_scale does strictly less work, so its median must not exceed the median of
    dg16_points_mul by more than the spread (max - min) dg16_points_mul itself showed in those five runs."""
    curve, group, n = "bn254", 1, 1 << 16
    c = ctx()
    pts = c.gen_bases(curve, group, 5, n)
    k = PS.random_scalars(curve)[7]
    ks = np.ascontiguousarray(np.tile(corc.ints_to_arr([k], 4), (n, 1)))
    out = np.zeros_like(pts)
    exp = c.points_mul(curve, group, pts, ks, in_subgroup=True)                        # warm-up, and the expected value
    assert np.array_equal(c.points_scale(curve, group, pts, k, in_subgroup=True, out=out), exp)
    t_scale, t_mul = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        c.points_scale(curve, group, pts, k, in_subgroup=True, out=out)
        t1 = time.perf_counter()
        c.points_mul(curve, group, pts, ks, in_subgroup=True)
        t2 = time.perf_counter()
        t_scale.append(t1 - t0)
        t_mul.append(t2 - t1)
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    print("dg16_points_scale median %.3f ms, dg16_points_mul median %.3f ms (spread %.3f ms)"
          % (1e3 * med(t_scale), 1e3 * med(t_mul), 1e3 * (max(t_mul) - min(t_mul))))
    assert med(t_scale) <= med(t_mul) + (max(t_mul) - min(t_mul))
