"""GPU: dg16_points_check (Context.points_check), curve and subgroup membership of affine points, all six groups.
Points and expected verdicts are built in plain Python (tests/points_check_cases.py: reduced / on the curve / r P in big
integers with the group law of oracle.pyref.curves); the CPU test (tests/test_points_check_host.py) runs the same cases
through the same header text."""

import ctypes

import numpy as np
import pytest

import points_check_cases as PC
from gpu_util import ctx

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 1000]


def context_still_proves():
    """A small proof through the resident prover equals the oracle's: the context is usable after an error."""
    import bench
    import torch
    _, ok = bench.cpu_baseline_and_parity(ctx(), torch.device("cuda", 0), 8)
    assert ok


@pytest.mark.parametrize("curve,group", PC.GROUPS)
def test_case_list_one_point_at_a_time(curve, group):
    """Every special point alone (n = 1), under subgroup = 0 and 1."""
    c = ctx()
    for name, w, v0, v1 in PC.cases(curve, group):
        for subgroup, v in ((False, v0), (True, v1)):
            assert c.points_check(curve, group, w[None, :], subgroup=subgroup) == ((1, 0) if v else (0, 1)), (name, subgroup)


@pytest.mark.parametrize("curve,group", PC.GROUPS)
def test_case_list_in_one_batch(curve, group):
    """The whole list in one call: the count and the smallest index are the list's; subgroup = 0 drops exactly the
    points that are only outside the subgroup."""
    cs = PC.cases(curve, group)
    pts = np.stack([w for _, w, _, _ in cs])
    for subgroup, col in ((False, 2), (True, 3)):
        bad = [i for i, case in enumerate(cs) if case[col]]
        assert ctx().points_check(curve, group, pts, subgroup=subgroup) == (len(bad), bad[0]), subgroup


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("curve,group", PC.GROUPS)
def test_batch_sizes_and_placement(curve, group, n):
    """Good filler with bad points placed: none; alone at 0; alone at n - 1 (the last lane of the tail block); three of
    them (count 3, the smallest index).  Every kind of bad point of the group takes its turn."""
    c = ctx()
    pts = PC.filler(curve, group, n)
    assert c.points_check(curve, group, pts) == (0, n)
    if not n:
        return
    bads = PC.bad_points(curve, group, True)
    for k, w in enumerate(bads):
        for at in sorted({0, n - 1}):
            p = pts.copy()
            p[at] = w
            assert c.points_check(curve, group, p) == (1, at), (k, at)
    if n >= 63:
        p = pts.copy()
        where = [n - 1, 17, n // 2]
        for k, at in enumerate(where):
            p[at] = bads[k % len(bads)]
        assert c.points_check(curve, group, p) == (3, 17)


@pytest.mark.parametrize("curve,group", PC.GROUPS)
def test_slices(curve, group):
    """n = 1000 in slices of 64: sixteen launches, the last one of 40 lanes.  The index is the global one, in the first
    slice, at a slice boundary and at the last lane of the last slice."""
    c = ctx()
    n = 1000
    pts = PC.filler(curve, group, n)
    bads = PC.bad_points(curve, group, True)
    c.set_points_mul_slice(64)
    try:
        assert c.points_check(curve, group, pts) == (0, n)
        for at in (0, 63, 64, 959, 960, n - 1):
            p = pts.copy()
            p[at] = bads[at % len(bads)]
            assert c.points_check(curve, group, p) == (1, at), at
        p = pts.copy()
        for k, at in enumerate((n - 1, 640, 333)):
            p[at] = bads[k % len(bads)]
        assert c.points_check(curve, group, p) == (3, 333)
    finally:
        c.set_points_mul_slice(0)


@pytest.mark.parametrize("curve,group", [g for g in PC.GROUPS if g != ("bn254", 1)])
def test_without_the_subgroup_test_curve_points_are_good(curve, group):
    pts = PC.filler(curve, group, 65)
    off = [w for _, w, v0, v1 in PC.cases(curve, group) if v0 == PC.GOOD and v1 == PC.OFF_SUBGROUP]
    assert off
    for k, w in enumerate(off):
        pts[(k * 31) % 65] = w
    assert ctx().points_check(curve, group, pts, subgroup=False) == (0, 65)
    assert ctx().points_check(curve, group, pts, subgroup=True)[0] == len(off)


def test_bn254_g1_has_cofactor_one():
    """subgroup changes nothing on BN254 G1: a random point of the curve is good either way."""
    from oracle.pyref.fields import FQ
    import points_mul_cases as PM
    q = FQ["bn254"].p
    x = 1
    while True:
        x += 1
        y = PM._sqrt_fq(q, x * x * x + 3)
        if y:
            break
    w = PM.pack_point("bn254", 1, (x, y))
    assert PC.decide("bn254", 1, w, True) == PC.GOOD
    for subgroup in (False, True):
        assert ctx().points_check("bn254", 1, w[None, :], subgroup=subgroup) == (0, 1)


def test_errors_leave_the_context_usable():
    from dg16_amd.lib import Dg16Error
    c = ctx()
    pts = PC.filler("bn254", 1, 4)
    with pytest.raises(Dg16Error) as e:
        c.points_check("bn254", 3, pts)
    assert e.value.code == 3
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    nb, fb = ctypes.c_size_t(7), ctypes.c_size_t(7)
    assert c.L.dg16_points_check(c.h, 0, 1, None, 4, 1, ctypes.byref(nb), ctypes.byref(fb)) == 3
    assert c.L.dg16_points_check(c.h, 0, 1, p(pts), 4, 1, None, ctypes.byref(fb)) == 3
    assert c.L.dg16_points_check(c.h, 0, 1, p(pts), 4, 1, ctypes.byref(nb), None) == 3
    assert c.L.dg16_points_check(c.h, 0, 0, p(pts), 4, 1, ctypes.byref(nb), ctypes.byref(fb)) == 3
    assert c.L.dg16_points_check(c.h, 9, 1, p(pts), 4, 1, ctypes.byref(nb), ctypes.byref(fb)) == 2
    assert c.L.dg16_points_check(c.h, 0, 1, None, 0, 1, ctypes.byref(nb), ctypes.byref(fb)) == 0     # n = 0 needs no pointer
    assert (nb.value, fb.value) == (0, 0)
    context_still_proves()
    assert c.points_check("bn254", 1, pts) == (0, 4)
