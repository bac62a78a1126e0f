"""GPU: dg16_points_mul (Context.points_mul), out[i] = k_i P_i, for all six groups.  Expected values come from the
oracle: `corc.point_mul` per index, and `oracle.pyref.curves.CURVES` (integer multiples) for points outside the
order-r subgroups.  The scalar list S and the special points are those of tests/points_mul_cases.py, which the CPU test
(tests/test_points_mul_host.py) runs through the same header text."""

import ctypes
import random

import numpy as np
import pytest

import points_mul_cases as PM
from oracle import corc
from oracle.pyref.curves import CURVES
from oracle.pyref.fields import FR
from gpu_util import ctx
from test_gpu_verify import context_still_proves

pytestmark = pytest.mark.gpu

_special = {}


def _neg(curve, group, p):
    """-P of a packed affine point (y negated in the coordinate field; the identity stays zero bytes)."""
    nl = corc.FQ_LIMBS[curve]
    q = p.copy()
    half = p.size // 2
    y = np.ascontiguousarray(p[half:].reshape(-1, nl))
    q[half:] = corc.field_op(curve, "fq", "neg", y).reshape(-1)
    return q


def special_case(curve, group):
    """n = 65: oracle points with the identity at 0 and 64, P and -P adjacent (10, 11), one point four times (20..23);
    S cycled.  Built once per group with its expected products: canonical scalars (values >= r included) and
    Montgomery scalars (values below r)."""
    key = (curve, group)
    if key not in _special:
        n = 65
        pts = corc.gen_points(curve, group, 31 + PM.gid(curve, group), n)
        pts[0] = 0
        pts[64] = 0
        pts[11] = _neg(curve, group, pts[10])
        pts[21:24] = pts[20]
        below, above = PM.scalar_list(curve)
        kc = [(below + above)[i % len(below + above)] for i in range(n)]
        km = [below[(i * 7) % len(below)] for i in range(n)]
        exp = {False: np.stack([corc.point_mul(curve, group, pts[i:i + 1], kc[i])[0] for i in range(n)]),
               True: np.stack([corc.point_mul(curve, group, pts[i:i + 1], km[i])[0] for i in range(n)])}
        _special[key] = (pts, {False: kc, True: km}, exp)
    return _special[key]


@pytest.mark.parametrize("in_subgroup", [False, True])
@pytest.mark.parametrize("mont", [False, True])
@pytest.mark.parametrize("curve,group", PM.GROUPS)
def test_scalar_list_over_special_points(curve, group, mont, in_subgroup):
    pts, ks, exp = special_case(curve, group)
    got = ctx().points_mul(curve, group, pts, PM.scalars_arr(curve, ks[mont], mont=mont), scalars_mont=mont,
                           in_subgroup=in_subgroup)
    bad = [i for i in range(len(pts)) if not np.array_equal(got[i], exp[mont][i])]
    assert not bad, [(i, hex(ks[mont][i])) for i in bad]
    assert not got[0].any() and not got[64].any()


_edges = {}


def edge_case(curve, group):
    if (curve, group) not in _edges:
        n = 300
        rng = random.Random(41)
        r = FR[curve].p
        pts = corc.gen_points(curve, group, 77, n)
        ks = [rng.randrange(r) for _ in range(n)]
        exp = np.stack([corc.point_mul(curve, group, pts[i:i + 1], ks[i])[0] for i in range(n)])
        _edges[curve, group] = (pts, ks, exp)
    return _edges[curve, group]


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 300])
@pytest.mark.parametrize("curve,group", [("bn254", 1), ("bls12_381", 2)])
def test_wave_and_workgroup_edges(curve, group, n):
    pts, ks, exp = edge_case(curve, group)
    for in_subgroup in (False, True):
        got = ctx().points_mul(curve, group, pts[:n], PM.scalars_arr(curve, ks[:n]), in_subgroup=in_subgroup)
        assert got.shape == exp[:n].shape and np.array_equal(got, exp[:n])


@pytest.mark.parametrize("curve,group", [("bn254", 1), ("bls12_377", 2)])
def test_more_than_one_slice(curve, group):
    """n = 4 133 with the slice lowered to 1 024 products: five launches, the last one short.  Every index has its own
    point and scalar (48-bit scalars keep the oracle's side quick; every 97th is full width)."""
    n = 4133
    rng = random.Random(43)
    r = FR[curve].p
    pts = corc.gen_points(curve, group, 79, n)
    ks = [rng.randrange(r) if i % 97 == 0 else rng.randrange(1 << 48) for i in range(n)]
    exp = np.stack([corc.point_mul(curve, group, pts[i:i + 1], ks[i])[0] for i in range(n)])
    c = ctx()
    c.set_points_mul_slice(1024)
    try:
        got = c.points_mul(curve, group, pts, PM.scalars_arr(curve, ks), in_subgroup=(group == 2))
    finally:
        c.set_points_mul_slice(0)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, bad[:8]


@pytest.mark.parametrize("curve,group", PM.COFACTOR_GROUPS)
def test_any_point_of_the_curve(curve, group):
    """Without DG16_F_BASES_IN_SUBGROUP a cofactor group takes the unsplit path: points OUTSIDE the order-r subgroup and
    scalars of S, those >= r included, give the integer multiple."""
    c = CURVES[curve, "g%d" % group]
    Q = PM.outside_point(curve, group)
    qs = [c.mul(Q, j) for j in (1, 2, 3, 5)]
    below, above = PM.scalar_list(curve)
    s = above + below
    n = 64
    ks = [s[i % len(s)] for i in range(n)]
    P = [qs[i % 4] for i in range(n)]
    pts = np.stack([PM.pack_point(curve, group, p) for p in P])
    got = ctx().points_mul(curve, group, pts, PM.scalars_arr(curve, ks))
    for i in range(n):
        assert np.array_equal(got[i], PM.ref_mul_any(curve, group, P[i], ks[i])), (i, hex(ks[i]))


def test_device_pointers_in_place_and_beside_an_ntt():
    import torch
    dev = torch.device("cuda", 0)
    c = ctx()
    curve, group = "bls12_381", 1
    pts, ks, exp = edge_case("bn254", 1)
    n = len(ks)
    # case one: out is points
    d_pts = torch.from_numpy(pts.view(np.int64)).to(dev)
    d_ks = torch.from_numpy(PM.scalars_arr("bn254", ks).view(np.int64)).to(dev)
    torch.cuda.synchronize()
    c.points_mul("bn254", 1, d_pts, d_ks, device=True, n=n)
    c.sync(0)
    assert np.array_equal(d_pts.cpu().numpy().view(np.uint64), exp)
    # case two: a separate out on channel 1 while channel 0 runs an NTT
    log_n = 14
    data = corc.rand_field("bn254", "fr", 5, 1 << log_n)
    want_ntt = corc.ntt("bn254", data)
    d_data = torch.from_numpy(data.view(np.int64)).to(dev)
    d_pts = torch.from_numpy(pts.view(np.int64)).to(dev)
    d_out = torch.zeros_like(d_pts)
    torch.cuda.synchronize()
    c.ntt_dev("bn254", d_data.data_ptr(), log_n, channel=0)
    c.points_mul("bn254", 1, d_pts, d_ks, in_subgroup=True, device=True, channel=1, out=d_out, n=n)
    c.sync(0)
    c.sync(1)
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), exp)
    assert np.array_equal(d_pts.cpu().numpy().view(np.uint64), pts)
    assert np.array_equal(d_data.cpu().numpy().view(np.uint64), want_ntt)


def test_errors_leave_the_context_usable():
    from dg16_amd.lib import Dg16Error
    c = ctx()
    pts, ks, exp = edge_case("bn254", 1)
    sc = PM.scalars_arr("bn254", ks)
    with pytest.raises(Dg16Error) as e:
        c.points_mul("bn254", 3, pts[:4], sc[:4])
    assert e.value.code == 3
    out = np.zeros_like(pts)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for args in ((None, p(sc), p(out)), (p(pts), None, p(out)), (p(pts), p(sc), None)):
        assert c.L.dg16_points_mul(c.h, 0, 1, args[0], args[1], 4, args[2], 0, 0) == 3
    assert c.L.dg16_points_mul(c.h, 0, 1, None, None, 0, None, 0, 0) == 0           # n = 0 needs no pointers
    assert c.L.dg16_points_mul(c.h, 9, 1, p(pts), p(sc), 4, p(out), 0, 0) == 2
    context_still_proves()
    assert np.array_equal(c.points_mul("bn254", 1, pts[:4], sc[:4]), exp[:4])
