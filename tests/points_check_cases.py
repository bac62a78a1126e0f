"""Shared cases of the membership tests (tests/test_points_check_host.py on a CPU, tests/test_gpu_points_check.py and
tests/test_gpu_srs_verify.py on the GPU): special points of all six groups with the verdict each must get, filler points
of the subgroups, and the plain-Python decision every expectation comes from -- reduced coordinates, the curve equation
and r P with the group law of oracle.pyref.curves, all in big integers.  Nothing here asks the library."""

import random

import numpy as np

import points_mul_cases as PM
from oracle.pyref.curves import CURVES
from oracle.pyref.fields import FQ, FR

GROUPS = PM.GROUPS
GOOD, UNREDUCED, OFF_CURVE, OFF_SUBGROUP = 0, 1, 2, 3       # pchk::Verdict of points_check.h


def _curve(curve, group):
    return CURVES[curve, "g%d" % group]


def coords(curve, group, words):
    """packed affine point -> the stored (Montgomery) integers, x then y, one per base-field element"""
    nl = FQ[curve].limbs64
    w = np.asarray(words, dtype=np.uint64).reshape(-1, nl)
    return [int.from_bytes(row.tobytes(), "little") for row in w]


def pack_raw(curve, vals):
    """stored integers (NOT reduced) -> packed words"""
    nb = FQ[curve].limbs64 * 8
    return np.concatenate([np.frombuffer(int(v).to_bytes(nb, "little"), dtype=np.uint64) for v in vals])


def decide(curve, group, words, subgroup):
    """The verdict of a packed point, in plain Python."""
    F = FQ[curve]
    vals = coords(curve, group, words)
    if not any(vals):
        return GOOD
    if any(v >= F.p for v in vals):
        return UNREDUCED
    v = [F.from_mont(x) for x in vals]
    P = (v[0], v[1]) if group == 1 else ((v[0], v[1]), (v[2], v[3]))
    c = _curve(curve, group)
    if not c.on_curve(P):
        return OFF_CURVE
    if subgroup and c.mul(P, FR[curve].p) is not None:
        return OFF_SUBGROUP
    return GOOD


def _bump_first(curve, words, coordinate, group):
    """stored value of x (coordinate 0) or y (1) plus q: the same field element, not reduced"""
    vals = coords(curve, group, words)
    per = 1 if group == 1 else 2
    vals[coordinate * per] += FQ[curve].p
    return pack_raw(curve, vals)


def twist_point_with_x_in_fq(curve, seed=5):
    """A point of the twist whose x lies in Fq (x = (x0, 0)); its y is a general element of Fq2."""
    c = _curve(curve, 2)
    q = FQ[curve].p
    rng = random.Random(seed)
    while True:
        x = (rng.randrange(1, q), 0)
        y = PM._sqrt_fq2(c.F, q, c.F.add(c.F.mul(c.F.mul(x, x), x), c.b))
        if y is not None and y != (0, 0) and c.on_curve((x, y)):
            return (x, y)


_cases = {}


def cases(curve, group):
    """[(name, packed point, verdict with subgroup = 0, verdict with subgroup = 1)] for one group.  The verdicts are
    decide()'s; the assertions pin that each case is what its name says."""
    key = (curve, group)
    if key in _cases:
        return _cases[key]
    c = _curve(curve, group)
    q = FQ[curve].p
    rng = random.Random(100 + PM.gid(curve, group))
    zero = c.F.zero
    gen = PM.pack_point(curve, group, c.gen)
    x, y = c.gen
    xb = c.F.add(x, c.F.one)
    out = [("identity", np.zeros_like(gen), GOOD, GOOD),
           ("generator", gen, GOOD, GOOD),
           ("x + q as x", _bump_first(curve, gen, 0, group), UNREDUCED, UNREDUCED),
           ("y + q as y", _bump_first(curve, gen, 1, group), UNREDUCED, UNREDUCED),
           ("(x + 1, -y)", PM.pack_point(curve, group, (xb, c.F.neg(y))), OFF_CURVE, OFF_CURVE)]
    xr = rng.randrange(1, q) if group == 1 else (rng.randrange(1, q), rng.randrange(1, q))
    out.append(("(random x, 0)", PM.pack_point(curve, group, (xr, zero)), OFF_CURVE, OFF_CURVE))
    if key != ("bn254", 1):
        out.append(("curve point outside the subgroup", PM.pack_point(curve, group, PM.outside_point(curve, group)),
                    GOOD, OFF_SUBGROUP))
    if key == ("bls12_381", 1):
        out.append(("order-3 point (0, 2)", PM.pack_point(curve, group, (0, 2)), GOOD, OFF_SUBGROUP))
    if key == ("bls12_377", 1):
        out.append(("order-2 point (q - 1, 0)", PM.pack_point(curve, group, (q - 1, 0)), GOOD, OFF_SUBGROUP))
    if group == 2:
        # a twist point with BOTH coordinates in Fq needs b' in Fq, which holds for none of the three twists (asserted);
        # the nearest thing every twist has is a point whose x lies in Fq
        assert c.b[1] != 0
        P = twist_point_with_x_in_fq(curve)
        out.append(("twist point with x in Fq", PM.pack_point(curve, group, P), GOOD,
                    OFF_SUBGROUP if c.mul(P, FR[curve].p) is not None else GOOD))
    for name, words, v0, v1 in out:
        assert decide(curve, group, words, False) == v0 and decide(curve, group, words, True) == v1, (key, name)
    _cases[key] = out
    return out


_fill = {}


def filler(curve, group, n=1000):
    """n distinct points of the order-r subgroup, built in plain Python: (k0 + i) G by repeated addition."""
    key = (curve, group)
    if key not in _fill or len(_fill[key]) < n:
        c = _curve(curve, group)
        k0 = random.Random(7 + PM.gid(curve, group)).randrange(1, FR[curve].p)
        P = c.mul(c.gen, k0)
        pts = []
        for _ in range(max(n, 1)):
            pts.append(PM.pack_point(curve, group, P))
            P = c.add(P, c.gen)
        _fill[key] = np.stack(pts)
    return _fill[key][:n].copy()


def bad_points(curve, group, subgroup):
    """the packed special points that are bad under `subgroup`"""
    return [w for _, w, v0, v1 in cases(curve, group) if (v1 if subgroup else v0) != GOOD]
