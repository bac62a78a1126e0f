"""Shared cases of the batched point multiplication and re-randomization tests (tests/test_points_mul_host.py on a CPU,
tests/test_gpu_points_mul.py and tests/test_gpu_rerandomize.py on the GPU): the scalar list S, points outside the
order-r subgroups, and the oracle's side of every comparison.  Expected values come from the oracle only."""

import random

import numpy as np

import verify_cases as VC
from oracle import corc
from oracle.pyref.curves import CURVES
from oracle.pyref.fields import FQ, FR

GROUPS = [("bn254", 1), ("bn254", 2), ("bls12_381", 1), ("bls12_381", 2), ("bls12_377", 1), ("bls12_377", 2)]
COFACTOR_GROUPS = [g for g in GROUPS if g != ("bn254", 1)]
W = 4                       # the window width of points_mul.h (checked against the header by the CPU test)


def gid(curve, group):
    return 2 * corc.CURVES[curve] + group - 1


def _pattern_below(nibble, r):
    v = int("%x" % nibble * 64, 16)
    while v >= r:
        v >>= 4
    return v


def forcing_scalars(r):
    """The scalars that drive the plain loop's accumulator onto +-(the table entry it adds), for a point of order r.
    Before the last window the accumulator is 16 v P with k = 16 v + d0, |d0| <= 8.  16 v = m r + e with |e| <= 8 makes it
    e P; the addend is d0 P.  e = -d0: k = m r (P - P); e = d0: k = m r + 2 e (a doubling), with e = -(m r) mod 16 taken in
    [-8, 8).  m = 1, 2, 3 where the scalar stays below 2^255."""
    out = []
    for m in (1, 2, 3):
        e = (-(m * r)) % 16
        if e >= 8:
            e -= 16
        for k in (m * r, m * r + 2 * e):
            if 0 < k < 1 << 255:
                out.append(k)
    return out


def scalar_list(curve):
    """S of the issue, as (canonical-or-Montgomery list of values < r, canonical-only list of values >= r)."""
    r = FR[curve].p
    s = [0, 1, 2, 3, 7, 8, 9, 15, 16, 17,
         (1 << W) - 1, 1 << W, (1 << W) + 1, 1 << (W - 1),
         _pattern_below(0x1, r), _pattern_below(0x8, r), _pattern_below(0xF, r),
         1 << 127, (1 << 128) - 1, 1 << 128, 1 << 253,
         r - 2, r - 1, (r - 1) // 2, (r + 1) // 2,
         r, r + 1, (1 << 255) - 1] + forcing_scalars(r)
    seen, below, above = set(), [], []
    for k in s:
        if k in seen:
            continue
        seen.add(k)
        (below if k < r else above).append(k)
    return below, above


def scalars_arr(curve, ks, mont=False):
    F = FR[curve]
    return corc.ints_to_arr([F.to_mont(k) if mont else k for k in ks], 4)


def pack_point(curve, group, P):
    return (VC.g1 if group == 1 else VC.g2)(curve, P)


def _sqrt_fq(q, a):
    """Tonelli-Shanks; None for a non-residue."""
    a %= q
    if a == 0:
        return 0
    if pow(a, (q - 1) // 2, q) != 1:
        return None
    s, t = 0, q - 1
    while t % 2 == 0:
        s, t = s + 1, t // 2
    z = 2
    while pow(z, (q - 1) // 2, q) != q - 1:
        z += 1
    m, c, u, x = s, pow(z, t, q), pow(a, t, q), pow(a, (t + 1) // 2, q)
    while u != 1:
        i, v = 0, u
        while v != 1:
            v, i = v * v % q, i + 1
        b = pow(c, 1 << (m - i - 1), q)
        m, c, u, x = i, b * b % q, u * b * b % q, x * b % q
    return x


def _sqrt_fq2(F2, q, a):
    """Square root of a = a0 + a1 u in Fq[u] / (u^2 - nr), by the norm; None for a non-square."""
    nr = F2.mul((0, 1), (0, 1))[0]
    if a[1] == 0:
        y0 = _sqrt_fq(q, a[0])
        if y0 is not None:
            return (y0, 0)
        y1 = _sqrt_fq(q, a[0] * pow(nr, q - 2, q))
        return None if y1 is None else (0, y1)
    s = _sqrt_fq(q, a[0] * a[0] - nr * a[1] * a[1])
    if s is None:
        return None
    for sg in (s, q - s):
        y0 = _sqrt_fq(q, (a[0] + sg) * pow(2, q - 2, q))
        if y0:
            y = (y0, a[1] * pow(2 * y0, q - 2, q) % q)
            if F2.mul(y, y) == (a[0] % q, a[1] % q):
                return y
    return None


def outside_point(curve, group, seed=1):
    """A point of the curve outside its order-r subgroup (cofactor groups only), as the oracle's Python tuple."""
    assert (curve, group) != ("bn254", 1), "BN254 G1 has cofactor one"
    c = CURVES[curve, "g%d" % group]
    q, r = FQ[curve].p, FR[curve].p
    rng = random.Random(seed)
    while True:
        if group == 1:
            x = rng.randrange(q)
            y = _sqrt_fq(q, x * x * x + c.b)
        else:
            x = (rng.randrange(q), rng.randrange(q))
            y = _sqrt_fq2(c.F, q, c.F.add(c.F.mul(c.F.mul(x, x), x), c.b))
        if y is None or y in (0, (0, 0)):
            continue
        P = (x, y)
        if c.on_curve(P) and c.mul(P, r) is not None:
            return P


def ref_mul_any(curve, group, P, k):
    """k P as an INTEGER multiple (k may be >= r, P outside the subgroup), packed."""
    return pack_point(curve, group, CURVES[curve, "g%d" % group].mul(P, k))


def oracle_rerandomize(curve, proof, delta_g2, r1, r2):
    """(r1^-1 A, r1 B + r1 r2 delta, C + r2 A) with the oracle's curve arithmetic; proof = (A, B, C) Python tuples."""
    r = FR[curve].p
    c1, c2 = CURVES[curve, "g1"], CURVES[curve, "g2"]
    A, B, C = proof
    return (c1.mul(A, pow(r1, r - 2, r)),
            c2.add(c2.mul(B, r1), c2.mul(delta_g2, r1 * r2 % r)),
            c1.add(C, c1.mul(A, r2)))
