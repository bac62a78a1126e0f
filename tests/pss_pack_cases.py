"""Shared cases of the share-packing tests (tests/test_pss_pack_host.py on a CPU, tests/test_gpu_pss_pack.py on the GPU):
the pack matrix as the oracle has it, the inputs that make the complete addition law work inside a chunk, and the
oracle's side of every comparison.  The method is the one of tests/test_gpu_dist_packing.py (exp_matrix,
apply_in_exponent), restated for party-major shares of identity-padded chunks.  Expected values come from the oracle
only."""

import functools
import os

import numpy as np

import points_mul_cases as PM
from oracle import corc
from oracle.pyref.curves import CURVES
from oracle.pyref.fields import FQ, FR
from oracle.pyref.pss import PackedSharingParams as RefPSS

GROUPS = PM.GROUPS
LS = (1, 2, 4, 8)
# (curve, group, split): every path -- plain for all six groups, DIM 2 / DIM 4 where the group splits
PATHS = [(c, g, s) for c, g in GROUPS for s in (0, 1)]


def dim_of(curve, group, split):
    return 1 if not split else 4 if group == 2 and curve != "bn254" else 2


def gpu_splits(curve, group, in_subgroup):
    """whether dg16_pss_pack_points splits (pmul::may_split): cofactor one, or the caller's word"""
    return (curve, group) == ("bn254", 1) or bool(in_subgroup)


@functools.lru_cache(maxsize=None)
def pack_matrix(curve, l):
    """M[r][c] of the oracle's pack_from_public, canonical: the images of the unit vectors."""
    ref = RefPSS(FR[curve], l)
    images = [ref.pack_from_public([int(i == c) for i in range(l)]) for c in range(l)]
    return tuple(tuple(row) for row in zip(*images))


def matrix_words(curve, l):
    """[4 l][l][8] 32-bit words, as the host shim takes the matrix"""
    flat = [v for row in pack_matrix(curve, l) for v in row]
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in flat), dtype=np.uint32).copy()


def pad_chunks(points, l):
    """[n_points][limbs] -> [chunks][l][limbs], the last chunk filled with identities (zero bytes)"""
    points = np.ascontiguousarray(points, dtype=np.uint64)
    pad = (-points.shape[0]) % l
    if pad:
        points = np.concatenate([points, np.zeros((pad, points.shape[1]), dtype=np.uint64)])
    return points.reshape(-1, l, points.shape[1])


def oracle_shares(curve, group, l, points):
    """[n][chunks][limbs]: share r of chunk e = sum_c M[r][c] P[e l + c] by the C oracle's MSM (subgroup points)."""
    rows = [corc.ints_to_arr(list(row), 4) for row in pack_matrix(curve, l)]
    P = pad_chunks(points, l)
    return np.stack([np.concatenate([corc.msm(curve, group, np.ascontiguousarray(Pe), sc, threads=1) for Pe in P])
                     for sc in rows])


def oracle_shares_any(curve, group, l, chunk):
    """[n][limbs] for ONE chunk of Python tuples (None = identity) that may lie outside the subgroup: integer multiples
    by the oracle's curve arithmetic."""
    c = CURVES[curve, "g%d" % group]
    out = []
    for row in pack_matrix(curve, l):
        acc = None
        for k, P in zip(row, chunk):
            acc = c.add(acc, c.mul(P, k))
        out.append(PM.pack_point(curve, group, acc))
    return np.stack(out)


OUTSIDE_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pss_pack_outside.npz")


def outside_key(curve, group, l):
    return "%s_g%d_l%d" % (curve, group, l)


@functools.lru_cache(maxsize=None)
def _outside_golden():
    with np.load(OUTSIDE_GOLDEN) as z:
        return {k: z[k] for k in z.files}


def outside_expected(curve, group, l):
    """oracle_shares_any(curve, group, l, outside_chunk(curve, group, l)) as recorded in tests/golden: the sums are pure
    Python (256 G2 products at l = 8, several seconds), so the GPU test reads them.  tests/test_pss_pack_host.py
    recomputes every one of them with the oracle and compares, which keeps the file honest; write_outside_golden()
    makes it."""
    return _outside_golden()[outside_key(curve, group, l)]


def write_outside_golden():
    out = {outside_key(c, g, l): oracle_shares_any(c, g, l, outside_chunk(c, g, l))
           for c, g in PM.COFACTOR_GROUPS for l in LS}
    np.savez_compressed(OUTSIDE_GOLDEN, **out)


def neg_point(curve, group, p):
    """-P of a packed affine Montgomery point (y -> q - y per coordinate; the identity stays)."""
    p = np.array(p, dtype=np.uint64)
    if not p.any():
        return p
    q = FQ[curve].p
    nl = corc.point_limbs(curve, group)
    fl = FQ[curve].p.bit_length() // 64 + 1
    half = nl // 2
    ys = []
    for i in range(half // fl):
        y = int.from_bytes(p[half + i * fl: half + (i + 1) * fl].tobytes(), "little")
        ys.append((q - y) % q)
    p[half:] = np.frombuffer(b"".join(y.to_bytes(8 * fl, "little") for y in ys), dtype=np.uint64)
    return p


@functools.lru_cache(maxsize=None)
def _base_points(curve, group):
    pts = corc.gen_points(curve, group, 77, 1100)
    pts.setflags(write=False)
    return pts


def subgroup_points(curve, group, n_points, l):
    """n_points points of the order-r group whose first chunks exercise the addition law: the identity (index 1), a
    duplicated point (0 and 2 where they share a chunk, else 0 and l - 1 .. ), a point and its negative in one chunk.
    For l = 1 a chunk is one point: the identity, a point and its negative still appear, in chunks of their own."""
    pts = np.array(_base_points(curve, group)[:n_points], dtype=np.uint64)
    n = pts.shape[0]
    if n > 1:
        pts[1] = 0
    if l >= 2 and n > l + 1:               # chunk 1: (P, P, ..)
        pts[l + 1] = pts[l]
    if l >= 2 and n > 2 * l + 1:           # chunk 2: (P, -P, ..)
        pts[2 * l + 1] = neg_point(curve, group, pts[2 * l])
    if l == 1 and n > 3:
        pts[3] = neg_point(curve, group, pts[2])
    return pts


def host_chunks(curve, group, l):
    """The 3-chunk cases of the host loop test as (name, [3 l] packed points): subgroup points; a chunk of identities;
    a chunk (P, P, ..); a chunk (P, -P, ..); a chunk with one identity."""
    base = _base_points(curve, group)
    g = base[:3 * l].copy()
    ident = g.copy()
    ident[l:2 * l] = 0
    same = g.copy()
    same[l:2 * l] = g[0]
    opp = g.copy()
    for i in range(l):
        opp[l + i] = g[0] if i % 2 == 0 else neg_point(curve, group, g[0])
    one = g.copy()
    one[l + (l - 1)] = 0
    return [("subgroup", g), ("identities", ident), ("equal", same), ("opposite", opp), ("one identity", one)]


def outside_chunk(curve, group, l):
    """One chunk of l curve points OUTSIDE the order-r subgroup (cofactor groups), as Python tuples: the point
    tests/points_mul_cases.py finds, its multiples, and where the curve has them the points of order three and two."""
    if (curve, group) not in PM.COFACTOR_GROUPS:
        return None
    c = CURVES[curve, "g%d" % group]
    P = PM.outside_point(curve, group)
    extra = []
    if (curve, group) == ("bls12_381", 1):
        extra.append((0, 2))
    if (curve, group) == ("bls12_377", 1):
        extra.append((FQ[curve].p - 1, 0))
    chunk = [P] + extra + [c.mul(P, 2 + i) for i in range(l)]
    return chunk[:l]
