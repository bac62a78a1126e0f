"""The schedule and the per-product loop of distributed-groth16_amd/csrc/points_scale.h, compiled with the host compiler
(tests/host_arith/host_points_scale.cpp) and compared with the oracle: the CPU runs the text the kernel runs.  Group
operations are counted by the shim's Ops and held against dg16_points_mul's rows of DESIGN.md 2.9."""

import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import points_mul_cases as PM
import points_scale_cases as PS
from oracle import corc
from oracle.pyref.curves import CURVES
from oracle.pyref.fields import FQ, FR

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_arith", "host_points_scale.cpp")
SO = os.path.join(HERE, "host_arith", "libhost_points_scale.so")
CSRC = os.path.join(HERE, "..", "distributed-groth16_amd", "csrc")

# (curve, group, split): every path -- plain for all six groups, DIM 2 / DIM 4 where the group splits
PATHS = [(c, g, s) for c, g in PM.GROUPS for s in (0, 1)]


@pytest.fixture(scope="module")
def hs():
    hdrs = [os.path.join(CSRC, f) for f in ("points_scale.h", "wnaf.h", "points_mul.h", "slices.h", "glv_endo.h", "glv.h",
                                            "fp.h", "fp2.h", "ec.h", "types.h", "consts_gen.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(SO) < os.path.getmtime(p) for p in [SRC] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-o", SO, SRC])
    L = ctypes.CDLL(SO)
    vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.hs_params.argtypes = [vp]
    L.hs_schedule.argtypes = [i, i, vp, vp, vp]
    L.hs_recode.argtypes = [i, vp, i, vp]
    L.hs_lambda.argtypes = [i, vp]
    L.hs_scale.argtypes = [i, i, vp, vp, sz, vp, vp]
    L.hs_invert.argtypes = [i, vp, vp]
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _params(hs):
    out = np.zeros(3, dtype=np.int32)
    hs.hs_params(_p(out))
    return [int(v) for v in out]


def _words(k):
    return np.frombuffer(int(k).to_bytes(32, "little"), dtype=np.uint32).copy()


def _schedule(hs, g, split, k):
    """-> (parts, [digit list per part], rows)"""
    _, _, max_rows = _params(hs)
    digits = np.zeros((4, max_rows), dtype=np.int8)
    n = ctypes.c_int(0)
    dim = hs.hs_schedule(g, split, _p(_words(k)), _p(digits), ctypes.byref(n))
    return dim, [[int(v) for v in digits[j, :n.value]] for j in range(dim)], n.value


def test_width_and_table(hs):
    w, table, max_rows = _params(hs)
    assert w >= 4 and table == 1 << (w - 2) and max_rows >= 257


@pytest.mark.parametrize("curve,group,split", PATHS)
def test_schedule_is_a_width_w_naf_of_the_scalar(hs, curve, group, split):
    """Digits odd or zero with |d| < 2^(w-1), non-zero digits at least w apart, and the signed parts recombine to k: as
    an integer on the plain path, mod r through the endomorphism's eigenvalue on the split paths."""
    w, _, _ = _params(hs)
    g = PM.gid(curve, group)
    r = FR[curve].p
    lw = np.zeros(8, dtype=np.uint32)
    assert hs.hs_lambda(g, _p(lw)) == 0
    lam = int.from_bytes(lw.tobytes(), "little")
    for k in PS.scalar_list(curve, w):
        dim, parts, rows = _schedule(hs, g, split, k)
        assert dim == (1 if not split else 4 if group == 2 and curve != "bn254" else 2)
        total = 0
        top = 0
        for j, d in enumerate(parts):
            nz = [i for i, v in enumerate(d) if v]
            assert all(d[i] % 2 == 1 and abs(d[i]) < 1 << (w - 1) for i in nz), (hex(k), j)
            assert all(b - a >= w for a, b in zip(nz, nz[1:])), (hex(k), j)
            total += sum(v << i for i, v in enumerate(d)) * pow(lam, j, r)
            top = max(top, nz[-1] + 1 if nz else 0)
        assert rows == top, hex(k)                      # the chain starts at a non-zero digit
        if dim == 1:
            assert total == k, hex(k)
        else:
            assert (total - k) % r == 0, hex(k)


def _recoder_integers(w):
    """0, 1, 2^w - 1, 2^(w-1) (and the odd value next to it, the first whose digit is negative), 2^255 - 1, r - 1 of each
    curve and 64 seeded random values below 2^256"""
    rng = random.Random(77)
    return ([0, 1, (1 << w) - 1, 1 << (w - 1), (1 << (w - 1)) + 1, (1 << 255) - 1]
            + [FR[c].p - 1 for c in ("bn254", "bls12_381", "bls12_377")] + [rng.randrange(1 << 256) for _ in range(64)])


def _recode(hs, w, m, neg):
    max_rows = _params(hs)[2]
    digits = np.full(max_rows, 99, dtype=np.int8)
    n = hs.hs_recode(w, _p(_words(m)), neg, _p(digits))
    assert 0 <= n <= max_rows and not digits[n:].any()     # every position is written; none past the length is set
    return [int(v) for v in digits[:n]]


@pytest.mark.parametrize("w", [5, 7])
def test_the_shared_recoder_is_the_textbook_width_w_naf(hs, w):
    """wnaf.h's recode_wnaf at the widths of points_scale.h and pss_pack.h, on the same integers, against the definition:
    digits odd or zero, |d| < 2^(w-1), non-zero digits at least w apart, sum d_i 2^i = m, or -m with the sign folded in;
    the length ends at a non-zero digit."""
    for m in _recoder_integers(w):
        for neg in (0, 1):
            d = _recode(hs, w, m, neg)
            nz = [i for i, v in enumerate(d) if v]
            assert all(d[i] % 2 == 1 and abs(d[i]) < 1 << (w - 1) for i in nz), (hex(m), neg)
            assert all(b - a >= w for a, b in zip(nz, nz[1:])), (hex(m), neg)
            assert sum(v << i for i, v in enumerate(d)) == (-m if neg else m), (hex(m), neg)
            assert len(d) == (nz[-1] + 1 if nz else 0), (hex(m), neg)
    assert hs.hs_recode(6, _p(_words(1)), 0, _p(np.zeros(_params(hs)[2], dtype=np.int8))) == -1


def test_recoder_and_schedule_under_the_sanitizers(hs, tmp_path):
    """The same text as a stand-alone program under the address and undefined-behaviour sanitizers, on the integers of
    both widths: a clean run, and the lengths it prints are those of the library above."""
    exe = str(tmp_path / "host_points_scale")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DHOST_POINTS_SCALE_MAIN", "-o", exe, SRC])
    ms = _recoder_integers(5) + _recoder_integers(7)
    fin = tmp_path / "integers.bin"
    fin.write_bytes(b"".join(m.to_bytes(32, "little") for m in ms))
    res = subprocess.run([exe, str(fin)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and not res.stderr, res.stderr[-2000:]
    lines = res.stdout.splitlines()
    assert len(lines) == len(ms)
    for m, line in zip(ms, lines):
        want = [str(len(_recode(hs, w, m, neg))) for w in (5, 7) for neg in (0, 1)]
        if m < 1 << 255:
            for g in range(6):
                for split in (0, 1):
                    dim, _, rows = _schedule(hs, g, split, m)
                    want.append("%d:%d" % (dim, rows))
        assert line.split() == want, hex(m)


def _subgroup_points(curve, group):
    return [corc.generator(curve, group)[0], corc.gen_points(curve, group, 21, 3)[2],
            np.zeros(corc.point_limbs(curve, group), dtype=np.uint64)]


def _outside_points(curve, group):
    """curve points outside the subgroup as Python tuples: the one tests/points_check_cases.py uses, and the points of
    order three and two it names"""
    if (curve, group) not in PM.COFACTOR_GROUPS:
        return []
    out = [PM.outside_point(curve, group)]
    if (curve, group) == ("bls12_381", 1):
        out.append((0, 2))
    if (curve, group) == ("bls12_377", 1):
        out.append((FQ[curve].p - 1, 0))
    return out


def _scale(hs, g, split, bases, k):
    out = np.zeros_like(bases)
    counts = np.zeros((bases.shape[0], 2), dtype=np.uint32)
    assert hs.hs_scale(g, split, _p(bases), _p(_words(k)), bases.shape[0], _p(out), _p(counts)) == 0
    return out, counts


@pytest.mark.parametrize("curve,group,split", PATHS)
def test_products_equal_the_oracle_within_the_rows_of_points_mul(hs, curve, group, split):
    """k P for the scalar list on a generator, a random subgroup point and the identity (and, on the plain path of a
    cofactor group, curve points outside the subgroup), byte-equal to the oracle's.  Counts, table included: for every
    scalar additions <= dg16_points_mul's row and doublings <= that row + 1; the mean of the additions over the 64
    random scalars <= 0.85 x the row (the density of a width-w NAF, w >= 4)."""
    w, _, _ = _params(hs)
    g = PM.gid(curve, group)
    pts = _subgroup_points(curve, group)
    outside = [] if split else _outside_points(curve, group)
    bases = np.ascontiguousarray(np.stack(pts + [PM.pack_point(curve, group, P) for P in outside]))
    dim = _schedule(hs, g, split, 1)[0]
    row_dbl, row_add = PS.POINTS_MUL_ROW[dim]
    fixed, rnd = PS.fixed_scalars(curve, w), PS.random_scalars(curve)
    adds_random = []
    worst = [0, 0]
    for k in fixed + rnd:
        out, counts = _scale(hs, g, split, bases, k)
        for i, P in enumerate(pts):
            assert np.array_equal(out[i], corc.point_mul(curve, group, P[None, :], k)[0]), (hex(k), i)
        for i, P in enumerate(outside):
            assert np.array_equal(out[len(pts) + i], PM.ref_mul_any(curve, group, P, k)), (hex(k), P)
        assert (counts == counts[0]).all()              # the sequence of operations depends on the scalar alone
        worst = [max(worst[0], int(counts[0, 0])), max(worst[1], int(counts[0, 1]))]
        assert counts[0, 1] <= row_add and counts[0, 0] <= row_dbl + 1, (hex(k), counts[0])
        if k in rnd:
            adds_random.append(int(counts[0, 1]))
    mean = sum(adds_random) / len(adds_random)
    print("%s G%d parts=%d: mean additions %.2f (row %d), worst doublings %d additions %d"
          % (curve, group, dim, mean, row_add, worst[0], worst[1]))
    assert mean <= 0.85 * row_add, mean


@pytest.mark.parametrize("curve", ["bn254", "bls12_381", "bls12_377"])
def test_the_inverse_of_a_contribution(hs, curve):
    """d^-1 mod r as dg16_groth16_contribute takes it; zero and values from r on are refused."""
    r = FR[curve].p
    out = np.zeros(8, dtype=np.uint32)
    for d in (1, 2, r - 1, 0x1234567 << 200 | 5):
        d %= r
        assert hs.hs_invert(corc.CURVES[curve], _p(_words(d)), _p(out)) == 0
        assert int.from_bytes(out.tobytes(), "little") == pow(d, r - 2, r)
    for d in (0, r, r + 1, (1 << 256) - 1):
        assert hs.hs_invert(corc.CURVES[curve], _p(_words(d)), _p(out)) == -1


def test_order_two_and_three_points_are_what_they_are_named():
    c = CURVES["bls12_381", "g1"]
    assert c.on_curve((0, 2)) and c.mul((0, 2), 3) is None
    c = CURVES["bls12_377", "g1"]
    T = (FQ["bls12_377"].p - 1, 0)
    assert c.on_curve(T) and c.mul(T, 2) is None
