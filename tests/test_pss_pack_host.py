"""The schedule, the table build and the combine loop of distributed-groth16_amd/csrc/pss_pack.h, compiled with the host
compiler (tests/host_arith/host_pss_pack.cpp) and compared with the oracle: the CPU runs the text the kernels run.  Group
operations are counted by the shim's Ops and held against the header's count and against one pscale::product per
matrix entry (what n l calls of the one-scalar path would cost)."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

import points_mul_cases as PM
import pss_pack_cases as PC
from oracle.pyref.fields import FR

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_arith", "host_pss_pack.cpp")
SO = os.path.join(HERE, "host_arith", "libhost_pss_pack.so")
CSRC = os.path.join(HERE, "..", "distributed-groth16_amd", "csrc")

# doublings per output, table share included: points_scale.h's budget, whatever l is
DBL_BOUND = {1: 256, 2: 128, 4: 68}


@pytest.fixture(scope="module")
def hp():
    hdrs = [os.path.join(CSRC, f) for f in ("pss_pack.h", "points_scale.h", "points_mul.h", "glv_endo.h", "glv.h", "fp.h",
                                            "fp2.h", "ec.h", "types.h", "consts_gen.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(SO) < os.path.getmtime(p) for p in [SRC] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-o", SO, SRC])
    L = ctypes.CDLL(SO)
    vp, sz, i, u = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint
    L.hp_params.argtypes = [vp]
    L.hp_schedule.argtypes = [i, i, u, vp, vp, vp]
    L.hp_lambda.argtypes = [i, vp]
    L.hp_pack.argtypes = [i, i, u, vp, vp, sz, vp, vp, vp]
    L.hp_one_product.argtypes = [i, i, vp, vp, vp]
    L.hp_slice_chunks.argtypes = [sz, u]
    L.hp_slice_chunks.restype = sz
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _params(hp):
    out = np.zeros(3, dtype=np.int32)
    hp.hp_params(_p(out))
    return [int(v) for v in out]


def _schedule(hp, curve, group, split, l):
    """-> (parts per scalar, digits[r][c][j] as lists over the row's positions, lens[r])"""
    _, _, max_rows = _params(hp)
    n = 4 * l
    dim = PC.dim_of(curve, group, split)
    digits = np.zeros((n, l * dim, max_rows), dtype=np.int8)
    lens = np.zeros(n, dtype=np.int32)
    got = hp.hp_schedule(PM.gid(curve, group), split, l, _p(PC.matrix_words(curve, l)), _p(digits), _p(lens))
    assert got == dim
    return dim, digits, [int(v) for v in lens]


def _pack(hp, curve, group, split, l, points):
    n = 4 * l
    points = np.ascontiguousarray(points, dtype=np.uint64)
    chunks = -(-points.shape[0] // l)
    out = np.zeros((n, chunks, points.shape[1]), dtype=np.uint64)
    tcounts = np.zeros((chunks * l, 2), dtype=np.uint32)
    ccounts = np.zeros((n, chunks, 2), dtype=np.uint32)
    assert hp.hp_pack(PM.gid(curve, group), split, l, _p(PC.matrix_words(curve, l)), _p(points), points.shape[0], _p(out),
                      _p(tcounts), _p(ccounts)) == 0
    return out, tcounts, ccounts


def test_width_table_and_slices(hp):
    w, table, max_rows = _params(hp)
    assert w >= 5 and table == 1 << (w - 2) and max_rows >= 257 and 1 << (w - 1) <= 128      # digits are signed bytes
    # chunks per slice: outputs within the setting, a multiple of 64, never below one wave
    for n in (4, 8, 16, 32):
        for setting in (1 << 16, 1 << 12, 64 * n, 64 * n + 63, 130 * n, 1):
            c = hp.hp_slice_chunks(setting, n)
            assert c % 64 == 0 and c >= 64 and (c * n <= setting or c == 64)


@pytest.mark.parametrize("l", PC.LS)
@pytest.mark.parametrize("curve,group,split", PC.PATHS)
def test_every_part_of_every_row_is_a_width_w_naf_of_the_matrix(hp, curve, group, split, l):
    """Digits odd or zero with |d| < 2^(w-1), non-zero digits at least w apart, the signed parts recombine to M[r][c] (as
    an integer on the plain path, mod r through the endomorphism's eigenvalue on the split paths), and the row's length
    is the top non-zero position of any of its parts plus one."""
    w, _, _ = _params(hp)
    r_mod = FR[curve].p
    lw = np.zeros(8, dtype=np.uint32)
    assert hp.hp_lambda(PM.gid(curve, group), _p(lw)) == 0
    lam = int.from_bytes(lw.tobytes(), "little")
    dim, digits, lens = _schedule(hp, curve, group, split, l)
    M = PC.pack_matrix(curve, l)
    for r in range(4 * l):
        top = 0
        for c in range(l):
            total = 0
            for j in range(dim):
                d = [int(v) for v in digits[r, c * dim + j]]
                nz = [i for i, v in enumerate(d) if v]
                assert all(d[i] % 2 == 1 and abs(d[i]) < 1 << (w - 1) for i in nz), (r, c, j)
                assert all(b - a >= w for a, b in zip(nz, nz[1:])), (r, c, j)
                total += sum(v << i for i, v in enumerate(d)) * pow(lam, j, r_mod)
                top = max(top, nz[-1] + 1 if nz else 0)
            if dim == 1:
                assert total == M[r][c], (r, c)
            else:
                assert (total - M[r][c]) % r_mod == 0, (r, c)
        assert lens[r] == top, r


@pytest.mark.parametrize("l", PC.LS)
@pytest.mark.parametrize("curve,group,split", PC.PATHS)
def test_loop_equals_the_oracle_with_exact_counts(hp, curve, group, split, l):
    """Three chunks per case -- subgroup points, a chunk of identities, (P, P, ..), (P, -P, ..), one identity -- equal the
    oracle's sums byte for byte, and the operation counts are exactly the schedule's: per input point one doubling and
    2^(w-2) - 1 additions for its table; for row r (top position) doublings and (non-zero digits) additions."""
    w, table, _ = _params(hp)
    dim, digits, lens = _schedule(hp, curve, group, split, l)
    nonzero = [int(np.count_nonzero(digits[r])) for r in range(4 * l)]
    for name, pts in PC.host_chunks(curve, group, l):
        out, tcounts, ccounts = _pack(hp, curve, group, split, l, pts)
        assert np.array_equal(out, PC.oracle_shares(curve, group, l, pts)), name
        assert (tcounts == [1, table - 1]).all() and table - 1 == (1 << (w - 2)) - 1, name
        for r in range(4 * l):
            assert (ccounts[r] == [max(lens[r] - 1, 0), nonzero[r]]).all(), (name, r)


@pytest.mark.parametrize("l", PC.LS)
@pytest.mark.parametrize("curve,group", PM.COFACTOR_GROUPS)
def test_plain_path_on_points_outside_the_subgroup(hp, curve, group, l):
    """The plain path is correct for ANY point of the curve: BLS12-377 and BLS12-381 G1 cofactor points (those of order
    two and three among them), and the G2 cofactors, BN254's included."""
    chunk = PC.outside_chunk(curve, group, l)
    pts = np.stack([PM.pack_point(curve, group, P) for P in chunk])
    out, _, _ = _pack(hp, curve, group, 0, l, pts)
    want = PC.oracle_shares_any(curve, group, l, chunk)
    assert np.array_equal(out[:, 0], want)
    # the recorded sums the GPU test reads are these
    assert np.array_equal(PC.outside_expected(curve, group, l), want)


@pytest.mark.parametrize("l", PC.LS)
@pytest.mark.parametrize("curve,group,split", PC.PATHS)
def test_count_is_below_one_product_per_matrix_entry(hp, curve, group, split, l):
    """Per chunk (l tables, n combines), doublings + additions stay below the sum over the n l matrix entries of ONE
    pscale::product under pscale::make_schedule for that entry.  Doublings per output, the table's share (l / n)
    included, stay within 256 / 128 / 68 on the plain / DIM 2 / DIM 4 paths, independent of l."""
    w, table, _ = _params(hp)
    n = 4 * l
    dim, digits, lens = _schedule(hp, curve, group, split, l)
    per_chunk = l * table + sum(max(v - 1, 0) for v in lens) + int(np.count_nonzero(digits))
    g = PM.gid(curve, group)
    point = PC.host_chunks(curve, group, 1)[0][1][0]
    old = 0
    cnt = np.zeros(2, dtype=np.uint32)
    for row in PC.pack_matrix(curve, l):
        for k in row:
            kw = np.frombuffer(int(k).to_bytes(32, "little"), dtype=np.uint32).copy()
            assert hp.hp_one_product(g, split, _p(point), _p(kw), _p(cnt)) == 0
            old += int(cnt.sum())
    print("%s G%d parts=%d l=%d: %d operations per chunk, %d by n l one-scalar products (%.2f)"
          % (curve, group, dim, l, per_chunk, old, per_chunk / old))
    assert per_chunk < old
    for r in range(n):
        assert max(lens[r] - 1, 0) + l / n <= DBL_BOUND[dim], (r, lens[r])
