"""The term function, the chunk loop and the slice plan of distributed-groth16_amd/csrc/points_series.h and the decision
function of dg16_srs_verify_contribution (points_check.h), compiled with the host compiler
(tests/host_arith/host_points_series.cpp) and compared with Python's pow(): the CPU runs the text the kernel runs."""

import ctypes
import itertools
import os
import random
import subprocess

import numpy as np
import pytest

from oracle.pyref.fields import FR

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_arith", "host_points_series.cpp")
SO = os.path.join(HERE, "host_arith", "libhost_points_series.so")
CSRC = os.path.join(HERE, "..", "distributed-groth16_amd", "csrc")
CURVES = {"bn254": 0, "bls12_381": 1, "bls12_377": 2}

STARTS = (0, 1, 2**32 - 1, 2**32 + 5, 2**63)
SLICE = 64


@pytest.fixture(scope="module")
def hps():
    hdrs = [os.path.join(CSRC, f) for f in ("points_series.h", "points_check.h", "points_scale.h", "points_mul.h",
                                            "fp.h", "types.h", "consts_gen.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(SO) < os.path.getmtime(p) for p in [SRC] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-o", SO, SRC])
    L = ctypes.CDLL(SO)
    vp, sz, i, u32, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64
    L.hps_chunk.restype = ctypes.c_uint
    L.hps_plan.argtypes = [sz, sz, u64, vp, sz, vp, sz]
    L.hps_plan.restype = sz
    L.hps_series.argtypes = [i, vp, vp, u64, sz, sz, vp]
    L.hps_term.argtypes = [i, vp, vp, u64, vp]
    L.hps_decide.argtypes = [u32, i, i, i, vp]
    L.hps_decide.restype = u32
    L.hps_skipped.argtypes = [u32, i, i]
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _words(k):
    return np.frombuffer(int(k).to_bytes(32, "little"), dtype=np.uint32).copy()


def _ints(a):
    return [int.from_bytes(row.tobytes(), "little") for row in a]


def _series(hps, curve, first, ratio, start, n, slice_):
    out = np.zeros((n, 8), dtype=np.uint32)
    assert hps.hps_series(CURVES[curve], _p(_words(first)), _p(_words(ratio)), start, n, slice_, _p(out)) == 0
    return _ints(out)


def _firsts_and_ratios(curve):
    r = FR[curve].p
    rng = random.Random(0x5e71e5 + CURVES[curve])
    return (0, 1, rng.randrange(2, r)), (0, 1, r - 1, rng.randrange(2, r))


def test_the_chunk_is_shorter_than_a_slice(hps):
    chunk = hps.hps_chunk()
    assert 2 <= chunk < SLICE and SLICE % chunk == 0


@pytest.mark.parametrize("curve", list(CURVES))
def test_terms_equal_pythons_pow(hps, curve):
    """first * ratio^(start + i) for every i of a call over 130 elements in slices of 64: i = 0, 1, the chunk length and
    its neighbours and the slice boundaries 64 and 128 and their neighbours are all among them.  start runs over 0, 1
    and the exponents around 2^32 and at 2^63; ratio over 0, 1, r - 1 and a random one; first over 0, 1 and a random
    one."""
    r = FR[curve].p
    chunk = hps.hps_chunk()
    n = 130
    must = {0, 1, chunk - 1, chunk, chunk + 1, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE - 1, 2 * SLICE, 2 * SLICE + 1}
    assert must <= set(range(n))
    firsts, ratios = _firsts_and_ratios(curve)
    for first, ratio, start in itertools.product(firsts, ratios, STARTS):
        got = _series(hps, curve, first, ratio, start, n, SLICE)
        base = first * pow(ratio, start, r) % r
        want = []
        for i in range(n):
            want.append(base)
            base = base * ratio % r
        if ratio == 0 and start == 0:
            assert want[0] == first and not any(want[1:])          # 0^0 = 1
        assert want[SLICE] == first * pow(ratio, start + SLICE, r) % r
        assert got == want, (curve, first, ratio, start, [i for i in range(n) if got[i] != want[i]][:4])


@pytest.mark.parametrize("curve", list(CURVES))
def test_the_term_function_alone(hps, curve):
    """term(first, ratio, e) at single exponents, the full 64-bit range included."""
    r = FR[curve].p
    firsts, ratios = _firsts_and_ratios(curve)
    out = np.zeros(8, dtype=np.uint32)
    for first, ratio in itertools.product(firsts, ratios):
        for e in (0, 1, 2, 15, 16, 17, 2**32 - 1, 2**32, 2**32 + 5, 2**63, 2**64 - 1):
            hps.hps_term(CURVES[curve], _p(_words(first)), _p(_words(ratio)), e, _p(out))
            assert _ints([out])[0] == first * pow(ratio, e, r) % r, (first, ratio, e)


def test_values_from_r_on_are_refused(hps):
    out = np.zeros((1, 8), dtype=np.uint32)
    for curve, c in CURVES.items():
        r = FR[curve].p
        for bad in (r, r + 1, (1 << 256) - 1):
            assert hps.hps_series(c, _p(_words(bad)), _p(_words(1)), 0, 1, SLICE, _p(out)) == -1
            assert hps.hps_series(c, _p(_words(1)), _p(_words(bad)), 0, 1, SLICE, _p(out)) == -1
        assert hps.hps_series(c, _p(_words(r - 1)), _p(_words(r - 1)), 0, 1, SLICE, _p(out)) == 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("start", [0, 2**32 - 1, 2**63])
def test_the_plan_covers_every_element_once(hps, n, start):
    """Slices and chunks tile [0, n): no gap, no overlap, no element past n; the exponent of a slice is start + lo."""
    chunk = hps.hps_chunk()
    slices = np.zeros((8, 4), dtype=np.uint64)
    chunks = np.zeros((64, 2), dtype=np.uint64)
    ns = hps.hps_plan(n, SLICE, start, _p(slices), 8, _p(chunks), 64)
    assert ns == -(-n // SLICE)
    seen = np.zeros(n, dtype=np.int64)
    n_chunks = 0
    for lo, cnt, exp0, nch in ([int(v) for v in row] for row in slices[:ns]):
        assert 1 <= cnt <= SLICE and lo % SLICE == 0 and lo + cnt <= n
        assert exp0 == start + lo
        assert nch == -(-cnt // chunk)
        for b, ln in ([int(v) for v in row] for row in chunks[n_chunks:n_chunks + nch]):
            assert lo <= b and b + ln <= lo + cnt and 1 <= ln <= chunk and (b - lo) % chunk == 0
            seen[b:b + ln] += 1
        n_chunks += nch
    assert (seen == 1).all()


def test_the_slice_is_rounded_up_to_a_wave(hps):
    slices = np.zeros((8, 4), dtype=np.uint64)
    chunks = np.zeros((64, 2), dtype=np.uint64)
    assert hps.hps_plan(130, 33, 0, _p(slices), 8, _p(chunks), 64) == 3
    assert [int(v) for v in slices[:3, 0]] == [0, 64, 128]


# ---- the decision function of dg16_srs_verify_contribution ---------------------------------------------------------------
AFTER, BAD_POINT, IDENTITY, BASE = 1, 2, 4, 8
RELATIONS = (16, 32, 64, 128, 256, 512, 1024, 2048)
SRS_BAD_POINT, SRS_IDENTITY, SRS_TAU_G1 = 1, 2, 4


def _decide(hps, after=0, bad_point=0, identity=0, base=0, relations=()):
    flags = np.array([1 if j in relations else 0 for j in range(8)], dtype=np.uint8)
    return hps.hps_decide(after, bad_point, identity, base, _p(flags))


def test_every_failing_check_sets_exactly_its_bit(hps):
    assert _decide(hps) == 0
    assert _decide(hps, after=SRS_TAU_G1) == AFTER
    assert _decide(hps, bad_point=1) == BAD_POINT
    assert _decide(hps, identity=1) == IDENTITY
    assert _decide(hps, base=1) == BASE
    for j, bit in enumerate(RELATIONS):
        assert _decide(hps, relations=(j,)) == bit
    assert _decide(hps, relations=range(8)) == sum(RELATIONS)
    assert _decide(hps, after=SRS_TAU_G1, base=1, relations=(0, 7)) == AFTER | BASE | RELATIONS[0] | RELATIONS[7]


def test_the_relations_are_skipped_without_membership(hps):
    """BAD_POINT or IDENTITY here, or in the report of `after`: no pairing bit, whatever the relations would say; any
    other failure of `after` leaves them in."""
    every = range(8)
    assert _decide(hps, bad_point=1, relations=every) == BAD_POINT
    assert _decide(hps, identity=1, relations=every) == IDENTITY
    assert _decide(hps, after=SRS_BAD_POINT, relations=every) == AFTER
    assert _decide(hps, after=SRS_IDENTITY, relations=every) == AFTER
    assert _decide(hps, after=SRS_IDENTITY | SRS_TAU_G1, base=1, relations=every) == AFTER | BASE
    assert _decide(hps, after=SRS_TAU_G1, relations=every) == AFTER | sum(RELATIONS)
    assert _decide(hps, base=1, relations=every) == BASE | sum(RELATIONS)
    for after, bad, ident in itertools.product((0, SRS_BAD_POINT, SRS_IDENTITY, SRS_TAU_G1, 64), (0, 1), (0, 1)):
        want = bool(bad or ident or after & (SRS_BAD_POINT | SRS_IDENTITY))
        assert bool(hps.hps_skipped(after, bad, ident)) == want
