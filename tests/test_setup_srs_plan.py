"""The planning of dg16_groth16_setup_srs (distributed-groth16_amd/csrc/setup_srs_plan.h) built with the host compiler:
every wire's segment takes exactly one of the paths (empty, lane, wave, MSM), the term counts add up to the matrices'
non-zeros plus the instance terms, and the term slices cover the lane and wave entries exactly once, in order, within
the slice size -- for the segment lengths 0, 1, wave_from - 1 .. msm_from + 1 and 2^20.  The expected values are written
out from the rule (a length below wave_from is a lane's, below msm_from a wave's), not read back from the header."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_srs_plan", "host_srs_plan.cpp")
SO = os.path.join(HERE, "host_srs_plan", "libhost_srs_plan.so")
HDR = os.path.join(HERE, "..", "distributed-groth16_amd", "csrc", "setup_srs_plan.h")

EMPTY, LANE, WAVE, MSM = 0, 1, 2, 3


@pytest.fixture(scope="module")
def sp():
    if not os.path.exists(SO) or any(os.path.getmtime(SO) < os.path.getmtime(p) for p in (SRC, HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    L = ctypes.CDLL(SO)
    vp, sz, u = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint
    L.sp_limits.argtypes = [vp]
    L.sp_path.argtypes = [sz]
    L.sp_path.restype = u
    L.sp_segment_len.argtypes = [u, u, u, ctypes.c_int]
    L.sp_segment_len.restype = sz
    L.sp_plan.argtypes = [vp, sz, sz, vp, vp, sz, vp, vp]
    L.sp_plan.restype = sz
    return L


def limits(sp):
    out = (ctypes.c_uint * 2)()
    sp.sp_limits(out)
    return out[0], out[1]


def rule(length, wave_from, msm_from):
    return EMPTY if length == 0 else LANE if length < wave_from else WAVE if length < msm_from else MSM


def plan(sp, lens, slice_):
    lens = np.asarray(lens, dtype=np.uint64)
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    nv = len(lens)
    cap = int(lens.sum()) // slice_ + 2 * nv + 4
    summary = np.zeros(11, dtype=np.uint64)
    slices = np.zeros((cap, 6), dtype=np.uint32)
    wave, msm = np.zeros(nv, dtype=np.uint32), np.zeros(nv, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)     # noqa: E731
    n = sp.sp_plan(p(seg), nv, slice_, p(summary), p(slices), cap, p(wave), p(msm))
    assert n <= cap and n == summary[8]
    return dict(seg=seg, columns=[int(x) for x in summary[:4]], terms=[int(x) for x in summary[4:8]],
                slices=slices[:n].astype(np.int64), wave=wave[:int(summary[9])].astype(np.int64),
                msm=msm[:int(summary[10])].astype(np.int64))


def test_limits_are_ordered(sp):
    wave_from, msm_from = limits(sp)
    assert 2 <= wave_from < msm_from <= 1 << 20
    assert wave_from <= 64                  # a wave has 64 lanes: a longer lane-path chain would leave them idle


def test_every_length_takes_exactly_one_path(sp):
    wave_from, msm_from = limits(sp)
    for length in [0, 1] + list(range(wave_from - 1, msm_from + 2)) + [1 << 20]:
        assert sp.sp_path(length) == rule(length, wave_from, msm_from), length


def test_segment_length_counts_the_instance_term(sp):
    assert sp.sp_segment_len(0, 0, 0, 0) == 0 and sp.sp_segment_len(0, 0, 0, 1) == 1
    assert sp.sp_segment_len(3, 4, 5, 0) == 12 and sp.sp_segment_len(3, 4, 5, 1) == 13
    assert sp.sp_segment_len(0xFFFFFFFF, 0xFFFFFFFF, 2, 1) == 2 * 0xFFFFFFFF + 3      # no 32-bit wrap


@pytest.mark.parametrize("slice_", [1 << 17, 1000, 37])
def test_plan_partitions_columns_and_terms(sp, slice_):
    wave_from, msm_from = limits(sp)
    ni = 3
    # column counts of three matrices per wire; the first ni wires carry the instance term
    rng = np.random.default_rng(slice_)
    totals = [0, 1] + list(range(wave_from - 1, msm_from + 2)) + [1 << 20]
    if slice_ < 1000:
        totals = [0, 1, 0, 0, wave_from - 1, wave_from, wave_from + 1, msm_from - 1, msm_from, msm_from + 1, 0, 5, 1 << 20,
                  msm_from, 2, 0]
    order = rng.permutation(len(totals))
    totals = [totals[i] for i in order]
    cols = []
    for t in totals:
        a = int(rng.integers(0, t + 1))
        b = int(rng.integers(0, t - a + 1))
        cols.append((a, b, t - a - b))
    nnz = sum(sum(c) for c in cols)
    lens = [sp.sp_segment_len(a, b, c, int(k < ni)) for k, (a, b, c) in enumerate(cols)]
    assert sum(lens) == nnz + ni
    pl = plan(sp, lens, slice_)
    seg = pl["seg"].astype(np.int64)
    paths = [rule(n, wave_from, msm_from) for n in lens]
    # every column exactly one path; the term counts add up to the non-zeros plus num_inputs
    assert pl["columns"] == [paths.count(p) for p in (EMPTY, LANE, WAVE, MSM)] and sum(pl["columns"]) == len(lens)
    assert pl["terms"] == [sum(n for n, q in zip(lens, paths) if q == p) for p in (EMPTY, LANE, WAVE, MSM)]
    assert sum(pl["terms"]) == nnz + ni
    assert list(pl["wave"]) == [k for k, p in enumerate(paths) if p == WAVE]
    assert list(pl["msm"]) == [k for k, p in enumerate(paths) if p == MSM]
    # the slices: the lane and wave entries, each exactly once and in order, never an MSM wire's, at most slice_ each
    want = [(int(seg[k]), int(seg[k + 1])) for k, p in enumerate(paths) if p in (LANE, WAVE)]
    covered = 0
    pos = 0            # index into want
    for lo, hi, k0, k1, w0, w1 in pl["slices"]:
        assert 0 < hi - lo <= slice_
        assert seg[k0] <= lo < seg[k0 + 1] and seg[k1] < hi <= seg[k1 + 1] and k0 <= k1
        assert all(paths[k] != MSM for k in range(k0, k1 + 1))
        assert list(pl["wave"][w0:w1]) == [k for k in range(k0, k1 + 1) if paths[k] == WAVE]
        covered += hi - lo
        # lo continues where the previous slice ended, or at the next lane / wave wire after an MSM wire
        while want[pos][1] <= lo:
            pos += 1
        assert want[pos][0] <= lo
    assert covered == pl["terms"][LANE] + pl["terms"][WAVE]
    los, his = pl["slices"][:, 0], pl["slices"][:, 1]
    assert np.all(los[1:] >= his[:-1])                       # disjoint and ascending
    # a cut happens only at the slice size or where an MSM wire (or the end) follows
    ends = {int(seg[k]) for k, p in enumerate(paths) if p == MSM} | {int(seg[-1])}
    for lo, hi in zip(los, his):
        assert hi - lo == slice_ or int(hi) in ends


def test_plan_of_nothing(sp):
    pl = plan(sp, [0, 0, 0], 64)
    assert pl["columns"] == [3, 0, 0, 0] and len(pl["slices"]) == 0 and len(pl["wave"]) == 0 and len(pl["msm"]) == 0
