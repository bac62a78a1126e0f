"""The MSM's planning arithmetic (distributed-groth16_amd/csrc/msm_geom.h) built with the host compiler and compared,
for exact equality, with its Python mirror (tests/witness_shapes.py) -- the mirror the GPU tests and MSM_INVARIANTS.md
lean on is checked against the code that ships, without a GPU.  Where the mirror has no counterpart (the sort's partition
choice, the table stride) the expected value is written out here from the rule itself."""

import ctypes
import os
import subprocess

import pytest

import witness_shapes as ws

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_geom", "host_geom.cpp")
SO = os.path.join(HERE, "host_geom", "libhost_geom.so")
HDR = os.path.join(HERE, "..", "distributed-groth16_amd", "csrc", "msm_geom.h")

NS = [1, 2, 3] + [v for k in range(4, 27)
                  for v in ((1 << k) - 5, 1 << k, (1 << k) + 1, 3 << (k - 1), (3 << (k - 1)) + 1)]
BITS = (65, 127, 253, 254, 255, 256)
PAIRS = [("bn254", 1), ("bn254", 2), ("bls12_381", 1), ("bls12_381", 2), ("bls12_377", 1), ("bls12_377", 2)]
GEOM_KEYS = ("c", "nwin", "log_nb", "seg_log", "seg_cap", "bw", "table", "rows", "region")


@pytest.fixture(scope="module")
def hg():
    for v in ("DG16_MSM_C", "DG16_MSM_TABLE_C", "DG16_MSM_SEG_LOG", "DG16_MSM_SORT"):
        os.environ.pop(v, None)          # the overrides are cached in statics: gone before the library loads
    if not os.path.exists(SO) or any(os.path.getmtime(SO) < os.path.getmtime(p) for p in (SRC, HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    L = ctypes.CDLL(SO)
    vp, sz, i, u = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint
    L.hg_window_bits.argtypes = [sz, i, u]
    L.hg_window_bits.restype = u
    L.hg_geometry.argtypes = [sz, u, i, u, u, vp]
    L.hg_row_geometry.argtypes = [u, vp]
    L.hg_giant_geometry.argtypes = [u, vp]
    L.hg_table_stride_for.argtypes = [sz, sz, u]
    L.hg_table_stride_for.restype = u
    L.hg_partition_plan.argtypes = [u, u, u, sz, vp]
    L.hg_plain_plan.argtypes = [i, u, sz, i, vp]
    L.hg_constants.argtypes = [vp]
    return L


def _geometry(hg, n, bits, table, c_fixed, stride):
    out = (ctypes.c_uint64 * 9)()
    hg.hg_geometry(n, bits, int(table), c_fixed, stride, out)
    return dict(zip(GEOM_KEYS, out))


def _mirror(n, bits, table, c_fixed, stride):
    g = ws.geometry(n, bits, table, c_fixed, stride)
    return {k: int(g[k]) for k in GEOM_KEYS}


def _partition(hg, nwin, bw, log_nb, n):
    out = (ctypes.c_uint * 4)()
    hg.hg_partition_plan(nwin, bw, log_nb, n, out)
    return {"partitioned": bool(out[0]), "low_bits": out[1], "nparts": out[2], "nblk1": out[3]}


def _partition_rule(nwin, bw, log_nb, n):
    """The choice as msm_sort_on made it inline: partitions are the slot index's bits above the low <= 12, the
    partitioned passes take sorts of >= 2^18 entries whose bins fit."""
    nbw = bw << log_nb
    lg_nbw = (nbw - 1).bit_length()
    low_bits = lg_nbw - 8 if lg_nbw > 8 else 0
    return {"partitioned": low_bits <= 12 and nwin * n >= (1 << 18), "low_bits": low_bits,
            "nparts": (nbw + (1 << low_bits) - 1) >> low_bits, "nblk1": (n + 1023) // 1024}


def test_constants(hg):
    out = (ctypes.c_uint * 10)()
    hg.hg_constants(out)
    assert list(out) == [ws.K_MIN_SEG_LOG, ws.K_MAX_SEG_LOG, ws.K_MIN_LANES_LOG, ws.K_GIANT_SEGS, ws.K_GIANT_SLICES,
                         ws.K_GIANT_SLICE_SEGS, 1024, 12, 127, 65]


def test_window_bits(hg):
    for n in NS:
        for table in (False, True):
            for bits in (0,) + BITS:
                assert hg.hg_window_bits(n, int(table), bits) == ws.window_bits(n, table, bits), (n, table, bits)


def test_geometry_and_partition_choice(hg):
    for n in NS:
        for bits in BITS:
            for table in (False, True):
                for c_fixed in (0, 8, 16):
                    nwin = ws.geometry(n, bits, table, c_fixed)["nwin"]
                    for stride in (1, 2, 3, nwin, nwin + 5):
                        case = (n, bits, table, c_fixed, stride)
                        g = _geometry(hg, *case)
                        assert g == _mirror(*case), case
                        assert _partition(hg, g["nwin"], g["bw"], g["log_nb"], n) == \
                            _partition_rule(g["nwin"], g["bw"], g["log_nb"], n), case


def test_partition_choice_at_its_thresholds(hg):
    cases = []
    for nwin in (16, 17, 9):                      # nwin * n just below and at 2^18 (and across it where nwin does not divide)
        n = (1 << 18) // nwin
        cases += [(nwin, nwin, 14, m) for m in (n - 1, n, n + 1)]
    for bw, log_nb in ((1, 8), (1, 9), (3, 7), (1, 20), (16, 16), (1, 21), (3, 19), (17, 17)):
        cases += [(17, bw, log_nb, m) for m in (1, 1 << 10, (1 << 20) + 1)]       # lg_nbw = 8, 9, 9, 20, 20, 21, 21, 22
    seen = set()
    for nwin, bw, log_nb, n in cases:
        got = _partition(hg, nwin, bw, log_nb, n)
        assert got == _partition_rule(nwin, bw, log_nb, n), (nwin, bw, log_nb, n)
        seen.add((got["partitioned"], min(got["low_bits"], 13)))
    assert {(True, 12), (False, 13), (False, 0), (True, 1)} <= seen      # both sides of kPartMaxLowBits and of 2^18


def test_row_geometry(hg):
    out = (ctypes.c_uint * 2)()
    for log_nb in range(3, 20):
        hg.hg_row_geometry(log_nb, out)
        assert (out[0], out[1]) == (min(log_nb, 8), log_nb - min(log_nb, 8))


def test_giant_geometry(hg):
    out = (ctypes.c_uint * 2)()
    for nseg in list(range(65, 71)) + list(range(511, 515)) + list(range(32767, 32771)) + [1 << 20]:
        hg.hg_giant_geometry(nseg, out)
        slices, per = ws.giant_slices(nseg)
        assert (out[0], out[1]) == (slices, per), nseg
        assert slices <= ws.K_GIANT_SLICES and slices * per >= nseg > (slices - 1) * per


def test_table_stride_for(hg):
    def smallest_stride(full, budget, nwin):
        """The smallest k whose ceil(nwin / k) rows fit the budget; one row is the floor, no budget is stride 1."""
        if not budget or full <= budget or nwin <= 1:
            return 1
        fit = max(budget // (full // nwin), 1)
        return next(k for k in range(1, nwin + 1) if (nwin + k - 1) // k <= fit)

    row = 96 * 1000
    for nwin in (16, 17, 1):
        full = row * nwin
        budgets = [0, full, full + 1, row - 1, 1] + [r * row + d for r in (1, 2, 3) for d in (-1, 0, 1)]
        for budget in budgets:
            assert hg.hg_table_stride_for(full, budget, nwin) == smallest_stride(full, budget, nwin), (nwin, budget)
    assert hg.hg_table_stride_for(row * 16, 3 * row, 16) == 6 and hg.hg_table_stride_for(row * 17, row, 17) == 17


def test_plain_plan(hg):
    out = (ctypes.c_uint * 3)()
    hows = set()
    for curve, group in PAIRS:
        dim = ws._glv_dim(curve, group)
        for in_subgroup in (True, False):
            applies = (curve, group) == ("bn254", 1) or in_subgroup
            for n in (0, 1 << 10, 1 << 12, 1 << 13, 1 << 16, 1 << 17, 1 << 18, 1 << 26):   # 2^26: DIM n 40 >= 2^31
                hg.hg_plain_plan(int(curve == "bn254"), dim, n, int(applies), out)
                split, c_small, bits = bool(out[0]), out[1], out[2]
                g, how = ws.plain_geometry(curve, group, n, in_subgroup)
                assert how == (("glv2" if dim == 2 else "glv4") if split else "full"), (curve, group, n, in_subgroup)
                if split:
                    sort = (dim * n, bits, False, c_small, 1)
                else:
                    assert (c_small, bits) == (0, 0)
                    sort = (max(n, 1), ws.SCALAR_BITS[curve], False, 0, 1)
                assert _geometry(hg, *sort) == {k: int(g[k]) for k in GEOM_KEYS}, (curve, group, n, in_subgroup)
                hows.add((how, c_small))
    assert hows == {("glv2", 0), ("glv2", 8), ("glv2", 16), ("glv4", 0), ("full", 0)}
