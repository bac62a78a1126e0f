"""The stage schedule and the butterfly of distributed-groth16_amd/csrc/group_ntt.h, compiled with the host compiler into
a stand-alone program (tests/host_arith/host_group_ntt.cpp, address and undefined-behaviour sanitizers on) and compared
with the oracle: the CPU runs the text the kernels run, on field elements and on points, and counts its multiplications."""

import os
import random
import struct
import subprocess

import numpy as np
import pytest

from oracle import corc
from oracle.pyref.fields import FR

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_arith", "host_group_ntt.cpp")
EXE = os.path.join(HERE, "host_arith", "host_group_ntt")
CSRC = os.path.join(HERE, "..", "distributed-groth16_amd", "csrc")
CURVES = ("bn254", "bls12_381", "bls12_377")
SLICE_DEFAULT = 1 << 16


def budget(log_n, inverse=False):
    """(n / 2) k - (n - 1) products for a forward transform of n = 2^k, n more for the inverse's n^-1"""
    n = 1 << log_n
    return (n // 2) * log_n - (n - 1) + (n if inverse and log_n else 0)


@pytest.fixture(scope="module")
def exe():
    hdrs = [os.path.join(CSRC, f) for f in ("group_ntt.h", "points_mul.h", "glv_endo.h", "glv.h", "fp.h", "fp2.h", "ec.h",
                                            "types.h", "consts_gen.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(EXE) < os.path.getmtime(p) for p in [SRC] + hdrs):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-o", EXE, SRC])
    return EXE


def run_cases(exe, tmp_path, cases):
    """cases: (kind, id, log_n, inverse, slice, root uint64[1][4], elements uint64[n][limbs]) -> [(results, counts)]"""
    blob = [struct.pack("<I", len(cases))]
    for kind, ident, log_n, inverse, slc, root, data in cases:
        assert data.shape[0] == 1 << log_n
        blob.append(struct.pack("<IIIIQ", kind, ident, log_n, int(inverse), slc))
        blob.append(np.ascontiguousarray(root, dtype=np.uint64).tobytes())
        blob.append(np.ascontiguousarray(data, dtype=np.uint64).tobytes())
    fin, fout = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    with open(fin, "wb") as f:
        f.write(b"".join(blob))
    res = subprocess.run([exe, "run", fin, fout], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    raw = open(fout, "rb").read()
    out, pos = [], 0
    for _, _, log_n, _, _, _, data in cases:
        nb = data.size * 8
        vals = np.frombuffer(raw[pos:pos + nb], dtype=np.uint64).reshape(data.shape)
        counts = struct.unpack("<4Q", raw[pos + nb:pos + nb + 32])
        out.append((vals, counts))
        pos += nb + 32
    assert pos == len(raw)
    return out


def test_lane_maps_and_slices(exe):
    """Every lane index of every stage maps to a distinct in-range pair, every position is read once and written once,
    the multiplying launches hold no twiddle 1 and the add/sub launches nothing else -- for slices of 64, 192 and the
    default, up to sizes the slices cut; and the multiplying lanes add up to the budget."""
    res = subprocess.run([exe, "plan"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    rows = [tuple(int(v) for v in ln.split()[1:]) for ln in res.stdout.splitlines() if ln.startswith("plan ")]
    assert {r[0] for r in rows} == {64, 192, 0}
    for slc, log_n, products, launches in rows:
        assert products == budget(log_n), (slc, log_n)
        lanes = slc or SLICE_DEFAULT
        half = (1 << log_n) // 2
        want = 0
        for s in range(1, log_n + 1):
            triv = 1 << (log_n - s)
            want += -(-triv // lanes) + -(-(half - triv) // lanes)
        assert launches == want, (slc, log_n)
    assert max(r[1] for r in rows if r[0] == 0) >= 18 and max(r[1] for r in rows if r[0] == 64) >= 10


@pytest.mark.parametrize("curve", CURVES)
def test_field_elements_equal_the_oracle_ntt(exe, tmp_path, curve):
    """The schedule on the additive group of Fr is dg16_ntt's transform: log_n = 0 .. 10, both directions, three slice
    settings; the counted products equal the budget and two additions go with every butterfly."""
    cid = corc.CURVES[curve]
    cases, exp = [], []
    for log_n in range(11):
        data = corc.rand_field(curve, "fr", 40 + log_n, 1 << log_n)
        root = corc.root_of_unity(curve, log_n)
        for inverse in (False, True):
            for slc in (0, 64, 192):
                cases.append((0, cid, log_n, inverse, slc, root, data))
                exp.append(corc.ntt(curve, data, inverse=inverse))
    for (kind, _, log_n, inverse, slc, _, _), want, (got, counts) in zip(cases, exp, run_cases(exe, tmp_path, cases)):
        assert np.array_equal(got, want), (log_n, inverse, slc)
        assert counts == (budget(log_n, inverse), (1 << log_n) * log_n, 0, 0), (log_n, inverse, slc, counts)


def _scalars_mont(curve, ks):
    return corc.field_op(curve, "fr", "to_mont", corc.ints_to_arr(ks, 4))


def _multiples(curve, group, ks):
    g = corc.generator(curve, group)
    return np.concatenate([corc.point_mul(curve, group, g, k) for k in ks])


@pytest.mark.parametrize("curve,group", [("bn254", 1), ("bls12_381", 2)])
def test_points_equal_the_oracle(exe, tmp_path, curve, group):
    """Points s_j G through the butterfly with points_mul.h's split products: the result is ntt(s)_i G, log_n = 0 .. 5,
    both directions; the table builds (one per product) equal the budget."""
    r = FR[curve].p
    gid = 2 * corc.CURVES[curve] + group - 1
    rng = random.Random(7 + gid)
    cases, exp = [], []
    for log_n in range(6):
        n = 1 << log_n
        ks = [rng.randrange(r) for _ in range(n)]
        if n >= 4:
            ks[1], ks[2] = 0, ks[0]                      # an identity and a repeated point among the inputs
        pts = _multiples(curve, group, ks)
        root = corc.root_of_unity(curve, log_n)
        for inverse in (False, True):
            cases.append((1, gid, log_n, inverse, 64 if log_n == 5 else 0, root, pts))
            t = corc.arr_to_ints(corc.field_op(curve, "fr", "from_mont",
                                               corc.ntt(curve, _scalars_mont(curve, ks), inverse=inverse)))
            exp.append(_multiples(curve, group, t))
    for (_, _, log_n, inverse, _, _, _), want, (got, counts) in zip(cases, exp, run_cases(exe, tmp_path, cases)):
        assert np.array_equal(got, want), (log_n, inverse)
        assert counts == (budget(log_n, inverse), (1 << log_n) * log_n, 0, 0), (log_n, inverse, counts)


@pytest.mark.parametrize("curve,group", [("bn254", 1), ("bls12_381", 2)])
def test_equal_inputs_put_doublings_and_cancellations_into_every_stage(exe, tmp_path, curve, group):
    """All inputs equal: every butterfly of every stage adds a point to itself or to its negative, or meets identities.
    Forward: n P, then identities; inverse: P, then identities."""
    gid = 2 * corc.CURVES[curve] + group - 1
    log_n, n = 4, 16
    p = corc.gen_points(curve, group, 5, 1)
    pts = np.ascontiguousarray(np.tile(p, (n, 1)))
    root = corc.root_of_unity(curve, log_n)
    (fwd, _), (inv, _) = run_cases(exe, tmp_path, [(1, gid, log_n, False, 0, root, pts), (1, gid, log_n, True, 0, root, pts)])
    assert np.array_equal(fwd[0], corc.point_mul(curve, group, p, n)[0]) and not fwd[1:].any()
    assert np.array_equal(inv[0], p[0]) and not inv[1:].any()
