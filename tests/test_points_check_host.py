"""The decision function of distributed-groth16_amd/csrc/points_check.h -- reduced coordinates, curve equation, r P by the
fixed chain on the 29-bit-limb arithmetic -- compiled with the host compiler into a stand-alone program
(tests/host_arith/host_points_check.cpp, address and undefined-behaviour sanitizers on): the CPU runs the text the kernel
runs.  Expected verdicts are plain-Python decisions (tests/points_check_cases.py: oracle.pyref.curves for the group law,
big integers for the rest)."""

import os
import random
import struct
import subprocess

import numpy as np
import pytest

import points_check_cases as PC
import points_mul_cases as PM
from oracle.pyref.curves import CURVES
from oracle.pyref.fields import FR

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_arith", "host_points_check.cpp")
EXE = os.path.join(HERE, "host_arith", "host_points_check")
CSRC = os.path.join(HERE, "..", "distributed-groth16_amd", "csrc")


@pytest.fixture(scope="module")
def exe():
    hdrs = [os.path.join(CSRC, f) for f in ("points_check.h", "ec29.h", "fp29.h", "fp29_asm_gen.h", "fp.h", "fp2.h", "ec.h",
                                            "types.h", "consts_gen.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(EXE) < os.path.getmtime(p) for p in [SRC] + hdrs):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-o", EXE, SRC])
    return EXE


def run_cases(exe, tmp_path, batches):
    """batches: (curve, group, subgroup, points uint64[n][limbs]) -> [int32[n][3]: verdict, doublings, additions]"""
    blob = [struct.pack("<I", len(batches))]
    for curve, group, subgroup, pts in batches:
        blob.append(struct.pack("<IIQ", PM.gid(curve, group), int(subgroup), len(pts)))
        blob.append(np.ascontiguousarray(pts, dtype=np.uint64).tobytes())
    fin, fout = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    with open(fin, "wb") as f:
        f.write(b"".join(blob))
    res = subprocess.run([exe, "run", fin, fout], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout + res.stderr
    raw = np.frombuffer(open(fout, "rb").read(), dtype=np.int32).reshape(-1, 3)
    out, pos = [], 0
    for _, _, _, pts in batches:
        out.append(raw[pos:pos + len(pts)])
        pos += len(pts)
    assert pos == len(raw)
    return out


def chain(exe):
    res = subprocess.run([exe, "chain"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
    return {int(g): (int(d), int(a)) for _, g, d, a in (ln.split() for ln in res.stdout.splitlines())}


def _naf(k):
    """(index of the top digit, non-zero digits below it) of the non-adjacent form, in plain Python"""
    digits = []
    while k:
        d = 0
        if k & 1:
            d = 2 - (k & 3)
            k -= d
        digits.append(d)
        k >>= 1
    return len(digits) - 1, sum(1 for d in digits[:-1] if d)


def test_the_chain_is_the_non_adjacent_form_of_r(exe):
    got = chain(exe)
    for curve, group in PC.GROUPS:
        assert got[PM.gid(curve, group)] == _naf(FR[curve].p), (curve, group)


@pytest.mark.parametrize("curve,group", PC.GROUPS)
def test_case_list(exe, tmp_path, curve, group):
    """Every special point under subgroup = 0 and 1 gets the verdict of the plain-Python decision, and the chain runs
    -- with its whole fixed budget -- exactly for the reduced points of the curve of a group with a cofactor."""
    cs = PC.cases(curve, group)
    pts = np.stack([w for _, w, _, _ in cs])
    doublings, additions = chain(exe)[PM.gid(curve, group)]
    r0, r1 = run_cases(exe, tmp_path, [(curve, group, 0, pts), (curve, group, 1, pts)])
    for i, (name, _, v0, v1) in enumerate(cs):
        assert r0[i, 0] == v0 and r1[i, 0] == v1, name
        assert tuple(r0[i, 1:]) == (0, 0), name
        ran = name != "identity" and v0 == PC.GOOD and (curve, group) != ("bn254", 1)
        assert tuple(r1[i, 1:]) == ((doublings, additions) if ran else (0, 0)), name


@pytest.mark.parametrize("curve,group", PC.GROUPS)
def test_random_subgroup_points(exe, tmp_path, curve, group):
    """300 random multiples of the generator per group are good; the decision in plain Python says so too."""
    c = CURVES[curve, "g%d" % group]
    r = FR[curve].p
    rng = random.Random(200 + PM.gid(curve, group))
    pts = np.stack([PM.pack_point(curve, group, c.mul(c.gen, rng.randrange(1, r))) for _ in range(300)])
    for w in pts:
        assert PC.decide(curve, group, w, True) == PC.GOOD
    (res,) = run_cases(exe, tmp_path, [(curve, group, 1, pts)])
    assert not res[:, 0].any()


@pytest.mark.parametrize("curve,group", PM.COFACTOR_GROUPS)
def test_multiples_of_a_point_outside_the_subgroup(exe, tmp_path, curve, group):
    """j Q for a curve point Q outside the subgroup: bad exactly where plain Python says r (j Q) != O (h Q for the
    cofactor h would be good; small j are not)."""
    c = CURVES[curve, "g%d" % group]
    Q = PM.outside_point(curve, group)
    pts = np.stack([PM.pack_point(curve, group, c.mul(Q, j)) for j in (1, 2, 3, 5, 7)])
    exp = [PC.decide(curve, group, w, True) for w in pts]
    (res,) = run_cases(exe, tmp_path, [(curve, group, 1, pts)])
    assert list(res[:, 0]) == exp and PC.OFF_SUBGROUP in exp
