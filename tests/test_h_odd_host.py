"""The index rule of distributed-groth16_amd/csrc/h_odd.h -- which gathered element and which unpack row feed position i
of output chunk c in h_king_kernel -- compiled with the host compiler into a stand-alone program
(tests/host_arith/host_h_odd.cpp) and compared with the Python rule of tests/h_odd_cases.py for every
(l, m/l <= 8, c, i).  The same program is built and run once more under the address and undefined-behaviour sanitizers:
it walks buffers of the sizes dg16_ext_wit_h allocates the way the kernel does."""

import os
import subprocess

import pytest

import h_odd_cases as HC

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_arith", "host_h_odd.cpp")


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *extra, "-o", exe, SRC])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr == ""
    return r.stdout


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    out = _build_and_run(tmp_path_factory.mktemp("h_odd"), "host_h_odd", [])
    return [tuple(int(x) for x in line.split()) for line in out.splitlines()]


def test_the_program_covers_every_case(rows):
    want = [(l, chunks, c, i) for l in HC.LS for chunks in range(1, 9) for c in range(chunks) for i in range(l)]
    assert [r[:4] for r in rows] == want


def test_the_compiled_rule_is_the_python_rule(rows):
    for l, chunks, c, i, elem, row, ev in rows:
        assert (elem, row) == HC.source(l, c, i), (l, chunks, c, i)
        assert ev == 2 * (c * l + i) + 1 and ev < 2 * chunks * l


def test_the_program_is_clean_under_the_sanitizers(tmp_path, rows):
    out = _build_and_run(tmp_path, "host_h_odd_san",
                         ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert [tuple(int(x) for x in line.split()) for line in out.splitlines()] == rows
