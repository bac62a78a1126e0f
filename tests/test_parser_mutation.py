"""Mutation testing of the host parsers under AddressSanitizer and UndefinedBehaviorSanitizer, without a GPU: the
stand-alone program tests/host_mutation/mutate_parsers.cpp, built by the host compiler together with the parser
sources themselves (csrc/formats.hip: `.r1cs`, `.zkey`, the arkworks key container; csrc/serialize.hip: proof.bin),
runs 20 000 mutants of a small seed file per format (2 000 for proof.bin, whose mutants each cost field
exponentiations) plus every count / size / length field of the seed overwritten with boundary values.

Pass: exit status 0, no sanitizer report, both accepted and refused mutants for every format, and no field that governs
how many bytes the parser reads accepted with a value larger than the file.

Not covered: the Python wrappers distributed-groth16_amd/{arkkey,zkey,r1cs}.py -- nothing is loaded into Python under a
sanitizer here -- and the decoding of the points inside key files, which is GPU code (tests/test_gpu_codec_edges.py)."""

import json
import os
import re
import struct
import subprocess

import pytest

from oracle.pyref import groth16 as G
from oracle.pyref.fields import FR

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "distributed-groth16_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mutate") / "mutate_parsers")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-x", "c++", os.path.join(HERE, "host_mutation", "mutate_parsers.cpp"),
                           os.path.join(CSRC, "formats.hip"), os.path.join(CSRC, "serialize.hip"), "-o", exe])
    return exe


def write_r1cs(r1cs):
    """A circom .r1cs (iden3 binary container): header, constraints, wire-to-label map."""
    F = FR["bn254"]
    nv = r1cs["num_instance"] + r1cs["num_witness"]
    header = (struct.pack("<I", 32) + F.p.to_bytes(32, "little")
              + struct.pack("<IIIIQI", nv, 1, r1cs["num_instance"] - 2, r1cs["num_witness"], nv, r1cs["num_constraints"]))
    body = b""
    for i in range(r1cs["num_constraints"]):
        for k in "abc":
            row = r1cs[k][i]
            body += struct.pack("<I", len(row)) + b"".join(struct.pack("<I", j) + (c % F.p).to_bytes(32, "little") for c, j in row)
    wire_map = b"".join(struct.pack("<Q", j) for j in range(nv))
    out = b"r1cs" + struct.pack("<II", 1, 3)
    for sid, payload in ((2, body), (1, header), (3, wire_map)):           # circom writes the header second
        out += struct.pack("<IQ", sid, len(payload)) + payload
    return out


@pytest.fixture(scope="module")
def seeds(tmp_path_factory):
    from test_arkkey import py_key_bytes
    from test_zkey_reader import small_key
    from zkey_writer import write_zkey
    d = tmp_path_factory.mktemp("seeds")
    r1cs, _ = G.synthetic_r1cs(FR["bn254"], num_constraints=200, num_instance=3, num_witness=60, seed=4, nnz=2)
    key_r1cs, _, pk, m = small_key()
    with open(os.path.join(HERE, "golden", "proof_bin_sha256.json")) as f:
        proof = bytes.fromhex(json.load(f)["hex"])
    files = {"r1cs": write_r1cs(r1cs), "zkey": write_zkey(pk, key_r1cs, m), "arkkey": py_key_bytes(pk),
             "arkkey_vk": py_key_bytes(pk, vk_only=True), "proof": proof, "proof_validate": proof}
    paths = {}
    for name, raw in files.items():
        paths[name] = str(d / name)
        with open(paths[name], "wb") as f:
            f.write(raw)
    assert len(files["r1cs"]) < 64 << 10 and len(files["zkey"]) < 64 << 10          # small seeds: thousands of parses a second
    return paths


def test_seed_r1cs_is_what_the_reader_reads(seeds):
    """The small writer above against the library's own reader (the plain build, through the Python wrapper)."""
    import dg16_amd  # noqa: F401
    from dg16_amd.r1cs import R1CS
    r = R1CS.from_file(seeds["r1cs"])
    assert (r.n_constraints, r.n_wires) == (200, 63)
    r1cs, _ = G.synthetic_r1cs(FR["bn254"], num_constraints=200, num_instance=3, num_witness=60, seed=4, nnz=2)
    assert r.rows(0) == [[(c, j) for c, j in row] for row in r1cs["a"]]


@pytest.mark.parametrize("fmt,count,min_fields", [("r1cs", 20000, 3 * 200 + 10), ("zkey", 20000, 16), ("arkkey", 20000, 6),
                                                  ("arkkey_vk", 20000, 1), ("proof", 2000, 0), ("proof_validate", 2000, 0)])
def test_mutants(program, seeds, fmt, count, min_fields):
    run = subprocess.run([program, fmt, seeds[fmt], str(count)], capture_output=True, text=True, timeout=600)
    print(run.stdout[-2000:])
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    assert not re.search(r"Sanitizer|runtime error", run.stderr), run.stderr[-4000:]
    assert run.stderr == ""
    val = {m.group(1): int(m.group(2)) for m in re.finditer(r"^(accepted|refused|field_violations) (\d+)$", run.stdout, re.M)}
    assert val["field_violations"] == 0
    assert val["accepted"] > 0 and val["refused"] > 0, val
    m = re.search(r"^fields (\d+) field_mutants (\d+) larger_than_file (\d+)$", run.stdout, re.M)
    fields, field_mutants, large = (int(x) for x in m.groups())
    assert fields >= min_fields and val["accepted"] + val["refused"] == count + field_mutants
    if fields:
        assert large >= 2 * (fields - 4)          # 2^31 and 2^32 - 1 at least, for every field but the four unread counts
