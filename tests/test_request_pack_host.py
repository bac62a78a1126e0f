"""The SHA-256 block, the 512-bit reduction, the seed expansion, the index plan and the pack-matrix entries of
distributed-groth16_amd/csrc/pss_scalars.h, compiled with the host compiler (tests/host_arith/host_request_pack.cpp) and
compared with hashlib, Python's % and the oracle: the CPU runs the text the kernels run, except the field product under
reduce512, which has a host body of its own in fp.h (the device's runs in tests/test_gpu_request_pack.py)."""

import ctypes
import hashlib
import itertools
import os
import random
import subprocess

import numpy as np
import pytest

import request_pack_cases as RC
from oracle.pyref import dist as OD
from oracle.pyref.fields import FR

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_arith", "host_request_pack.cpp")
SO = os.path.join(HERE, "host_arith", "libhost_request_pack.so")
CSRC = os.path.join(HERE, "..", "distributed-groth16_amd", "csrc")
CURVES = RC.CURVES


@pytest.fixture(scope="module")
def hrp():
    hdrs = [os.path.join(CSRC, f) for f in ("pss_scalars.h", "slices.h", "fp.h", "types.h", "consts_gen.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(SO) < os.path.getmtime(p) for p in [SRC] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-o", SO, SRC])
    L = ctypes.CDLL(SO)
    vp, sz, i, u, u32, u64 = (ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint, ctypes.c_uint32,
                              ctypes.c_uint64)
    L.hrp_block.argtypes = [ctypes.c_char_p, u64, u64, u32, vp, vp]
    L.hrp_reduce512.argtypes = [i, vp, vp, vp]
    L.hrp_expand.argtypes = [i, ctypes.c_char_p, u64, u64, sz, i, vp]
    L.hrp_chunks.argtypes = [i, sz, u]
    L.hrp_chunks.restype = sz
    L.hrp_dfft_size_ok.argtypes = [sz, u]
    L.hrp_source_index.argtypes = [i, u, sz, sz, u]
    L.hrp_source_index.restype = sz
    L.hrp_slice_chunks.argtypes = [sz, u]
    L.hrp_slice_chunks.restype = sz
    L.hrp_matrix.argtypes = [i, u, vp]
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _words(k):
    return np.frombuffer(int(k).to_bytes(32, "little"), dtype=np.uint32).copy()


SEEDS = (bytes(32), bytes(range(32)), b"\xff" * 32, hashlib.sha256(b"request pack").digest())
STREAMS = (0, 1, 4, 2**32, 2**64 - 1)
INDICES = (0, 1, 255, 256, 2**16, 2**32 - 1, 2**32, 2**32 + 5, 2**48 + 2**40 + 7, 2**63, 2**64 - 1)


# ---- SHA-256 ----------------------------------------------------------------------------------------------------------------
def test_the_block_is_the_padded_message_and_its_compression_is_sha256(hrp):
    """Every byte position of the index and of the stream is exercised; j = 0 and 1 are the two the expansion uses, 255
    shows that j is one whole byte."""
    block = np.zeros(64, dtype=np.uint8)
    digest = np.zeros(32, dtype=np.uint8)
    for seed, stream, index, j in itertools.product(SEEDS, STREAMS, INDICES, (0, 1, 255)):
        msg = RC.message(seed, stream, index, j)
        assert len(msg) == 55
        hrp.hrp_block(seed, stream, index, j, _p(block), _p(digest))
        assert block.tobytes() == msg + b"\x80" + (55 * 8).to_bytes(8, "big"), (stream, index, j)
        assert digest.tobytes() == hashlib.sha256(msg).digest(), (stream, index, j)


# ---- the reduction ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", list(CURVES))
def test_reduce512_equals_pythons_mod_on_the_edge_words(hrp, curve):
    r = FR[curve].p
    rng = random.Random(0x512 + CURVES[curve])
    top = (1 << 256) - 1
    edges = [0, 1, r - 1, r, r + 1, 2 * r - 1, 2 * r, top // r * r - 1, top // r * r, top - 1, top, 1 << 255, (1 << 255) - 1]
    edges += [rng.randrange(1 << 256) for _ in range(6)]
    out = np.zeros(8, dtype=np.uint32)
    for lo, hi in itertools.product(edges, edges):
        hrp.hrp_reduce512(CURVES[curve], _p(_words(lo)), _p(_words(hi)), _p(out))
        assert int.from_bytes(out.tobytes(), "little") == (lo + (hi << 256)) % r, (hex(lo), hex(hi))


# ---- the expansion --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", list(CURVES))
def test_the_expansion_equals_the_python_model(hrp, curve):
    n = 9
    for seed, stream, first, mont in itertools.product(SEEDS[1:3], (0, 3, 2**64 - 1), (0, 2**32 - 4, 2**63 - 4), (0, 1)):
        out = np.zeros((n, 4), dtype=np.uint64)
        hrp.hrp_expand(CURVES[curve], seed, stream, first, n, mont, _p(out))
        assert RC.to_ints(out, curve, bool(mont)) == RC.model_expand(curve, seed, stream, first, n)
        if mont:
            assert all(v < FR[curve].p for v in RC.to_ints(out))         # the Montgomery form is reduced too


def test_streams_and_indices_are_separate(hrp):
    """A window of a stream is the stream (element i does not depend on `first`), and two streams of one seed, or one
    stream of two seeds, share no element."""
    def expand(seed, stream, first, n):
        out = np.zeros((n, 4), dtype=np.uint64)
        hrp.hrp_expand(0, seed, stream, first, n, 0, _p(out))
        return RC.to_ints(out)

    seed = SEEDS[1]
    a = expand(seed, 0, 0, 4)
    assert a == RC.model_expand("bn254", seed, 0, 0, 4)
    assert a[1:] == expand(seed, 0, 1, 3)
    assert len(set(a + expand(seed, 1, 0, 4) + expand(SEEDS[3], 0, 0, 4))) == 12


# ---- the index plan --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l", RC.LS)
def test_the_dfft_layout_is_share_for_dffts_index_map(hrp, l):
    """Every (e, c) of every m = l .. 2^10: the source index equals the one oracle.pyref.dist.share_for_dfft reads (its
    bit reversal applied to the identity, then the stride-m/l tuples), the map is a bijection, and the l sources of a
    chunk are one contiguous run."""
    m = l
    while m <= 1 << 10:
        assert hrp.hrp_dfft_size_ok(m, l) == 1
        chunks = hrp.hrp_chunks(RC.DFFT, m, l)
        assert chunks == m // l
        want = RC.chunk_sources(RC.DFFT, l, list(range(m)))
        assert len(want) == chunks
        seen = []
        for e in range(chunks):
            got = [hrp.hrp_source_index(RC.DFFT, l, m, e, c) for c in range(l)]
            assert got == want[e], (m, e)
            assert min(got) % l == 0 and sorted(got) == list(range(min(got), min(got) + l))
            seen += got
        assert sorted(seen) == list(range(m))
        m *= 2
    # the model itself against the oracle's packing of real values, once
    vals = list(range(100, 100 + 8 * l))
    x = OD.fft_in_place_rearrange(vals)
    assert [[vals[i] for i in row] for row in RC.chunk_sources(RC.DFFT, l, vals)] == [x[i::8] for i in range(8)]


@pytest.mark.parametrize("l", RC.LS)
def test_dfft_sizes_that_are_refused(hrp, l):
    for m in (0, 3, 5, 6, 12, 1000, l // 2, (1 << 20) + 1):
        if m and m >= l and m & (m - 1) == 0:
            continue
        assert hrp.hrp_dfft_size_ok(m, l) == 0, m


@pytest.mark.parametrize("l", RC.LS)
def test_the_chunks_layout_cuts_and_pads(hrp, l):
    for n in (1, l - 1, l, l + 1, 2 * l - 1, 2 * l + 1, 7 * l + (l + 1) // 2, 1000, 1023):
        if n <= 0:
            continue
        chunks = hrp.hrp_chunks(RC.CHUNKS, n, l)
        want = RC.chunk_sources(RC.CHUNKS, l, list(range(n)))
        assert chunks == len(want) == -(-n // l)
        seen = []
        for e in range(chunks):
            got = [hrp.hrp_source_index(RC.CHUNKS, l, n, e, c) for c in range(l)]
            assert [g if g < n else None for g in got] == want[e], (n, e)
            seen += [g for g in got if g < n]
            # padding only at the end of the last chunk
            assert all(g < n for g in got) or e == chunks - 1
        assert seen == list(range(n))
        assert chunks * l - n < l


def test_slices_are_whole_waves(hrp):
    for outputs, n in itertools.product((0, 1, 63, 64, 4096, 2**16, 2**21, 2**21 + 17), (4, 8, 16, 32)):
        c = hrp.hrp_slice_chunks(outputs, n)
        assert c >= 64 and c % 64 == 0
        assert c == 64 or c * n <= outputs


# ---- the matrix --------------------------------------------------------------------------------------------------------------------
_MATRIX = {}


def _matrix(hrp, curve, l):
    if (curve, l) not in _MATRIX:
        out = np.zeros((4 * l, 2 * l, 8), dtype=np.uint32)
        hrp.hrp_matrix(CURVES[curve], l, _p(out))
        _MATRIX[(curve, l)] = [[int.from_bytes(out[j, i].tobytes(), "little") for i in range(2 * l)] for j in range(4 * l)]
    return _MATRIX[(curve, l)]


@pytest.mark.parametrize("l", RC.LS)
@pytest.mark.parametrize("curve", list(CURVES))
def test_shares_from_the_matrix_equal_the_oracles_blinded_packing(hrp, curve, l):
    """Exactly: random secrets and blinds, the unit vectors (which read every column off alone) and zero blinds (which
    is pack_from_public)."""
    r = FR[curve].p
    P = _matrix(hrp, curve, l)
    assert all(0 <= v < r for row in P for v in row)
    rng = random.Random(0xb11d + 8 * CURVES[curve] + l)
    pp = RC.opp(curve, l)
    cases = [[rng.randrange(r) for _ in range(2 * l)] for _ in range(3)]
    cases += [[1 if i == k else 0 for i in range(2 * l)] for k in range(2 * l)]
    cases += [[rng.randrange(r) for _ in range(l)] + [0] * l, [r - 1] * (2 * l)]
    for x in cases:
        got = [sum(P[j][i] * x[i] for i in range(2 * l)) % r for j in range(4 * l)]
        assert got == RC.oracle_pack_rand(curve, l, x[:l], x[l:])
        if not any(x[l:]):
            assert got == pp.pack_from_public(x[:l])
        assert pp.unpack(got) == x[:l]                       # the blind slots are truncated by unpack


def _rank(rows, p):
    rows = [list(r) for r in rows]
    rank = 0
    for col in range(len(rows[0])):
        piv = next((i for i in range(rank, len(rows)) if rows[i][col]), None)
        if piv is None:
            continue
        rows[rank], rows[piv] = rows[piv], rows[rank]
        inv = pow(rows[rank][col], -1, p)
        rows[rank] = [v * inv % p for v in rows[rank]]
        for i in range(len(rows)):
            if i != rank and rows[i][col]:
                f = rows[i][col]
                rows[i] = [(a - f * b) % p for a, b in zip(rows[i], rows[rank])]
        rank += 1
    return rank


@pytest.mark.parametrize("l", RC.LS)
@pytest.mark.parametrize("curve", list(CURVES))
def test_hiding_any_t_parties_blind_block_has_rank_t(hrp, curve, l):
    """For any t = l - 1 parties the t x (t + 1) block of blind columns has full row rank: whatever the secrets, the
    blinds reach every vector of those parties' shares, so a matching blind vector exists for any other secrets.  All
    subsets for l <= 4, a fixed sample of 200 for l = 8."""
    r = FR[curve].p
    P = _matrix(hrp, curve, l)
    t, n = l - 1, 4 * l
    if l <= 4:
        subsets = list(itertools.combinations(range(n), t))
    else:
        rng = random.Random(0x41de)
        subsets = [tuple(sorted(rng.sample(range(n), t))) for _ in range(200)]
    assert subsets
    for sub in subsets:
        block = [P[j][l:] for j in sub]
        if t:
            assert _rank(block, r) == t, sub
    if t:
        # and t + 1 parties do learn something: no hiding beyond the threshold is claimed
        assert _rank([P[j][l:] for j in range(t + 1)], r) == t + 1
