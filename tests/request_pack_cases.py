"""Shared by tests/test_request_pack_host.py and tests/test_gpu_request_pack.py: the Python model of the seed expansion
(include/dg16.h: dg16_fr_expand), the oracle's form of a blinded packing, and the index rules of the two layouts stated
from oracle.pyref.dist, none of it taken from the code under test."""

import hashlib
import struct

import numpy as np

from oracle.pyref import dist as OD
from oracle.pyref.fields import FR
from oracle.pyref.pss import PackedSharingParams as OPP

CURVES = {"bn254": 0, "bls12_381": 1, "bls12_377": 2}
CHUNKS, DFFT = 0, 1
LS = (1, 2, 4, 8)


def message(seed, stream, index, j):
    assert len(seed) == 32
    return b"dg16fe" + seed + struct.pack("<Q", stream) + struct.pack("<Q", index) + bytes([j])


def model_element(curve, seed, stream, index):
    """int_le(SHA-256(msg(0)) || SHA-256(msg(1))) mod r."""
    d = hashlib.sha256(message(seed, stream, index, 0)).digest() + hashlib.sha256(message(seed, stream, index, 1)).digest()
    return int.from_bytes(d, "little") % FR[curve].p


def model_expand(curve, seed, stream, first, n):
    return [model_element(curve, seed, stream, first + i) for i in range(n)]


def to_words(vals, curve=None, mont=False):
    """ints -> uint64 [len][4]; mont: x R mod r with R = 2^256."""
    if mont:
        p = FR[curve].p
        vals = [v * (1 << 256) % p for v in vals]
    if not len(vals):
        return np.zeros((0, 4), dtype=np.uint64)
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def to_ints(a, curve=None, mont=False):
    out = [int.from_bytes(row.tobytes(), "little") for row in np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)]
    if mont:
        p = FR[curve].p
        rinv = pow(1 << 256, -1, p)
        out = [v * rinv % p for v in out]
    return out


_OPP = {}


def opp(curve, l):
    if (curve, l) not in _OPP:
        _OPP[(curve, l)] = OPP(FR[curve], l)
    return _OPP[(curve, l)]


def oracle_pack_rand(curve, l, secrets, blinds):
    """pack_from_public_rand (secret-sharing/src/pss.rs:72-82) with the caller's randomness: the l secrets and the
    t + 1 = l blinds fill the secret domain, interpolate there, evaluate on the share domain."""
    pp = opp(curve, l)
    assert len(secrets) == l and len(blinds) == l
    return pp.share.fft(pp.secret.ifft(list(secrets) + list(blinds)))


def chunk_sources(layout, l, values):
    """The chunks of a vector as lists of (index into values or None for padding), by the reference's rules: CHUNKS cuts
    l-chunks and pads the last (sha256.rs:97-121); DFFT is oracle.pyref.dist.share_for_dfft's map applied to the
    indices (bit-reverse, then stride m / l)."""
    n = len(values)
    if layout == CHUNKS:
        return [[(e * l + c) if e * l + c < n else None for c in range(l)] for e in range(-(-n // l))]
    x = OD.fft_in_place_rearrange(list(range(n)))
    stride = n // l
    return [x[i::stride] for i in range(stride)]


def oracle_shares(curve, l, layout, values, blinds=None):
    """[n][chunks] ints: every chunk through oracle_pack_rand (blinds None = zeros = pack_from_public)."""
    src = chunk_sources(layout, l, values)
    out = []
    for e, idx in enumerate(src):
        sec = [values[i] if i is not None else 0 for i in idx]
        bl = blinds[e] if blinds is not None else [0] * l
        out.append(oracle_pack_rand(curve, l, sec, bl))
    return [list(col) for col in zip(*out)] if out else [[] for _ in range(4 * l)]
