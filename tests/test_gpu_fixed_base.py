"""GPU parity of dg16_fixed_base_mul with the C oracle's big-int double-and-add (corc.point_mul), bit-exact on affine
points.  One corc.point_mul per point is the reference; where a call has more points than that can check in test time
(the oracle takes ~1 ms per point), EVERY output still goes through the oracle once -- corc.msm(outputs, random
weights) must equal point_mul(base, sum_i w_i k_i) -- and the block / chunk tails plus a random sample are compared
point by point."""

import random

import numpy as np
import pytest

from oracle import corc
from oracle.pyref.fields import FR
from gpu_util import ctx

pytestmark = pytest.mark.gpu

CURVES = ["bn254", "bls12_381", "bls12_377"]
BITS = {"bn254": 254, "bls12_381": 255, "bls12_377": 253}


def enc(vals):
    return corc.ints_to_arr(list(vals), 4)


def window_bits(n):
    from dg16_amd.lib import load
    return load().dg16_fixed_base_window_bits(n)


def check(curve, group, base, ks, got, full_below=130, sample=24, seed=0):
    """got[i] == ks[i] * base: point by point for small calls and for a sample (tails included) of large ones, and in
    one random linear combination over ALL points."""
    n = len(ks)
    assert got.shape == (n, corc.point_limbs(curve, group))
    rng = random.Random(seed)
    idx = range(n) if n <= full_below else sorted(set(list(range(3)) + list(range(n - 3, n)) +
                                                      [rng.randrange(n) for _ in range(sample)]))
    for i in idx:
        exp = corc.point_mul(curve, group, base, ks[i])
        assert np.array_equal(got[i:i + 1], exp), (curve, group, n, i, hex(ks[i]))
        if ks[i] == 0:
            assert not got[i].any()
    if n > full_below:
        r = FR[curve].p
        w = [rng.randrange(1, 2**64) for _ in range(n)]
        lhs = corc.msm(curve, group, got, enc(w))
        assert np.array_equal(lhs, corc.point_mul(curve, group, base, sum(a * b for a, b in zip(w, ks)) % r)), (curve, group, n)


def edge_scalars(curve):
    r, bits = FR[curve].p, BITS[curve]
    ks = [0, 1, 2, r - 1, r - 2, (r - 1) // 2]
    for j in range(bits):
        ks += [2**j, 2**j - 1, 2**j + 1]
    for c in range(8, 21):                      # every c-bit digit equal (to 1, to 2^(c-1), to 2^c - 1)
        for d in (1, 2**(c - 1), 2**c - 1):
            k = sum(d << (c * w) for w in range(bits // c + 1))
            ks.append(k % r)
    return [k % r for k in ks]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("group", [1, 2])
def test_uniform_scalars_all_sizes(curve, group):
    r = FR[curve].p
    g = corc.generator(curve, group)
    rng = random.Random(17 * group)
    for n in (1, 2, 63, 64, 65, 1000, 2**14):
        ks = [rng.randrange(r) for _ in range(n)]
        got = ctx().fixed_base_mul(curve, group, enc(ks))
        check(curve, group, g, ks, got, seed=n)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("group", [1, 2])
def test_edge_scalars(curve, group):
    """0, 1, 2, r-1, r-2, (r-1)/2, 2^j, 2^j +- 1, equal digits: identity / P + P / P - P inside the accumulation."""
    g = corc.generator(curve, group)
    ks = edge_scalars(curve)
    got = ctx().fixed_base_mul(curve, group, enc(ks))
    check(curve, group, g, ks, got, full_below=len(ks) + 1)
    assert not got[0].any()                                   # zero scalar -> all-zero bytes
    rep = [ks[3]] * 1000                                      # one scalar (r - 1) a thousand times
    got = ctx().fixed_base_mul(curve, group, enc(rep))
    assert np.array_equal(got, np.repeat(corc.point_mul(curve, group, g, rep[0]), 1000, axis=0))


@pytest.mark.parametrize("pad_to", [2**13, 2**16, 2**19])
def test_edge_scalars_under_wide_windows(pad_to):
    """The same edge scalars inside calls whose size selects 10-, 13- and 16-bit windows (BN254 G1: the oracle checks
    ~900 points per call one by one)."""
    curve, group = "bn254", 1
    r = FR[curve].p
    rng = random.Random(pad_to)
    ks = edge_scalars(curve)
    n_edge = len(ks)
    ks = ks + [rng.randrange(r) for _ in range(pad_to - n_edge)]
    assert window_bits(len(ks)) == {2**13: 10, 2**16: 13, 2**19: 16}[pad_to]
    got = ctx().fixed_base_mul(curve, group, enc(ks))
    g = corc.generator(curve, group)
    check(curve, group, g, ks[:n_edge], got[:n_edge], full_below=n_edge + 1)
    tail = 0 if pad_to <= 2**16 else len(ks) - 4096      # (the oracle's MSM over 2^19 points is too slow: the last 4096)
    check(curve, group, g, ks[tail:], got[tail:], full_below=0, sample=16, seed=pad_to)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("group", [1, 2])
def test_other_base_montgomery_and_device_pointers(curve, group):
    import torch
    F = FR[curve]
    r = F.p
    rng = random.Random(3)
    base = corc.point_mul(curve, group, corc.generator(curve, group), 7)
    ks = [0, 1, r - 1] + [rng.randrange(r) for _ in range(200)]
    got = ctx().fixed_base_mul(curve, group, enc(ks), base=base)
    check(curve, group, base, ks, got, full_below=60)
    mont = ctx().fixed_base_mul(curve, group, enc([F.to_mont(k) for k in ks]), base=base, scalars_mont=True)
    assert np.array_equal(mont, got)
    dev = torch.device("cuda", 0)
    sc = torch.from_numpy(enc(ks).view(np.int64)).to(dev)
    out = torch.zeros(got.size * 8, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx().fixed_base_mul_dev(curve, group, sc.data_ptr(), len(ks), out.data_ptr(), base=base)
    ctx().sync(0)
    assert np.array_equal(out.cpu().numpy().view(np.uint64).reshape(got.shape), got)


def test_sizes_around_every_window_switch():
    """The window width is floor(log2 n) - 3 clamped to 4..16: it changes at n = 2^8 .. 2^19.  Two sizes on either side
    of every switch (BN254 G1; G2 and the other curves run the same host code and are covered at 2^8 and 2^13)."""
    rng = random.Random(99)
    for j in range(8, 20):
        below, above = window_bits(2**j - 1), window_bits(2**j)
        assert above == below + 1 == j - 3, (j, below, above)
        pairs = [("bn254", 1)] + ([("bls12_381", 2), ("bls12_377", 1), ("bn254", 2)] if j in (8, 13) else [])
        for curve, group in pairs:
            r = FR[curve].p
            g = corc.generator(curve, group)
            for n in (2**j - 2, 2**j - 1, 2**j, 2**j + 1):
                ks = [0, 1, r - 1] + [rng.randrange(r) for _ in range(n - 3)]
                got = ctx().fixed_base_mul(curve, group, enc(ks))
                if n <= 2**14:
                    check(curve, group, g, ks, got, sample=6, seed=n)
                else:       # the oracle's MSM over 2^19 points is too slow for eight calls: sample + the last 4096 points
                    check(curve, group, g, ks[:64], got[:64], full_below=0, sample=2, seed=n)
                    check(curve, group, g, ks[-4096:], got[-4096:], full_below=0, sample=4, seed=n)


def test_arguments():
    import dg16_amd
    c_ = ctx()
    out = c_.fixed_base_mul("bn254", 1, np.zeros((0, 4), dtype=np.uint64))       # n = 0: a no-op
    assert out.shape == (0, 8)
    one = enc([1])
    buf = np.zeros(16, dtype=np.uint64)
    for curve_id, group, code in ((7, 1, 2), (0, 3, 3), (0, 0, 3)):
        rc = c_.L.dg16_fixed_base_mul(c_.h, curve_id, group, None, one.ctypes.data, 1, buf.ctypes.data, 0, 0)
        assert rc == code
    assert c_.L.dg16_fixed_base_mul(c_.h, 0, 1, None, None, 1, buf.ctypes.data, 0, 0) == 3
    assert c_.L.dg16_fixed_base_mul(c_.h, 0, 1, None, one.ctypes.data, 1, None, 0, 0) == 3
    assert c_.L.dg16_fixed_base_mul(c_.h, 0, 1, None, one.ctypes.data, 1, buf.ctypes.data, 0, 5) == 3
    with pytest.raises(dg16_amd.Dg16Error):
        c_.fixed_base_mul("bn254", 3, one)
    # ... and the context still multiplies
    assert np.array_equal(c_.fixed_base_mul("bn254", 1, one), corc.generator("bn254", 1))
