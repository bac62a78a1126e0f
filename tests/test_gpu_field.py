"""GPU parity: Montgomery field kernels and group arithmetic (through the C ABI) vs the oracle.
Bit-exact (integer arithmetic)."""

import numpy as np
import pytest

from oracle import corc
from oracle.pyref.fields import FQ, FR
from gpu_util import ctx

pytestmark = pytest.mark.gpu
ALL = ["bn254", "bls12_381", "bls12_377"]


@pytest.mark.parametrize("curve", ALL)
@pytest.mark.parametrize("kind", ["fq", "fr"])
def test_field_ops_bit_exact(curve, kind):
    F = (FQ if kind == "fq" else FR)[curve]
    n = 1 << 16
    A = corc.rand_field(curve, kind, 21, n)
    B = corc.rand_field(curve, kind, 22, n)
    edge = corc.ints_to_arr([0, F.R, F.p - 1, 1, F.to_mont(F.p - 1)], F.limbs64)
    A[:5] = edge
    B[:5] = edge[::-1]
    c = ctx()
    for op in ("add", "sub", "mul", "sqr", "neg", "from_mont"):
        got = c.field_op(curve, kind, op, A, B)
        assert np.array_equal(got, corc.field_op(curve, kind, op, A, B)), op
    canon = corc.field_op(curve, kind, "from_mont", A)
    assert np.array_equal(c.field_op(curve, kind, "to_mont", canon), A)
    assert np.array_equal(c.field_op(curve, kind, "inv", A[:256]), corc.field_op(curve, kind, "inv", A[:256]))


def boundary_values(F):
    """Operands at the edges of the 32-bit Montgomery code of fp.h (raw limb values below p; not sampled)."""
    p = F.p
    nl = 2 * F.limbs64                                   # 32-bit limbs
    top_shift = 32 * (nl - 1)
    ptop = p >> top_shift
    assert ptop > 1
    vals = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, F.R, F.R * F.R % p]
    for k in range(32, p.bit_length(), 32):              # every 32-bit limb boundary below bits(p)
        vals += [1 << k, (1 << k) - 1]
    low_ones = (1 << top_shift) - 1                      # all limbs 0xFFFFFFFF below the top limb
    vals += [(t << top_shift) | low_ones for t in (1, ptop // 2, ptop - 1)]
    assert all(0 <= v < p for v in vals)
    return list(dict.fromkeys(vals))


def boundary_pairs(F):
    p = F.p
    S = boundary_values(F)
    pairs = [(x, y) for x in S for y in S]
    pairs += [(x, p - x) for x in S if x]                # the sum is exactly p
    pairs += [(x, p - 1 - x) for x in S]                 # the sum is p - 1
    pairs += [(x, x) for x in S]                         # subtraction: no borrow, result 0
    pairs += [(x, x + 1) for x in S if x + 1 < p]        # subtraction: borrow through every limb, result p - 1
    pairs += [(x, F.inv(x)) for x in S if x]
    return pairs


@pytest.mark.parametrize("curve", ALL)
@pytest.mark.parametrize("kind", ["fq", "fr"])
def test_field_ops_on_boundary_operands(curve, kind):
    """add, sub, mul, sqr, neg, to_mont, from_mont, inv on a table of boundary operand pairs, against Python integers
    (Montgomery R = 2^(64 limbs64): mul is a b / R, to_mont a R, from_mont a / R, inv R^2 / a on the raw values) and
    against the C oracle.  The device product is inline assembly that exists only on the GPU."""
    F = (FQ if kind == "fq" else FR)[curve]
    p, R, nl = F.p, F.R, F.limbs64
    rinv = F.inv(R)
    pairs = boundary_pairs(F)
    assert len(pairs) > 300
    xs, ys = [a for a, _ in pairs], [b for _, b in pairs]
    A, B = corc.ints_to_arr(xs, nl), corc.ints_to_arr(ys, nl)
    want = {
        "add": [(a + b) % p for a, b in pairs],
        "sub": [(a - b) % p for a, b in pairs],
        "mul": [a * b * rinv % p for a, b in pairs],
        "sqr": [a * a * rinv % p for a in xs],
        "neg": [(p - a) % p for a in xs],
        "to_mont": [a * R % p for a in xs],
        "from_mont": [a * rinv % p for a in xs],
        "inv": [F.inv(a) * R * R % p for a in xs],
    }
    c = ctx()
    for op, exp in want.items():
        got = c.field_op(curve, kind, op, A, B)
        bad = [i for i, (g, e) in enumerate(zip(corc.arr_to_ints(got), exp)) if g != e]
        assert not bad, (op, len(bad), [(hex(xs[i]), hex(ys[i])) for i in bad[:4]])
        assert np.array_equal(got, corc.field_op(curve, kind, op, A, B)), op


def test_field_mul_million_pairs_bn254():
    # >= 10^6 random pairs, bit-exact
    n = 1 << 20
    for kind in ("fq", "fr"):
        A = corc.rand_field("bn254", kind, 31, n)
        B = corc.rand_field("bn254", kind, 32, n)
        assert np.array_equal(ctx().field_op("bn254", kind, "mul", A, B),
                              corc.field_op("bn254", kind, "mul", A, B))


@pytest.mark.parametrize("curve,group", [("bn254", 1), ("bn254", 2), ("bls12_381", 1),
                                         ("bls12_381", 2), ("bls12_377", 1)])
def test_gen_bases_matches_oracle(curve, group):
    # exercises scalar_mul, madd, batch inversion and to_affine on the GPU
    n = 1000
    got = ctx().gen_bases(curve, group, 5, n)
    exp = corc.gen_points(curve, group, 5, n)
    assert np.array_equal(got, exp)


def test_empty_inputs():
    c = ctx()
    z = np.zeros((0, 4), dtype=np.uint64)
    assert c.field_op("bn254", "fr", "mul", z, z).shape == (0, 4)
    assert c.gen_bases("bn254", 1, 1, 0).shape == (0, 8)
