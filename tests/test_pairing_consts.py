"""CPU: every constant of distributed-groth16_amd/csrc/pairing_consts_gen.h recomputed with Python integers from the
base-field prime q (the oracle's), the tower's non-residue xi (the oracle's) and the curve parameter x -- which is
itself tied to q and r by the family's polynomials -- without importing the generator; then the generator is asked
whether the committed header is what it would write."""

import os
import re
import subprocess
import sys

import pytest

from oracle.pyref import pairing as PR
from oracle.pyref.fields import FQ, FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "distributed-groth16_amd", "csrc", "pairing_consts_gen.h")
X = {"bn254": 4965661367192848881, "bls12_381": -0xd201000000010000}


def block(curve):
    text = open(HDR).read()
    blk = text[text.index("struct %s_pairing_consts {" % curve):]
    return blk[:blk.index("\n};")]


def f2mul(a, b, q):
    return ((a[0] * b[0] - a[1] * b[1]) % q, (a[0] * b[1] + a[1] * b[0]) % q)


def f2pow(a, e, q):
    acc = (1, 0)
    for bit in bin(e)[2:]:
        acc = f2mul(acc, acc, q)
        if bit == "1":
            acc = f2mul(acc, a, q)
    return acc


def test_curve_parameter_gives_the_primes():
    x = X["bn254"]
    assert FQ["bn254"].p == 36 * x ** 4 + 36 * x ** 3 + 24 * x ** 2 + 6 * x + 1
    assert FR["bn254"].p == 36 * x ** 4 + 36 * x ** 3 + 18 * x ** 2 + 6 * x + 1
    x = X["bls12_381"]
    assert FR["bls12_381"].p == x ** 4 - x ** 2 + 1
    assert FQ["bls12_381"].p == (x - 1) ** 2 * FR["bls12_381"].p // 3 + x


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_every_generated_constant(curve):
    blk = block(curve)
    q, r, x = FQ[curve].p, FR[curve].p, X[curve]
    xi, twist = PR._TOWER[curve]
    nl = (q.bit_length() + 31) // 32
    R = 1 << (32 * nl)
    ints = dict(re.findall(r"static constexpr int (\w+) = (-?\d+)[;,]", blk))
    m = re.search(r"static constexpr int XI_C0 = (\d+), XI_C1 = (\d+);", blk)
    assert (int(m.group(1)), int(m.group(2))) == xi
    bools = dict(re.findall(r"static constexpr bool (\w+) = (true|false);", blk))
    assert bools == {"M_TWIST": "true" if twist == "M" else "false", "IS_BN": "true" if curve == "bn254" else "false",
                     "X_NEG": "true" if x < 0 else "false"}
    assert int(re.search(r"X_ABS = 0x([0-9a-f]+)ull", blk).group(1), 16) == abs(x)
    # the Miller loop scalar: digits below the leading one, most significant first
    m = re.search(r"static constexpr int8_t ATE\[(\d+)\] = \{([^}]*)\}", blk)
    digits = [int(d) for d in m.group(2).split(",")]
    assert len(digits) == int(m.group(1)) == int(ints["ATE_LEN"])
    assert int(ints["ATE_ADDS"]) == sum(1 for d in digits if d)
    value = 1
    for d in digits:
        assert d in (-1, 0, 1)
        value = 2 * value + d
    assert value == (6 * x + 2 if curve == "bn254" else abs(x))
    if curve == "bn254":     # non-adjacent form
        assert all(not (a and b) for a, b in zip([1] + digits, digits))
    # Frobenius coefficients xi^(i (q - 1) / 6) in Montgomery form
    body = blk[blk.index("FROB[5][2][%d]" % nl):]
    rows = re.findall(r"\{((?:0x[0-9a-f]{8}u(?:, )?)+)\}", body)
    assert len(rows) == 10
    vals = [sum(int(w.strip().rstrip("u"), 16) << (32 * k) for k, w in enumerate(row.split(","))) for row in rows]
    assert all(len(row.split(",")) == nl for row in rows)
    assert (q - 1) % 6 == 0
    for i in range(1, 6):
        g = f2pow(xi, i * (q - 1) // 6, q)
        assert (vals[2 * (i - 1)], vals[2 * (i - 1) + 1]) == (g[0] * R % q, g[1] * R % q), i
    # w^6 = xi defines a field: xi is neither a square nor a cube in Fq2
    assert f2pow(xi, (q * q - 1) // 2, q) != (1, 0) and f2pow(xi, (q * q - 1) // 3, q) != (1, 0)
    # the exponent of the hard part's x-chain (pairing.h: final_exp) is m (q^4 - q^2 + 1) / r with gcd(m, r) = 1
    if curve == "bn254":
        a = 12 * x ** 3 + 6 * x ** 2 + 6 * x
        b = a - 2 * x
        h = (a + 6 * x ** 2 + 1) + b * q + a * q ** 2 + (b - 1) * q ** 3
    else:
        h = (x - 1) ** 2 * (x + q) * (x ** 2 + q ** 2 - 1) + 3
    cyc, rem = divmod(q ** 4 - q ** 2 + 1, r)
    assert rem == 0 and h % cyc == 0 and (h // cyc) % r != 0


def test_committed_header_is_what_the_generator_writes():
    gen = os.path.join(ROOT, "tools", "gen_pairing_consts.py")
    assert subprocess.run([sys.executable, gen, "--check"]).returncode == 0
