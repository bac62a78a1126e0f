"""Structured NTT inputs with their transforms in closed form (test infrastructure; verified on the CPU by
tests/test_ntt_cases.py before any GPU test uses it).

Random vectors never make a butterfly produce an exact multiple of p, and never give an output that is 0.  The vectors
here do: for most of them every output but one is 0, reached through the lazy butterflies of csrc/ntt.hip as some
multiple of p below kNttBound and brought home by canon().

Conventions (include/dg16.h, ark-poly's Radix2EvaluationDomain), w = Domain(F, n).group_gen:
  forward        X_k = sum_i x_i w^(i k)
  inverse        x_i = n^-1 sum_k X_k w^(-i k)
  coset forward  multiplies x_i by g^i first
  coset inverse  multiplies output i by g^-i

Only oracle.pyref.poly.Domain (for w) is taken from the oracle.  Two forms of the same cases:
  * cases(F, n) / coset_cancelling(F, n, g): Python integers (standard form, not Montgomery) with the expected
    transforms as full lists -- for sizes where big-int lists are cheap;
  * arrays(F, n) / coset_cancelling_arrays(F, n, g): the inputs as (n, 4) uint64 Montgomery limbs, built without a
    per-case O(n) big-int loop, and the expected transform as `Sparse` where it has at most one non-zero entry -- for
    every size.  test_ntt_cases.py checks that the two forms agree.
"""

import random
from collections import namedtuple

import numpy as np

from oracle.pyref.poly import Domain

# x: input; fwd / inv: expected forward / inverse transform, or None where no closed form is given (the caller takes the
# oracle's).  Lists of integers in cases(), arrays / Sparse in arrays().
Case = namedtuple("Case", "name x fwd inv")
# a vector that is `value` (an integer, standard form) at `pos` and 0 elsewhere; value == 0: the zero vector
Sparse = namedtuple("Sparse", "pos value")

WITNESS_SEED = 0x5EED


def scalars(F):
    """c in {1, p - 1, a fixed random value}."""
    return [("1", 1), ("p-1", F.p - 1), ("rnd", random.Random(F.p % 1000003).randrange(2, F.p - 1))]


def impulse_positions(n):
    return [0, 1 % n, n // 2, n - 1]


def geometric_exponents(n):
    return [1 % n, n // 2, n - 1]


def witness_len(n):
    return (3 * n + 7) // 8


# ---- integers <-> Montgomery limb arrays ------------------------------------------------------------------------------
def enc(F, vals):
    """Integers in [0, p) -> (n, 4) uint64, Montgomery form."""
    R, p = F.R, F.p
    buf = b"".join((v * R % p).to_bytes(32, "little") for v in vals)
    return np.frombuffer(buf, dtype=np.uint64).reshape(-1, 4).copy()


def dec(F, arr):
    """(n, 4) uint64 Montgomery form -> integers."""
    rinv, p = F.inv(F.R), F.p
    raw = np.ascontiguousarray(arr, dtype=np.uint64).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") * rinv % p for i in range(0, len(raw), 32)]


def sparse_arr(F, n, s):
    out = np.zeros((n, 4), dtype=np.uint64)
    if s.value:
        out[s.pos] = enc(F, [s.value])[0]
    return out


def sparse_list(n, s):
    out = [0] * n
    out[s.pos] = s.value
    return out


def neg_arr(F, a):
    """Element-wise p - a on canonical limbs (0 stays 0), without big integers."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    out = np.empty_like(a)
    borrow = np.zeros(a.shape[0], dtype=np.uint64)
    for j in range(4):
        pj = np.uint64((F.p >> (64 * j)) & 0xFFFFFFFFFFFFFFFF)
        t = pj - a[:, j]                       # wraps mod 2^64
        b1 = (a[:, j] > pj).astype(np.uint64)
        out[:, j] = t - borrow
        b2 = (borrow > t).astype(np.uint64)
        borrow = b1 | b2
    out[~a.any(axis=1)] = 0
    return out


def powers_arr(F, base, n, c=1):
    """c base^i for i < n as Montgomery limbs (one modular product per element)."""
    p = F.p
    v = c * F.R % p
    parts = []
    for _ in range(n):
        parts.append(v.to_bytes(32, "little"))
        v = v * base % p
    return np.frombuffer(b"".join(parts), dtype=np.uint64).reshape(-1, 4).copy()


def witness_arr(F, n, seed=WITNESS_SEED):
    """Witness-shaped: random field elements below ceil(3 n / 8), 0 above (a QAP vector is 0 above nc + ni).  The limbs
    are drawn directly (below 2^(bits(p) - 1) < p), so the array is its own definition at every size."""
    rng = np.random.RandomState((seed + 31 * n + F.p % 65521) % (1 << 32))
    k = witness_len(n)
    out = np.zeros((n, 4), dtype=np.uint64)
    lo = rng.randint(0, 1 << 32, size=(k, 4), dtype=np.uint64)
    hi = rng.randint(0, 1 << 32, size=(k, 4), dtype=np.uint64)
    out[:k] = (hi << np.uint64(32)) | lo
    out[:k, 3] &= np.uint64((1 << (F.p.bit_length() - 1 - 192)) - 1)
    return out


# ---- the families on Python integers ----------------------------------------------------------------------------------
def cases(F, n):
    """Every family on the plain domain of size n, with full expected lists where the closed form is given."""
    p = F.p
    dom = Domain(F, n)
    w, wi, ninv = dom.group_gen, dom.group_gen_inv, dom.size_inv
    out = [Case("zero", [0] * n, [0] * n, [0] * n)]
    for cn, c in scalars(F):
        nc = n * c % p
        out.append(Case("constant c=%s" % cn, [c] * n, sparse_list(n, Sparse(0, nc)), sparse_list(n, Sparse(0, c))))
        for j in impulse_positions(n):
            x = sparse_list(n, Sparse(j, c))
            wj, wij = pow(w, j, p), pow(wi, j, p)
            fwd, inv, a, b = [], [], c, c * ninv % p
            for _ in range(n):
                fwd.append(a)
                inv.append(b)
                a, b = a * wj % p, b * wij % p
            out.append(Case("impulse j=%d c=%s" % (j, cn), x, fwd, inv))
        for t in geometric_exponents(n):
            wit, x, a = pow(wi, t, p), [], c
            for _ in range(n):
                x.append(a)
                a = a * wit % p
            out.append(Case("geometric t=%d c=%s" % (t, cn), x, sparse_list(n, Sparse(t, nc)), None))
        x = [c if i % 2 == 0 else (p - c) % p for i in range(n)]
        out.append(Case("alternating c=%s" % cn, x, sparse_list(n, Sparse(n // 2, nc)), None))
    out.append(Case("witness-shaped", dec(F, witness_arr(F, n)), None, None))
    return out


def coset_cancelling(F, n, g):
    """x_i = c g^-i: the coset-forward transform with offset g is n c at 0 and 0 elsewhere.  (name, x, expected)."""
    p = F.p
    gi = F.inv(g % p)
    out = []
    for cn, c in scalars(F):
        x, a = [], c
        for _ in range(n):
            x.append(a)
            a = a * gi % p
        out.append(("coset-cancelling c=%s" % cn, x, sparse_list(n, Sparse(0, n * c % p))))
    return out


# ---- the same families as limb arrays, for every size -----------------------------------------------------------------
def _scaled(F, base_pows, c):
    """c base^i from base^i: itself for c = 1, the negation for c = p - 1, None otherwise (the caller recomputes)."""
    if c == 1:
        return base_pows
    if c == F.p - 1:
        return neg_arr(F, base_pows)
    return None


def arrays(F, n):
    """cases(F, n) as Montgomery arrays; fwd / inv are Sparse where at most one output is non-zero, else None.  The
    geometric rows also carry the closed-form inverse (c at (n - t) mod n), which cases() leaves to the oracle."""
    p = F.p
    dom = Domain(F, n)
    wi = dom.group_gen_inv
    zero = np.zeros((n, 4), dtype=np.uint64)
    out = [Case("zero", zero, Sparse(0, 0), Sparse(0, 0))]
    idx = np.arange(n)
    wpow = powers_arr(F, wi, n)                                         # w^-i
    for cn, c in scalars(F):
        nc = n * c % p
        ce = enc(F, [c])
        nce = neg_arr(F, ce)
        geo1 = _scaled(F, wpow, c)
        if geo1 is None:
            geo1 = powers_arr(F, wi, n, c)                              # c w^-i
        out.append(Case("constant c=%s" % cn, np.repeat(ce, n, axis=0), Sparse(0, nc), Sparse(0, c)))
        for j in impulse_positions(n):
            x = zero.copy()
            x[j] = ce[0]
            out.append(Case("impulse j=%d c=%s" % (j, cn), x, None, None))
        alt = np.where((idx % 2 == 0)[:, None], ce, nce)               # c (-1)^i
        for t in geometric_exponents(n):
            if t == 0:
                x = np.repeat(ce, n, axis=0)                            # n = 1
            elif t == n // 2:
                x = alt                                                 # w^(-n/2) = -1
            elif t == 1:
                x = geo1
            else:
                assert t == n - 1
                x = geo1[(n - idx) % n]                                 # w^(-(n-1) i) = w^i = w^(-(n - i))
            out.append(Case("geometric t=%d c=%s" % (t, cn), x, Sparse(t, nc), Sparse((n - t) % n, c)))
        out.append(Case("alternating c=%s" % cn, alt, Sparse(n // 2, nc), Sparse(n // 2, c)))
    out.append(Case("witness-shaped", witness_arr(F, n), None, None))
    return out


def coset_cancelling_arrays(F, n, g):
    """(name, x, Sparse): coset_cancelling(F, n, g) as Montgomery arrays."""
    p = F.p
    gi = F.inv(g % p)
    base = powers_arr(F, gi, n)
    out = []
    for cn, c in scalars(F):
        x = _scaled(F, base, c)
        if x is None:
            x = powers_arr(F, gi, n, c)
        out.append(("coset-cancelling c=%s" % cn, x, Sparse(0, n * c % p)))
    return out
