"""tests/ntt_cases.py checked on the CPU: every closed form against the big-int transform of oracle/pyref/poly.py
(Domain.fft / ifft) and against the C oracle (corc.ntt) with the same arguments, all three scalar fields, log_n = 0 .. 8
(n = 1 and n = 2, where the impulse positions and the geometric exponents coincide, included).  The GPU tests
(tests/test_gpu_ntt_structured.py) then use a generator that is already known to be right."""

import numpy as np
import pytest

from oracle import corc
from oracle.pyref.fields import FR
from oracle.pyref.poly import Domain
import ntt_cases as NC

ALL = ["bn254", "bls12_381", "bls12_377"]
LOGS = list(range(9))


def offsets(F, n):
    """The coset offsets of the GPU tests: the field's generator, 1, p - 1 and w_2n (the h-polynomial's shift)."""
    return [("generator", F.generator), ("1", 1), ("p-1", F.p - 1), ("w_2n", F.root_of_unity(2 * n))]


def test_codec_and_negation():
    for curve in ALL:
        F = FR[curve]
        vals = [0, 1, 2, F.p - 1, F.p - 2, (F.p - 1) // 2, 1 << 64, (1 << 128) - 1, (1 << 192) + 5, F.R, F.inv(F.R)]
        A = NC.enc(F, vals)
        assert np.array_equal(A, corc.ints_to_arr([F.to_mont(v) for v in vals], 4))
        assert NC.dec(F, A) == vals
        assert NC.dec(F, NC.neg_arr(F, A)) == [(F.p - v) % F.p for v in vals]
        # raw limb patterns with borrows through every limb
        raw = [0, 1, 1 << 64, 1 << 128, 1 << 192, (1 << 64) - 1, (1 << 192) - 1, F.p - 1, F.p - (1 << 64), F.p - (1 << 128)]
        got = corc.arr_to_ints(NC.neg_arr(F, corc.ints_to_arr(raw, 4)))
        assert got == [(F.p - v) % F.p for v in raw]
        assert np.array_equal(NC.powers_arr(F, 3, 50, 7), NC.enc(F, [7 * pow(3, i, F.p) % F.p for i in range(50)]))


@pytest.mark.parametrize("curve", ALL)
@pytest.mark.parametrize("log_n", LOGS)
def test_closed_forms_equal_both_oracles(curve, log_n):
    F = FR[curve]
    n = 1 << log_n
    dom = Domain(F, n)
    cs = NC.cases(F, n)
    names = [c.name for c in cs]
    # zero, 3 x (constant, 4 impulses, 3 geometric, alternating), witness-shaped
    assert len(cs) == 1 + 3 * 9 + 1 and (n < 4 or len(set(names)) == len(cs))
    for c in cs:
        assert len(c.x) == n and all(0 <= v < F.p for v in c.x), c.name
        X = NC.enc(F, c.x)
        fwd, inv = dom.fft(c.x), dom.ifft(c.x)
        if c.fwd is not None:
            assert c.fwd == fwd, c.name
        if c.inv is not None:
            assert c.inv == inv, c.name
        assert np.array_equal(corc.ntt(curve, X), NC.enc(F, fwd)), c.name
        assert np.array_equal(corc.ntt(curve, X, inverse=True), NC.enc(F, inv)), c.name
    # the rows the issue cares most about: one non-zero output
    sparse = [c for c in cs if c.name.startswith(("geometric", "alternating", "constant"))]
    assert len(sparse) == 15 and all(sum(1 for v in c.fwd if v) == 1 for c in sparse)
    w = [c for c in cs if c.name == "witness-shaped"][0]
    k = NC.witness_len(n)
    assert k == -(-3 * n // 8) and all(v == 0 for v in w.x[k:]) and (n < 8 or sum(1 for v in w.x[:k] if v) >= k - 1)


@pytest.mark.parametrize("curve", ALL)
@pytest.mark.parametrize("log_n", LOGS)
def test_array_form_equals_integer_form(curve, log_n):
    F = FR[curve]
    n = 1 << log_n
    dom = Domain(F, n)
    cs, arrs = NC.cases(F, n), NC.arrays(F, n)
    assert [c.name for c in cs] == [a.name for a in arrs]
    for c, a in zip(cs, arrs):
        assert a.x.shape == (n, 4) and a.x.dtype == np.uint64
        assert np.array_equal(a.x, NC.enc(F, c.x)), c.name
        if a.fwd is not None:
            assert NC.sparse_list(n, a.fwd) == dom.fft(c.x), c.name
            assert np.array_equal(NC.sparse_arr(F, n, a.fwd), corc.ntt(curve, a.x)), c.name
        if a.inv is not None:
            assert NC.sparse_list(n, a.inv) == dom.ifft(c.x), c.name
            assert np.array_equal(NC.sparse_arr(F, n, a.inv), corc.ntt(curve, a.x, inverse=True)), c.name
        # every family whose transform has one entry says so (an impulse has one only at n = 1)
        if not c.name.startswith(("impulse", "witness")):
            assert a.fwd is not None and a.inv is not None, c.name


@pytest.mark.parametrize("curve", ALL)
@pytest.mark.parametrize("log_n", LOGS)
def test_coset_cancelling_closed_form(curve, log_n):
    F = FR[curve]
    n = 1 << log_n
    for oname, g in offsets(F, n):
        dom = Domain(F, n, g)
        ge = NC.enc(F, [g])
        ints, arrs = NC.coset_cancelling(F, n, g), NC.coset_cancelling_arrays(F, n, g)
        assert len(ints) == 3 and [x[0] for x in ints] == [x[0] for x in arrs]
        for (name, x, exp), (_, xa, sp) in zip(ints, arrs):
            assert exp == dom.fft(x), (oname, name)
            assert sum(1 for v in exp if v) == 1 and exp[0] == n * x[0] % F.p
            assert np.array_equal(xa, NC.enc(F, x)), (oname, name)
            assert NC.sparse_list(n, sp) == exp
            assert np.array_equal(corc.ntt(curve, xa, coset=ge), NC.enc(F, exp)), (oname, name)
            # the coset inverse of the C oracle is Domain.ifft's
            assert np.array_equal(corc.ntt(curve, xa, inverse=True, coset=ge), NC.enc(F, dom.ifft(x))), (oname, name)
