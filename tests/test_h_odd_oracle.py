"""The yardstick of tests/test_gpu_ext_wit_h_odd.py, on the CPU: the reference's ext_wit::h rounds with the king keeping
s1[2 i + 1], i < m (tests/h_odd_cases.py), unpack to CircomReduction's witness map at EVERY packing factor, and at l = 2
they are the reference's own shares.  This holds without the library; it says that the rule is the right one."""

import pytest

import h_odd_cases as HC
from oracle.pyref import dist as R, groth16 as G
from oracle.pyref.fields import FR
from oracle.pyref.poly import Domain
from oracle.pyref.pss import PackedSharingParams as RefPSS

CURVES_ = ["bn254", "bls12_381", "bls12_377"]


@pytest.mark.parametrize("l", HC.LS)
@pytest.mark.parametrize("curve", CURVES_)
def test_odd_positions_unpack_to_the_witness_map(curve, l):
    F = FR[curve]
    pp = RefPSS(F, l)
    for log_m in HC.log_ms(l, 5):
        m = 1 << log_m
        dom = Domain(F, m)
        a, b, c, qs, want = HC.case(curve, l, log_m)
        got = HC.ext_wit_h_odd(qs, dom, pp)
        assert len(got) == pp.n and all(len(g) == m // l for g in got)
        assert [v for sh in R.transpose(got) for v in pp.unpack(sh)] == G.witness_map_from_abc(a, b, c, dom), log_m
        assert got == want, log_m       # pack_from_public is deterministic: the shares themselves


@pytest.mark.parametrize("curve", CURVES_)
def test_at_l_2_it_is_the_references_output(curve):
    F = FR[curve]
    pp = RefPSS(F, 2)
    for log_m in HC.log_ms(2, 5):
        dom = Domain(F, 1 << log_m)
        _, _, _, qs, _ = HC.case(curve, 2, log_m)
        assert HC.ext_wit_h_odd(qs, dom, pp) == G.ext_wit_h(qs, dom, pp), log_m


@pytest.mark.parametrize("l", HC.LS)
def test_the_rule_names_the_odd_evaluations(l):
    """(element, row) of position i of chunk c is evaluation 2 (c l + i) + 1; a chunk reads elements 2c and 2c + 1 only,
    odd rows only for l >= 2, and element 2c + 1 alone for l = 1."""
    for chunks in range(1, 9):
        for c in range(chunks):
            got = [HC.source(l, c, i) for i in range(l)]
            assert [e * l + r for e, r in got] == [2 * (c * l + i) + 1 for i in range(l)]
            assert all(e in (2 * c, 2 * c + 1) and e < 2 * chunks for e, _ in got)
            if l == 1:
                assert got == [(2 * c + 1, 0)]
            else:
                assert all(r % 2 == 1 and r < l for _, r in got)
                assert sorted(got) == [(2 * c + k, r) for k in (0, 1) for r in range(1, l, 2)]
