"""The restatement of dist-primitives in oracle/pyref (pss.py, dist.py, groth16.py) at every packing factor the
library accepts, l = 1, 2, 4, 8 (4, 8, 16, 32 parties).  tests/test_gpu_dist_packing.py compares the GPU with this
restatement bit for bit; before it can be the yardstick there, it has to hold the relations the reference's own tests
assert (pss.rs:150-241, dfft/mod.rs:273-460, dpp/mod.rs:90-150, ext_wit.rs:118-190) at those l, not only at l = 2."""

import random

import pytest

from oracle.pyref import dist as R, groth16 as G
from oracle.pyref.fields import FR
from oracle.pyref.poly import Domain
from oracle.pyref.pss import PackedSharingParams as RefPSS

LS = [1, 2, 4, 8]
CURVES_ = ["bn254", "bls12_377"]


def log2(l):
    return l.bit_length() - 1


def unpack_all(shares, pp, degree2=False):
    """Per-party share vectors [n][k] -> the k * l secrets in order."""
    un = pp.unpack2 if degree2 else pp.unpack
    return [v for sh in R.transpose(shares) for v in un(sh)]


@pytest.mark.parametrize("l", LS)
@pytest.mark.parametrize("curve", CURVES_)
def test_pack_unpack_round_trip(curve, l):
    F = FR[curve]
    pp = RefPSS(F, l)
    assert (pp.n, pp.t) == (4 * l, l - 1)
    rng = random.Random(l)
    cases = [[rng.randrange(F.p) for _ in range(l)] for _ in range(8)]
    cases += [[0] * l, [F.p - 1] * l] + [[int(i == j) for i in range(l)] for j in range(l)]
    for s in cases:
        sh = pp.pack_from_public(s)
        assert len(sh) == pp.n
        assert pp.unpack(sh) == s
        assert pp.unpack2(sh) == s          # a degree-(t + l) sharing is also a degree-2(t + l) one
    a, b = cases[0], cases[1]
    prod = [x * y % F.p for x, y in zip(pp.pack_from_public(a), pp.pack_from_public(b))]
    assert pp.unpack2(prod) == [x * y % F.p for x, y in zip(a, b)]


def dfft_log_ms(l):
    return sorted({lm for lm in (log2(l), log2(l) + 1, 6) if lm >= 1})


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("l", LS)
@pytest.mark.parametrize("curve", CURVES_)
def test_d_fft_unpacks_to_the_plain_transform(curve, l, inverse):
    F = FR[curve]
    pp = RefPSS(F, l)
    for log_m in dfft_log_ms(l):
        m = 1 << log_m
        dom = Domain(F, m)
        rng = random.Random(100 * l + log_m)
        x = [rng.randrange(F.p) for _ in range(m)]
        shares = R.share_for_dfft(x, pp)
        assert len(shares) == pp.n and len(shares[0]) == m // l
        got = (R.d_ifft if inverse else R.d_fft)(shares, False, 1, False, dom, pp)
        assert unpack_all(got, pp) == (dom.ifft(x) if inverse else dom.fft(x)), log_m


@pytest.mark.parametrize("l", LS)
@pytest.mark.parametrize("curve", CURVES_)
def test_d_pp_unpacks_to_the_running_product(curve, l):
    F = FR[curve]
    pp = RefPSS(F, l)
    rng = random.Random(7 + l)
    m = 8 * l
    num = [rng.randrange(1, F.p) for _ in range(m)]
    den = [rng.randrange(1, F.p) for _ in range(m)]
    ns = R.transpose(R.pack_vec(num, pp))
    ds = R.transpose(R.pack_vec(den, pp))
    exp, acc = [], 1
    for a, b in zip(num, den):
        acc = acc * a % F.p * F.inv(b) % F.p
        exp.append(acc)
    assert unpack_all(R.d_pp(ns, ds, pp), pp) == exp


def abc(F, m, seed):
    rng = random.Random(seed)
    return tuple([rng.randrange(F.p) for _ in range(m)] for _ in range(3))


@pytest.mark.parametrize("curve", CURVES_)
def test_ext_wit_h_is_the_witness_map_at_l_2(curve):
    F = FR[curve]
    pp = RefPSS(F, 2)
    m = 16
    dom = Domain(F, m)
    a, b, c = abc(F, m, 2)
    got = G.ext_wit_h(G.qap_pss(a, b, c, pp), dom, pp)
    assert unpack_all(got, pp) == G.witness_map_from_abc(a, b, c, dom)


@pytest.mark.parametrize("curve", CURVES_)
def test_ext_wit_h_runs_at_l_1_and_is_not_the_witness_map(curve):
    """t = 0: `s1.swap(i, i * l + t)` (ext_wit.rs:74-76) is the identity, so the first m of the 2m evaluations are kept,
    not the odd ones.  The library mirrors this output; nobody should take it for h."""
    F = FR[curve]
    pp = RefPSS(F, 1)
    m = 8
    dom = Domain(F, m)
    a, b, c = abc(F, m, 1)
    got = G.ext_wit_h(G.qap_pss(a, b, c, pp), dom, pp)
    assert len(got) == 4 and all(len(g) == m for g in got)
    assert unpack_all(got, pp) != G.witness_map_from_abc(a, b, c, dom)


@pytest.mark.parametrize("l", [4, 8])
@pytest.mark.parametrize("curve", CURVES_)
def test_ext_wit_h_indexes_past_the_vector_above_l_2(curve, l):
    """The reference's panic (index i * l + t up to l m - 1 in a Vec of 2m), restated: the ground on which
    dg16_ext_wit_h returns DG16_ERR_UNSUPPORTED for these l."""
    F = FR[curve]
    pp = RefPSS(F, l)
    m = 32
    a, b, c = abc(F, m, l)
    with pytest.raises(IndexError):
        G.ext_wit_h(G.qap_pss(a, b, c, pp), Domain(F, m), pp)
