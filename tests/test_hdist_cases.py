"""tests/hdist_cases.py checked on the CPU: the stage-by-stage expectations against Domain.fft / ifft and the single
prover's witness map at every minimal shape (log_n = 2 lg, 2 lg + 1, 2 lg + 2; N = 2, 4, 8; three fields), the layout
formulas against their definitions, and the shape table against the plans it claims to reach.  The GPU tests
(tests/test_gpu_hdist_shapes.py) then use helpers that are already known to be right."""

import random

import pytest

from oracle.pyref import groth16 as G
from oracle.pyref.fields import FR
from oracle.pyref.poly import Domain
import hdist_cases as HC

MINIMAL = [(n, 2 * HC.lg(n) + d) for n in HC.RANKS for d in (0, 1, 2)]


@pytest.mark.parametrize("curve", HC.ALL)
@pytest.mark.parametrize("n_ranks,log_n", MINIMAL)
def test_transform_stages_equal_the_domain_transform(curve, n_ranks, log_n):
    F, p = FR[curve], FR[curve].p
    m = 1 << log_n
    N, M = n_ranks, m // n_ranks
    S = M // N
    rng = random.Random(7 * m + N)
    x = [rng.randrange(p) for _ in range(m)]
    dom = Domain(F, m)
    for inverse in (False, True):
        X = dom.ifft(x) if inverse else dom.fft(x)
        out = HC.ntt_out(x, F, N, inverse)
        send = HC.ntt_send(x, F, N, inverse)
        w = dom.group_gen_inv if inverse else dom.group_gen
        n_inv = F.inv(N) if inverse else 1
        for r in range(N):
            idx = HC.ntt_out_index(N, M, r)
            assert idx.tolist() == [M * k1 + r * S + j for k1 in range(N) for j in range(S)]
            assert out[r] == [X[i] for i in idx]
            for row, i in enumerate(idx.tolist()):
                assert HC.locate_ntt(N, M, i) == (r, row)
        # the send buffers are the right intermediate: X[k] = (1 / N) sum_i1 w^(i1 k) Y_i1[k mod M]
        for k in range(m):
            assert X[k] == sum(pow(w, i1 * k, p) * send[i1][k % M] for i1 in range(N)) * n_inv % p
        # ... and a piece is what the exchange moves: rank sigma receives Y_i1[sigma S + j] at [i1][j]
        recv = HC.exchange(send)
        for sigma in range(N):
            assert recv[sigma] == [send[i1][sigma * S + j] for i1 in range(N) for j in range(S)]


@pytest.mark.parametrize("curve", HC.ALL)
@pytest.mark.parametrize("n_ranks,log_m", MINIMAL)
def test_h_stages_equal_the_witness_map(curve, n_ranks, log_m):
    F, p = FR[curve], FR[curve].p
    m = 1 << log_m
    N, M = n_ranks, m // n_ranks
    S = M // N
    rng = random.Random(11 * m + N)
    a, b, c = ([rng.randrange(p) for _ in range(m)] for _ in range(3))
    ref = G.witness_map_from_abc(a, b, c, Domain(F, m))
    send0, send1, out = HC.h_stages(a, b, c, F, N)
    domM = Domain(F, M)
    dom = Domain(F, m)
    g = Domain(F, 2 * m).group_gen
    for r in range(N):
        assert out[r] == [ref[i] for i in HC.h_out_index(N, M, r)] == ref[r::N]
        assert len(send0[r]) == len(send1[r]) == 3 * M
        for vi, v in enumerate((a, b, c)):
            Y = domM.ifft(v[r::N])
            for q in range(N):
                assert send0[r][(3 * q + vi) * S:(3 * q + vi + 1) * S] == Y[q * S:(q + 1) * S]
    # send buffer 2, independently of hdist.stage1: U_rho[q][v][j] = w^(q k2) sum_k1 w_N^(k1 q) g^(M k1 + k2) c[M k1 + k2],
    # k2 = rho S + j, c = the coefficients of the vector (the single prover's inverse transform)
    wN = pow(dom.group_gen, M, p)
    for vi, v in enumerate((a, b, c)):
        coef = dom.ifft(v)
        for rho in range(N):
            for q in range(N):
                for j in range(S):
                    k2 = rho * S + j
                    u = sum(pow(wN, k1 * q, p) * pow(g, M * k1 + k2, p) * coef[M * k1 + k2] for k1 in range(N))
                    assert send1[rho][(3 * q + vi) * S + j] == u * pow(dom.group_gen, q * k2, p) % p


def test_exchange_is_the_chunk_transpose():
    bufs = [[100 * r + i for i in range(12)] for r in range(4)]
    recv = HC.exchange(bufs)
    for dst in range(4):
        for src in range(4):
            assert recv[dst][3 * src:3 * src + 3] == bufs[src][3 * dst:3 * dst + 3]


def test_shape_table_reaches_the_plans_it_claims():
    for k, pl in HC.CLAIMED_PLAN.items():
        assert HC.plan(k) == pl and sum(pl) == k
    # make_plan's own thresholds
    assert [len(HC.plan(k)) for k in (1, 10, 11, 20, 21, 27)] == [1, 1, 2, 2, 3, 3]
    pts = HC.sweep()
    assert len(pts) == len(set(pts))
    seen_plans, seen_S, seen_cls = set(), set(), set()
    for n in HC.RANKS:
        l = HC.lg(n)
        logs = HC.sweep_log_M(n)
        assert set(logs) == {l, l + 1, 5, 9, 10, 11, 12, 17} and logs == sorted(set(logs))
        for k in logs:
            fields = [c for c, n_, k_ in pts if (n_, k_) == (n, k)]
            assert fields == (HC.ALL if k <= 12 else HC.FIELDS_AT_17)
            pl, log_S, cls = HC.describe(n, k)
            assert log_S >= 0 and (k not in HC.CLAIMED_PLAN or pl == HC.CLAIMED_PLAN[k])
            seen_plans.add(pl)
            seen_S.add((n, log_S))
            seen_cls.add(cls)
    # S = 1 and S = 2 on every rank count; one-pass lengths 1 .. 5, 9, 10; the two-pass plans; every piece class
    assert all((n, 0) in seen_S and (n, 1) in seen_S for n in HC.RANKS)
    assert {(1,), (2,), (3,), (4,), (5,), (9,), (10,), (5, 6), (6, 6), (8, 9)} == seen_plans
    assert seen_cls == {"below a tile line", "below a tile", "a tile", "above a tile"}
    for curve, n, k, with_h in HC.EXTRA:
        assert curve == "bn254" and n == 2
    assert [HC.describe(n, k)[:2] for _, n, k, _ in HC.EXTRA] == [((10, 10), 19), ((7, 7, 7), 20)]
    # the structured shapes: S = 1 and one multi-pass size per rank count; the contract shapes stay at or below 2^8
    ss = HC.structured_shapes()
    for n in HC.RANKS:
        mine = [k for n_, k in ss if n_ == n]
        assert mine[0] == 2 * HC.lg(n) and len(mine) == 2 and mine[1] - HC.lg(n) >= 11
    assert all(2 * HC.lg(n) <= k <= 8 for n, k in HC.contract_shapes()) and len(HC.contract_shapes()) == 15
