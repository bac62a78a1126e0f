"""Shapes, layouts and stage-by-stage expectations of the sharded transforms of csrc/ntt.hip (dg16_ntt_dist_stage,
dg16_h_poly_dist_stage) -- test infrastructure, verified on the CPU by tests/test_hdist_cases.py before
tests/test_gpu_hdist_shapes.py uses it.

Notation: N ranks, lg = log2 N, m = 2^log_n the global domain, M = m / N the per-rank transform, log_M = log_n - lg,
S = M / N the exchange piece.  Rank rho owns the cyclic elements x[N j + rho].

Layouts (include/dg16.h):
  transform, send buffer       Y_rho = the M-point transform of rank rho's elements, natural order = N pieces of S
  transform, output            out[k1 S + j] = X[M k1 + rho S + j]                         (ntt_out_index)
  h-polynomial, send buffers   [peer][vector a, b, c][S]: element (peer, v, j) at (3 peer + v) S + j
  h-polynomial, output         out[j] = h[rho + N j]                                        (h_out_index)

The integer helpers restate nothing: every value comes from oracle/pyref/hdist.py (stage0 / stage1 / stage2) or from
Domain.fft / ifft; this module only puts those values where the header says they sit.
"""

import numpy as np

from oracle.pyref import hdist
from oracle.pyref.poly import Domain

ALL = ["bn254", "bls12_381", "bls12_377"]
RANKS = (2, 4, 8)
TILE_LOG = 10               # csrc/ntt.hip: kTileLog = kMaxStepLog = 10


def lg(n_ranks):
    l = n_ranks.bit_length() - 1
    assert 1 << l == n_ranks
    return l


def plan(log_len):
    """make_plan of csrc/ntt.hip: one pass up to 2^10, (log / 2, rest) up to 2^20, three passes above."""
    if log_len <= TILE_LOG:
        return (log_len,)
    if log_len <= 2 * TILE_LOG:
        return (log_len // 2, log_len - log_len // 2)
    s0 = log_len // 3
    s1 = (log_len - s0) // 2
    return (s0, s1, log_len - s0 - s1)


# ---- the shape table ---------------------------------------------------------------------------------------------------
# log_M -> the per-rank plan it must reach (checked against plan() by test_hdist_cases.py); "lg" / "lg+1" are S = 1, 2
SWEEP_LOG_M = ("lg", "lg+1", 5, 9, 10, 11, 12, 17)
CLAIMED_PLAN = {5: (5,), 9: (9,), 10: (10,), 11: (5, 6), 12: (6, 6), 17: (8, 9), 20: (10, 10), 21: (7, 7, 7)}
FIELDS_AT_17 = ["bn254", "bls12_381"]
# (curve, N, log_M, runs the h-polynomial too): BN254 on two ranks only
EXTRA = [("bn254", 2, 20, False), ("bn254", 2, 21, True)]


def sweep_log_M(n_ranks):
    l = lg(n_ranks)
    out = []
    for k in SWEEP_LOG_M:
        k = {"lg": l, "lg+1": l + 1}.get(k, k)
        if k not in out:
            out.append(k)
    return sorted(out)


def sweep():
    """[(curve, N, log_M)]: every field up to log_M = 12, BN254 and BLS12-381 at 17."""
    return [(curve, n, k) for n in RANKS for k in sweep_log_M(n) for curve in ALL
            if k <= 12 or curve in FIELDS_AT_17]


def describe(n_ranks, log_M):
    """(plan, log_S, class of the piece against the 2^10-element tile of ntt_step_kernel)."""
    log_S = log_M - lg(n_ranks)
    pl = plan(log_M)
    if log_S > TILE_LOG:
        cls = "above a tile"
    elif log_S == TILE_LOG:
        cls = "a tile"
    elif log_S < pl[-1]:
        cls = "below a tile line"        # a line = the 2^s points of the last pass: piece boundaries fall inside a line
    else:
        cls = "below a tile"
    return pl, log_S, cls


# shapes of the structured-value and stage-contract tests
def structured_shapes():
    """[(N, log_n)]: log_n = 2 lg (S = 1) and one size with log_M >= 11 per N -- (5,6), (6,6) and (5,6) again with
    S = 2^10, 2^10 and 2^8."""
    return [(2, 2), (2, 12), (4, 4), (4, 14), (8, 6), (8, 14)]


def contract_shapes():
    """[(N, log_m)]: every domain from N^2 (S = 1) to 2^8."""
    return [(n, k) for n in RANKS for k in range(2 * lg(n), 9)]


# ---- output layouts ----------------------------------------------------------------------------------------------------
def ntt_out_index(n_ranks, M, rank):
    """idx[k1 S + j] = M k1 + rank S + j: positions of the global transform that rank `rank` ends with."""
    S = M // n_ranks
    k1, j = np.divmod(np.arange(M), S)
    return M * k1 + rank * S + j


def h_out_index(n_ranks, M, rank):
    return rank + n_ranks * np.arange(M)


def locate_ntt(n_ranks, M, pos):
    """Inverse of ntt_out_index: global position -> (rank, local row)."""
    S = M // n_ranks
    k1, k2 = divmod(pos, M)
    rank, j = divmod(k2, S)
    return rank, k1 * S + j


# ---- the exchange ------------------------------------------------------------------------------------------------------
def exchange(bufs):
    """bufs[r]: rank r's send buffer, N equal chunks by peer (list).  Returns the receive buffers: chunk src of
    recv[dst] = chunk dst of bufs[src]."""
    n = len(bufs)
    c = len(bufs[0]) // n
    return [[x for src in range(n) for x in bufs[src][dst * c:(dst + 1) * c]] for dst in range(n)]


# ---- the transform, stage by stage, on integers ------------------------------------------------------------------------
def ntt_send(x, F, n_ranks, inverse):
    """[rank] -> stage 0's output: the M-point (i)NTT of the rank's cyclic elements (1 / M included when inverse)."""
    dom = Domain(F, len(x) // n_ranks)
    return [(dom.ifft(x[r::n_ranks]) if inverse else dom.fft(x[r::n_ranks])) for r in range(n_ranks)]


def ntt_out(x, F, n_ranks, inverse):
    """[rank] -> stage 1's output (hdist.ntt_sharded)."""
    return hdist.ntt_sharded(x, F, n_ranks, inverse)


# ---- the h-polynomial, stage by stage, on integers ---------------------------------------------------------------------
def _pack(vecs_by_peer, S):
    """vecs_by_peer[peer][v] = S integers -> [peer][vector][S] flat."""
    return [x for per_peer in vecs_by_peer for vec in per_peer for x in vec]


def _piece(buf, peer, v, S):
    o = (3 * peer + v) * S
    return buf[o:o + S]


def h_stages(a, b, c, F, n_ranks):
    """a, b, c: the global evaluation vectors (integers).  Returns (send0, send1, out), each [rank] -> list: the send
    buffers after stage 0 and stage 1 in the layout [peer][vector][S] and h[rank + N j]."""
    N, m = n_ranks, len(a)
    M = m // N
    S = M // N
    assert S >= 1 and S * N * N == m
    send0 = []
    for r in range(N):
        Y = [hdist.stage0(hdist.rows_of(v, r, N), F, m, N) for v in (a, b, c)]
        send0.append(_pack([[Y[v][q * S:(q + 1) * S] for v in range(3)] for q in range(N)], S))
    recv0 = exchange(send0)
    send1 = []
    for r in range(N):
        U = [hdist.stage1([_piece(recv0[r], i1, v, S) for i1 in range(N)], F, m, N, r) for v in range(3)]
        send1.append(_pack([[U[v][q] for v in range(3)] for q in range(N)], S))
    recv1 = exchange(send1)
    out = []
    for r in range(N):
        W = [[x for q in range(N) for x in _piece(recv1[r], q, v, S)] for v in range(3)]
        out.append(hdist.stage2(W[0], W[1], W[2], F, m, N))
    return send0, send1, out
