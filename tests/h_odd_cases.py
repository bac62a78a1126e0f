"""ext_wit::h with the odd-position rule (DG16_F_H_ODD), restated from the oracle's own parts: the reference's six
d_ifft / d_fft rounds (oracle.pyref.dist), `pp.unpack` of every gathered element, the selection s1[2 i + 1] for i < m in
place of the reference's `s1.swap(i, i * l + t)` (ext_wit.rs:74-76), h = p q - w, `pack_vec`, `transpose`.  Also the
index rule of csrc/h_odd.h in Python, and the inputs the GPU tests share."""

import functools
import random

from oracle.pyref import dist as R, groth16 as G
from oracle.pyref.fields import FR
from oracle.pyref.poly import Domain
from oracle.pyref.pss import PackedSharingParams as RefPSS

LS = [1, 2, 4, 8]


def log2(l):
    return l.bit_length() - 1


def log_ms(l, top):
    """One chunk per party (a lane's two elements are the whole vector), two chunks, several."""
    return sorted({max(1, log2(l)), log2(l) + 1, top})


def source(l, c, i):
    """(packed element, unpack row) whose secret is evaluation 2 (c l + i) + 1 of the 2m: csrc/h_odd.h's rule."""
    if l == 1:
        return 2 * c + 1, 0
    pos = 2 * i + 1
    return 2 * c + pos // l, pos % l


def abc(F, m, seed):
    """a, b, c of m field elements that include 0 and r - 1 in every vector (when there is room) and at one position of
    all three."""
    rng = random.Random(seed)
    v = [[rng.randrange(F.p) for _ in range(m)] for _ in range(3)]
    edge = [0, F.p - 1]
    for k in range(3):
        for j, e in enumerate(edge):
            v[k][(k + 2 * j) % m] = e
    v[0][m - 1] = v[1][m - 1] = v[2][m - 1] = F.p - 1
    return tuple(v)


def ext_wit_h_odd(qap_shares, dom, pp):
    """Per-party packed shares of h: oracle.pyref.groth16.ext_wit_h with the king's selection corrected."""
    F, p, m = dom.F, dom.p, dom.size
    dom2 = Domain(F, 2 * m)
    outs = []
    for k in range(3):
        shares = [q[k] for q in qap_shares]
        coeff = R.d_ifft(shares, True, 2, False, dom, pp)
        outs.append(R.d_fft(coeff, False, 1, False, dom2, pp))

    def odd(v):
        s1 = [x for sh in R.transpose(v) for x in pp.unpack(sh)]
        assert len(s1) == 2 * m
        return [s1[2 * i + 1] for i in range(m)]

    pe, qe, we = (odd(v) for v in outs)
    h = [(x * y - z) % p for x, y, z in zip(pe, qe, we)]
    return R.transpose(R.pack_vec(h, pp))


@functools.lru_cache(maxsize=None)
def case(curve, l, log_m):
    """(a, b, c, qap shares per party, expected h shares per party) -- computed once, never modified.  The expectation
    is the one the issue names: transpose(pack_vec(witness_map_from_abc(a, b, c, dom), pp))."""
    F = FR[curve]
    pp = RefPSS(F, l)
    m = 1 << log_m
    dom = Domain(F, m)
    a, b, c = abc(F, m, 1000 * l + log_m)
    qs = G.qap_pss(a, b, c, pp)
    want = R.transpose(R.pack_vec(G.witness_map_from_abc(a, b, c, dom), pp))
    return a, b, c, qs, want
