"""Party contexts for the distributed-primitive GPU tests, shared by every module of the process.

A party is a host thread with its own libdg16 context; the largest packing factor (l = 8) needs 32.  Each module keeping
its own contexts per (curve, l) would hold 64 and more, so there is one pool: at most 32 `Context(0)` for the process,
the (curve, l) parameters built lazily on the first 4 l of them, one `LocalTestNet` per party count."""

MAX_PARTIES = 32

_ctxs = []
_pps = {}
_nets = {}


def contexts(n):
    """The first n contexts of the pool (created on first use)."""
    assert 1 <= n <= MAX_PARTIES
    import dg16_amd
    while len(_ctxs) < n:
        _ctxs.append(dg16_amd.Context(0))
    return _ctxs[:n]


def params(curve, l, parties=None):
    """PackedSharingParams of (curve, l) on the first `parties` contexts (default: all 4 l)."""
    from dg16_amd import dist as D
    n = 4 * l if parties is None else parties
    have = _pps.setdefault((curve, l), [])
    for c in contexts(n)[len(have):]:
        have.append(D.PackedSharingParams(c, curve, l))
    return have[:n]


def net(n):
    from dg16_amd import dist as D
    if n not in _nets:
        _nets[n] = D.LocalTestNet(n)
    return _nets[n]


def parties(curve, l=2):
    """(contexts, params, net, dg16_amd.dist) for the 4 l parties of packing factor l."""
    from dg16_amd import dist as D
    n = 4 * l
    return contexts(n), params(curve, l), net(n), D
