"""Key-shaped bases and their host mirror (plain Python + numpy + the C oracle, no GPU).

A real proving key is not `gen_bases` output: most rows of b_g1_query / b_g2_query are the identity (most wires do not
occur in B), wires with equal columns give repeated points, the reference's own benchmark CRS is a doubling chain and its
d_msm test uses M copies of one point.  Such bases make equal, opposite and identity operands meet in every kernel that
adds points.  This module makes those bases (`SHAPES`), the scalars that force the meeting (`same`, `sparse_live`), the
closed forms that need no Pippenger, a mirror of the GLV splits (csrc/glv.h: what the plain MSM's sort sees) and of the
bucket contents (`pair_buckets`), and the parametrisations of tests/test_gpu_key_shapes.py -- test_key_shapes.py mirrors
exactly those cases on the host, so the two cannot drift apart.

Points are host arrays in the C ABI layout: (n, 2 L) uint64 for G1 (x | y), (n, 4 L) for G2 (x.c0 x.c1 y.c0 y.c1),
Montgomery limbs, the identity all zeros."""

import os
import re

import numpy as np

from oracle import corc
import witness_shapes as ws

GROUPS = [("bn254", 1), ("bn254", 2), ("bls12_381", 1), ("bls12_381", 2), ("bls12_377", 1), ("bls12_377", 2)]
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "distributed-groth16_amd", "csrc")


def modulus(curve):
    return ws.modulus(curve)


def cofactor_one(curve, group):
    return (curve, group) == ("bn254", 1)


def subgroup_flags(curve, group):
    """The in_subgroup values worth a run: BN254 G1 (cofactor one) splits either way."""
    return (True,) if cofactor_one(curve, group) else (False, True)


# ---- bases -------------------------------------------------------------------------------------------------------
def negate(curve, group, pts):
    """-P row by row: y -> -y (both components in G2); the identity stays the identity."""
    pts = np.array(pts, dtype=np.uint64, copy=True).reshape(len(pts), -1)
    L = corc.FQ_LIMBS[curve]
    half = pts.shape[1] // 2
    zero = ~pts.any(axis=1)
    for lo in range(half, pts.shape[1], L):
        pts[:, lo:lo + L] = corc.field_op(curve, "fq", "neg", np.ascontiguousarray(pts[:, lo:lo + L]))
    pts[zero] = 0
    return pts


def identity_heavy(rows, frac=0.75, block=1, seed=0):
    """A fraction `frac` of the rows -- of the aligned runs of `block` rows -- set to the identity.  Returns
    (bases, live): live[i] is False where row i is the identity."""
    n = len(rows)
    rng = np.random.default_rng([seed, n, block])
    nblk = (n + block - 1) // block
    dead = np.zeros(nblk, dtype=bool)
    dead[rng.permutation(nblk)[:int(round(frac * nblk))]] = True
    live = ~np.repeat(dead, block)[:n]
    out = np.array(rows, copy=True)
    out[~live] = 0
    return out, live


def pairs(rows):
    """P[2i+1] = P[2i] (an odd last row stays alone)."""
    out = np.array(rows, copy=True)
    m = len(out) // 2
    out[1:2 * m:2] = out[0:2 * m:2]
    return out


def opposites(curve, group, rows):
    """P[2i+1] = -P[2i]."""
    out = np.array(rows, copy=True)
    m = len(out) // 2
    out[1:2 * m:2] = negate(curve, group, out[0:2 * m:2])
    assert corc.on_curve(curve, group, out[1:2]) and corc.on_curve(curve, group, out[2 * m - 1:2 * m])
    return out


def all_equal(point, n):
    return np.repeat(np.asarray(point, dtype=np.uint64).reshape(1, -1), n, axis=0)


def alternating(curve, group, point, n):
    """P, -P, P, -P, .."""
    out = all_equal(point, n)
    out[1::2] = negate(curve, group, out[1:2])[0]
    assert corc.on_curve(curve, group, out[1:2])
    return out


def chain_exponents(curve, n):
    """2^i mod r, i < n."""
    r, out, v = modulus(curve), [], 1
    for _ in range(n):
        out.append(v)
        v = v * 2 % r
    return out


def chain(curve, group, p0, n, mul=None):
    """P[i+1] = 2 P[i] (local_dummy_crs).  mul(scalars (n, 4) uint64, base) -> the n multiples of base, e.g. the library's
    fixed_base_mul; without it every row is a corc.point_add.  The first 64 rows are pinned to repeated corc.point_add
    either way."""
    p0 = np.asarray(p0, dtype=np.uint64).reshape(1, -1)
    out = np.empty((n, p0.shape[1]), dtype=np.uint64)
    head = n if mul is None else min(n, 64)
    out[0] = p0[0]
    for i in range(1, head):
        out[i] = corc.point_add(curve, group, out[i - 1:i], out[i - 1:i])[0]
    if head < n:
        got = np.asarray(mul(ws._to_limbs(chain_exponents(curve, n)), p0)).reshape(n, -1)
        assert np.array_equal(got[:head], out[:head]), "the chain's first rows are not repeated doublings"
        out[head:] = got[head:]
    return out


def real_key(curve, group, rows, seed=0):
    """60 % identities, 10 % copies of an earlier non-identity row, 2 % negatives of one, the rest distinct: the copies
    and negatives are live points that meet their source in a bucket, not further identities."""
    n = len(rows)
    rng = np.random.default_rng([seed, n, 77])
    u = rng.random(n)
    pick = rng.random(n)
    out = np.array(rows, copy=True)
    out[u < 0.60] = 0
    alive = []                                                       # the non-identity rows so far
    for i in range(n):
        if u[i] < 0.60:
            continue
        if u[i] < 0.72 and alive:
            j = alive[int(pick[i] * len(alive))]                     # in order: a copy of a copy is a copy
            out[i] = negate(curve, group, out[j:j + 1])[0] if u[i] >= 0.70 else out[j]
        alive.append(i)
    return out


# ---- scalars -----------------------------------------------------------------------------------------------------
def same(curve, n, seed=0):
    """Dense scalars, both members of a pair the SAME one: their GLV halves, quarters and every digit coincide, so the
    two points land in the same bucket of every window at any window width."""
    out = ws.dense(curve, n, seed)
    m = n // 2
    out[1:2 * m:2] = out[0:2 * m:2]
    return out


def sparse_live(curve, n, k, seed=0):
    """Only k pairs carry a (dense, per pair equal) scalar; everything else is zero."""
    out = np.zeros((n, 4), dtype=np.uint64)
    rng = np.random.default_rng([seed, n, k])
    which = np.sort(rng.permutation(n // 2)[:k])
    vals = ws.dense(curve, k, seed + 1)
    out[2 * which] = vals
    out[2 * which + 1] = vals
    return out


def sparse_live_k(g, entries_per_pair):
    """The largest k for which the live entries of one bucket set (k pairs x entries_per_pair x the windows that share
    the set) stay at or under 1/8 of its buckets: most non-empty buckets then hold exactly one pair, whose second
    accumulation is necessarily P + P or P + (-P)."""
    share = (g["nwin"] + g["bw"] - 1) // g["bw"]
    return max(1, (1 << g["log_nb"]) // (8 * entries_per_pair * share))


def scalars_of(kind, curve, n, seed=0, k=0):
    if kind == "dense":
        return ws.dense(curve, n, seed)
    if kind == "same":
        return same(curve, n, seed)
    if kind == "sparse_live":
        return sparse_live(curve, n, k, seed)
    return ws.shape(curve, n, kind, seed)


# ---- closed forms (Python integers; one corc.point_mul each) --------------------------------------------------------
def sum_mod_r(curve, sc):
    return sum(ws.to_ints(sc)) % modulus(curve)


def chain_scalar(curve, sc):
    """sum_i k_i 2^i mod r: MSM(chain, k) = chain_scalar * P_0."""
    r = modulus(curve)
    return sum(k * e for k, e in zip(ws.to_ints(sc), chain_exponents(curve, len(sc))) if k) % r


# ---- GLV mirror (csrc/glv.h; tests/test_host_arith.py holds the header's code equal to this arithmetic) ------------
def _consts(name):
    text = open(os.path.join(CSRC, "consts_gen.h")).read()
    blk = text[text.index("struct %s {" % name):]
    return blk[:blk.index("\n};")]


def _words(body):
    return sum(int(x.strip().rstrip("u"), 16) << (32 * i) for i, x in enumerate(body.split(",")))


def glv_signed(curve, group, scalars):
    """The signed parts k_j of every scalar, k = sum_j k_j LAMBDA^j mod r: DIM lists of Python integers (the arithmetic
    tests/test_host_arith.py holds csrc/glv.h's code equal to)."""
    ks = ws.to_ints(scalars)
    if ws._glv_dim(curve, group) == 2:
        blk = _consts("bn254_g2_glv_consts" if (curve, group) == ("bn254", 2) else "%s_glv_consts" % curve)
        val = {m.group(1): _words(m.group(2))
               for m in re.finditer(r"static constexpr uint32_t (\w+)\[\d+\] = \{([^}]*)\}", blk)}
        sign = {m.group(1): -1 if m.group(2) == "true" else 1
                for m in re.finditer(r"static constexpr bool (\w+)_NEG = (\w+);", blk)}
        a1, b1, a2, b2 = (sign[k] * val[k] for k in ("A1", "B1", "A2", "B2"))
        parts = [[], []]
        for k in ks:
            c1, c2 = (val["G1"] * k + (1 << 255)) >> 256, (val["G2"] * k + (1 << 255)) >> 256
            parts[0].append(k - c1 * a1 - c2 * a2)
            parts[1].append(-c1 * b1 - c2 * b2)
    else:
        blk = _consts("%s_g2_glv4_consts" % curve)
        inner = lambda pat: re.findall(r"\{([^{}]*)\}", re.search(pat, blk).group(1))                 # noqa: E731
        flags = lambda pat: [x.strip() == "true" for x in re.search(pat, blk).group(1).split(",")]     # noqa: E731
        Bm = [_words(m) for m in inner(r" B\[16\]\[3\] = \{(.*)\};")]
        Bn = flags(r"B_NEG\[16\] = \{([^}]*)\}")
        Gm = [_words(m) for m in inner(r" G\[4\]\[7\] = \{(.*)\};")]
        Cn = flags(r"C_NEG\[4\] = \{([^}]*)\}")
        B = [[(-Bm[4 * i + j] if Bn[4 * i + j] else Bm[4 * i + j]) for j in range(4)] for i in range(4)]
        parts = [[], [], [], []]
        for k in ks:
            c = [(-1 if Cn[i] else 1) * ((Gm[i] * k + (1 << 255)) >> 256) for i in range(4)]
            for j in range(4):
                parts[j].append((k if j == 0 else 0) - sum(c[i] * B[i][j] for i in range(4)))
    return parts


def glv_lambda(curve, group):
    name = ("bn254_g2_glv_consts" if (curve, group) == ("bn254", 2) else "%s_glv_consts" % curve) \
        if ws._glv_dim(curve, group) == 2 else "%s_g2_glv4_consts" % curve
    return _words(re.search(r"LAMBDA\[8\] = \{([^}]*)\}", _consts(name)).group(1))


def glv_parts(curve, group, scalars):
    """|k_j| of every scalar, as the sort of a split plain MSM sees them: (DIM n, 4) uint64, part j at rows j n .. (the
    sign travels in bit 255 in the library and only flips a digit's sign: the bucket is the same)."""
    return np.concatenate([ws._to_limbs([abs(v) for v in p]) for p in glv_signed(curve, group, scalars)])


def plain_sort(curve, group, scalars, in_subgroup=True):
    """(geometry, the scalars the plain MSM's sort sees, DIM): the GLV parts where msm_run splits, the scalars otherwise."""
    g, how = ws.plain_geometry(curve, group, len(scalars), in_subgroup)
    if how == "full":
        return g, np.asarray(scalars, dtype=np.uint64), 1
    return g, glv_parts(curve, group, scalars), ws._glv_dim(curve, group)


def pair_buckets(g, sort_scalars, n_base):
    """For each bucket set of geometry g: (live entries, buckets holding EXACTLY the two entries of one pair -- entries
    (window, image, 2i) and (window, image, 2i + 1)).  Such a bucket's accumulator meets its own point (or its negative)
    at its second addition, whatever order the atomics gave the entries."""
    d = ws.digits_np(sort_scalars, g["c"], g["scalar_bits"])
    W, N = d.shape
    bw, log_nb = g["bw"], g["log_nb"]
    e = np.arange(N, dtype=np.int64)
    base, img = e % n_base, e // n_base
    half = (n_base + 1) // 2
    paired = (base // 2 * 2 + 1 < n_base)
    live_tot = np.zeros(bw, dtype=np.int64)
    alone = np.zeros(bw, dtype=np.int64)
    keys, pids, ok = [], [], []
    for w in range(W):
        nz = d[w] != 0
        keys.append((((w % bw) << log_nb) + np.abs(d[w][nz]) - 1).astype(np.int64))
        pids.append(((w * (N // n_base) + img[nz]) * half + base[nz] // 2).astype(np.int64))
        ok.append(paired[nz])
    key, pid, okk = np.concatenate(keys), np.concatenate(pids), np.concatenate(ok)
    order = np.argsort(key, kind="stable")
    key, pid, okk = key[order], pid[order], okk[order]
    uniq, first, cnt = np.unique(key, return_index=True, return_counts=True)
    two = cnt == 2
    f = first[two]
    good = (pid[f] == pid[f + 1]) & okk[f]
    np.add.at(alone, uniq[two][good] >> log_nb, 1)
    np.add.at(live_tot, uniq >> log_nb, cnt)
    return live_tot, alone


# ---- the GPU cases (tests/test_gpu_key_shapes.py runs them, tests/test_key_shapes.py mirrors them) -------------------
SEEDS = {"rows": 300, "plain": 41, "resident": 42, "budget": 43, "alias": 44, "proof": 45}
N_DIRECT, N_PARTITIONED = 1 << 10, (1 << 14) + 37            # the direct atomic sort / the LDS-partitioned sort

BASE_SHAPES = ("pairs", "opposites", "identity_frac", "identity_block64", "identity_block256", "real_key", "chain")


def make_bases(shape, curve, group, rows, seed=0, mul=None):
    """The bases of `shape` from n distinct rows.  Returns (bases, live) with live None but for the identity shapes."""
    n = len(rows)
    if shape == "pairs":
        return pairs(rows), None
    if shape == "opposites":
        return opposites(curve, group, rows), None
    if shape.startswith("identity_"):
        block = 1 if shape == "identity_frac" else int(shape[len("identity_block"):])
        return identity_heavy(rows, 0.75, block, seed)
    if shape == "real_key":
        return real_key(curve, group, rows, seed), None
    if shape == "chain":
        return chain(curve, group, rows[:1], n, mul), None
    if shape == "all_equal":
        return all_equal(rows[0], n), None
    if shape == "alternating":
        return alternating(curve, group, rows[0], n), None
    raise ValueError(shape)


def plain_scalar_kind(shape, n):
    """(a): pairs and opposites take `same` at 2^10 and `sparse_live` at 2^14 + 37, the other shapes dense scalars."""
    if shape in ("pairs", "opposites"):
        return "same" if n == N_DIRECT else "sparse_live"
    return "dense"


def plain_sparse_k(curve, group, n, in_subgroup):
    """sparse_live_k of the plain sort.  The quarters of a BLS G2 scalar (65 bits in 12-bit windows) leave the top window
    6 bits -- 2^5 reachable buckets, whatever the window's 2^log_nb: there k is sized against those instead, so that the
    4 k pair images of the top window fill at most a quarter of them and a pair is alone in a bucket of EVERY window."""
    g, how = ws.plain_geometry(curve, group, n, in_subgroup)
    dim = {"full": 1, "glv2": 2, "glv4": 4}[how]
    k = sparse_live_k(g, 2 * dim)
    if dim == 4:
        top_bits = g["scalar_bits"] + 1 - (g["nwin"] - 1) * g["c"]
        k = min(k, max(1, (1 << (top_bits - 1)) // (4 * dim)))
    return k


def plain_scalars(curve, group, n, shape, in_subgroup):
    kind = plain_scalar_kind(shape, n)
    k = plain_sparse_k(curve, group, n, in_subgroup) if kind == "sparse_live" else 0
    return kind, scalars_of(kind, curve, n, SEEDS["plain"], k)


PLAIN = [(c, g, n, s) for (c, g) in GROUPS for n in (N_DIRECT, N_PARTITIONED) for s in BASE_SHAPES]

# one point n times / P, -P, ..: (curve, group, n, shape, scalar kind); 2^20 by closed forms only
ONE_POINT = [("bn254", 1, 1 << 12, "all_equal", "dense")]
ONE_POINT += [(c, g, 1 << 16, s, "ones") for (c, g) in GROUPS[:4] for s in ("all_equal", "alternating")]
ONE_POINT += [(c, g, 1 << 20, s, "ones") for (c, g) in GROUPS[:2] for s in ("all_equal", "alternating")]

RESIDENT_SIZES = [("bn254", 1, 1 << 13), ("bn254", 1, 1 << 16), ("bn254", 2, 1 << 13), ("bls12_381", 1, 1 << 14),
                  ("bls12_381", 2, 1 << 12), ("bls12_377", 1, 1 << 13), ("bls12_377", 2, 1 << 12)]
RESIDENT_SHAPES = BASE_SHAPES + ("all_equal", "alternating")
RESIDENT = [(c, g, n, s) for (c, g, n) in RESIDENT_SIZES for s in RESIDENT_SHAPES]


def resident_scalar_kinds(shape):
    if shape in ("pairs", "opposites"):
        return ("same", "sparse_live", "bits")
    if shape in ("all_equal", "alternating"):
        return ("ones", "dense")
    return ("dense", "bits", "const")


def table_geometry(curve, n, stride=1, c=0):
    bits = ws.SCALAR_BITS[curve]
    return ws.geometry(n, bits, True, c or ws.window_bits(n, True, bits), stride)


def resident_scalars(curve, n, kind, g):
    return scalars_of(kind, curve, n, SEEDS["resident"], sparse_live_k(g, 2))


# thinned tables: (curve, group, n, table rows the budget pays for, base shape, scalar kinds)
THINNED = [("bn254", 1, 1 << 14, 3, "real_key", ("dense", "bits")),
           ("bn254", 1, 1 << 14, 3, "pairs", ("same", "sparse_live")),
           ("bls12_381", 2, 1 << 12, 4, "real_key", ("dense", "bits"))]


def thinned_stride(curve, n, rows):
    """The stride a budget of `rows` table rows leaves: every stride-th window's row is kept."""
    g = table_geometry(curve, n)
    return (g["nwin"] + rows - 1) // rows


# row aliasing on chain bases: (curve, group, n, triples)
ALIAS = [("bn254", 1, 1 << 13, 300), ("bls12_381", 2, 1 << 12, 200)]


def alias_triples(curve, n, c, count, seed=0):
    """`count` triples (i, j, d), 1 <= d < 2^(c-1), j >= 1, d 2^(c j) < r, every index i and i + c j used once."""
    r = modulus(curve)
    nwin = ws.nwin_of(c, ws.SCALAR_BITS[curve])
    rng = np.random.default_rng([seed, n, c])
    used, out = set(), []
    while len(out) < count:
        j = int(rng.integers(1, nwin))
        i = int(rng.integers(0, n - c * j))
        dmax = min(1 << (c - 1), r >> (c * j))
        if dmax < 2 or i in used or i + c * j in used:
            continue
        d = int(rng.integers(1, dmax))
        used.update((i, i + c * j))
        out.append((i, j, d))
    return out


def alias_scalars(curve, n, c, triples, twin):
    """k[i] = d 2^(c j), k[i + c j] = d -- or, for the negative twin, 2^c - d (digits -d, +1)."""
    k = [0] * n
    for i, j, d in triples:
        k[i] = d << (c * j)
        k[i + c * j] = ((1 << c) - d) if twin else d
    return ws._to_limbs(k)


def alias_closed_form(curve, c, triples, twin):
    """The scalar of P_0 both ways: sum 2 d 2^(c j) 2^i, or for the twin sum 2^c 2^(i + c j) (what bucket 1 of row 1 keeps)."""
    r = modulus(curve)
    if twin:
        return sum(pow(2, i + c * j + c, r) for i, j, _ in triples) % r
    return sum(2 * d * pow(2, c * j + i, r) for i, j, d in triples) % r


# whole proofs: (curve, log_m, Workload shape, key shape, table budget as a fraction of the full tables or None)
CONFIG4 = dict(nv=29823, nc=29400, ni=2)
PROOFS = [("bn254", 15, CONFIG4, "real", None), ("bn254", 15, CONFIG4, "chain", None),
          ("bn254", 15, CONFIG4, "degenerate", None), ("bn254", 16, {}, "real", None),
          ("bn254", 14, {}, "real", 0.26),
          ("bls12_381", 12, {}, "real", None), ("bls12_381", 12, {}, "degenerate", None),
          ("bls12_381", 14, {}, "real", None), ("bls12_381", 14, {}, "degenerate", None)]
PROOFS_377 = [(12, "real"), (12, "chain")]
PROOF_SEPARATE = ("bn254", 16, "real")          # three separate A / B1 / L launches: DG16_ABL_MERGED=0 in a child process
SHARDED = ("bn254", 12, "real", 2)              # groth16_msms per shard + groth16_assemble
PROOF_WITNESSES = ("dense", "bits")
RS_ZERO_CASES = {("bn254", 15, "real"), ("bls12_381", 12, "real"), ("bls12_377", 12, "real")}   # also r = s = 0


def proof_nv(log_m, shape):
    return shape.get("nv", 1 << log_m)


def real_masks(nv, seed=0):
    """The identity rows of a *real* key: b1q and b2q on the SAME 70 % of the wires, aq on 30 %."""
    rng = np.random.default_rng([seed, nv, 5])
    return rng.random(nv) < 0.70, rng.random(nv) < 0.30


def with_copies(rows, frac, seed=0):
    """A fraction of the rows replaced by copies of an earlier row."""
    n = len(rows)
    rng = np.random.default_rng([seed, n, 9])
    out = np.array(rows, copy=True)
    idx = np.nonzero((rng.random(n) < frac) & (np.arange(n) > 0))[0]
    src = (rng.random(len(idx)) * idx).astype(np.int64)
    for i, j in zip(idx, src):
        out[i] = out[j]
    return out


def key_queries(shape, curve, q, seed=0, mul=None):
    """q: dict a, b1, b2, h, l -> distinct host rows (group 2 for b2).  Returns the five queries of key shape `shape`."""
    grp = {"a": 1, "b1": 1, "b2": 2, "h": 1, "l": 1}
    out = {k: np.array(v, copy=True) for k, v in q.items()}
    if shape == "real":
        b_dead, a_dead = real_masks(len(q["a"]), seed)
        out["b1"][b_dead] = 0
        out["b2"][b_dead] = 0
        out["a"][a_dead] = 0
        out["l"] = with_copies(q["l"], 0.05, seed)
    elif shape == "chain":
        for k in out:
            out[k] = chain(curve, grp[k], q[k][:1], len(q[k]), None if mul is None else (lambda s, b, g=grp[k]: mul(g, s, b)))
    elif shape == "degenerate":
        for k in out:
            out[k] = all_equal(q[k][0], len(q[k]))
        out["b2"] = alternating(curve, 2, q["b2"][0], len(q["b2"]))
    else:
        raise ValueError(shape)
    return out


def proof_witness(curve, nv, kind, i):
    """w[1:] of the i-th witness of a proof case."""
    return scalars_of(kind, curve, nv - 1, SEEDS["proof"] + i)
