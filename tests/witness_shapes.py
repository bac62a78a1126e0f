"""Witness-shaped scalars and a host mirror of the MSM digit / bucket geometry (plain Python + numpy, no GPU).

A circom witness is mostly bits, some small integers and some field negatives r - k: the scalars of four of the
prover's five MSMs (A, B1, B2, L).  Such scalars put almost every bucket entry into one bucket and leave the others
empty -- paths that uniform random scalars reach only by chance.  This module makes those scalars (`shape`), mirrors
the signed-digit recoding of csrc/msm_sort.h (`digits`, `msm_digit`), builds scalars whose digits sit on the recoding's
edges (`boundary_scalars`), and mirrors the planning arithmetic of csrc/msm_geom.h (`window_bits`, `geometry`,
`plain_geometry`, `giant_slices`; tests/test_msm_geom_host.py holds the two equal) and the partial counts (`bucket_regime`) so that a test can assert which reduction path a GPU case reaches.
"""

import numpy as np

from oracle.pyref.fields import FR

SCALAR_BITS = {"bn254": 254, "bls12_381": 255, "bls12_377": 253}
KINDS = ("bits", "ones", "sparse", "u32", "u64", "neg_small", "const", "sha256_mix", "zero")

# the shape seeds of test_gpu_witness_shapes.py's cases: test_witness_shapes.py mirrors exactly those scalars
SEEDS = {"plain": 1, "giant": 2, "subgroup": 3, "resident": 4, "budget": 5, "proof": 10}

# csrc/msm_geom.h
K_MIN_SEG_LOG, K_MAX_SEG_LOG = 3, 9
K_MIN_LANES_LOG = 18
K_GIANT_SEGS = 64
K_GIANT_SLICES = 64
K_GIANT_SLICE_SEGS = 512


def modulus(curve):
    return FR[curve].p


def _to_limbs(vals):
    """Python ints (< 2^256) -> (n, 4) uint64."""
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        for j in range(4):
            out[i, j] = (v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
    return out


def to_ints(arr):
    arr = np.asarray(arr, dtype=np.uint64).reshape(-1, 4)
    return [int(a) | int(b) << 64 | int(c) << 128 | int(d) << 192 for a, b, c, d in arr]


def _dense(rng, curve, n):
    """Uniform-ish scalars below r: three random limbs and a top limb below r's (what bench.rand_fr draws)."""
    top = modulus(curve) >> 192
    out = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    out[:, 3] = rng.integers(0, top, size=n, dtype=np.uint64)
    return out


def dense(curve, n, seed=0):
    return _dense(np.random.default_rng([seed, n]), curve, n)


def shape(curve, n, kind, seed=0):
    """(n, 4) uint64 canonical scalars below r of the given kind:
      bits        0 / 1, half ones
      ones        all 1 (one bucket of window 0 holds every entry: 2^16 16-entry segments at 2^20 points)
      sparse      98 % zero, the rest 1
      u32, u64    small integers: the upper windows are empty
      neg_small   r - k, k in [1, 4]: every window carries, the top window is r's
      const       one dense value repeated
      sha256_mix  ~90 % bits, 8 % 32-bit words, 2 % dense.  An approximation of a sha256 circuit's witness made up
                  for these tests, NOT measured from a real one.
      zero        all zeros"""
    rng = np.random.default_rng([seed, n, KINDS.index(kind)])
    r = modulus(curve)
    out = np.zeros((n, 4), dtype=np.uint64)
    if kind == "bits":
        out[:, 0] = rng.integers(0, 2, n, dtype=np.uint64)
    elif kind == "ones":
        out[:, 0] = 1
    elif kind == "sparse":
        out[:, 0] = (rng.random(n) < 0.02).astype(np.uint64)
    elif kind == "u32":
        out[:, 0] = rng.integers(0, 2**32, n, dtype=np.uint64)
    elif kind == "u64":
        out[:, 0] = rng.integers(0, 2**64, n, dtype=np.uint64)
    elif kind == "neg_small":
        ks = rng.integers(1, 5, n)
        table = _to_limbs([r - k for k in range(5)])
        out[:] = table[ks]
    elif kind == "const":
        out[:] = _dense(rng, curve, 1)[0]
    elif kind == "sha256_mix":
        u = rng.random(n)
        out[:, 0] = rng.integers(0, 2, n, dtype=np.uint64)
        word = (u >= 0.90) & (u < 0.98)
        out[word, 0] = rng.integers(0, 2**32, int(word.sum()), dtype=np.uint64)
        dense = u >= 0.98
        out[dense] = _dense(rng, curve, int(dense.sum()))
    elif kind != "zero":
        raise ValueError(kind)
    return out


# ---- the signed-digit recoding (csrc/msm_sort.h: msm_digit, msm_digits_kernel) -----------------------------------
def nwin_of(c, bits):
    return (bits + 1 + c - 1) // c          # one spare bit absorbs the last carry


def msm_digit(l32, w, c, carry):
    """Line for line msm_digit: l32 = the scalar's eight 32-bit limbs.  Returns (d, carry)."""
    NL = len(l32)
    half = 1 << (c - 1)
    bit = w * c
    limb, off = bit >> 5, bit & 31
    v = 0
    if limb < NL:
        v = l32[limb]
        if limb + 1 < NL:
            v |= (l32[limb + 1] << 32) & 0xFFFFFFFFFFFFFFFF
        v >>= off
    d = (v & 0xFFFFFFFF & ((1 << c) - 1)) + carry
    if d > half:
        d -= 1 << c
        carry = 1
    else:
        carry = 0
    return d, carry


def digits(k, c, bits):
    """The W = ceil((bits + 1) / c) signed digits the library gives scalar k (an int below 2^256)."""
    l32 = [(k >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
    out, carry = [], 0
    for w in range(nwin_of(c, bits)):
        d, carry = msm_digit(l32, w, c, carry)
        out.append(d)
    return out


def digits_np(scalars, c, bits):
    """digits() for an (n, 4) uint64 array at once: (W, n) int64."""
    s = np.ascontiguousarray(scalars, dtype=np.uint64)
    l32 = s.view(np.uint32).reshape(-1, 8).astype(np.uint64)
    n = l32.shape[0]
    W = nwin_of(c, bits)
    half = 1 << (c - 1)
    mask = np.uint64((1 << c) - 1)
    out = np.empty((W, n), dtype=np.int64)
    carry = np.zeros(n, dtype=np.int64)
    for w in range(W):
        bit = w * c
        limb, off = bit >> 5, bit & 31
        if limb < 8:
            v = l32[:, limb].copy()
            if limb + 1 < 8:
                v |= l32[:, limb + 1] << np.uint64(32)
            v >>= np.uint64(off)
            raw = (v & mask).astype(np.int64)
        else:
            raw = np.zeros(n, dtype=np.int64)
        d = raw + carry
        carry = (d > half).astype(np.int64)
        out[w] = d - (carry << c)
    return out


def boundary_scalars(c, bits, n, curve, seed=0):
    """n scalars below r whose recoded digits sit on the recoding's edges, window by window: a raw window of `half`
    (stays +half), `half + 1` (becomes -(half - 1) and carries), `2^c - 1` with an incoming carry (digit 0, carries on)
    and `0` with an incoming carry (digit 1).  Structured rows first (one pattern in every window, runs of all-ones
    windows, alternations), random mixes of the edge values after them, and r - 1, r - 2 (the largest top window)."""
    r = modulus(curve)
    half, full = 1 << (c - 1), (1 << c) - 1
    nw = (bits - 1) // c                       # whole windows below 2^(bits - 1) < r
    edges = [half - 1, half, half + 1, full, 0]

    def of(raws):
        return sum(v << (c * w) for w, v in enumerate(raws))

    vals = [r - 1, r - 2]
    for v in (half, half + 1, full):
        vals.append(of([v] * nw))
    vals.append(of([half - 1, half] * (nw // 2)))            # half - 1 + no carry, then half
    vals.append(of([full, 0] * (nw // 2)))                   # 0 with an incoming carry -> 1
    vals.append(of([half + 1, full, full, 0] * (nw // 4)))   # a carry run through all-ones windows
    for m in range(1, nw + 1):
        vals.append((1 << (c * m)) - 1)                      # m all-ones windows: one carry run of length m
        vals.append(half << (c * (m - 1)))                   # a lone +half in window m - 1
    vals.append(r - 1 - of([half] * 2))
    rng = np.random.default_rng([seed, c, bits])
    while len(vals) < n:
        vals.append(of([edges[i] for i in rng.integers(0, len(edges), nw)]))
    vals = vals[:n]
    assert all(0 <= v < r for v in vals)
    return _to_limbs(vals)


# ---- geometry (csrc/msm_geom.h: msm_window_bits, msm_geometry; msm_plain_plan: msm_run's choice of width and GLV split) --
def window_bits(n, table, scalar_bits=0):
    lg = max(n, 1).bit_length() - 1
    if n > (3 << lg) // 2:
        lg += 1
    c = lg - 3 if table else lg - 4
    if table and c < 16:
        c = min(lg + 1, 16)
        if scalar_bits and lg >= 13:
            def top(w):
                b = scalar_bits + 1
                return b - ((b + w - 1) // w - 1) * w
            t15, t16 = top(15), top(16)
            if t15 >= t16:
                c = 15 if (t15 > t16 or lg <= 16) else 16
    return max(4, min(20 if table else 16, c))


def _flog2(x):
    return max(int(x), 1).bit_length() - 1


def geometry(n, scalar_bits, table=False, c_fixed=0, stride=1):
    c = c_fixed or window_bits(n, table, scalar_bits if table else 0)
    nwin = (scalar_bits + 1 + c - 1) // c
    log_nb = c - 1
    stride = min(max(stride, 1), nwin)
    bw = stride if table else nwin
    rows = (nwin + bw - 1) // bw
    region = rows * n
    mean = region >> log_nb
    lm = _flog2(mean) if mean >= 2 else 0
    le_all = _flog2(region * bw)
    sl = min(max(le_all - 20, 4), 5)
    sl = max(min(sl, lm - 2), 4)
    le = _flog2(nwin * n)
    cap = le - K_MIN_LANES_LOG
    if not table and le == 20 and cap < 4:
        cap = 4
    sl = min(sl, cap)
    seg_log = min(max(sl, K_MIN_SEG_LOG), K_MAX_SEG_LOG)
    seg_cap = (1 << log_nb) + ((region + (1 << seg_log) - 1) >> seg_log)
    return {"c": c, "nwin": nwin, "log_nb": log_nb, "seg_log": seg_log, "seg_cap": seg_cap, "bw": bw,
            "table": table, "rows": rows, "region": region, "n": n, "scalar_bits": scalar_bits}


def acc_wg_log(curve, group):
    """msm_acc_wg_log: BN254 G1 (36-byte stored coordinates) adds a bucket's partials inside 256-lane accumulation
    workgroups (the tree; one partial per workgroup a bucket spans); every other group leaves one partial per segment."""
    return 8 if (curve, group) == ("bn254", 1) else 0


def _glv_dim(curve, group):
    return 4 if (group == 2 and curve != "bn254") else 2


def plain_geometry(curve, group, n, in_subgroup=True):
    """The sort msm_run makes for a plain dg16_msm of n points: (geometry, how the scalars enter it) where the second
    item is 'glv2' / 'glv4' (split by the endomorphism: DIM n half scalars) or 'full'."""
    bits = SCALAR_BITS[curve]
    glv = (curve, group) == ("bn254", 1) or in_subgroup
    dim = _glv_dim(curve, group)
    if glv and n and dim * n * 40 < (1 << 31):
        if dim == 2:
            c0 = window_bits(2 * n, False)
            c_small = 0
            if curve == "bn254" and c0 in (7, 9):      # nine-limb fields (RR<..>::N == 9)
                c_small = 8
            if c0 in (14, 15):
                c_small = 16
            return geometry(2 * n, 127, False, c_small), "glv2"
        return geometry(4 * n, 65, False), "glv4"
    return geometry(max(n, 1), bits, False), "full"


def _glv_trivial(scalars, dim):
    """The GLV halves / quarters of scalars below 2^64: (k, 0, ..) -- Babai's rounding of k b / r is 0 for every
    lattice vector b of the splits (entries <= 2^128 against r > 2^252).  Larger scalars are not mirrored."""
    s = np.asarray(scalars, dtype=np.uint64)
    assert not s[:, 1:].any(), "the GLV mirror covers scalars below 2^64 only"
    return np.concatenate([s] + [np.zeros_like(s)] * (dim - 1))


def giant_slices(nseg):
    """giant_geometry: a giant bucket's nseg partials in at most K_GIANT_SLICES slices of `per` partials."""
    slices = min((nseg + K_GIANT_SLICE_SEGS - 1) // K_GIANT_SLICE_SEGS, K_GIANT_SLICES)
    per = (nseg + slices - 1) // slices
    return (nseg + per - 1) // per, per


def bucket_regime(g, scalars, wg_log, ninst=1):
    """Which finalize / giant paths the sort of `scalars` (the sort's own input: halves for GLV) reaches in geometry g.
    Mirrors the histogram, the segment-count scan (seg_off) and msm_nparts / giant_geometry."""
    c, bw, log_nb, seg_log = g["c"], g["bw"], g["log_nb"], g["seg_log"]
    d = digits_np(scalars, c, g["scalar_bits"])
    nb = 1 << log_nb
    w_idx = np.repeat(np.arange(d.shape[0]) % bw, d.shape[1])
    flat = d.reshape(-1)
    live = flat != 0
    slots = (w_idx[live] << log_nb) + np.abs(flat[live]) - 1
    counts = np.bincount(slots, minlength=bw * nb).reshape(bw, nb).astype(np.int64)
    k = (counts + (1 << seg_log) - 1) >> seg_log
    first = np.cumsum(k, axis=1) - k                          # exclusive scan per bucket-window
    np_ = np.where(k > 0, ((first + k - 1) >> wg_log) - (first >> wg_log) + 1, 0)
    giants = np_ > K_GIANT_SEGS
    pers = [giant_slices(int(v))[1] for v in np_[giants]]
    return {"c": c, "seg_log": seg_log, "buckets": bw * nb, "nonempty": int((counts > 0).sum()),
            "max_count": int(counts.max()), "max_np": int(np_.max()), "giants": int(giants.sum()) * ninst,
            "max_per": max(pers) if pers else 0, "stitched": int(((np_ >= 2) & ~giants).sum()),
            "entries": int(counts.sum())}


def plain_regime(curve, group, scalars, in_subgroup=True):
    n = len(scalars)
    g, how = plain_geometry(curve, group, n, in_subgroup)
    sc = scalars if how == "full" else _glv_trivial(scalars, 2 if how == "glv2" else 4)
    return bucket_regime(g, sc, acc_wg_log(curve, group))


def table_regime(curve, group, scalars, stride=1, c=0):
    n = len(scalars)
    bits = SCALAR_BITS[curve]
    g = geometry(n, bits, True, c or window_bits(n, True, bits), stride)
    return bucket_regime(g, scalars, acc_wg_log(curve, group))


def prover_ab_scalars(curve, w):
    """The scalars of the prover's A / B1 / B2 / L sort for a one-shard key: w[1 ..] and three dense scalars
    (prover_scalar_prep_kernel; dense stand-ins here -- three entries do not move a bucket's partial count)."""
    rng = np.random.default_rng(3)
    return np.concatenate([np.asarray(w[1:], dtype=np.uint64), _dense(rng, curve, 3)])


def prover_abl_merged(curve, nv):
    """prover_impl.h: A, B1 and L run as three instances of one accumulation launch when region * bw <= 2^22."""
    bits = SCALAR_BITS[curve]
    n = nv - 1 + 3
    g = geometry(n, bits, True, window_bits(n, True, bits))
    return g["region"] * g["bw"] <= (1 << 22)
