"""The helpers of test_gpu_key_shapes.py, on the host: the key-shaped bases are what they claim, their closed forms agree
with the oracle's two MSMs (Pippenger and double-and-add), and the mirror of the sort (GLV parts, signed digits, bucket
sets: witness_shapes.py + key_shapes.py) puts each GPU case where that file's docstrings say -- a pair alone in a bucket
of every bucket set, one bucket of equal full segments past the giant threshold, two table rows of one chain point in one
bucket, the merged or the separate A / B1 / L launches.  The cases are imported from key_shapes.py, like the GPU file's."""

import numpy as np
import pytest

from oracle import corc
import key_shapes as ks
import witness_shapes as ws


def _rows(curve, group, n, seed=7):
    return corc.gen_points(curve, group, seed, n)


def _msm_both(curve, group, bases, sc):
    a0 = corc.msm(curve, group, bases, sc, algo=0)
    a1 = corc.msm(curve, group, bases, sc, algo=1)
    assert np.array_equal(a0, a1)
    return a0


# ---- shapes and closed forms ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,group", ks.GROUPS)
def test_closed_forms_agree_with_both_oracle_msms(curve, group):
    n = 256
    rows = _rows(curve, group, n)
    same = ks.same(curve, n, 1)
    assert np.array_equal(same[0::2], same[1::2]) and len({tuple(r) for r in same[0::2]}) == n // 2
    ones = ws.shape(curve, n, "ones")
    dense = ws.dense(curve, n, 2)

    p = ks.pairs(rows)
    assert np.array_equal(p[0::2], p[1::2]) and np.array_equal(p[0::2], rows[0::2])
    half = _msm_both(curve, group, rows[0::2], same[0::2])
    assert np.array_equal(_msm_both(curve, group, p, same), corc.point_add(curve, group, half, half))

    o = ks.opposites(curve, group, rows)
    assert all(corc.on_curve(curve, group, o[i:i + 1]) for i in (1, 3, n - 1))
    assert not corc.point_add(curve, group, o[0:1], o[1:2]).any() and not np.array_equal(o[0], o[1])
    assert not _msm_both(curve, group, o, same).any()

    alt = ks.alternating(curve, group, rows[0], n)
    assert np.array_equal(alt[0], alt[2]) and np.array_equal(alt[1], alt[3]) and not np.array_equal(alt[0], alt[1])
    assert not _msm_both(curve, group, alt, ones).any()

    eq = ks.all_equal(rows[0], n)
    assert np.array_equal(_msm_both(curve, group, eq, dense), corc.point_mul(curve, group, rows[:1], ks.sum_mod_r(curve, dense)))
    assert np.array_equal(_msm_both(curve, group, eq, ones), corc.point_mul(curve, group, rows[:1], n))

    ch = ks.chain(curve, group, rows[:1], n)
    assert np.array_equal(ch[5:6], corc.point_mul(curve, group, rows[:1], 32)) and corc.on_curve(curve, group, ch[n - 1:n])
    assert np.array_equal(_msm_both(curve, group, ch, dense),
                          corc.point_mul(curve, group, rows[:1], ks.chain_scalar(curve, dense)))

    for block in (1, 64):
        ih, live = ks.identity_heavy(rows, 0.75, block, 3)
        assert live.sum() == n // 4 and not ih[~live].any() and np.array_equal(ih[live], rows[live])
        if block > 1:
            assert all(len(set(live[b:b + block])) == 1 for b in range(0, n, block))
        assert np.array_equal(_msm_both(curve, group, ih, dense), _msm_both(curve, group, rows[live], dense[live]))

    _msm_both(curve, group, ks.real_key(curve, group, rows, 4), dense)


@pytest.mark.parametrize("curve,group", [("bn254", 1), ("bls12_381", 2)])
def test_real_key_has_its_fractions(curve, group):
    n = 2000
    rows = _rows(curve, group, n)
    rk = ks.real_key(curve, group, rows, 1)
    dead = ~rk.any(axis=1)
    assert 0.57 < dead.mean() < 0.63                          # the copies and negatives are live points
    own = np.array([np.array_equal(rk[i], rows[i]) for i in range(n)])
    assert 0.25 < own.mean() < 0.31
    index = {tuple(r): i for i, r in reversed(list(enumerate(rk)))}      # first occurrence
    neg = ks.negate(curve, group, rk)
    copies = sum(1 for i in range(n) if not dead[i] and index[tuple(rk[i])] < i)
    negs = sum(1 for i in range(n) if not dead[i] and index.get(tuple(neg[i]), n) < i)
    assert 0.08 * n <= copies <= 0.12 * n and 0.012 * n <= negs <= 0.03 * n, (copies, negs)
    assert all(corc.on_curve(curve, group, rk[i:i + 1]) for i in np.nonzero(~dead & ~own)[0][:20])
    assert np.array_equal(rk, ks.real_key(curve, group, rows, 1))         # seeded


def test_chain_with_a_multiplier_is_pinned_to_doublings():
    curve, group, n = "bn254", 1, 100
    rows = _rows(curve, group, 1)

    def mul(sc, base):
        return np.concatenate([corc.point_mul(curve, group, base, k) for k in ws.to_ints(sc)])

    assert np.array_equal(ks.chain(curve, group, rows, n, mul), ks.chain(curve, group, rows, n))
    with pytest.raises(AssertionError):
        ks.chain(curve, group, rows, n, lambda sc, base: mul(sc, corc.point_add(curve, group, base, base)))


@pytest.mark.parametrize("curve,group", ks.GROUPS)
def test_glv_mirror_recomposes_the_scalar(curve, group):
    """sum_j k_j LAMBDA^j = k mod r with the signed parts, the magnitudes the sort sees within its bit bounds, pair members
    equal."""
    n = 64
    sc = ks.same(curve, n, 5)
    dim = ws._glv_dim(curve, group)
    signed = ks.glv_signed(curve, group, sc)
    parts = ks.glv_parts(curve, group, sc)
    assert len(signed) == dim and parts.shape == (dim * n, 4) and np.array_equal(parts[0::2], parts[1::2])
    lam, r = ks.glv_lambda(curve, group), ks.modulus(curve)
    vals = ws.to_ints(parts)
    for i, k in enumerate(ws.to_ints(sc)):
        p = [signed[j][i] for j in range(dim)]
        assert sum(v * pow(lam, j, r) for j, v in enumerate(p)) % r == k
        assert [abs(v) for v in p] == [vals[j * n + i] for j in range(dim)]
        assert all(abs(v) < 1 << (127 if dim == 2 else 65) for v in p)


# ---- what each GPU case reaches ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,group", ks.GROUPS)
def test_plain_sparse_live_leaves_a_pair_alone_in_every_bucket_window(curve, group):
    """(a) at 2^14 + 37, pairs and opposites: in EVERY window of the sort (the GLV parts' where msm_run splits) at least one
    bucket holds exactly the two entries of one pair -- its second addition is P + P (pairs) or P + (-P) (opposites) -- and
    the live entries of a window fill at most 1/8 of its buckets (of the 2^5 the top window of a quarter split can reach:
    at most half)."""
    n = ks.N_PARTITIONED
    for sub in ks.subgroup_flags(curve, group):
        kind, sc = ks.plain_scalars(curve, group, n, "pairs", sub)
        assert kind == "sparse_live" and np.array_equal(sc, ks.plain_scalars(curve, group, n, "opposites", sub)[1])
        g, sort_sc, dim = ks.plain_sort(curve, group, sc, sub)
        assert g["nwin"] * g["n"] >= 1 << 18                                   # the LDS-partitioned sort
        assert dim == (1 if not (sub or ks.cofactor_one(curve, group)) else ws._glv_dim(curve, group))
        live, alone = ks.pair_buckets(g, sort_sc, n)
        assert len(alone) == g["nwin"] and (alone >= 1).all(), (sub, alone)
        assert (live <= (1 << g["log_nb"]) // 8).all() and (live > 0).all(), (sub, live)
        if dim == 4:
            # the quarters' top window has 6 bits, 2^5 reachable buckets: k is sized against those (plain_sparse_k)
            top_bits = g["scalar_bits"] + 1 - (g["nwin"] - 1) * g["c"]
            assert top_bits == 6 and live[-1] <= 2 * dim * ks.plain_sparse_k(curve, group, n, sub) <= (1 << (top_bits - 1)) // 2


def test_plain_grid_sizes_take_both_sorts():
    for curve, group in ks.GROUPS:
        for sub in ks.subgroup_flags(curve, group):
            g = ws.plain_geometry(curve, group, ks.N_DIRECT, sub)[0]
            assert g["nwin"] * g["n"] < 1 << 18                                # the direct atomic sort
    assert {(c, g, n) for c, g, n, _ in ks.PLAIN} == {(c, g, n) for c, g in ks.GROUPS for n in (1 << 10, (1 << 14) + 37)}
    assert {s for *_, s in ks.PLAIN} == set(ks.BASE_SHAPES)


@pytest.mark.parametrize("curve,group,n,shape,kind", [c for c in ks.ONE_POINT if c[4] == "ones"])
def test_one_point_with_ones_is_one_bucket_of_equal_full_segments(curve, group, n, shape, kind):
    """all_equal / alternating with `ones`: all n entries in bucket 1 of window 0, in n / 2^seg_log FULL segments (every
    segment partial is 2^seg_log P, or the identity when the points alternate).  Without the tree that is one partial per
    segment: a giant (> 64 partials; at 2^20 also slices of > 512 partials).  BN254 G1 adds 256 segments per workgroup:
    a stitched bucket at 2^16 (16 partials), a giant through the stitch kernel at 2^20 (256)."""
    sc = ws.shape(curve, n, "ones")
    p = ws.plain_regime(curve, group, sc, True)
    seg = 1 << p["seg_log"]
    assert p["nonempty"] == 1 and p["max_count"] == n and n % seg == 0
    nseg = n // seg
    assert p["seg_log"] == 4 and nseg == {1 << 16: 4096, 1 << 20: 65536}[n]
    if ks.cofactor_one(curve, group):
        assert p["max_np"] == nseg // 256                    # the first bucket of the set: workgroup-aligned
        assert (p["giants"], p["stitched"]) == ((0, 1) if n == 1 << 16 else (1, 0)), p
    else:
        assert p["max_np"] == nseg > ws.K_GIANT_SEGS and p["giants"] == 1, p
        assert (p["max_per"] > ws.K_GIANT_SLICE_SEGS) == (n == 1 << 20), p
    if not ks.cofactor_one(curve, group) and n == 1 << 16:                      # without the flag: the full-width sort
        q = ws.plain_regime(curve, group, sc, False)
        assert q["nonempty"] == 1 and q["giants"] == 1 and q["max_count"] == n, q


def test_all_equal_at_2e12_takes_the_split_path():
    c, g, n, shape, kind = ks.ONE_POINT[0]
    assert (c, g, n, shape, kind) == ("bn254", 1, 1 << 12, "all_equal", "dense")
    assert ws.plain_geometry(c, g, n, False)[1] == "glv2"


@pytest.mark.parametrize("curve,group,n", ks.RESIDENT_SIZES)
def test_resident_sparse_live_leaves_a_pair_alone_in_the_bucket_set(curve, group, n):
    g = ks.table_geometry(curve, n)
    assert g["bw"] == 1 and g["c"] == ws.window_bits(n, True, ws.SCALAR_BITS[curve])
    sc = ks.resident_scalars(curve, n, "sparse_live", g)
    live, alone = ks.pair_buckets(g, sc, n)
    assert alone[0] >= 1 and 0 < live[0] <= (1 << g["log_nb"]) // 8, (live, alone)
    assert {(c, g_, n_) for c, g_, n_, _ in ks.RESIDENT} == set(ks.RESIDENT_SIZES)


@pytest.mark.parametrize("curve,group,n,rows,shape,kinds", ks.THINNED)
def test_thinned_tables_have_several_bucket_sets(curve, group, n, rows, shape, kinds):
    stride = ks.thinned_stride(curve, n, rows)
    g = ks.table_geometry(curve, n, stride)
    assert stride > 1 and g["bw"] == stride and g["rows"] <= rows and g["rows"] > 1          # sets + the Horner tail
    if "sparse_live" in kinds:
        sc = ks.scalars_of("sparse_live", curve, n, ks.SEEDS["budget"], ks.sparse_live_k(g, 2))
        live, alone = ks.pair_buckets(g, sc, n)
        assert len(alone) == stride and (alone >= 1).all() and (live <= (1 << g["log_nb"]) // 8).all(), (live, alone)
    for kind in kinds:
        # which bucket sets the Horner tail folds: all of them live, or (bits: window 0 alone) every set but the first EMPTY
        live, _ = ks.pair_buckets(g, ks.scalars_of(kind, curve, n, ks.SEEDS["budget"], ks.sparse_live_k(g, 2)), n)
        assert live[0] > 0 and ((live[1:] == 0).all() if kind == "bits" else (live[1:] > 0).all()), (kind, live)


@pytest.mark.parametrize("curve,group,n,count", ks.ALIAS)
def test_row_aliasing_puts_one_point_twice_into_one_bucket(curve, group, n, count):
    """k[i] = d 2^(c j) has digit d in window j (table row j of P_i = 2^(c j) P_i = P_(i + c j) on a chain) and k[i + c j] = d
    digit d in window 0 (row 0 of P_(i + c j)): with a full table all windows share ONE bucket set, so the same affine point
    enters bucket d twice.  The twin's 2^c - d recodes to digits (-d, +1): bucket d gets P and -P."""
    bits = ws.SCALAR_BITS[curve]
    c = ws.window_bits(n, True, bits)
    g = ks.table_geometry(curve, n)
    assert g["bw"] == 1 and g["c"] == c
    tr = ks.alias_triples(curve, n, c, count, ks.SEEDS["alias"])
    assert len(tr) == count and len({i for i, _, _ in tr} | {i + c * j for i, j, _ in tr}) == 2 * count
    assert {j for _, j, _ in tr} >= set(range(1, ws.nwin_of(c, bits) - 1))          # every table row but the top one
    r = ks.modulus(curve)
    for twin in (False, True):
        k = ws.to_ints(ks.alias_scalars(curve, n, c, tr, twin))
        assert all(v < r for v in k) and sum(1 for v in k if v) == 2 * count
        for i, j, d in tr:
            assert 1 <= d < 1 << (c - 1) and j >= 1
            di = ws.digits(k[i], c, bits)
            assert di[j] == d and not any(di[:j]) and not any(di[j + 1:])
            dm = ws.digits(k[i + c * j], c, bits)
            assert dm[0] == (-d if twin else d) and dm[1] == (1 if twin else 0) and not any(dm[2:])


def test_row_aliasing_closed_form_on_a_small_chain():
    curve, group, n = "bn254", 1, 512
    c = ws.window_bits(n, True, 254)
    p0 = _rows(curve, group, 1, 9)
    ch = ks.chain(curve, group, p0, n)
    tr = ks.alias_triples(curve, n, c, 40, 1)
    i, j, _ = tr[0]
    assert np.array_equal(ch[i + c * j:i + c * j + 1], corc.point_mul(curve, group, ch[i:i + 1], 1 << (c * j)))
    for twin in (False, True):
        sc = ks.alias_scalars(curve, n, c, tr, twin)
        assert np.array_equal(_msm_both(curve, group, ch, sc),
                              corc.point_mul(curve, group, p0, ks.alias_closed_form(curve, c, tr, twin)))


def test_which_proofs_merge_the_a_b1_l_launch():
    """prover_impl.h merges A, B1 and L into one three-instance launch while region * bw <= 2^22 -- every full-table key of
    at most 2^16 wires here, the config-4 shape and 2^16 included; three separate launches would need a key of more than
    2^17 wires, beyond what the oracle proves in seconds, so ONE case pins them with DG16_ABL_MERGED=0 in a child process."""
    for curve, log_m, shape, key, budget in ks.PROOFS:
        nv = ks.proof_nv(log_m, shape)
        if budget is None:
            assert ws.prover_abl_merged(curve, nv), (curve, log_m)
        else:                                     # a thinned key: merged at whatever stride the budget leaves
            full = ks.table_geometry(curve, nv - 1 + 3)
            for stride in range(2, full["nwin"] + 1):
                g = ks.table_geometry(curve, nv - 1 + 3, stride)
                assert g["bw"] == stride and g["region"] * g["bw"] <= 1 << 22, (curve, log_m, stride)
    assert all(ws.prover_abl_merged("bls12_377", 1 << log_m) for log_m, _ in ks.PROOFS_377)
    assert not ws.prover_abl_merged("bn254", 1 << 18)
    assert ks.PROOF_SEPARATE == ("bn254", 16, "real")
    assert {k for c, m, s, k, b in ks.PROOFS if s is ks.CONFIG4} == {"real", "chain", "degenerate"}


def test_real_proof_key_masks():
    b_dead, a_dead = ks.real_masks(29823, ks.SEEDS["proof"])
    assert 0.68 < b_dead.mean() < 0.72 and 0.28 < a_dead.mean() < 0.32
    rows = _rows("bn254", 1, 400)
    lq = ks.with_copies(rows, 0.05, 1)
    changed = [i for i in range(400) if not np.array_equal(lq[i], rows[i])]
    assert 8 <= len(changed) <= 40 and all(any(np.array_equal(lq[i], lq[j]) for j in range(i)) for i in changed)
