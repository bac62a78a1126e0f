"""The helpers of test_gpu_witness_shapes.py, on the host: the witness-shaped scalars are canonical, the digit mirror is
msm_digit's recoding, the boundary scalars carry the digits they are built for, and the geometry mirror puts each GPU
case on the reduction path that file claims for it -- so a later change of csrc/msm_geom.h's geometry fails here
instead of leaving a GPU test that silently stopped reaching its path."""

import numpy as np
import pytest

import witness_shapes as ws

CURVES = ("bn254", "bls12_381", "bls12_377")
WIDTHS = (8, 13, 15, 16, 17)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("kind", ws.KINDS)
def test_every_shape_is_canonical(curve, kind):
    n = 5000
    s = ws.shape(curve, n, kind, 1)
    assert s.shape == (n, 4) and s.dtype == np.uint64
    r = ws.modulus(curve)
    vals = ws.to_ints(s)
    assert all(0 <= v < r for v in vals)
    nz = sum(1 for v in vals if v)
    if kind == "bits":
        assert set(vals) == {0, 1} and 0.45 < nz / n < 0.55
    elif kind == "ones":
        assert set(vals) == {1}
    elif kind == "sparse":
        assert set(vals) <= {0, 1} and 0.01 < nz / n < 0.03
    elif kind == "u32":
        assert max(vals) < 1 << 32 and max(vals) >= 1 << 30
    elif kind == "u64":
        assert max(vals) < 1 << 64 and max(vals) >= 1 << 62
    elif kind == "neg_small":
        assert set(r - v for v in vals) == {1, 2, 3, 4}
    elif kind == "const":
        assert len(set(vals)) == 1 and vals[0] > 1 << 200
    elif kind == "sha256_mix":
        small = sum(1 for v in vals if v < 2)
        word = sum(1 for v in vals if 2 <= v < 1 << 32)
        dense = sum(1 for v in vals if v >= 1 << 32)
        assert 0.87 < small / n < 0.93 and 0.06 < word / n < 0.10 and 0.01 < dense / n < 0.03
    else:
        assert nz == 0


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("c", WIDTHS)
def test_digits_reconstruct_the_scalar(curve, c):
    """sum_w d_w 2^(c w) = k, every digit in [-(2^(c-1) - 1), 2^(c-1)], for every shape and the boundary scalars; the
    vectorised mirror gives the same digits as the line-for-line one."""
    bits = ws.SCALAR_BITS[curve]
    half = 1 << (c - 1)
    rows = [ws.shape(curve, 64, kind, 3) for kind in ws.KINDS] + [ws.boundary_scalars(c, bits, 256, curve)]
    sc = np.concatenate(rows)
    dn = ws.digits_np(sc, c, bits)
    for i, k in enumerate(ws.to_ints(sc)):
        d = ws.digits(k, c, bits)
        assert sum(v << (c * w) for w, v in enumerate(d)) == k
        assert all(-(half - 1) <= v <= half for v in d)
        assert list(dn[:, i]) == d


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("c", WIDTHS)
def test_boundary_scalars_hit_the_recoding_edges(curve, c):
    bits = ws.SCALAR_BITS[curve]
    half, full = 1 << (c - 1), (1 << c) - 1
    sc = ws.boundary_scalars(c, bits, 512, curve)
    vals = ws.to_ints(sc)
    r = ws.modulus(curve)
    assert vals[0] == r - 1 and vals[1] == r - 2
    seen = set()
    W = ws.nwin_of(c, bits)
    for k in vals:
        d = ws.digits(k, c, bits)
        carry = 0
        for w in range(W):
            raw = (k >> (c * w)) & full
            if raw == half and carry == 0:
                assert d[w] == half
                seen.add("half")
            if raw == half + 1 and carry == 0:
                assert d[w] == -(half - 1)
                seen.add("half+1")
            if raw == full and carry == 1:
                assert d[w] == 0
                seen.add("full+carry")
            if raw == 0 and carry == 1:
                assert d[w] == 1
                seen.add("zero+carry")
            carry = 1 if raw + carry > half else 0
        assert carry == 0                                    # the spare bit absorbed the last carry
    assert seen == {"half", "half+1", "full+carry", "zero+carry"}
    # r - 1 has the largest top digit of any scalar below r
    tops = [ws.digits(k, c, bits)[-1] for k in vals]
    assert tops[0] == max(tops) and tops[0] == ws.digits(r - 1, c, bits)[-1]


def test_geometry_mirror_agrees_with_bench_plan():
    import bench
    for n in (1 << 13, (1 << 15) + 7, 1 << 16, 1 << 17, 29825, 1 << 20, (1 << 20) + 2):
        for bits in (253, 254, 255):
            assert ws.window_bits(n, True, bits) == bench.table_window_bits(n, bits)


def _claim_plain(curve, group, n, kind, seed, in_subgroup=True):
    return ws.plain_regime(curve, group, ws.shape(curve, n, kind, ws.SEEDS[seed]), in_subgroup)


def _claim_table(curve, group, n, kind):
    return ws.table_regime(curve, group, ws.shape(curve, n, kind, ws.SEEDS["resident"]))


def _claim_prover(curve, nv, kind, i):
    """The A / B1 / B2 / L sort of test_proof_on_witness_shapes' i-th witness of this key."""
    w = np.zeros((nv, 4), dtype=np.uint64)
    w[0, 0] = 1
    w[1:] = ws.shape(curve, nv - 1, kind, ws.SEEDS["proof"] + i)
    sc = ws.prover_ab_scalars(curve, w)
    return ws.table_regime(curve, 1, sc), ws.table_regime(curve, 2, sc)


def test_regime_bn254_g1_2e20_reaches_the_stitch_giant():
    """BN254 G1 is the one group with the in-workgroup tree: a bucket turns giant only when it spans > 64 accumulation
    workgroups of 256 segments.  A 2^20 bits / ones witness puts ~2^19 / 2^20 entries in one bucket -- in the resident
    key, the plain MSM and the proof's A, B1, L -- and every other bucket of the set is the identity."""
    for kind in ("bits", "ones"):
        t = _claim_table("bn254", 1, 1 << 20, kind)
        assert t["c"] == 17 and t["seg_log"] == 4
        assert t["giants"] == 1 and t["max_np"] > ws.K_GIANT_SEGS, t
        assert t["nonempty"] == 1 and t["buckets"] == 1 << 16, t
        p = _claim_plain("bn254", 1, 1 << 20, kind, "giant")
        assert p["giants"] == 1 and p["max_np"] > ws.K_GIANT_SEGS, p
    for i, kind in enumerate(("bits", "ones")):
        assert not ws.prover_abl_merged("bn254", 1 << 20)                    # three separate A / B1 / L launches
        g1, _ = _claim_prover("bn254", 1 << 20, kind, i)
        assert g1["giants"] == 1 and g1["max_np"] > ws.K_GIANT_SEGS, g1
    # ... and uniform scalars do not: no bucket of a uniform 2^20 table MSM spans more than a few workgroups
    u = ws.table_regime("bn254", 1, ws.dense("bn254", 1 << 20, 1))
    assert u["giants"] == 0 and u["max_np"] <= 3, u


def test_regime_ones_at_2e20_slices_longer_than_512_partials():
    """Without the tree, a giant of more than 64 x 512 partials is cut into 64 slices of per > kGiantSliceSegs: `ones`
    at 2^20 in the plain MSM (BN254 G2, BLS12-381 G1), the resident BN254 G2 key and the proof's B2.  `bits` sits at the
    edge (~2^15 partials): over 2^15 for the plain cases' seed, at or under it for the resident key's and the proof's."""
    for curve, group in (("bls12_381", 1), ("bn254", 2)):
        p = _claim_plain(curve, group, 1 << 20, "ones", "giant")
        assert p["max_np"] > ws.K_GIANT_SLICES * ws.K_GIANT_SLICE_SEGS and p["max_per"] > ws.K_GIANT_SLICE_SEGS, p
        b = _claim_plain(curve, group, 1 << 20, "bits", "giant")
        assert b["giants"] == 1 and b["max_per"] == ws.K_GIANT_SLICE_SEGS + 1, b
    t = _claim_table("bn254", 2, 1 << 20, "ones")
    assert t["max_per"] > ws.K_GIANT_SLICE_SEGS, t
    assert _claim_table("bn254", 2, 1 << 20, "bits")["max_per"] <= ws.K_GIANT_SLICE_SEGS
    _, g2 = _claim_prover("bn254", 1 << 20, "ones", 1)
    assert g2["max_per"] > ws.K_GIANT_SLICE_SEGS, g2
    _, g2 = _claim_prover("bn254", 1 << 20, "bits", 0)
    assert g2["giants"] == 1 and g2["max_per"] <= ws.K_GIANT_SLICE_SEGS, g2


def test_regime_2e17_sixteen_bit_windows():
    """2^17 bits: one bucket of eight 2^15-bucket sets; BN254 G1's tree keeps it to <= 64 workgroups (a stitched sum),
    the other groups leave a giant of one partial per segment."""
    for curve, group in (("bn254", 1), ("bn254", 2), ("bls12_381", 1)):
        p = _claim_plain(curve, group, 1 << 17, "bits", "giant")
        assert p["c"] == 16 and p["nonempty"] == 1 and p["buckets"] == 8 << 15, p
        if group == 1 and curve == "bn254":
            assert p["giants"] == 0 and p["stitched"] == 1, p
        else:
            assert p["giants"] == 1, p


def test_regime_plain_grid_sizes():
    """2^10: the direct atomic sort; 2^14 + 37: the LDS-partitioned sort (W n >= 2^18); 2^16: 16-entry segments in the
    G1 groups (the plain-MSM exception of msm_geometry)."""
    for curve, group in (("bn254", 1), ("bn254", 2), ("bls12_381", 1), ("bls12_381", 2), ("bls12_377", 1),
                         ("bls12_377", 2)):
        g = {n: ws.plain_geometry(curve, group, n)[0] for n in (1 << 10, (1 << 14) + 37, 1 << 16)}
        assert g[1 << 10]["nwin"] * g[1 << 10]["n"] < 1 << 18
        assert g[(1 << 14) + 37]["nwin"] * g[(1 << 14) + 37]["n"] >= 1 << 18
        if group == 1:
            assert g[1 << 16]["seg_log"] == 4


def test_regime_bls12_381_without_the_split_is_the_full_width_sort():
    for group in (1, 2):
        g, how = ws.plain_geometry("bls12_381", group, 1 << 14, in_subgroup=False)
        assert how == "full" and g["scalar_bits"] == 255
        p = _claim_plain("bls12_381", group, 1 << 14, "bits", "subgroup", in_subgroup=False)
        assert p["giants"] == 1, p


def test_regime_prover_merged_launch():
    """Config 4 (2^15, 29 823 wires) runs A, B1, L as one three-instance launch with one giant list.  On a bits or
    sha256-like witness the BN254 G1 tree keeps the big bucket within <= 64 workgroups (a stitched sum: that shared
    giant list stays empty); B2 (G2, no tree) has a giant."""
    assert ws.prover_abl_merged("bn254", 29823) and ws.prover_abl_merged("bn254", 1 << 16)
    for i, kind in enumerate(("sha256_mix", "bits")):
        g1, g2 = _claim_prover("bn254", 29823, kind, i)
        assert g1["giants"] == 0 and g1["stitched"] >= 1, g1
        assert g2["giants"] >= 1, g2
