"""The batched point codec on the GPU (csrc/ark_codec.hip: csrc/codec_impl.h compiled for gfx950) on the inputs of
tests/codec_cases.py -- the branches random subgroup points never take (right-hand sides in Fq, y next to q / 2, a root
y = 0), every error code, and the error word (an atomicMin over (index + 1) << 8 | code) with several failing points,
outside the first workgroup and in the tail block.  The expected bytes and points are the plain-Python encoders'; the
host compilation of the same text is shown to agree with them in tests/test_codec_cases.py.  Every comparison is byte
or array equality.

Not covered here: the Python wrappers arkkey.py / zkey.py / r1cs.py around the codec (tests/test_arkkey.py runs them on
ordinary keys)."""

import ctypes
import random
import struct

import numpy as np
import pytest

import ark_points_py as A
import codec_cases as K
import dg16_amd
from dg16_amd import lib
from gpu_util import ctx
from oracle import corc
from oracle.pyref.curves import CURVES
from oracle.pyref.fields import FQ, FR

pytestmark = pytest.mark.gpu

PAIRS = [(c, g) for c in K.CURVE_NAMES for g in (1, 2)]


def _material(curve, group):
    cases = K.valid_points(curve, group)
    pts = [P for _, P, _ in cases]
    inside = [ins for _, _, ins in cases]
    return pts, inside, K.affine_arr(curve, group, pts), [K.encode(curve, group, P) for P in pts]


def _cyclic(rows, n):
    return [rows[i % len(rows)] for i in range(n)]


# ---- compress / decompress against Python ---------------------------------------------------------------------------
@pytest.mark.parametrize("curve,group", PAIRS)
def test_compress_and_decompress_agree_with_python(curve, group):
    c = ctx()
    pts, inside, arr, raws = _material(curve, group)
    want = b"".join(raws)
    assert c.points_compress(curve, group, arr) == want
    assert np.array_equal(c.points_decompress(curve, group, want, validate=False), arr)
    sel = np.array(inside)
    assert np.array_equal(c.points_decompress(curve, group, b"".join(r for r, ins in zip(raws, inside) if ins), validate=True),
                          arr[sel])
    outside = [k for k, ins in enumerate(inside) if not ins]
    assert outside or (curve, group) == ("bn254", 1)
    for k in outside:
        with pytest.raises(dg16_amd.Dg16Error, match="subgroup"):
            c.points_decompress(curve, group, raws[k], validate=True)
    for label, raw, code, validate in K.malformed(curve, group):
        with pytest.raises(dg16_amd.Dg16Error) as e:
            c.points_decompress(curve, group, raw, validate=validate)
        assert K.ERR_TEXT[code] in str(e.value) and "(point 0)" in str(e.value), label


def test_order_two_point_decodes_to_y_zero_with_either_sign_flag():
    """BLS12-377 G1's T = (q - 1, 0): the host code accepts the string with and without the sign flag (both roots are
    equal), as arkworks does; the GPU must equal the host."""
    c = ctx()
    T = K.affine_arr("bls12_377", 1, [K.order2_point()])
    plain, flagged = K.order2_strings()
    assert c.points_compress("bls12_377", 1, T) == plain
    for raw in (plain, flagged):
        assert np.array_equal(c.points_decompress("bls12_377", 1, raw, validate=False), T)
        with pytest.raises(dg16_amd.Dg16Error, match="subgroup"):
            c.points_decompress("bls12_377", 1, raw, validate=True)


@pytest.mark.parametrize("curve,group", PAIRS)
def test_batch_shapes(curve, group):
    """n = 0, one lane, one short of / exactly / one more than a 64-lane workgroup, and 1000 (15 workgroups and a tail of
    40), the case list repeated cyclically."""
    c = ctx()
    pts, inside, arr, raws = _material(curve, group)
    in_idx = [k for k, ins in enumerate(inside) if ins]
    for n in (0, 1, 63, 64, 65, 1000):
        idx = _cyclic(list(range(len(pts)))[::-1], n)                 # from the back: the special points come first
        a = arr[idx] if n else arr[:0]
        want = b"".join(raws[k] for k in idx)
        assert c.points_compress(curve, group, a) == want, n
        got = c.points_decompress(curve, group, want, validate=False)
        assert got.shape == a.shape and np.array_equal(got, a), n
        idx = _cyclic(in_idx, n)
        got = c.points_decompress(curve, group, b"".join(raws[k] for k in idx), validate=True)
        assert np.array_equal(got, arr[idx] if n else arr[:0]), n


# ---- the error word ------------------------------------------------------------------------------------------------------
def _decompress_dev(c, curve, group, raws, validate=False):
    """points_decompress_dev on a batch; the output buffer starts as 0xAB bytes.  (error text or None, rows)."""
    import torch
    dev = torch.device("cuda", 0)
    n = len(raws)
    pb = 2 * K.fb(curve) * group
    din = torch.from_numpy(np.frombuffer(b"".join(raws), dtype=np.uint8).copy()).to(dev)
    dout = torch.full((n * pb,), 0xAB, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    err = None
    try:
        c.points_decompress_dev(curve, group, din.data_ptr(), n, dout.data_ptr(), validate=validate)
    except dg16_amd.Dg16Error as e:
        err = str(e)
        assert c.L.dg16_codec_error().decode() in err
    c.sync(0)
    return err, dout.cpu().numpy().view(np.uint64).reshape(n, -1)


@pytest.mark.parametrize("curve,group", PAIRS)
def test_error_word_with_several_failing_points(curve, group):
    c = ctx()
    pts, inside, arr, raws = _material(curve, group)
    n = 1000
    idx = _cyclic(list(range(len(pts))), n)
    good = [raws[k] for k in idx]
    want = arr[idx]
    bad = {700: 1, 130: 3, 70: 2}
    batch = list(good)
    for at, code in bad.items():
        batch[at] = K.malformed_with_code(curve, group, code)
    err, rows = _decompress_dev(c, curve, group, batch)
    assert err is not None and "(point 70)" in err and "coordinate not reduced" in err
    keep = np.ones(n, dtype=bool)
    keep[list(bad)] = False
    assert not rows[~keep].any()
    assert np.array_equal(rows[keep], want[keep])
    # the context is not poisoned: a clean batch succeeds
    err, rows = _decompress_dev(c, curve, group, good)
    assert err is None and np.array_equal(rows, want)
    # the only bad point in the last lane of the tail block (1000 = 15 * 64 + 40)
    batch = list(good)
    batch[999] = K.malformed_with_code(curve, group, 3)
    err, rows = _decompress_dev(c, curve, group, batch)
    assert err is not None and "(point 999)" in err and "x is not on the curve" in err
    assert not rows[999].any() and np.array_equal(rows[:999], want[:999])
    err, rows = _decompress_dev(c, curve, group, good)
    assert err is None and np.array_equal(rows, want)


# ---- Vec<Fr> on the wire ----------------------------------------------------------------------------------------------------
def _wire(vals):
    return struct.pack("<Q", len(vals)) + b"".join(v.to_bytes(32, "little") for v in vals)


def _wire_decode_dev(c, curve, raw):
    """dg16_wire_fr_decode on device pointers: (return code, error text, n, rows)."""
    import torch
    dev = torch.device("cuda", 0)
    n_max = (len(raw) - 8) // 32
    din = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(dev)
    dout = torch.full((max(n_max, 1) * 32,), 0xAB, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    n = ctypes.c_size_t()
    rc = c.L.dg16_wire_fr_decode(c.h, lib.CURVES[curve], ctypes.c_void_p(din.data_ptr()), len(raw),
                                 ctypes.c_void_p(dout.data_ptr()), ctypes.byref(n), lib.F_DEVICE_PTRS, 0)
    text = c.L.dg16_last_error(c.h).decode() if rc else ""
    c.sync(0)
    return rc, text, n.value, dout.cpu().numpy().view(np.uint64).reshape(-1, 4)[:n_max]


@pytest.mark.parametrize("curve", K.CURVE_NAMES)
def test_wire_fr_edges(curve):
    c = ctx()
    F = FR[curve]
    ok, refused = K.wire_fr(curve)
    rng = random.Random(6)
    fill = [rng.randrange(F.p) for _ in range(1000)]
    mont = lambda vals: corc.ints_to_arr([F.to_mont(v) for v in vals], 4)      # noqa: E731
    # accepted values: alone, and spread over a batch of 1000 (four workgroups of 256, a tail of 232)
    for vals in ([v] for v in ok):
        assert np.array_equal(c.wire_fr_decode(curve, _wire(vals)), mont(vals))
    vals = list(fill)
    vals[0], vals[255], vals[256], vals[700], vals[999] = ok[2], ok[2], ok[0], ok[1], ok[2]
    raw = _wire(vals)
    assert np.array_equal(c.wire_fr_decode(curve, raw), mont(vals))
    assert c.wire_fr_encode(curve, mont(vals)) == raw
    rc, _, n, rows = _wire_decode_dev(c, curve, raw)
    assert (rc, n) == (0, 1000) and np.array_equal(rows, mont(vals))
    # refused values: alone and at index 700 of 1000, host and device pointers, and the element is named
    for v in refused:
        for at, vals in ((0, [v]), (700, fill[:700] + [v] + fill[701:])):
            raw = _wire(vals)
            with pytest.raises(dg16_amd.Dg16Error, match=r"element %d is not reduced" % at):
                c.wire_fr_decode(curve, raw)
            rc, text, n, rows = _wire_decode_dev(c, curve, raw)
            assert rc == 3 and "element %d is not reduced" % at in text        # DG16_ERR_BAD_ARG
            good = [k for k in range(len(vals)) if k != at]
            assert np.array_equal(rows[good], mont([vals[k] for k in good])) and not rows[at].any()
    # two refused elements: the first one is named
    vals = list(fill)
    vals[900], vals[300] = refused[0], refused[2]
    with pytest.raises(dg16_amd.Dg16Error, match="element 300 is not reduced"):
        c.wire_fr_decode(curve, _wire(vals))
    assert np.array_equal(c.wire_fr_decode(curve, _wire(fill)), mont(fill))


# ---- round trip at 4096 points ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", ["bls12_381", "bls12_377"])
@pytest.mark.parametrize("group", [1, 2])
def test_round_trip_4096_on_device_pointers(curve, group):
    import torch
    c = ctx()
    Fq = FQ[curve]
    n, fb = 4096, K.fb(curve)
    dev = torch.device("cuda:0")
    pts = torch.empty(n * 2 * fb * group, dtype=torch.uint8, device=dev)
    c.gen_bases_dev(curve, group, 77 + group, n, pts.data_ptr())
    comp = torch.empty(n * fb * group, dtype=torch.uint8, device=dev)
    back = torch.full_like(pts, 0xAB)
    c.points_compress_dev(curve, group, pts.data_ptr(), n, comp.data_ptr())
    c.points_decompress_dev(curve, group, comp.data_ptr(), n, back.data_ptr(), validate=True)
    c.sync(0)
    assert torch.equal(pts, back)
    # the first 64 strings against the Python encoder of the same points
    head = pts[:64 * 2 * fb * group].cpu().numpy().view(np.uint64).reshape(64, -1)
    ints = [Fq.from_mont(v) for v in corc.arr_to_ints(head.reshape(-1, fb // 8))]
    per = 2 * group
    rows = [ints[per * k:per * (k + 1)] for k in range(64)]
    points = [(r[0], r[1]) if group == 1 else ((r[0], r[1]), (r[2], r[3])) for r in rows]
    assert all(CURVES[curve, "g%d" % group].on_curve(P) for P in points)
    want = b"".join(K.encode(curve, group, P) for P in points)
    assert comp[:64 * fb * group].cpu().numpy().tobytes() == want


# ---- the point of order two in an MSM and in points_mul ----------------------------------------------------------------
def _g1_points_on_the_curve(curve, n):
    """n points of E(Fq) from x = 1, 2, ...: almost surely outside the order-r subgroup (checked on the first few)."""
    C = CURVES[curve, "g1"]
    p = C.F.p
    pts, x = [], 0
    while len(pts) < n:
        x += 1
        y = A.sqrt_fq(p, (x ** 3 + C.b) % p)
        if y:
            pts.append((x, y if len(pts) % 2 else p - y))
    assert all(C.mul(P, C.order) is not None for P in pts[:3])
    return pts


def test_order_two_point_in_an_msm_and_in_points_mul():
    """One MSM without DG16_F_BASES_IN_SUBGROUP on BLS12-377 G1 over 40 curve points and T = (q - 1, 0) at four
    positions -- three odd scalars, two of them equal (the same buckets: T + T is a doubling with y = 0, or with the
    y = K p a negated digit makes of it), and an even one.  k T is T for odd k and the identity for even k, by hand; the
    rest is double-and-add in Python.  The same points through points_mul."""
    curve = "bls12_377"
    c = ctx()
    C = CURVES[curve, "g1"]
    T = K.order2_point()
    rng = random.Random(40)
    pts = _g1_points_on_the_curve(curve, 40)
    ks = [rng.randrange(1 << 248) for _ in pts]
    k_odd, k_even, k_last = rng.randrange(1 << 248) | 1, rng.randrange(1 << 248) & ~1, rng.randrange(1 << 248) | 1
    for at, k in ((0, k_odd), (17, k_odd), (29, k_even), (43, k_last)):
        pts.insert(at, T)
        ks.insert(at, k)
    assert len(pts) == 44 and [k for P, k in zip(pts, ks) if P == T] == [k_odd, k_odd, k_even, k_last]
    products, rest, t_odd = [], None, 0
    for P, k in zip(pts, ks):
        if P == T:
            products.append(T if k & 1 else None)
            t_odd += k & 1
        else:
            products.append(C.mul(P, k))
            rest = C.add(rest, products[-1])
    assert t_odd == 3
    total = C.add(rest, T)                                   # three odd multiples of T: T
    bases = K.affine_arr(curve, 1, pts)
    scal = corc.ints_to_arr(ks, 4)
    jac = c.msm(curve, 1, bases, scal, in_subgroup=False)
    assert np.array_equal(corc.jac_to_affine(curve, 1, jac), K.affine_arr(curve, 1, [total]))
    got = c.points_mul(curve, 1, bases, scal, in_subgroup=False)
    assert np.array_equal(got, K.affine_arr(curve, 1, products))
    # T alone: every window sum is a multiple of T, so the doublings between the windows meet it too
    for ks_t, want in (([k_odd], T), ([k_even], None), ([k_odd, k_last], None), ([k_odd, k_even, k_last, k_odd], T)):
        jac = c.msm(curve, 1, K.affine_arr(curve, 1, [T] * len(ks_t)), corc.ints_to_arr(ks_t, 4), in_subgroup=False)
        assert np.array_equal(corc.jac_to_affine(curve, 1, jac), K.affine_arr(curve, 1, [want])), ks_t
