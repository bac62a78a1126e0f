"""The point-codec cases of tests/codec_cases.py, checked without a GPU: every point is on its curve and has the
property it was built for (right-hand side in Fq, limbs shared with the negative, outside the subgroup), the Python
decoder inverts the Python encoder, and the HOST compilation of csrc/codec_impl.h (tests/host_arith/, `ha_codec`:
CodecT<0..2>::encode / decode) gives the same bytes, points and error codes on every case -- the reference the GPU
tests (tests/test_gpu_codec_edges.py) compare the gfx950 compilation with, shown to hold on these inputs."""

import numpy as np
import pytest

import codec_cases as K
from oracle.pyref.curves import CURVES
from oracle.pyref.fields import FQ, FR
from test_host_arith import ha, _codec  # noqa: F401  (ha: the fixture that builds and loads the host library)

PAIRS = [(c, g) for c in K.CURVE_NAMES for g in (1, 2)]


@pytest.mark.parametrize("curve,group", PAIRS)
def test_points_are_on_the_curve_and_where_they_claim_to_be(curve, group):
    C = CURVES[curve, "g%d" % group]
    pts = K.valid_points(curve, group)
    assert sum(label == "ordinary" for label, _, _ in pts) == 304
    checked = 0
    for k, (label, P, inside) in enumerate(pts):
        assert C.on_curve(P), label
        if label != "ordinary" or k < 4 or P is C.gen:
            if not (curve == "bn254" and group == 1):
                assert (C.mul(P, C.order) is None) == inside, label
            checked += 1
    assert checked >= 10
    if group == 2:
        kinds = [kind for kind, _ in K.rhs_in_fq(curve)]
        assert kinds.count("real") >= 6 and kinds.count("imag") >= 6          # three x of each kind, both signs
        for kind, (x, y) in K.rhs_in_fq(curve):
            rhs = C.F.add(C.F.mul(C.F.sqr(x), x), C.b)
            assert rhs[1] == 0 and x[1] != 0
            assert (y[1] == 0 and y[0] != 0) if kind == "real" else (y[0] == 0 and y[1] != 0)


@pytest.mark.parametrize("curve,group", PAIRS)
def test_deciding_coordinate_next_to_half_the_modulus(curve, group):
    p, nl = FQ[curve].p, K.nl32(curve)
    cases = K.near_half(curve, group)
    assert [s for s, _ in cases] == [None, None, 1, 1, 2, 2]
    for shared, (x, y) in cases:
        key = y if group == 1 else y[1]
        small = min(key, p - key)
        if shared is None:
            assert (p - 1) // 2 - small < 64
        else:
            assert K.shared_top_limbs(curve, key, p - key) == shared
            k = nl - shared
            assert (p - 1) // 2 - small <= (1 << (32 * k)) // 3 and p - 2 * small > 1 << (32 * (k - 1))
    # y = (q +- 1) / 2 itself is on none of the curves (G1), so "next to" is the best there is
    C = CURVES[curve, "g1"]
    for y in ((p - 1) // 2, (p + 1) // 2):
        assert K.cube_root(K._fq_field(p), (y * y - C.b) % p) is None


def test_cube_roots():
    import random
    rng = random.Random(3)
    for curve in K.CURVE_NAMES:
        p, F2 = FQ[curve].p, CURVES[curve, "g2"].F
        assert p % 3 == 1
        for K_, draw in ((K._fq_field(p), lambda: rng.randrange(1, p)),
                         (K._fq2_field(F2), lambda: (rng.randrange(p), rng.randrange(1, p)))):
            found = 0
            for _ in range(12):
                a = draw()
                cube = K_.mul(K_.mul(a, a), a)
                r = K.cube_root(K_, cube)
                assert r is not None and K_.mul(K_.mul(r, r), r) == cube
                found += K.cube_root(K_, a) is not None
            assert found < 12                                                   # non-cubes are told apart


@pytest.mark.parametrize("curve,group", PAIRS)
def test_only_bls12_377_g1_has_a_point_with_y_zero(curve, group):
    """y = 0 needs x^3 = -b: a cube root of -b in the coordinate field.  csrc/ec29.h (HasOrderTwoPoint) compiles the
    y = 0 case of its doublings for the groups listed here and for no other."""
    C = CURVES[curve, "g%d" % group]
    K_ = K._fq_field(C.F.p) if group == 1 else K._fq2_field(C.F)
    root = K.cube_root(K_, C.F.neg(C.b))
    assert (root is not None) == ((curve, group) == ("bls12_377", 1))


def test_order_two_point_of_bls12_377():
    C = CURVES["bls12_377", "g1"]
    T = K.order2_point()
    assert C.on_curve(T) and T[1] == 0 and C.mul(T, 2) is None and C.mul(T, C.order) == T
    plain, flagged = K.order2_strings()
    assert plain[-1] & 0xC0 == 0 and flagged[-1] & 0xC0 == 0x80 and plain[:-1] == flagged[:-1]
    assert K.decode("bls12_377", 1, plain) == (0, T) and K.decode("bls12_377", 1, flagged) == (0, T)


@pytest.mark.parametrize("curve,group", PAIRS)
def test_python_decoder_inverts_the_python_encoder(curve, group):
    for label, P, inside in K.valid_points(curve, group):
        raw = K.encode(curve, group, P)
        assert K.decode(curve, group, raw) == (0, P), label
    for label, raw, code, validate in K.malformed(curve, group):
        assert K.decode(curve, group, raw, validate)[0] == code, label
        if code == 4:
            assert K.decode(curve, group, raw, False)[0] == 0
    codes = {code for _, _, code, _ in K.malformed(curve, group)}
    assert codes == ({1, 2, 3} if (curve, group) == ("bn254", 1) else {1, 2, 3, 4})


@pytest.mark.parametrize("curve,group", PAIRS)
def test_host_codec_agrees_on_every_case(ha, curve, group):  # noqa: F811
    cb, pb = K.fb(curve) * group, 2 * K.fb(curve) * group
    cases = K.valid_points(curve, group)
    pts = [P for _, P, _ in cases]
    n = len(pts)
    arr = K.affine_arr(curve, group, pts)
    want = b"".join(K.encode(curve, group, P) for P in pts)
    got, _ = _codec(ha, curve, group, 0, 0, arr.view(np.uint8).reshape(-1), n, cb * n)
    assert got.tobytes() == want
    back, rc = _codec(ha, curve, group, 1, 0, want, n, pb * n)
    assert not rc.any() and np.array_equal(back.view(np.uint64).reshape(n, -1), arr)
    back, rc = _codec(ha, curve, group, 1, 1, want, n, pb * n)
    inside = np.array([ins for _, _, ins in cases])
    assert np.array_equal(rc, np.where(inside, 0, 4).astype(np.int32))
    assert np.array_equal(back.view(np.uint64).reshape(n, -1)[inside], arr[inside])
    for label, raw, code, validate in K.malformed(curve, group):
        _, rc = _codec(ha, curve, group, 1, int(validate), raw, 1, pb)
        assert rc[0] == code, (label, raw.hex())
    if (curve, group) == ("bls12_377", 1):
        T = K.affine_arr(curve, 1, [K.order2_point()])
        for raw in K.order2_strings():
            dec, rc = _codec(ha, curve, 1, 1, 0, raw, 1, pb)
            assert rc[0] == 0 and np.array_equal(dec.view(np.uint64).reshape(1, -1), T)
            assert not T[0, 6:].any()                                           # y = 0


def test_wire_fr_values():
    for curve in K.CURVE_NAMES:
        r = FR[curve].p
        ok, bad = K.wire_fr(curve)
        assert all(v < r for v in ok) and all(r <= v < 1 << 256 for v in bad)
        assert r + 1 in bad and any(v - r == 1 << 224 for v in bad)
