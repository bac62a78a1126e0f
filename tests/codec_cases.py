"""TEST INFRASTRUCTURE: inputs for the point codec (csrc/codec_impl.h) that random subgroup points never reach, with the
bytes and points they must give -- built in plain Python integers from the independent encoders the suite already has
(tests/ark_points_py.py, the oracle's curve objects).  Shared by tests/test_codec_cases.py (the cases themselves and
the HOST compilation of the codec, no GPU) and tests/test_gpu_codec_edges.py (the gfx950 compilation of the same text).

Per curve (bn254, bls12_381 in its zcash form, bls12_377) and group:
  rhs_in_fq      G2 points x = (a, b) whose x^3 + B has c1 = 0: `sqrt_fq2`'s a.c1 == 0 branch with both outcomes, a root
                 (t, 0) in Fq and a purely imaginary root (0, t); the (t, 0) roots also take `is_neg(Fq2)`'s c1 == 0
                 fallback.  Both signs of every y.  Outside the order-r subgroup (asserted by the CPU test).
  near_half      points whose deciding coordinate (G1: y, G2: y.c1) is the closest value below q / 2 that lies on the
                 curve, and values about 2^(32 k) / 3 below q / 2 for k = nl - 1, nl - 2, so that y and q - y agree in
                 their top one and top two 32-bit limbs and `cmp()` has to walk past equal limbs.  Both signs.  x is a
                 cube root of y^2 - b (Fq, and Fq2 for G2: the same routine over the field's operations, so G2 IS
                 covered).  Outside the subgroup except on BN254 G1 (cofactor one).
  order2         BLS12-377 G1's point of order two T = (q - 1, 0) (b = 1, even cofactor): a root y = 0, with and
                 without the sign flag.  The codec accepts both and returns y = 0, as arkworks'
                 get_point_from_x_unchecked does when both roots are equal.
  ordinary       300 random subgroup points, the identity, both signs of one x, the generator.
  malformed      one string per error code 1-4 of the codec and per way of earning it.
  wire_fr        Vec<Fr> elements at the edge of "reduced".
"""

import functools
import random

import numpy as np

import ark_points_py as A
from oracle.pyref.curves import CURVES
from oracle.pyref.fields import FQ, FR

CURVE_NAMES = ("bn254", "bls12_381", "bls12_377")
CURVE_IDS = {"bn254": 0, "bls12_381": 1, "bls12_377": 2}
ERR_TEXT = {1: "invalid flags", 2: "coordinate not reduced", 3: "x is not on the curve",
            4: "point is not in the prime-order subgroup"}


def fb(curve):
    return A.fbytes(curve)


def nl32(curve):
    return fb(curve) // 4


def is_zcash(curve):
    return curve == "bls12_381"


# ---- the two encodings, and decoders written from their definitions -------------------------------------------------
def encode(curve, group, P):
    return A.encode_zcash(group, P) if is_zcash(curve) else A.encode(curve, group, P)


def _y_is_larger(p, group, y):
    if group == 1:
        return y > (-y) % p
    return y[1] > (-y[1]) % p if y[1] != 0 else y[0] > (-y[0]) % p


def decode(curve, group, raw, validate=False):
    """(code, point): code 0 and the point, or the codec's error code 1-4 and None.  The order of the checks is the
    format's: flags, reduced coordinates, an identity with x != 0, a y on the curve, the subgroup."""
    C = CURVES[curve, "g%d" % group]
    p, n = C.F.p, fb(curve)
    assert len(raw) == n * group
    if is_zcash(curve):
        if not raw[0] & 0x80:
            return 1, None
        inf, neg = bool(raw[0] & 0x40), bool(raw[0] & 0x20)
        body = bytes([raw[0] & 0x1F]) + raw[1:]
        co = [int.from_bytes(body[i * n:(i + 1) * n], "big") for i in range(group)][::-1]       # c1 || c0 on the wire
    else:
        neg, inf = bool(raw[-1] & 0x80), bool(raw[-1] & 0x40)
        body = raw[:-1] + bytes([raw[-1] & 0x3F])
        co = [int.from_bytes(body[i * n:(i + 1) * n], "little") for i in range(group)]
    if neg and inf:
        return 1, None
    if any(v >= p for v in co):
        return 2, None
    if inf:
        return (1, None) if any(co) else (0, None)
    if group == 1:
        x = co[0]
        y = A.sqrt_fq(p, (x ** 3 + C.b) % p)
    else:
        x = (co[0], co[1])
        y = A.sqrt_fq2(C.F, C.F.add(C.F.mul(C.F.sqr(x), x), C.b))
    if y is None:
        return 3, None
    if _y_is_larger(p, group, y) != neg:
        y = C.F.neg(y)
    if validate and C.mul((x, y), C.order) is not None:
        return 4, None
    return 0, (x, y)


def affine_arr(curve, group, pts):
    """uint64 [n][2 * limbs * group]: x || y in Montgomery form, the identity as zeros -- the library's affine layout."""
    Fq = FQ[curve]
    n = fb(curve)
    out = np.zeros((len(pts), n // 8 * 2 * group), dtype=np.uint64)
    for k, P in enumerate(pts):
        if P is None:
            continue
        co = [P[0], P[1]] if group == 1 else [P[0][0], P[0][1], P[1][0], P[1][1]]
        out[k] = np.frombuffer(b"".join(Fq.to_mont(v).to_bytes(n, "little") for v in co), dtype=np.uint64)
    return out


# ---- cube roots in Fq and Fq2 -----------------------------------------------------------------------------------------
class _Field:
    """What cube_root needs of a finite field: its multiplication, its unit, the order of its multiplicative group and
    candidates for a non-cube."""

    def __init__(self, mul, one, order, small):
        self.mul, self.one, self.order, self.small = mul, one, order, small

    def pow(self, a, e):
        acc = self.one
        for bit in bin(e)[2:]:
            acc = self.mul(acc, acc)
            if bit == "1":
                acc = self.mul(acc, a)
        return acc


def _fq_field(p):
    return _Field(lambda a, b: a * b % p, 1, p - 1, lambda k: k % p)


def _fq2_field(F2):
    return _Field(F2.mul, (1, 0), F2.p * F2.p - 1, lambda k: (k // 8, 1 + k % 8))


def cube_root(K, a):
    """A cube root of a != 0 in the field K whose group order n = 3^s t is divisible by three, or None: a^(1 / 3 mod t),
    corrected inside the 3-Sylow subgroup (3^s elements: searched)."""
    n = K.order
    assert n % 3 == 0
    if K.pow(a, n // 3) != K.one:
        return None
    s, t = 0, n
    while t % 3 == 0:
        s, t = s + 1, t // 3
    e = pow(3, -1, t)
    r0 = K.pow(a, e)                                   # r0^3 = a * (a^t)^m with 3 e - 1 = m t
    h = K.pow(K.pow(a, t), (3 * e - 1) // t)           # in the 3-Sylow subgroup, and a cube there
    z = next(K.small(k) for k in range(2, 200) if K.pow(K.small(k), n // 3) != K.one)
    g = K.pow(z, t)                                    # generates the 3-Sylow subgroup
    w = K.one
    for _ in range(3 ** s):
        if K.mul(K.mul(w, w), w) == h:                 # r = r0 / w: multiply by w^-1 = w^(3^s - 1)
            r = K.mul(r0, K.pow(w, 3 ** s - 1))
            assert K.mul(K.mul(r, r), r) == a
            return r
        w = K.mul(w, g)
    raise AssertionError("no cube root in the 3-Sylow subgroup")


# ---- (a) G2 points whose right-hand side lies in Fq -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rhs_in_fq(curve):
    """[(kind, P)]: kind "real" for y = (t, 0), "imag" for y = (0, t); at least three x of each kind, both signs of y."""
    C = CURVES[curve, "g2"]
    F2, p = C.F, C.F.p
    beta = (-F2.nr) % p                                # Fq2 = Fq[u] / (u^2 + beta)
    out, count = [], {"real": 0, "imag": 0}
    for b in range(1, 400):
        a = A.sqrt_fq(p, (beta * b ** 3 - C.b[1]) * pow(3 * b, -1, p) % p)
        if a is None:
            continue
        x = (a, b)
        rhs = F2.add(F2.mul(F2.sqr(x), x), C.b)
        assert rhs[1] == 0
        y = A.sqrt_fq2(F2, rhs)
        assert y is not None and (y[0] == 0) != (y[1] == 0), "an element of Fq has a root in Fq or in u Fq"
        kind = "real" if y[1] == 0 else "imag"
        if count[kind] >= 3:
            continue
        count[kind] += 1
        out += [(kind, (x, y)), (kind, (x, F2.neg(y)))]
        if min(count.values()) >= 3:
            return out
    raise AssertionError("b < 400 did not give three points of each kind: %r" % count)


# ---- (b) deciding coordinate next to q / 2 ----------------------------------------------------------------------------
def shared_top_limbs(curve, v, w):
    n = nl32(curve)
    k = 0
    while k < n and (v >> (32 * (n - 1 - k))) & 0xFFFFFFFF == (w >> (32 * (n - 1 - k))) & 0xFFFFFFFF:
        k += 1
    return k


def _near_half_targets(curve):
    """[(shared limbs wanted, starting value)]: the midpoint itself, then about 2^(32 k) / 3 below it.  The distance d is
    kept inside [2^(32 (k - 1)), what the low limbs of q / 2 leave room for], so that y = half - d and q - y = half + 1 + d
    agree in exactly nl - k top limbs."""
    p, n = FQ[curve].p, nl32(curve)
    half = (p - 1) // 2
    out = [(None, half)]
    for k in (n - 1, n - 2):
        low = half % (1 << (32 * k))
        d = min((1 << (32 * k)) // 3, low, (1 << (32 * k)) - 2 - low)
        assert d >= 4 << (32 * (k - 1)), "q / 2 leaves no room for a pair sharing %d limbs" % (n - k)
        out.append((n - k, half - d))
    return out


@functools.lru_cache(maxsize=None)
def near_half(curve, group):
    """[(shared, P)]: shared = the number of equal top 32-bit limbs of the deciding coordinate and its negative (None for
    the point next to the midpoint, where it is whatever q gives).  Both signs of every point."""
    C = CURVES[curve, "g%d" % group]
    F, p = C.F, C.F.p
    K = _fq_field(p) if group == 1 else _fq2_field(F)
    out = []
    for shared, start in _near_half_targets(curve):
        for j in range(64):
            # the deciding coordinate moves towards the midpoint (G1) or stays (G2: y.c0 takes the tries)
            y = start + j if group == 1 and shared else start - j if group == 1 else (1 + j, start)
            rhs = F.sub(F.sqr(y), C.b)
            x = cube_root(K, rhs) if not F.is_zero(rhs) else None
            if x is not None:
                break
        else:
            raise AssertionError("no curve point within 64 tries")
        key = y if group == 1 else y[1]
        if shared is not None:
            assert shared_top_limbs(curve, key, p - key) == shared
        assert key < p - key
        out += [(shared, (x, y)), (shared, (x, F.neg(y)))]
    return out


# ---- (c) BLS12-377 G1's point of order two ----------------------------------------------------------------------------
def order2_point():
    return (FQ["bls12_377"].p - 1, 0)


def order2_strings():
    """T's compressed form as the encoder writes it, and the same with the sign flag set: both decode to T."""
    plain = A.encode("bls12_377", 1, order2_point())
    flagged = plain[:-1] + bytes([plain[-1] | 0x80])
    return plain, flagged


# ---- (d) ordinary material --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ordinary(curve, group):
    C = CURVES[curve, "g%d" % group]
    rng = random.Random(1000 * CURVE_IDS[curve] + group)
    pts = [C.mul(C.gen, rng.randrange(1, C.order)) for _ in range(300)]
    return pts + [None, C.neg(pts[0]), pts[0], C.gen]


@functools.lru_cache(maxsize=None)
def outside_subgroup(curve, group):
    if group == 2:
        return A.twist_point_outside_subgroup(curve)
    return A.g1_point_outside_subgroup(curve) if curve != "bn254" else None


@functools.lru_cache(maxsize=None)
def valid_points(curve, group):
    """[(label, P, in_subgroup)] of (a)-(d): every point the codec must encode and decode, in one list.  in_subgroup is
    what the construction says; tests/test_codec_cases.py checks it with a multiplication by r."""
    out = [("ordinary", P, True) for P in ordinary(curve, group)]
    if group == 2:
        out += [("rhs_in_fq/" + kind, P, False) for kind, P in rhs_in_fq(curve)]
    cofactor_one = curve == "bn254" and group == 1
    out += [("near_half/%s" % shared, P, cofactor_one) for shared, P in near_half(curve, group)]
    if (curve, group) == ("bls12_377", 1):
        out.append(("order2", order2_point(), False))
    P = outside_subgroup(curve, group)
    if P is not None:
        out.append(("outside", P, False))
    return out


# ---- (e) malformed strings --------------------------------------------------------------------------------------------
def _x_off_curve_g2(curve):
    C = CURVES[curve, "g2"]
    F2 = C.F
    return next((k, 1) for k in range(200) if A.sqrt_fq2(F2, F2.add(F2.mul(F2.sqr((k, 1)), (k, 1)), C.b)) is None)


def _raw_x(curve, group, x, flags=0):
    """The string of a non-identity point with this x (an integer, or (c0, c1)) whatever x is, reduced or not; flags:
    extra bits for the flag byte."""
    n = fb(curve)
    co = [x] if group == 1 else list(x)
    if is_zcash(curve):
        out = bytearray(b"".join(v.to_bytes(n, "big") for v in co[::-1]))
        out[0] |= 0x80 | flags
    else:
        out = bytearray(b"".join(v.to_bytes(n, "little") for v in co))
        out[-1] |= flags
    return bytes(out)


@functools.lru_cache(maxsize=None)
def malformed(curve, group):
    """[(label, raw, code, validate)]: the string, the error code it must earn and the mode it earns it in (codes 1-3 in
    both modes: listed with validate False; code 4 only with validate True, where the string decodes otherwise)."""
    C = CURVES[curve, "g%d" % group]
    p, n = C.F.p, fb(curve)
    cb = n * group
    gen = encode(curve, group, C.gen)
    out = []
    if is_zcash(curve):
        out.append(("compressed bit missing", bytes([gen[0] & 0x7F]) + gen[1:], 1, False))
        out.append(("both flags", bytes([0xE0]) + bytes(cb - 1), 1, False))
        out.append(("identity with x != 0", bytes([0xC0]) + bytes(cb - 2) + b"\x01", 1, False))
        ones_flagged, ones_plain = (1 << 381) - 1, (1 << 384) - 1
    else:
        both = bytearray(cb)
        both[-1] = 0xC0
        out.append(("both flags", bytes(both), 1, False))
        inf_x = bytearray(cb)
        inf_x[0], inf_x[-1] = 1, 0x40
        out.append(("identity with x != 0", bytes(inf_x), 1, False))
        ones_flagged, ones_plain = (1 << (8 * n - 2)) - 1, (1 << (8 * n)) - 1
    gx = C.gen[0]
    for name, v in (("q", p), ("q + 1", p + 1), ("all ones", None)):
        if group == 1:
            out.append(("x = %s" % name, _raw_x(curve, 1, ones_flagged if v is None else v), 2, False))
        else:
            # the coordinate that carries the flag bits has fewer bits to fill: c1 in both forms
            out.append(("x.c0 = %s" % name, _raw_x(curve, 2, (ones_plain if v is None else v, gx[1])), 2, False))
            out.append(("x.c1 = %s" % name, _raw_x(curve, 2, (gx[0], ones_flagged if v is None else v)), 2, False))
    off = A.x_off_curve(curve) if group == 1 else _x_off_curve_g2(curve)
    out.append(("x off the curve", _raw_x(curve, group, off), 3, False))
    P = outside_subgroup(curve, group)
    if P is not None:
        out.append(("outside the subgroup", encode(curve, group, P), 4, True))
    return out


def malformed_with_code(curve, group, code):
    return next(raw for _, raw, c, _ in malformed(curve, group) if c == code)


# ---- (f) Vec<Fr> wire elements -----------------------------------------------------------------------------------------
def wire_fr(curve):
    """(accepted, refused) canonical integers below 2^256."""
    r = FR[curve].p
    refused = [r, r + 1, (1 << 256) - 1, r + 1, r + (1 << 224)]       # ..., limb 0 raised by one, only the top limb raised
    assert all(v < 1 << 256 for v in refused)
    return [0, 1, r - 1], refused
