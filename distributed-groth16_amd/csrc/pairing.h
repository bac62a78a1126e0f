// Optimal ate pairing on BN254 and BLS12-381 and the Groth16 verification decision built on it -- one proof per
// lane on the device (pairing_curve.hip), the same text on the host for the per-key work of dg16_vk_create and for
// tests/host_pairing.
//
// Tower: Fq12 = Fq2[w] / (w^6 - xi) stored FLAT as six Fq2 coefficients c[0..5] of w^0..w^5 (the representation of the
// test oracle, so no basis change anywhere).  Products go through Fq6 = Fq2[s] / (s^3 - xi), s = w^2: an element is
// A + w B with A = (c0, c2, c4), B = (c1, c3, c5) (Karatsuba, 18 Fq2 products; squaring 12).  Elements of the
// cyclotomic subgroup are squared as three Fq4 = Fq2[v] / (v^2 - xi) squarings, v = w^3, on the pairs (c0, c3),
// (c1, c4), (c2, c5) (Granger-Scott: Fq12 = Fq4[w] / (w^3 - v)).
//
// Miller loop: f_{6x+2,Q}(P) l_{T,pi(Q)}(P) l_{T,-pi^2(Q)}(P) (BN, NAF digits) / f_{|x|,Q}(P) conjugated (BLS12, x < 0);
// the running point T on the twist in homogeneous projective coordinates (Costello-Lange-Naehrig formulas as
// ark-ec's bn / bls12 `doubling_step` / `addition_step` write them), every line scaled by factors from proper
// subfields, which the final exponentiation kills.  A line is three Fq2 values (cy, cx, cc):
//   D-twist (BN254):     cy yp + cx xp w   + cc w^3
//   M-twist (BLS12-381): cc    + cx xp w^2 + cy yp w^3        (the line times w^3, an element of Fq4)
// so the lines of a FIXED G2 point (gamma, delta of a verifying key) are a table computed once per key.
// Final exponentiation: (q^6 - 1)(q^2 + 1), then the hard part by an x-chain (Fuentes-Castaneda et al. for BN;
// (x - 1)^2 (x + q)(x^2 + q^2 - 1) + 3 for BLS12, i.e. the CUBE of the reduced pairing): a fixed power m of the
// reduced pairing with gcd(m, r) = 1, which is one exactly when the reduced pairing is
// (tools/gen_pairing_consts.py asserts both facts on the integers).
//
// Everything is plain fp.h Montgomery arithmetic (Fp2 products call the out-of-line Fp product), functions are
// out of line: the code is a few hundred KB instead of tens of MB and a lane's Fq12 values live in scratch memory.
#pragma once
#include "pairing_consts_gen.h"
#include "types.h"

namespace dg16 {

template <int CURVE> struct PairingConstsOf;
template <> struct PairingConstsOf<0> { using type = bn254_pairing_consts; };
template <> struct PairingConstsOf<1> { using type = bls12_381_pairing_consts; };

template <int CURVE>
struct Pairing {
  using CT = CurveTypes<CURVE>;
  using Fq = typename CT::Fq;
  using Fq2 = typename CT::Fq2;
  using Fr = typename CT::Fr;
  using PC = typename PairingConstsOf<CURVE>::type;
  static constexpr int NL = Fq::NL;
  // lines of one Miller loop: a doubling per digit, an addition per non-zero digit, BN's two Frobenius steps
  static constexpr int N_LINES = PC::ATE_LEN + PC::ATE_ADDS + (PC::IS_BN ? 2 : 0);

  struct Fq6 { Fq2 a0, a1, a2; };
  struct Fq12 { Fq2 c[6]; };
  struct Line { Fq2 cy, cx, cc; };
  struct G2Proj { Fq2 x, y, z; };

  // ---- Fq2 helpers -------------------------------------------------------------------------------------------
  DG_HD static Fq2 mul_xi(const Fq2& a) {   // (a0 + a1 u)(XI_C0 + u)
    static_assert(PC::XI_C1 == 1 && (PC::XI_C0 == 1 || PC::XI_C0 == 9), "non-residue not wired");
    if constexpr (PC::XI_C0 == 1) {
      return {a.c0 - a.c1, a.c0 + a.c1};
    } else {
      Fq n0 = a.c0.dbl().dbl().dbl() + a.c0, n1 = a.c1.dbl().dbl().dbl() + a.c1;
      return {n0 - a.c1, a.c0 + n1};
    }
  }
  DG_HD static Fq2 conj2(const Fq2& a) { return {a.c0, a.c1.neg()}; }
  DG_HD static Fq2 scale(const Fq2& a, const Fq& k) { return {Fq::mul_call(a.c0, k), Fq::mul_call(a.c1, k)}; }
  DG_HD static Fq2 triple(const Fq2& a) { return a.dbl() + a; }
  DG_HD static Fq2 frob_coeff(int i) {   // xi^(i (q - 1) / 6), i = 1..5
    Fq2 g;
    for (int k = 0; k < NL; k++) { g.c0.l[k] = PC::FROB[i - 1][0][k]; g.c1.l[k] = PC::FROB[i - 1][1][k]; }
    return g;
  }
  DG_HD static Fq2 twist_b() {
    Fq2 b;
    for (int k = 0; k < NL; k++) { b.c0.l[k] = CT::G2c::B_C0[k]; b.c1.l[k] = CT::G2c::B_C1[k]; }
    return b;
  }
  DG_HD static Fq g1_b() {
    Fq b;
    for (int k = 0; k < NL; k++) b.l[k] = CT::G1c::B[k];
    return b;
  }

  // ---- Fq6 = Fq2[s] / (s^3 - xi) -------------------------------------------------------------------------------
  DG_HD static Fq6 add6(const Fq6& a, const Fq6& b) { return {a.a0 + b.a0, a.a1 + b.a1, a.a2 + b.a2}; }
  DG_HD static Fq6 sub6(const Fq6& a, const Fq6& b) { return {a.a0 - b.a0, a.a1 - b.a1, a.a2 - b.a2}; }
  DG_HD static Fq6 mul_s(const Fq6& a) { return {mul_xi(a.a2), a.a0, a.a1}; }
  static DG_COLD Fq6 mul6(const Fq6& a, const Fq6& b) {
    Fq2 v0 = a.a0 * b.a0, v1 = a.a1 * b.a1, v2 = a.a2 * b.a2;
    Fq2 c0 = v0 + mul_xi((a.a1 + a.a2) * (b.a1 + b.a2) - v1 - v2);
    Fq2 c1 = (a.a0 + a.a1) * (b.a0 + b.a1) - v0 - v1 + mul_xi(v2);
    Fq2 c2 = (a.a0 + a.a2) * (b.a0 + b.a2) - v0 - v2 + v1;
    return {c0, c1, c2};
  }
  static DG_COLD Fq6 inv6(const Fq6& a) {
    Fq2 t0 = a.a0.sqr() - mul_xi(a.a1 * a.a2);
    Fq2 t1 = mul_xi(a.a2.sqr()) - a.a0 * a.a1;
    Fq2 t2 = a.a1.sqr() - a.a0 * a.a2;
    Fq2 d = (a.a0 * t0 + mul_xi(a.a2 * t1 + a.a1 * t2)).inv();
    return {t0 * d, t1 * d, t2 * d};
  }

  // ---- Fq12 ----------------------------------------------------------------------------------------------------
  DG_HD static Fq6 even(const Fq12& f) { return {f.c[0], f.c[2], f.c[4]}; }
  DG_HD static Fq6 odd(const Fq12& f) { return {f.c[1], f.c[3], f.c[5]}; }
  DG_HD static Fq12 join(const Fq6& e, const Fq6& o) { return {{e.a0, o.a0, e.a1, o.a1, e.a2, o.a2}}; }
  DG_HD static Fq12 one12() {
    Fq12 r;
    for (int i = 0; i < 6; i++) r.c[i] = Fq2::zero();
    r.c[0] = Fq2::one();
    return r;
  }
  DG_HD static bool is_one12(const Fq12& f) {
    bool ok = f.c[0] == Fq2::one();
    for (int i = 1; i < 6; i++) ok = ok && f.c[i].is_zero();
    return ok;
  }
  static DG_COLD Fq12 mul12(const Fq12& a, const Fq12& b) {
    Fq6 a0 = even(a), a1 = odd(a), b0 = even(b), b1 = odd(b);
    Fq6 t0 = mul6(a0, b0), t1 = mul6(a1, b1), t2 = mul6(add6(a0, a1), add6(b0, b1));
    return join(add6(t0, mul_s(t1)), sub6(sub6(t2, t0), t1));
  }
  static DG_COLD Fq12 sqr12(const Fq12& a) {   // complex squaring: (A + B)(A + s B) = A^2 + s B^2 + (1 + s) A B
    Fq6 a0 = even(a), a1 = odd(a);
    Fq6 t = mul6(a0, a1);
    Fq6 u = mul6(add6(a0, a1), add6(a0, mul_s(a1)));
    return join(sub6(sub6(u, t), mul_s(t)), add6(t, t));
  }
  DG_HD static Fq12 conj12(const Fq12& a) {    // a^(q^6): w -> -w; the inverse on the cyclotomic subgroup
    return {{a.c[0], a.c[1].neg(), a.c[2], a.c[3].neg(), a.c[4], a.c[5].neg()}};
  }
  static DG_COLD Fq12 inv12(const Fq12& a) {   // (A + w B)^-1 = (A - w B) / (A^2 - s B^2)
    Fq6 a0 = even(a), a1 = odd(a);
    Fq6 n = inv6(sub6(mul6(a0, a0), mul_s(mul6(a1, a1))));
    Fq6 o = mul6(a1, n);
    return join(mul6(a0, n), {o.a0.neg(), o.a1.neg(), o.a2.neg()});
  }
  static DG_COLD Fq12 frob12(const Fq12& a) {  // a^q: c_i -> conj(c_i) xi^(i (q - 1) / 6)
    Fq12 r;
    r.c[0] = conj2(a.c[0]);
    for (int i = 1; i < 6; i++) r.c[i] = conj2(a.c[i]) * frob_coeff(i);
    return r;
  }
  // (a + b v)^2 in Fq4, v^2 = xi
  DG_HD static void sqr4(const Fq2& a, const Fq2& b, Fq2& r0, Fq2& r1) {
    Fq2 t0 = a.sqr(), t1 = b.sqr();
    r1 = (a + b).sqr() - t0 - t1;
    r0 = t0 + mul_xi(t1);
  }
  // a^2 for a in the cyclotomic subgroup (a^(q^4 - q^2 + 1) = 1): with g0 = (c0, c3), g1 = (c1, c4), g2 = (c2, c5) in Fq4,
  // a^2 = (3 g0^2 - 2 g0~) + (3 v g2^2 + 2 g1~) w + (3 g1^2 - 2 g2~) w^2, x~ the Fq4 conjugate
  static DG_COLD Fq12 cyc_sqr12(const Fq12& a) {
    Fq2 s00, s01, s10, s11, s20, s21;
    sqr4(a.c[0], a.c[3], s00, s01);
    sqr4(a.c[1], a.c[4], s10, s11);
    sqr4(a.c[2], a.c[5], s20, s21);
    Fq12 r;
    r.c[0] = triple(s00) - a.c[0].dbl();
    r.c[3] = triple(s01) + a.c[3].dbl();
    r.c[1] = triple(mul_xi(s21)) + a.c[1].dbl();
    r.c[4] = triple(s20) - a.c[4].dbl();
    r.c[2] = triple(s10) - a.c[2].dbl();
    r.c[5] = triple(s11) + a.c[5].dbl();
    return r;
  }
  // f * (v0 w^p0 + v1 w^p1 + v2 w^p2): 18 Fq2 products
  static DG_COLD Fq12 mul_sparse12(const Fq12& f, const Fq2& v0, int p0, const Fq2& v1, int p1, const Fq2& v2, int p2) {
    Fq12 r;
    for (int k = 0; k < 6; k++) r.c[k] = Fq2::zero();
    const Fq2* v[3] = {&v0, &v1, &v2};
    const int p[3] = {p0, p1, p2};
    for (int j = 0; j < 3; j++)
      for (int i = 0; i < 6; i++) {
        Fq2 t = f.c[i] * *v[j];
        int k = i + p[j];
        if (k >= 6) { k -= 6; t = mul_xi(t); }
        r.c[k] = r.c[k] + t;
      }
    return r;
  }
  // f * line(P), P = (xp, yp) affine on G1
  DG_HD static Fq12 mul_line(const Fq12& f, const Line& l, const Fq& xp, const Fq& yp) {
    if constexpr (PC::M_TWIST) return mul_sparse12(f, l.cc, 0, scale(l.cx, xp), 2, scale(l.cy, yp), 3);
    else return mul_sparse12(f, scale(l.cy, yp), 0, scale(l.cx, xp), 1, l.cc, 3);
  }

  // ---- Miller loop -----------------------------------------------------------------------------------------------
  // T <- 2T; the tangent's line
  static DG_COLD Line dbl_step(G2Proj& t) {
    Fq2 b = t.y.sqr(), c = t.z.sqr(), j = t.x.sqr();
    Fq2 e = twist_b() * triple(c);          // 3 b' Z^2
    Fq2 f = triple(e);
    Fq2 h = (t.y + t.z).sqr() - b - c;      // 2 Y Z
    Fq2 xy = t.x * t.y;
    Fq2 bf = b + f;
    // X3 = XY (b - f) / 2, Y3 = ((b + f) / 2)^2 - 3 e^2, Z3 = b h; scaled by (4, 4, 4) to stay clear of halving:
    // the point (2 XY (b - f), (b + f)^2 - 12 e^2, 4 b h) is the same projective point
    Line l = {h, triple(j).neg(), b - e};
    t.x = (xy * (b - f)).dbl();
    t.y = bf.sqr() - triple(e.sqr()).dbl().dbl();
    t.z = (b * h).dbl().dbl();
    return l;
  }
  // T <- T + Q (Q affine, != +-T, neither the identity); the chord's line
  static DG_COLD Line add_step(G2Proj& t, const Fq2& qx, const Fq2& qy) {
    Fq2 theta = t.y - qy * t.z, lambda = t.x - qx * t.z;
    Fq2 c = theta.sqr(), d = lambda.sqr();
    Fq2 e = lambda * d, f = t.z * c, g = t.x * d;
    Fq2 h = e + f - g.dbl();
    Line l = {lambda, theta.neg(), theta * qx - lambda * qy};
    t.x = lambda * h;
    t.y = theta * (g - h) - e * t.y;
    t.z = t.z * e;
    return l;
  }
  // the lines of Q in loop order (N_LINES of them); Q in the order-r subgroup, not the identity
  static DG_COLD void prepare_g2(const Affine<Fq2>& q, Line* out) {
    G2Proj t = {q.x, q.y, Fq2::one()};
    int n = 0;
    Fq2 nqy = q.y.neg();
    for (int i = 0; i < PC::ATE_LEN; i++) {
      out[n++] = dbl_step(t);
      int d = PC::ATE[i];
      if (d) out[n++] = add_step(t, q.x, d > 0 ? q.y : nqy);
    }
    if constexpr (PC::IS_BN) {
      Fq2 x1 = conj2(q.x) * frob_coeff(2), y1 = conj2(q.y) * frob_coeff(3);
      Fq2 x2 = conj2(x1) * frob_coeff(2), y2 = conj2(y1) * frob_coeff(3);
      out[n++] = add_step(t, x1, y1);
      out[n++] = add_step(t, x2, y2.neg());
    }
  }
  // Product of up to three Miller values with one shared squaring chain: (pa, qb) with qb's lines computed on the fly,
  // (pg, table tg), (pd, table td).  A null table or an identity point drops that factor (e(O, Q) = e(P, O) = 1).
  static DG_COLD Fq12 miller3(const Affine<Fq>& pa, const Affine<Fq2>& qb, const Affine<Fq>& pg, const Line* tg,
                              const Affine<Fq>& pd, const Line* td) {
    const bool ub = !pa.is_inf() && !qb.is_inf();
    const bool ug = tg && !pg.is_inf(), ud = td && !pd.is_inf();
    Fq12 f = one12();
    G2Proj t = {qb.x, qb.y, Fq2::one()};
    Fq2 nqy = qb.y.neg();
    int n = 0;
    for (int i = 0; i < PC::ATE_LEN; i++) {
      if (i) f = sqr12(f);
      if (ub) { Line l = dbl_step(t); f = mul_line(f, l, pa.x, pa.y); }
      if (ug) f = mul_line(f, tg[n], pg.x, pg.y);
      if (ud) f = mul_line(f, td[n], pd.x, pd.y);
      n++;
      int d = PC::ATE[i];
      if (d) {
        if (ub) { Line l = add_step(t, qb.x, d > 0 ? qb.y : nqy); f = mul_line(f, l, pa.x, pa.y); }
        if (ug) f = mul_line(f, tg[n], pg.x, pg.y);
        if (ud) f = mul_line(f, td[n], pd.x, pd.y);
        n++;
      }
    }
    if constexpr (PC::IS_BN) {
      Fq2 x1 = conj2(qb.x) * frob_coeff(2), y1 = conj2(qb.y) * frob_coeff(3);
      Fq2 x2 = conj2(x1) * frob_coeff(2), y2 = conj2(y1) * frob_coeff(3);
      for (int k = 0; k < 2; k++) {
        if (ub) {
          Line l = k ? add_step(t, x2, y2.neg()) : add_step(t, x1, y1);
          f = mul_line(f, l, pa.x, pa.y);
        }
        if (ug) f = mul_line(f, tg[n], pg.x, pg.y);
        if (ud) f = mul_line(f, td[n], pd.x, pd.y);
        n++;
      }
    }
    if constexpr (PC::X_NEG) f = conj12(f);
    return f;
  }
  static DG_COLD Fq12 miller(const Affine<Fq>& p, const Affine<Fq2>& q) {
    return miller3(p, q, Affine<Fq>::inf(), nullptr, Affine<Fq>::inf(), nullptr);
  }

  // ---- final exponentiation ----------------------------------------------------------------------------------------
  static DG_COLD Fq12 exp_x(const Fq12& a) {   // a^x, a in the cyclotomic subgroup
    Fq12 r = a;
    for (int i = 62; i >= 0; i--) {
      // (X_ABS has bit 63 or 62 as its top bit)
      if (i == 62 && !(PC::X_ABS >> 63)) continue;
      r = cyc_sqr12(r);
      if ((PC::X_ABS >> i) & 1) r = mul12(r, a);
    }
    if constexpr (PC::X_NEG) r = conj12(r);
    return r;
  }
  static DG_COLD Fq12 final_exp(const Fq12& f0) {
    Fq12 f = mul12(conj12(f0), inv12(f0));   // f^(q^6 - 1)
    f = mul12(frob12(frob12(f)), f);         // ^(q^2 + 1): now in the cyclotomic subgroup
    if constexpr (PC::IS_BN) {
      Fq12 fx = exp_x(f), f2x = cyc_sqr12(fx), f4x = cyc_sqr12(f2x), f6x = mul12(f4x, f2x);
      Fq12 f6x2 = exp_x(f6x), f12x2 = cyc_sqr12(f6x2), f12x3 = exp_x(f12x2);
      Fq12 a = mul12(mul12(f12x3, f6x2), f6x);
      Fq12 b = mul12(a, conj12(f2x));
      Fq12 r = mul12(mul12(a, f6x2), f);
      r = mul12(r, frob12(b));
      r = mul12(r, frob12(frob12(a)));
      return mul12(r, frob12(frob12(frob12(mul12(b, conj12(f))))));
    } else {
      Fq12 a = mul12(exp_x(f), conj12(f));              // f^(x - 1)
      a = mul12(exp_x(a), conj12(a));                   // ^(x - 1)
      Fq12 b = mul12(exp_x(a), frob12(a));              // ^(x + q)
      Fq12 c = mul12(mul12(exp_x(exp_x(b)), frob12(frob12(b))), conj12(b));   // ^(x^2 + q^2 - 1)
      return mul12(c, mul12(cyc_sqr12(f), f));          // * f^3
    }
  }

  // ---- input checks (the rules of dg16_groth16_verify, plus the G1 subgroup where G1 has a cofactor) ----------------
  template <class P>
  DG_HD static bool canonical(const Fp<P>& v) {
    for (int i = P::NL - 1; i >= 0; i--)
      if (v.l[i] != P::P[i]) return v.l[i] < P::P[i];
    return false;
  }
  DG_HD static bool canonical(const Fq2& v) { return canonical(v.c0) && canonical(v.c1); }
  DG_HD static bool on_curve(const Affine<Fq>& p) { return p.is_inf() || p.y.sqr() == p.x.sqr() * p.x + g1_b(); }
  DG_HD static bool on_curve(const Affine<Fq2>& p) { return p.is_inf() || p.y.sqr() == p.x.sqr() * p.x + twist_b(); }
  template <class F>
  static DG_COLD bool in_subgroup(const Affine<F>& p) {
    if (p.is_inf()) return true;
    return scalar_mul<F, Fr::NL>(XYZZ<F>::from_affine(p), Fr::Params::P).is_inf();
  }
  static constexpr bool G1_COFACTOR = CURVE != 0;
  static DG_COLD bool valid_g1(const Affine<Fq>& p) {
    if (!canonical(p.x) || !canonical(p.y) || !on_curve(p)) return false;
    if constexpr (G1_COFACTOR) return in_subgroup(p);
    return true;
  }
  static DG_COLD bool valid_g2(const Affine<Fq2>& p) {
    return canonical(p.x) && canonical(p.y) && on_curve(p) && in_subgroup(p);
  }

  // ---- one proof ----------------------------------------------------------------------------------------------------
  struct Proof {
    Affine<Fq> a;
    Affine<Fq2> b;
    Affine<Fq> c;
  };
  struct Key {              // a prepared verifying key as the kernels see it
    const Affine<Fq>* ic;   // n_public + 1 points
    const Line* gamma;      // N_LINES lines, or null if gamma is the identity
    const Line* delta;
    const Fq12* alpha_beta; // Miller value of (-alpha, beta)
  };
  // The per-key work (what ark-groth16's prepare_verifying_key does, plus the Validate::Yes checks): false for a
  // malformed key.  tg / td receive N_LINES lines each unless gamma / delta is the identity.
  static DG_COLD bool prepare_key(const Affine<Fq>& alpha, const Affine<Fq2>& beta, const Affine<Fq2>& gamma,
                                  const Affine<Fq2>& delta, const Affine<Fq>* ic, size_t n_ic, Line* tg, Line* td,
                                  Fq12* alpha_beta) {
    if (!valid_g1(alpha) || !valid_g2(beta) || !valid_g2(gamma) || !valid_g2(delta)) return false;
    for (size_t i = 0; i < n_ic; i++)
      if (!valid_g1(ic[i])) return false;
    if (!gamma.is_inf()) prepare_g2(gamma, tg);
    if (!delta.is_inf()) prepare_g2(delta, td);
    *alpha_beta = miller(alpha.is_inf() ? alpha : Affine<Fq>{alpha.x, alpha.y.neg()}, beta);
    return true;
  }
  // Checks of one proof and its inputs; on success *nacc = -(IC_0 + sum_j x_j IC_(j+1)).
  static DG_COLD bool prepare_one(const Key& k, const Fr* inputs, size_t n_public, bool mont, const Proof& pr,
                                  Affine<Fq>* nacc) {
    if (!valid_g1(pr.a) || !valid_g2(pr.b) || !valid_g1(pr.c)) return false;
    XYZZ<Fq> acc = XYZZ<Fq>::from_affine(k.ic[0]);
    for (size_t j = 0; j < n_public; j++) {
      Fr x = inputs[j];
      if (!canonical(x)) return false;     // x and x + r are not the same input
      if (mont) x = x.from_mont();
      acc = acc.add(scalar_mul<Fq, Fr::NL>(XYZZ<Fq>::from_affine(k.ic[j + 1]), x.l));
    }
    Affine<Fq> s = acc.to_affine();
    *nacc = s.is_inf() ? s : Affine<Fq>{s.x, s.y.neg()};
    return true;
  }
  // e(A, B) e(-acc, gamma) e(-C, delta) e(-alpha, beta) == 1
  static DG_COLD bool decide_one(const Key& k, const Proof& pr, const Affine<Fq>& nacc) {
    Affine<Fq> nc = pr.c.is_inf() ? pr.c : Affine<Fq>{pr.c.x, pr.c.y.neg()};
    Fq12 f = miller3(pr.a, pr.b, nacc, k.gamma, nc, k.delta);
    f = mul12(f, *k.alpha_beta);
    return is_one12(final_exp(f));
  }
};

}  // namespace dg16
