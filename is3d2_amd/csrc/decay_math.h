// decay_math.h -- host/device math of the resonance-decay feed-down of the continuous spectra, shared by the kernels
// (decay.hip) and the CPU emulator (tests/native/decay_emulator.cpp).  DESIGN.md 7.6 has the derivation.
//
// The reference has no working routine (src/cpp/jail/emissionfunction_resonance_decays.cpp is in no makefile and
// starts with exit(-1)); this file defines one.  The formula is Sollfrank, Koch and Heinz, Z. Phys. C 52 (1991) 593.
//
// Spectra S[species][pT][phi][y] = dN/(dy pT dpT dphi), updated in place.  One channel R -> 1 + 2 (+ 3); for daughter 1
// with the other daughters' invariant mass^2 W2:
//     E* = (M^2 + m1^2 - W2) / 2M     p* = sqrt(E*^2 - m1^2)     mT^2 = pT^2 + m1^2     dY = asinh(p* / mT)
// two-body (W2 = m2^2):
//     dS1(pT, phi, y) = b / (4 pi p*)  int_-1^1 dv dY  int_0^pi dzeta  M MT / sqrt(mT^2 c^2 - pT^2)
//                                      [S_R(MT, phi + delta, Y) + S_R(MT, phi - delta, Y)]
//     c = cosh(v dY)   Y = y + v dY   MT = MTbar + dMT cos(zeta)
//     MTbar = M E* mT c / (mT^2 c^2 - pT^2)     dMT = M pT sqrt(E*^2 + pT^2 - mT^2 c^2) / (mT^2 c^2 - pT^2)
//     PT = sqrt(MT^2 - M^2)     delta = acos(clamp((MT mT c - M E*) / (PT pT), -1, 1))
// (SKH's double integral with MT -> zeta substituted, which removes both endpoint singularities; the jail file's
// prefactor M b / (8 p*) is the same with the pi / 2 of zeta = (1 + x) pi / 2 folded in).  Both integrals: 12-point
// Gauss-Legendre, nodes computed here in FP64.
// three-body: sum_k w_k x (two-body with W2 = s_k), s_k the 12 Gauss-Legendre nodes on [(m2 + m3)^2, (M - m1)^2],
//     w_k = x_k f(s_k) / sum_j x_j f(s_j),   f(s) = sqrt(((M+m1)^2 - s)((M-m1)^2 - s)(s - (m2+m3)^2)(s - (m2-m3)^2)) / s
// (SKH's g(s) normalised by the rule that integrates it: the weights sum to 1, no separate Q factor).
//
// Every daughter slot that is a chosen species receives its own term (identical daughters one term each); a slot's
// W2 is that of the OTHER daughter(s) (the jail file takes particle_2's mass for both slots: a slip, not reproduced).
// four-body (kept only by is3d_set_decays4): the same sum over the 12 nodes on [(m2 + m3 + m4)^2, (M - m1)^2] with
//     h(s) = sqrt(lambda(M^2, m1^2, s)) Phi3(s; m2, m3, m4) in place of f(s) (phi3 below: the flat four-body marginal of
//     the invariant mass^2 recoiling against daughter 1; the kernel sees two-body terms only)
// Skipped: 1-body rows (the stability marker), >= 4 bodies (is3d_set_decays4: >= 5; a 4-body row that is not open
// counts as closed) and closed 3-body channels (counted); a closed 2-body
// channel takes the jail rule (:239-256) M += Gamma_R / 4, m_i -= Gamma_i / 2 until it opens -- skipped and counted
// when every width is 0, a mass would go negative, or kAdjustCap rounds do not open it (never a loop, never an exit).
//
// Parent value S_R(MT, Phi, Y), in this order: (1) at each grid phi_j and the two bracketing y rows interpolate along
// MT over the abscissa MT_i = sqrt(pT_i^2 + M^2): linear in ln S where both bracketing values are > 0 (jail
// difference 4), else linear in S; outside the table the end interval's line continues, and that value is 0 when an
// end value is <= 0 or the upper line does not fall; (2) linear in Y between the two rows, 0 outside [y_0, y_n-1]
// (ny = 1: no Y dependence); (3) linear and periodic in Phi over the ascending phi table in [0, 2 pi).
//
// Order: a species decays after every channel that feeds it was applied (topological levels over the kept channels;
// within a level heavier parents first, then the higher chosen index; a cycle is an error).  Every output element
// sums its terms in one fixed order -- level, parent order, canonical channel order, slot, s node, v node, zeta node --
// so the result does not depend on the launch geometry or on the order the channels were listed in.
#pragma once
#include <math.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/is3d_amd.h"

#ifndef IS3D_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define IS3D_HD __host__ __device__ inline
#else
#define IS3D_HD inline
#endif
#endif

namespace is3d {
namespace decay {

constexpr int kGL = 12;                 // Gauss-Legendre points of the v, zeta and s rules
constexpr int kNodes = kGL * kGL;       // (v, zeta) nodes of one two-body term
constexpr long kAdjustCap = 100000;     // rounds of the closed-channel mass adjustment
constexpr double kPi = 3.14159265358979323846;

// one two-body term: a 2-body slot, or one s node of a 3-body slot.  coef = b w_k / (4 pi p*)
struct Sub {
  double M, m1, Estar, dY0;   // dY0 = p* (dY = asinh(p* / mT) depends on pT)
  double coef;
  int parent, pad;
};

// the (v, zeta) rule: x, w on [-1, 1]; cz = cos(zeta), wz = w pi / 2
struct Rule {
  double x[kGL], w[kGL], cz[kGL], wz[kGL];
};

// what one (v, zeta) node needs of the parent, the same for every phi
struct Node {
  double weight;   // coef w_v dY w_zeta M MT / sqrt(mT^2 c^2 - pT^2)
  double delta;
  double t;        // position in the MT bracket [i0, i0 + 1] (outside [0, 1]: extrapolation)
  double ty;
  int i0, iy0;     // iy0 < 0: Y outside the y table
};

// largest i in [0, n - 2] with x_i <= v (clamped): the bracket of a table ascending in x
template <class F>
IS3D_HD int bracket(int n, double v, F x) {
  int lo = 0, hi = n - 1;   // invariant: x(lo) <= v < x(hi) once v is inside
  if (n < 2) return 0;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (x(mid) <= v) lo = mid; else hi = mid;
  }
  return lo;
}

IS3D_HD Node node_eval(const Sub& s, const Rule& r, int iv, int iz, double pT, double y, int npT, const double* pTtab, int ny,
                       const double* ytab) {
  Node nd;
  const double mT2 = pT * pT + s.m1 * s.m1, mT = sqrt(mT2);
  const double dY = asinh(s.dY0 / mT);
  const double v = r.x[iv];
  const double c = cosh(v * dY);
  const double den = mT2 * c * c - pT * pT;
  const double MTbar = s.M * s.Estar * mT * c / den;
  const double rad = s.Estar * s.Estar + pT * pT - mT2 * c * c;
  const double dMT = s.M * pT * sqrt(rad > 0.0 ? rad : 0.0) / den;
  const double MT = MTbar + dMT * r.cz[iz];
  nd.weight = s.coef * r.w[iv] * dY * r.wz[iz] * s.M * MT / sqrt(den);
  const double PT2 = MT * MT - s.M * s.M;
  const double PT = sqrt(PT2 > 0.0 ? PT2 : 0.0);
  const double d = PT * pT;
  double cd = d > 0.0 ? (MT * mT * c - s.M * s.Estar) / d : 1.0;
  cd = cd > 1.0 ? 1.0 : (cd < -1.0 ? -1.0 : cd);
  nd.delta = acos(cd);
  const double M2 = s.M * s.M;
  nd.i0 = bracket(npT, MT, [&](int i) { return sqrt(pTtab[i] * pTtab[i] + M2); });
  const double a0 = sqrt(pTtab[nd.i0] * pTtab[nd.i0] + M2), a1 = sqrt(pTtab[nd.i0 + 1] * pTtab[nd.i0 + 1] + M2);
  nd.t = (MT - a0) / (a1 - a0);
  nd.iy0 = 0;
  nd.ty = 0.0;
  if (ny > 1) {
    const double Y = y + v * dY;
    if (!(Y >= ytab[0] && Y <= ytab[ny - 1])) {
      nd.iy0 = -1;
    } else {
      nd.iy0 = bracket(ny, Y, [&](int i) { return ytab[i]; });
      nd.ty = (Y - ytab[nd.iy0]) / (ytab[nd.iy0 + 1] - ytab[nd.iy0]);
    }
  }
  return nd;
}

// the log table of a parent: ln S where S > 0, else NaN (the interpolation then reads S itself)
IS3D_HD double log_or_nan(double s) { return s > 0.0 ? log(s) : NAN; }

// step 1 at one (phi_j, y row): a, b = S at the bracket's two MT nodes (read only when a log is NaN)
IS3D_HD double interp_mt(const double* S, const double* L, long ia, long ib, double t) {
  const double la = L[ia], lb = L[ib];
  const bool pos = la == la && lb == lb;   // both values > 0
  if (t >= 0.0 && t <= 1.0) {
    if (pos) return exp(la + t * (lb - la));
    const double a = S[ia], b = S[ib];
    return a + t * (b - a);
  }
  if (!pos) return 0.0;
  if (t > 1.0 && !(lb < la)) return 0.0;
  return exp(la + t * (lb - la));
}

// steps 1 and 2: the parent's value at (MT, phi_j, Y); S, L: the parent's slab [pT][phi][y]
IS3D_HD double parent_value(const double* S, const double* L, int nphi, int ny, const Node& nd, int j) {
  if (nd.iy0 < 0) return 0.0;
  const long ia = ((long)nd.i0 * nphi + j) * ny + nd.iy0, ib = ia + (long)nphi * ny;
  const double f0 = interp_mt(S, L, ia, ib, nd.t);
  if (ny == 1) return f0;
  const double f1 = interp_mt(S, L, ia + 1, ib + 1, nd.t);
  return (1.0 - nd.ty) * f0 + nd.ty * f1;
}

// step 3: the row g[nphi] at the angle Phi, linear and periodic; the wrap interval is phi_n-1 .. phi_0 + 2 pi
IS3D_HD double phi_interp(const double* g, const double* phitab, int nphi, double Phi) {
  if (nphi == 1) return g[0];
  const double two_pi = 2.0 * kPi;
  Phi -= floor(Phi / two_pi) * two_pi;
  if (!(Phi < two_pi)) Phi = 0.0;   // rounding of a tiny negative angle
  int j0, j1;
  double left, right;
  if (Phi < phitab[0]) {
    j0 = nphi - 1; j1 = 0; left = phitab[nphi - 1] - two_pi; right = phitab[0];
  } else if (Phi >= phitab[nphi - 1]) {
    j0 = nphi - 1; j1 = 0; left = phitab[nphi - 1]; right = phitab[0] + two_pi;
  } else {
    j0 = bracket(nphi, Phi, [&](int i) { return phitab[i]; });
    j1 = j0 + 1; left = phitab[j0]; right = phitab[j1];
  }
  const double u = (Phi - left) / (right - left);
  return (1.0 - u) * g[j0] + u * g[j1];
}

// ---------------------------------------------------------------------------------------------------------
// host: Gauss-Legendre rule, channel table -> plan
// ---------------------------------------------------------------------------------------------------------
// n-point Gauss-Legendre nodes (ascending) and weights on [-1, 1]: Newton on P_n from the Chebyshev guess
inline void gauss_legendre(int n, double* x, double* w) {
  for (int i = 0; i < n; i++) {
    double z = cos(kPi * (i + 0.75) / (n + 0.5)), pp = 1.0;
    for (int it = 0; it < 100; it++) {
      double p1 = 1.0, p2 = 0.0;
      for (int j = 1; j <= n; j++) {
        const double p3 = p2;
        p2 = p1;
        p1 = ((2.0 * j - 1.0) * z * p2 - (j - 1.0) * p3) / j;
      }
      pp = n * (z * p1 - p2) / (z * z - 1.0);
      const double dz = p1 / pp;
      z -= dz;
      if (fabs(dz) < 1e-16) break;
    }
    x[n - 1 - i] = z;
    w[n - 1 - i] = 2.0 / ((1.0 - z * z) * pp * pp);
  }
}

inline Rule make_rule() {
  Rule r;
  gauss_legendre(kGL, r.x, r.w);
  for (int i = 0; i < kGL; i++) {
    r.cz[i] = cos(0.5 * kPi * (1.0 + r.x[i]));
    r.wz[i] = r.w[i] * 0.5 * kPi;
  }
  return r;
}

// a kept channel: the row as given (slots past n_body cleared) with the masses the closed-channel rule left it with
struct Kept { is3d_decay_channel4 c; double M, m[4]; };

constexpr int kPhi3 = 24;               // Gauss-Legendre points of the inner rule of a 4-body slot (Phi3 below)

// the launch plan: levels of parents, and per level the receivers with their two-body terms in summation order
struct Plan {
  // what every consumer of the channel table needs (the feed-down below, the Monte Carlo decays of decay_mc_math.h):
  // the kept channels in canonical order, species p's being kept[first[p] .. first[p + 1]), and the level at which a
  // parent decays (-1: no kept channel)
  std::vector<Kept> kept;
  std::vector<int> first, level_of;
  std::vector<Sub> subs;
  std::vector<int> recv_d, recv_s0, recv_s1;   // receiver r: daughter species, its terms subs[s0 .. s1)
  std::vector<int> lvl_r0;                     // level l: receivers [lvl_r0[l], lvl_r0[l + 1])
  std::vector<int> par, lvl_p0;                // ... and parents par[lvl_p0[l] .. lvl_p0[l + 1])
  long slots = 0;                              // daughter slots that receive a term (the bench's work unit)
  is3d_decay_stats stats{};
  int levels() const { return (int)lvl_p0.size() - 1; }
};

// a two-body channel is open when both daughters get a rest-frame momentum p* > 0 in floating point (a channel a few
// ulp above its threshold can round p*^2 to <= 0; it counts as closed)
inline bool open_two_body(double M, double m1, double m2) {
  if (!(M > m1 + m2)) return false;
  const double e1 = (M * M + m1 * m1 - m2 * m2) / (2.0 * M), e2 = (M * M + m2 * m2 - m1 * m1) / (2.0 * M);
  return e1 * e1 - m1 * m1 > 0.0 && e2 * e2 - m2 * m2 > 0.0;
}

// the inner rule of a 4-body slot: n-point Gauss-Legendre on [-1, 1]
struct Inner {
  std::vector<double> x, w;
};
inline Inner make_inner(int n) {
  Inner in;
  in.x.resize((size_t)n);
  in.w.resize((size_t)n);
  gauss_legendre(n, in.x.data(), in.w.data());
  return in;
}

// Phi3(s; a, b, c) = int_t0^t1 dt sqrt(lambda(s, a^2, t) lambda(t, b^2, c^2)) / (s t), t0 = (b + c)^2, t1 = (sqrt s - a)^2:
// the three-body phase space of invariant mass^2 s up to a constant.  lambda(s, a^2, t) = (t1 - t)((sqrt s + a)^2 - t)
// and lambda(t, b^2, c^2) = (t - t0)(t - (b - c)^2): the integrand ends in a square root at both ends.  With
// t = tm - th cos(theta), tm = (t0 + t1) / 2, th = (t1 - t0) / 2: sqrt((t - t0)(t1 - t)) = th sin(theta) and
// dt = th sin(theta) dtheta, so
//     Phi3 = th^2 int_0^pi dtheta sin^2(theta) sqrt(((sqrt s + a)^2 - t)(t - (b - c)^2)) / (s t)
// whose integrand is smooth on [0, pi]: Gauss-Legendre in theta (kPhi3 points; doubling them changes the weights of
// the UrQMD 4-body rows by less than DESIGN.md 7.6 records)
inline double phi3(const Inner& in, double s, double a, double b, double c) {
  const double rs = sqrt(s), t0 = (b + c) * (b + c), t1 = (rs - a) * (rs - a);
  if (!(rs > a) || !(t1 > t0)) return 0.0;
  const double tm = 0.5 * (t0 + t1), th = 0.5 * (t1 - t0), up = (rs + a) * (rs + a), dn = (b - c) * (b - c);
  double sum = 0.0;
  for (size_t i = 0; i < in.x.size(); i++) {
    const double theta = 0.5 * kPi * (1.0 + in.x[i]), sn = sin(theta), t = tm - th * cos(theta);
    const double q = (up - t) * (t - dn);
    sum += in.w[i] * sn * sn * sqrt(q > 0.0 ? q : 0.0) / (s * t);
  }
  return th * th * 0.5 * kPi * sum;
}

// the two-body terms of one daughter slot; false (nothing usable pushed) when a term has no p* > 0 or the 3- or 4-body
// weights have no positive norm in floating point.  nother = 3 (needs `in`): the s rule runs over
// [(ma + mb + mc)^2, (M - m1)^2] with the density h(s) = sqrt(lambda(M^2, m1^2, s)) Phi3(s; ma, mb, mc), the flat
// four-body marginal of the invariant mass^2 recoiling against the slot's daughter
inline bool push_terms(std::vector<Sub>& out, const Rule& r, int parent, double b, double M, double m1, int nother,
                       const double* mo, const Inner* in = nullptr) {
  if (nother == 1) {
    Sub s{};
    s.M = M; s.m1 = m1; s.parent = parent;
    s.Estar = (M * M + m1 * m1 - mo[0] * mo[0]) / (2.0 * M);
    const double p2 = s.Estar * s.Estar - m1 * m1;
    s.dY0 = sqrt(p2 > 0.0 ? p2 : 0.0);
    s.coef = b / (4.0 * kPi * s.dY0);
    out.push_back(s);
    return p2 > 0.0;
  }
  const double hi = (M - m1) * (M - m1);
  double sk[kGL], fk[kGL], norm = 0.0;
  if (nother == 2) {
    const double lo = (mo[0] + mo[1]) * (mo[0] + mo[1]), dm2 = (mo[0] - mo[1]) * (mo[0] - mo[1]);
    for (int k = 0; k < kGL; k++) {
      sk[k] = lo + 0.5 * (hi - lo) * (1.0 + r.x[k]);
      const double q = ((M + m1) * (M + m1) - sk[k]) * (hi - sk[k]) * (sk[k] - lo) * (sk[k] - dm2);
      fk[k] = r.w[k] * sqrt(q > 0.0 ? q : 0.0) / sk[k];
      norm += fk[k];
    }
  } else {
    if (!in) return false;
    const double lo = (mo[0] + mo[1] + mo[2]) * (mo[0] + mo[1] + mo[2]);
    for (int k = 0; k < kGL; k++) {
      sk[k] = lo + 0.5 * (hi - lo) * (1.0 + r.x[k]);
      const double q = ((M + m1) * (M + m1) - sk[k]) * (hi - sk[k]);
      fk[k] = r.w[k] * sqrt(q > 0.0 ? q : 0.0) * phi3(*in, sk[k], mo[0], mo[1], mo[2]);
      norm += fk[k];
    }
  }
  if (!(norm > 0.0)) return false;
  bool ok = true;
  for (int k = 0; k < kGL; k++) {
    Sub s{};
    s.M = M; s.m1 = m1; s.parent = parent;
    s.Estar = (M * M + m1 * m1 - sk[k]) / (2.0 * M);
    const double p2 = s.Estar * s.Estar - m1 * m1;
    s.dY0 = sqrt(p2 > 0.0 ? p2 : 0.0);
    s.coef = b * (fk[k] / norm) / (4.0 * kPi * s.dY0);
    ok = ok && p2 > 0.0;
    out.push_back(s);
  }
  return ok;
}

// a three-body channel is open when M > m1 + m2 + m3 and, in floating point, every slot's s rule has a positive norm
// and a p* > 0 at every node (a channel a few ulp above its threshold has neither; it counts as closed)
inline bool open_three_body(const Rule& r, double M, const double* m) {
  if (!(M > m[0] + m[1] + m[2])) return false;
  std::vector<Sub> tmp;
  for (int s = 0; s < 3; s++) {
    const double mo[2] = {m[(s + 1) % 3], m[(s + 2) % 3]};
    if (!push_terms(tmp, r, 0, 1.0, M, m[s], 2, mo)) return false;
  }
  return true;
}

// a four-body channel is open when M > m1 + m2 + m3 + m4 and, in floating point, every slot's s rule has a positive
// norm and a p* > 0 at every node
inline bool open_four_body(const Rule& r, const Inner& in, double M, const double* m) {
  if (!(M > m[0] + m[1] + m[2] + m[3])) return false;
  std::vector<Sub> tmp;
  for (int s = 0; s < 4; s++) {
    const double mo[3] = {m[(s + 1) % 4], m[(s + 2) % 4], m[(s + 3) % 4]};
    if (!push_terms(tmp, r, 0, 1.0, M, m[s], 3, mo, &in)) return false;
  }
  return true;
}

// Channel table -> plan.  species_mass[npart]: the chosen species' masses (the order of parents within a level).
// keep_four: open 4-body rows are kept and rows with >= 5 bodies skipped (is3d_set_decays4); without it every row
// with >= 4 bodies is skipped (is3d_set_decays).  phi3_points: the inner rule of a 4-body slot (kPhi3; a test doubles it).
// Returns an empty string, or what is wrong with the table (an IS3D_ERR_ARG for the caller).
inline std::string build_plan(Plan& P, const Rule& r, int npart, const double* species_mass, int n,
                              const is3d_decay_channel4* ch, bool keep_four, int phi3_points = kPhi3) {
  P = Plan{};
  P.stats.channels = n;
  std::vector<Kept>& kept = P.kept;
  const Inner inner = keep_four ? make_inner(phi3_points) : Inner{};
  const int max_body = keep_four ? 4 : 3;
  for (int i = 0; i < n; i++) {
    const is3d_decay_channel4& c = ch[i];
    if (c.n_body < 1) return "decay channel " + std::to_string(i) + ": n_body < 1";
    if (c.parent < 0 || c.parent >= npart) return "decay channel " + std::to_string(i) + ": parent index out of range";
    for (int k = 0; k < std::min(c.n_body, max_body); k++)
      if (c.daughter[k] < -1 || c.daughter[k] >= npart)
        return "decay channel " + std::to_string(i) + ": daughter index out of range";
    if (c.n_body == 1) continue;
    if (c.n_body > max_body) {
      P.stats.skipped_many_body++;
      P.stats.branching_skipped += c.branching;
      continue;
    }
    Kept k{c, c.mass_parent, {c.mass[0], c.mass[1], c.n_body >= 3 ? c.mass[2] : 0.0, c.n_body == 4 ? c.mass[3] : 0.0}};
    // the slots past n_body are the caller's leftovers: they must not reach the canonical order
    for (int d = c.n_body; d < 4; d++) { k.c.daughter[d] = -1; k.c.mass[d] = 0.0; k.c.width[d] = 0.0; }
    bool open = true;
    if (c.n_body == 4) {
      open = open_four_body(r, inner, k.M, k.m);
    } else if (c.n_body == 3) {
      open = open_three_body(r, k.M, k.m);
    } else if (!open_two_body(k.M, k.m[0], k.m[1])) {
      const bool can = c.width_parent > 0.0 || c.width[0] > 0.0 || c.width[1] > 0.0;
      open = false;
      for (long it = 0; can && it < kAdjustCap; it++) {
        k.M += 0.25 * c.width_parent;
        k.m[0] -= 0.5 * c.width[0];
        k.m[1] -= 0.5 * c.width[1];
        if (k.m[0] < 0.0 || k.m[1] < 0.0) break;
        if (open_two_body(k.M, k.m[0], k.m[1])) { open = true; break; }
      }
      if (open) P.stats.adjusted++;
    }
    if (!open) {
      P.stats.skipped_closed++;
      P.stats.branching_skipped += c.branching;
      continue;
    }
    P.stats.kept++;
    kept.push_back(k);
  }
  // canonical channel order: whatever order the caller listed them in
  auto key_less = [&](const Kept& a, const Kept& b) {
    if (a.c.parent != b.c.parent) return a.c.parent < b.c.parent;
    if (a.c.n_body != b.c.n_body) return a.c.n_body < b.c.n_body;
    for (int k = 0; k < 3; k++) if (a.c.daughter[k] != b.c.daughter[k]) return a.c.daughter[k] < b.c.daughter[k];
    if (a.c.branching != b.c.branching) return a.c.branching < b.c.branching;
    if (a.M != b.M) return a.M < b.M;
    for (int k = 0; k < 3; k++) if (a.m[k] != b.m[k]) return a.m[k] < b.m[k];
    // the fourth slot after every earlier key: plans without a 4-body row keep their order
    if (a.c.daughter[3] != b.c.daughter[3]) return a.c.daughter[3] < b.c.daughter[3];
    if (a.m[3] != b.m[3]) return a.m[3] < b.m[3];
    return false;
  };
  std::stable_sort(kept.begin(), kept.end(), key_less);
  // levels (Kahn by rounds): indeg[d] = kept slots that feed d
  std::vector<int> indeg(npart, 0);
  std::vector<int>& first = P.first;
  first.assign((size_t)npart + 1, 0);
  P.level_of.assign((size_t)npart, -1);
  std::vector<char> is_parent(npart, 0), done(npart, 0);
  for (const Kept& k : kept) {
    is_parent[k.c.parent] = 1;
    for (int s = 0; s < k.c.n_body; s++) if (k.c.daughter[s] >= 0) indeg[k.c.daughter[s]]++;
  }
  // kept is sorted by parent: first[p] .. first[p + 1] are p's channels
  for (const Kept& k : kept) first[k.c.parent + 1]++;
  for (int p = 0; p < npart; p++) first[p + 1] += first[p];
  long left = 0;
  for (int p = 0; p < npart; p++) left += is_parent[p];
  P.lvl_r0.push_back(0);
  P.lvl_p0.push_back(0);
  while (left > 0) {
    std::vector<int> lvl;
    for (int p = 0; p < npart; p++) if (is_parent[p] && !done[p] && indeg[p] == 0) lvl.push_back(p);
    if (lvl.empty()) return "the decay channels contain a cycle";
    std::sort(lvl.begin(), lvl.end(), [&](int a, int b) {
      if (species_mass[a] != species_mass[b]) return species_mass[a] > species_mass[b];
      return a > b;
    });
    std::vector<int> recv;
    for (int p : lvl) {
      done[p] = 1;
      P.level_of[p] = (int)P.lvl_p0.size() - 1;
      left--;
      for (int q = first[p]; q < first[p + 1]; q++)
        for (int s = 0; s < kept[q].c.n_body; s++) {
          const int d = kept[q].c.daughter[s];
          if (d < 0) continue;
          indeg[d]--;
          recv.push_back(d);
        }
    }
    std::sort(recv.begin(), recv.end());
    recv.erase(std::unique(recv.begin(), recv.end()), recv.end());
    for (int d : recv) {
      P.recv_d.push_back(d);
      P.recv_s0.push_back((int)P.subs.size());
      for (int p : lvl)
        for (int q = first[p]; q < first[p + 1]; q++) {
          const Kept& k = kept[q];
          for (int s = 0; s < k.c.n_body; s++) {
            if (k.c.daughter[s] != d) continue;
            double mo[3];
            int no = 0;
            for (int o = 0; o < k.c.n_body; o++) if (o != s) mo[no++] = k.m[o];
            push_terms(P.subs, r, p, k.c.branching, k.M, k.m[s], no, mo, &inner);
            P.slots++;
          }
        }
      P.recv_s1.push_back((int)P.subs.size());
    }
    for (int p : lvl) P.par.push_back(p);
    P.lvl_r0.push_back((int)P.recv_d.size());
    P.lvl_p0.push_back((int)P.par.size());
  }
  P.stats.levels = P.levels();
  return "";
}

// a row of three daughter slots in the four-slot form (slot 3 empty)
inline is3d_decay_channel4 widen(const is3d_decay_channel& c) {
  is3d_decay_channel4 w{};
  w.parent = c.parent; w.n_body = c.n_body; w.branching = c.branching;
  w.mass_parent = c.mass_parent; w.width_parent = c.width_parent;
  for (int k = 0; k < 3; k++) { w.daughter[k] = c.daughter[k]; w.mass[k] = c.mass[k]; w.width[k] = c.width[k]; }
  w.daughter[3] = -1;
  return w;
}

// the plan of is3d_set_decays: rows of three slots, every row with >= 4 bodies skipped
inline std::string build_plan(Plan& P, const Rule& r, int npart, const double* species_mass, int n,
                              const is3d_decay_channel* ch) {
  std::vector<is3d_decay_channel4> wide((size_t)(n > 0 ? n : 0));
  for (int i = 0; i < n; i++) wide[(size_t)i] = widen(ch[i]);
  return build_plan(P, r, npart, species_mass, n, wide.data(), false);
}

// pT > 0 and ascending; phi ascending in [0, 2 pi); y ascending (3+1D)
inline std::string check_grid(int npT, const double* pT, int nphi, const double* phi, int ny, const double* y) {
  if (npT < 2) return "the feed-down needs at least two pT points";
  for (int i = 0; i < npT; i++) {
    if (!(pT[i] > 0.0)) return "the feed-down needs pT > 0";
    if (i && !(pT[i] > pT[i - 1])) return "the feed-down needs an ascending pT table";
  }
  for (int j = 0; j < nphi; j++)
    if (!(phi[j] >= 0.0 && phi[j] < 2.0 * kPi) || (j && !(phi[j] > phi[j - 1])))
      return "the feed-down needs a phi table ascending in [0, 2 pi)";
  for (int k = 1; k < ny; k++)
    if (!(y[k] > y[k - 1])) return "the feed-down needs an ascending y table";
  return "";
}

}  // namespace decay
}  // namespace is3d
