// polzn_math.h -- host/device math of the spin-polarization integral (mode 5), shared by k_polzn (polzn.hip)
// and the CPU emulator (tests/native/polzn_emulator.cpp).
//
// Reference: EmissionFunctionArray::calculate_spin_polzn (Polarization.cpp:25-263).  For a species (mass m,
// sign s), a momentum point (pT, phi, y) and a cell (eta: the cell's in 3+1D with w = 1; the eta-table node in
// 2+1D with y = 0 and w = eta weight x (eta_2 - eta_1), Polarization.cpp:58,68):
//
//   pt = mT cosh(y - eta), pn = (mT / tau) sinh(y - eta), px = pT cos phi, py = pT sin phi
//   p.dsigma = pt dat + px dax + py day + pn dan
//   u.p = pt ut - px ux - py uy - tau^2 pn un,  ut = sqrt(|1 + ux^2 + uy^2 + tau^2 un^2|)
//   f0 = 1 / (exp(u.p / T) + s)        T = Plasma::temperature (one value for the surface), no muB
//   S_mu += w (p.dsigma) f0 (1 - s f0) (-1 / (4 m)) bracket_mu(w^{ab}, p),   Snorm += w (p.dsigma) f0
//
// Decomposition: with T constant exp(-u.p / T) = x = b' ainv,
//   ainv = exp(M - mT A),  A = (ut cosh d - tau un sinh d) / T      per (cell, q, class, pT)     [Lane]
//   b'   = exp(Eb - M),    Eb = (px ux + py uy) / T                 per (cell, pT, phi)          [PhiTerm]
//   M    = pT sqrt(ux^2 + uy^2) / T >= Eb                           per (cell, pT)
// f0 = x / (1 + s x) and f0 (1 - s f0) = x / (1 + s x)^2.  p.dsigma and the four brackets are c0 + c_phi with c0 per
// (cell, q) x mT [QTerm, Lane] and c_phi per (cell, phi) [PhiTerm]; -1 / (4 m) is applied once, to the sum.
//
// Exactness: u is a unit timelike vector by construction of ut and p is on shell, so u.p >= m: x <= 1 and
// neither factor can overflow (both exponents are <= 0 up to rounding) -- every input stays on this path.  Large
// exponents are only shifted by M, never dropped.  The reference's exp(u.p / T) overflows to inf for
// u.p / T > 709.78 and that term is 1 / (inf + s) = 0 exactly; here x < 2^-1024 (= 1 / DBL_MAX to rounding) is
// set to 0, which also covers an underflow of either factor (then u.p / T > 745).
//
// Two deliberate departures from the reference:
//  1. Polarization.cpp:131-136 indexes the vorticity by the chunk-local cell while every other field uses the
//     global one, so past its first 10 000-cell chunk it pairs cells with the wrong vorticity.  Here the vorticity
//     of cell c is w[c] (identical for surfaces of <= 10 000 cells).
//  2. The reference writer (EmissionFunction.cpp:591) reads another index than the loop filled and, in 2+1D, loops
//     y_tab_length rows over one filled y slot; the host writer here prints on each row the value its
//     (y, phi, pT, species) labels name (host_io.cpp write_polzn_files).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define IS3D_PZ_HD __host__ __device__ __forceinline__
#else
#define IS3D_PZ_HD inline
#endif

namespace is3d {
namespace polzn {

// x below this is the reference's exp overflow: 1 / (inf + s) = 0
constexpr double kXmin = 5.562684646268003e-309;   // 2^-1024

struct Cell {      // 18 doubles
  double tau, eta, dat, dax, day, dan, ux, uy, un;
  double ut;       // sqrt(|1 + ux^2 + uy^2 + tau^2 un^2|)   (Polarization.cpp:126)
  double wtx, wty, wtn, wxy, wxn, wyn;
  double hT;       // sqrt(ux^2 + uy^2) / T: M = pT hT
  double pad;
};
constexpr int kCellDoubles = 18;

struct QTerm { double A, P, T, X, Y, N; };     // per (cell, q): q = y (3+1D) or the eta node (2+1D)
struct PhiTerm { double b, D, T, X, Y, N; };   // per (cell, phi) at one pT
struct Lane { double ainv, P0, T0, X0, Y0, N0; };

IS3D_PZ_HD void cell_finish(Cell& c, double T) {
  c.ut = sqrt(fabs(1.0 + c.ux * c.ux + c.uy * c.uy + c.tau * c.tau * c.un * c.un));
  c.hT = sqrt(c.ux * c.ux + c.uy * c.uy) / T;
  c.pad = 0.0;
}

// d = y - eta; w = 1 (3+1D) or eta weight x delta eta (2+1D), folded into p.dsigma's coefficient
IS3D_PZ_HD QTerm q_terms(const Cell& c, double d, double w, double T) {
  const double ch = cosh(d), sh = sinh(d), sht = sh / c.tau;
  QTerm q;
  q.A = (c.ut * ch - c.tau * c.un * sh) / T;
  q.P = w * (ch * c.dat + sht * c.dan);
  q.T = c.wxy * sht;
  q.X = c.wyn * ch + c.wty * sht;
  q.Y = -(c.wxn * ch + c.wtx * sht);
  q.N = c.wxy * ch;
  return q;
}

IS3D_PZ_HD PhiTerm phi_terms(const Cell& c, double px, double py, double pT, double T) {
  PhiTerm f;
  f.b = exp((px * c.ux + py * c.uy) / T - pT * c.hT);
  f.D = c.dax * px + c.day * py;
  f.T = c.wyn * px - c.wxn * py;
  f.X = -(c.wtn * py);
  f.Y = c.wtn * px;
  f.N = c.wtx * py - c.wty * px;
  return f;
}

IS3D_PZ_HD Lane lane_setup(const QTerm& q, double mT, double M) {
  Lane L;
  L.ainv = exp(M - mT * q.A);
  L.P0 = mT * q.P; L.T0 = mT * q.T; L.X0 = mT * q.X; L.Y0 = mT * q.Y; L.N0 = mT * q.N;
  return L;
}

// x = exp(-u.p / T) of one point, with the reference's overflow -> exactly 0
IS3D_PZ_HD double point_x(const Lane& L, const PhiTerm& F) {
  const double x = F.b * L.ainv;
  return x < kXmin ? 0.0 : x;
}

// acc[0..4] += S_t, S_x, S_y, S_n (without -1/(4m)), Snorm of one point; r = 1 / (1 + s x)
IS3D_PZ_HD void point_add(const Lane& L, const PhiTerm& F, double w, double x, double r, double* acc) {
  const double f0 = x * r, g = f0 * r;
  const double pds = fma(w, F.D, L.P0);
  const double h = pds * g;
  acc[0] = fma(h, L.T0 + F.T, acc[0]);
  acc[1] = fma(h, L.X0 + F.X, acc[1]);
  acc[2] = fma(h, L.Y0 + F.Y, acc[2]);
  acc[3] = fma(h, L.N0 + F.N, acc[3]);
  acc[4] = fma(pds, f0, acc[4]);
}

// KJ consecutive phi points of one (cell, lane).  Four denominators share one division (each is in (0, 2]: their
// product cannot overflow, and 1 - x > 0 for bosons since x <= exp(-m / T) < 1).
template <int KJ>
IS3D_PZ_HD void points(const Lane& L, const PhiTerm* F, double s, double w, double (*acc)[5]) {
  int j = 0;
  if constexpr (KJ >= 4) {
#pragma unroll
    for (; j + 4 <= KJ; j += 4) {
      const double x0 = point_x(L, F[j]), x1 = point_x(L, F[j + 1]), x2 = point_x(L, F[j + 2]), x3 = point_x(L, F[j + 3]);
      const double d0 = fma(s, x0, 1.0), d1 = fma(s, x1, 1.0), d2 = fma(s, x2, 1.0), d3 = fma(s, x3, 1.0);
      const double p01 = d0 * d1, p23 = d2 * d3;
      const double r = 1.0 / (p01 * p23);
      const double r01 = r * p23, r23 = r * p01;
      point_add(L, F[j], w, x0, r01 * d1, acc[j]);
      point_add(L, F[j + 1], w, x1, r01 * d0, acc[j + 1]);
      point_add(L, F[j + 2], w, x2, r23 * d3, acc[j + 2]);
      point_add(L, F[j + 3], w, x3, r23 * d2, acc[j + 3]);
    }
  }
#pragma unroll
  for (; j < KJ; j++) {
    const double x = point_x(L, F[j]);
    point_add(L, F[j], w, x, 1.0 / fma(s, x, 1.0), acc[j]);
  }
}

}  // namespace polzn
}  // namespace is3d
