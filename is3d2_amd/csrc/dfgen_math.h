// dfgen_math.h -- host/device math of the delta-f coefficient generator, shared by the kernel (dfgen.hip) and the CPU
// emulator (tests/native/dfgen_emulator.cpp).  DESIGN.md 7.9 has the method.
//
// The reference's offline generator (generate_delta_f_coefficients/*/df_vh_dimensionless: deltaf_table.cpp,
// thermal_integrands.cpp, gauss_integration.cpp) on one (T, muB) point: 20 hadron-gas integrals, each a sum over the
// hadron list of a Gauss-Laguerre sum over pbar = p / T, closed into the ten coefficients
//     c0 c1 c2 c3 c4 (14-moment, deltaf_table.cpp:215-225)   F G betabulk betaV betapi (Chapman-Enskog, :354-366)
// in the order of is3d_set_df_tables, scaled by the powers of T the files hold.
//
// With mbar = m / T, Ebar = sqrt(pbar^2 + mbar^2), x = Ebar - b muB / T and the node (pbar_k, w_k) of family alpha:
//     f = 1 / (e^x + Theta)                g = e^x / (e^x + Theta)^2
// written from r = e^-x as d = 1 / (1 + Theta r), f = r d, g = f d: one exp and one reciprocal, and a large x
// underflows to 0 where the reference's e^x / (e^x + Theta)^2 would be inf / inf.  Every reference integrand is
// e^pbar x (a power of pbar and Ebar) x (f or g), so a node carries W_k = w_k e^{pbar_k} (node_weight, built once
// on the host) and the kernel of each integral is
//     alpha = 1 (baryons only)   N10 = b p g            nB = b p f         M10 = b^2 p g        M11 = b^2 p^3 / E^2 g
//     alpha = 2                  J20 = E g              J21 = p^2 / E g    e = E f              p = p^2 / E f
//               (baryons only)   M20 = b^2 E g          M21 = b^2 p^2 / E g                     N20 = b E g
//     alpha = 3                  J30 = E^2 / p g        J32 = p^3 / E^2 g
//               (baryons only)   N30 = b E^2 / p g      N31 = b p g
//     alpha = 4                  J40 = E^3 / p^2 g      J41 = E g
// A20, A21, B10 are m^2 x the integrands of J20, J21, N10.  Hadrons of mass 0 (the photon) are skipped.
//
// Order of the sums (the same on the host and on the device, so a value is a pure function of the hadron list, the
// Gauss-Laguerre table, T and muB): a lane owns the nodes lane, lane + 64, ... of one family; for each node it adds the
// degeneracy-weighted terms hadron by hadron in list order, multiplies the sum by W_k and adds it to the lane's total;
// the 64 lane totals are summed by the xor tree 32, 16, 8, 4, 2, 1; the prefactor T^n / (2 pi^2 hbarc^3 [x 3 | 15]) is
// applied to the finished sum (the reference applies it to every hadron's term: equal up to rounding).  The baryon-only
// sums of a list whose baryons are each followed by their antibaryon are exactly 0 at muB = 0, as in the reference: the
// two terms are exact negatives and no product is fused into the running sum (add_hadron).
#pragma once
#include <math.h>

#ifndef IS3D_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define IS3D_HD __host__ __device__ inline
#else
#define IS3D_HD inline
#endif
#endif

namespace is3d {
namespace dfgen {

constexpr double kHbarC = 0.197327053;   // GeV fm (deltaf_table.cpp:18)
constexpr double kPi = 3.14159265358979323846;
constexpr int kLanes = 64;               // lanes of a family's wavefront
constexpr int kFamilies = 4;             // Gauss-Laguerre alpha = 1 .. 4: rows 1 .. 4 of the engine's table
constexpr int kHadronStride = 4;         // a hadron row: mass, degeneracy, baryon, sign (Theta)

// slots of the 20 integrals
enum Slot : int {
  J20, J21, J40, J41, N10, N30, N31, M20, M21, A20, A21, B10,   // 14-moment
  NB, EN, PR, J30, J32, N20, M10, M11,                           // Chapman-Enskog
  kSlots
};

// codes of one point: the 14-moment block in bits 0-3, the Chapman-Enskog block in bits 4-7 (the reference runs the
// whole grid of the first block before the second, first_error)
enum Code : int { OK = 0, BULK_ZERO = 1, DIFFUSION_ZERO = 2, SHEAR_ZERO = 3, NOT_FINITE = 4 };

IS3D_HD const char* message(int code) {
  switch (code) {
    case BULK_ZERO: return "Bulk denominator is zero";
    case DIFFUSION_ZERO: return "Diffusion denominator is zero";
    case SHEAR_ZERO: return "Shear denominator is zero";
    case NOT_FINITE: return "a delta-f coefficient is not finite";
    default: return "";
  }
}

IS3D_HD double node_weight(double root, double weight) { return weight * exp(root); }

// the sums a family keeps (9 at most) and the slot each goes to
template <int FAM> struct Family;
template <> struct Family<1> { static constexpr int n = 5; IS3D_HD static int slot(int i) { const int s[5] = {N10, B10, NB, M10, M11}; return s[i]; } };
template <> struct Family<2> { static constexpr int n = 9; IS3D_HD static int slot(int i) { const int s[9] = {J20, J21, A20, A21, EN, PR, M20, M21, N20}; return s[i]; } };
template <> struct Family<3> { static constexpr int n = 4; IS3D_HD static int slot(int i) { const int s[4] = {J30, J32, N30, N31}; return s[i]; } };
template <> struct Family<4> { static constexpr int n = 2; IS3D_HD static int slot(int i) { const int s[2] = {J40, J41}; return s[i]; } };

// one hadron's terms at one node (pbar = p, p2 = p^2, rp = 1 / p), added to the family's sums s[Family<FAM>::n].
// mbar2 = (m / T)^2, a = b muB / T, dof = the degeneracy, m2 = m^2, b = the baryon number, th = Theta
template <int FAM>
IS3D_HD void add_hadron(double* s, double p, double p2, double rp, double mbar2, double a, double dof, double m2, double b,
                        double th) {
#pragma clang fp contract(off)   // a product is rounded before it is added: a baryon's term and its antibaryon's cancel exactly
  if constexpr (FAM == 1) { if (b == 0.0) return; }
  const double E2 = p2 + mbar2, E = sqrt(E2);
  const double r = exp(a - E), d = 1.0 / (1.0 + th * r);
  const double f = r * d, g = f * d;
  const double dg = dof * g;
  if constexpr (FAM == 1) {
    const double bp = b * p;
    s[0] += dg * bp;                       // N10
    s[1] += m2 * dg * bp;                  // B10
    s[2] += dof * f * bp;                  // nB
    s[3] += dg * b * bp;                   // M10
    s[4] += dg * b * bp * (p2 / E2);       // M11
  } else if constexpr (FAM == 2) {
    const double q = p2 / E, df = dof * f;
    s[0] += dg * E;                        // J20
    s[1] += dg * q;                        // J21
    s[2] += m2 * dg * E;                   // A20
    s[3] += m2 * dg * q;                   // A21
    s[4] += df * E;                        // e
    s[5] += df * q;                        // p
    if (b != 0.0) {
      s[6] += dg * b * b * E;              // M20
      s[7] += dg * b * b * q;              // M21
      s[8] += dg * b * E;                  // N20
    }
  } else if constexpr (FAM == 3) {
    const double u = E2 * rp;
    s[0] += dg * u;                        // J30
    s[1] += dg * (p * p2 / E2);            // J32
    if (b != 0.0) {
      s[2] += dg * b * u;                  // N30
      s[3] += dg * b * p;                  // N31
    }
  } else {
    s[0] += dg * (E * E2 * rp * rp);       // J40
    s[1] += dg * E;                        // J41
  }
}

// a lane's total of family FAM: nodes lane, lane + 64, ... of roots / wts[npts] (wts = node_weight), every hadron of
// had[nh][kHadronStride] in list order
template <int FAM>
IS3D_HD void lane_sums(double* tot, int lane, int npts, const double* roots, const double* wts, int nh, const double* had,
                       double T, double muB) {
  constexpr int n = Family<FAM>::n;
  for (int i = 0; i < n; i++) tot[i] = 0.0;
  for (int k = lane; k < npts; k += kLanes) {
    const double p = roots[k], p2 = p * p, rp = 1.0 / p;
    double s[n];
    for (int i = 0; i < n; i++) s[i] = 0.0;
    for (int h = 0; h < nh; h++) {
      const double m = had[kHadronStride * h];
      if (m == 0.0) continue;              // the photon
      const double dof = had[kHadronStride * h + 1], b = had[kHadronStride * h + 2], th = had[kHadronStride * h + 3];
      const double mbar = m / T;
      add_hadron<FAM>(s, p, p2, rp, mbar * mbar, b * muB / T, dof, m * m, b, th);
    }
    const double W = wts[k];
    for (int i = 0; i < n; i++) tot[i] += W * s[i];
  }
}

// the closing algebra: the finished sums I[kSlots] (no prefactors yet) -> out[10] in table order; returns the codes
IS3D_HD int close_point(const double* I, double T, double* out) {
  const double t2h = 2.0 * kPi * kPi * kHbarC * kHbarC * kHbarC;
  const double T2 = T * T, T3 = T2 * T, T4 = T2 * T2, T5 = T4 * T, T6 = T3 * T3;
  // 14-moment (deltaf_table.cpp:145-225)
  const double vJ20 = I[J20] * (T4 / t2h), vJ21 = I[J21] * (T4 / (3.0 * t2h));
  const double vJ40 = I[J40] * (T6 / t2h), vJ41 = I[J41] * (T6 / (3.0 * t2h));
  const double vN10 = I[N10] * (T3 / t2h), vN30 = I[N30] * (T5 / t2h), vN31 = I[N31] * (T5 / (3.0 * t2h));
  const double vM20 = I[M20] * (T4 / t2h), vM21 = I[M21] * (T4 / (3.0 * t2h));
  const double vA20 = I[A20] * (T4 / t2h), vA21 = I[A21] * (T4 / (3.0 * t2h)), vB10 = I[B10] * (T3 / t2h);
  // update 3/25
  const double bulk0 = (4.0 * vN30 - vB10) * vN30 - vM20 * (4.0 * vJ40 - vA20);
  const double bulk1 = (vB10 - vN30) * (4.0 * vJ40 - vA20) - (4.0 * vN30 - vB10) * (vA20 - vJ40);
  const double bulk2 = vM20 * (vA20 - vJ40) - (vB10 - vN30) * vN30;
  const double denom = (vA21 - vJ41) * bulk0 + vN31 * bulk1 + (4.0 * vJ41 - vA21) * bulk2;
  const double diff = vN31 * vN31 - vM21 * vJ41;
  out[0] = bulk0 / denom * T4;
  out[1] = bulk1 / denom * T3;
  out[2] = bulk2 / denom * T4;
  out[3] = vJ41 / diff * T4;
  out[4] = -vN31 / diff * T5;
  int grad = OK;
  if (vJ21 * bulk0 - vN31 * bulk1 + vJ41 * bulk2 == 0.0) grad = BULK_ZERO;      // the reference's checks, in its order
  else if (diff == 0.0) grad = DIFFUSION_ZERO;
  // Chapman-Enskog, alphaB form (deltaf_table.cpp:305-366)
  const double nB = I[NB] * (T3 / t2h), e = I[EN] * (T4 / t2h), pr = I[PR] * (T4 / (3.0 * t2h));
  const double vJ30 = I[J30] * (T5 / t2h), vJ32 = I[J32] * (T5 / (15.0 * t2h)), vN20 = I[N20] * (T4 / t2h);
  const double vM10 = I[M10] * (T3 / t2h), vM11 = I[M11] * (T3 / (3.0 * t2h));
  const double cd = vJ30 * vM10 - vN20 * vN20;
  const double G = ((e + pr) * vN20 - vJ30 * nB) / cd;
  const double F = T * T * (vN20 * nB - (e + pr) * vM10) / cd;
  const double betabulk = G * nB * T + F * (e + pr) / T + 5.0 * vJ32 / (3.0 * T);
  const double betaV = vM11 - nB * nB * T / (e + pr);
  const double betapi = vJ32 / T;
  out[5] = F / T;
  out[6] = G;
  out[7] = betabulk / T4;
  out[8] = betaV / T3;
  out[9] = betapi / T4;
  int ce = OK;
  if (betapi == 0.0) ce = SHEAR_ZERO;
  else if (betabulk == 0.0) ce = BULK_ZERO;
  else if (betaV == 0.0) ce = DIFFUSION_ZERO;
  for (int k = 0; k < 5; k++)
    if (grad == OK && !isfinite(out[k])) grad = NOT_FINITE;
  for (int k = 5; k < 10; k++)
    if (ce == OK && !isfinite(out[k])) ce = NOT_FINITE;
  return grad | (ce << 4);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// the point on the host, in the kernel's order.  roots / wts: [kFamilies][npts], family alpha = row alpha - 1
template <int FAM>
inline void family_host(double* I, int npts, const double* roots, const double* wts, int nh, const double* had, double T,
                        double muB) {
  constexpr int n = Family<FAM>::n;
  double lane[kLanes][n];
  for (int l = 0; l < kLanes; l++)
    lane_sums<FAM>(lane[l], l, npts, roots + (FAM - 1) * npts, wts + (FAM - 1) * npts, nh, had, T, muB);
  for (int off = kLanes / 2; off >= 1; off >>= 1) {     // every lane adds its xor partner, as the shuffles do
    double next[kLanes][n];
    for (int l = 0; l < kLanes; l++)
      for (int i = 0; i < n; i++) next[l][i] = lane[l][i] + lane[l ^ off][i];
    for (int l = 0; l < kLanes; l++)
      for (int i = 0; i < n; i++) lane[l][i] = next[l][i];
  }
  for (int i = 0; i < n; i++) I[Family<FAM>::slot(i)] = lane[0][i];
}

inline int point_host(int npts, const double* roots, const double* wts, int nh, const double* had, double T, double muB,
                      double* out) {
  double I[kSlots];
  family_host<1>(I, npts, roots, wts, nh, had, T, muB);
  family_host<2>(I, npts, roots, wts, nh, had, T, muB);
  family_host<3>(I, npts, roots, wts, nh, had, T, muB);
  family_host<4>(I, npts, roots, wts, nh, had, T, muB);
  return close_point(I, T, out);
}
#endif

// the first failing point in the reference's order (the 14-moment block over the whole grid, muB outer and T inner,
// then the Chapman-Enskog block); -1: none.  *code: its Code
inline long first_error(const int* codes, long n, int* code) {
  for (int shift = 0; shift <= 4; shift += 4)
    for (long i = 0; i < n; i++)
      if ((codes[i] >> shift) & 15) { *code = (codes[i] >> shift) & 15; return i; }
  *code = OK;
  return -1;
}

}  // namespace dfgen
}  // namespace is3d
