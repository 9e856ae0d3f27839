// sampler_bins.h -- host/device binning math of the sampler's test_sampler = 1 distributions, shared by the sampling
// kernel (sampler.hip, k_sample's binned variants) and the CPU emulator (tests/native/sampler_bins_emulator.cpp).
//
// Reference: BinSampledParticle.cpp:9-133 (sample_dN_dy, sample_dN_deta, sample_dN_dphipdy, sample_dN_2pipTdpTdy,
// sample_vn, sample_dN_dX), with the bin widths of EmissionFunction.cpp:223-247.  A particle outside a histogram's
// range is dropped from that histogram only; a wrapped angle that rounds to exactly 2 pi lands in index phip_bins and
// is dropped, as there.  dN_2pipTdpTdy_count and pT_count have the same condition and are one array here.
//
// Host and device agree bit for bit in everything but the last bits of atan2 and log: px^2 + py^2 and x^2 + y^2 and the
// harmonic recurrence are computed without FMA contraction (clang: the pragma below; g++: build with
// -ffp-contract=off), and the subtractions, divisions and square roots of the index formulas are exactly rounded.
//
// Sums.  Counts are 64-bit integers.  The vn sums are fixed-point: every cos(k phi), sin(k phi) is rounded to a
// multiple of the quantum q = 2^-32 (kVnQuantum) and added as a signed 64-bit integer, converted to double once at the
// end.  Integer addition is exact, so no sum depends on the order of arrival, the batches, the cell windows or the
// shards; the quantisation is at most q / 2 per particle and a bin holds up to 2^31 particles.
//
// Harmonics come from (px / pT, py / pT) by the complex-power recurrence, seven steps of a few ulp each, instead of one
// atan2 and 14 trigonometric calls; they agree with cos(k phi), sin(k phi) to rounding (1e-13 bounds it).
//
// Layout of a histogram (8-byte words): counts, each part [npart][bins] in chosen-species order,
//     dN_dy | dN_deta | dN_dphipdy | pT | tau | r | phis
// then the vn sums [2][7][npart][pT_bins], real then imaginary (in the engine's buffers: their integer form).
#pragma once
#include <cmath>
#include <cstdint>

#include "sampler_math.h"

namespace is3d {
namespace sampler {

static constexpr int kVnMax = 7;                       // v_1 .. v_7 (K_MAX)
static constexpr double kVnScale = 4294967296.0;       // 1 / q
static constexpr double kVnQuantum = 1.0 / 4294967296.0;

struct Bins {
  double pT_min, pT_width, y_cut, y_width, phip_width, eta_cut, eta_width, tau_min, tau_width, r_min, r_width;
  int pT_bins, y_bins, phip_bins, eta_bins, tau_bins, r_bins;
};

// widths as EmissionFunction.cpp:223-247
IS3D_HD Bins make_bins(double pT_min, double pT_max, int pT_bins, double y_cut, int y_bins, int phip_bins, double eta_cut,
                       int eta_bins, double tau_min, double tau_max, int tau_bins, double r_min, double r_max, int r_bins) {
  Bins b;
  b.pT_min = pT_min; b.pT_bins = pT_bins; b.pT_width = (pT_max - pT_min) / (double)pT_bins;
  b.y_cut = y_cut; b.y_bins = y_bins; b.y_width = 2.0 * y_cut / (double)y_bins;
  b.phip_bins = phip_bins; b.phip_width = kTwoPi / (double)phip_bins;
  b.eta_cut = eta_cut; b.eta_bins = eta_bins; b.eta_width = 2.0 * eta_cut / (double)eta_bins;
  b.tau_min = tau_min; b.tau_bins = tau_bins; b.tau_width = (tau_max - tau_min) / (double)tau_bins;
  b.r_min = r_min; b.r_bins = r_bins; b.r_width = (r_max - r_min) / (double)r_bins;
  return b;
}

enum HistPart : int { H_Y = 0, H_ETA, H_PHIP, H_PT, H_TAU, H_R, H_PHIS, H_PARTS };

IS3D_HD int part_bins(const Bins& b, int part) {
  return part == H_Y ? b.y_bins : part == H_ETA ? b.eta_bins : part == H_PT ? b.pT_bins : part == H_TAU ? b.tau_bins
       : part == H_R ? b.r_bins : b.phip_bins;
}
// word offset of part's block in a histogram of npart species; part = H_PARTS: the number of counts
IS3D_HD long part_offset(const Bins& b, int npart, int part) {
  long o = 0;
  for (int k = 0; k < part; k++) o += (long)npart * part_bins(b, k);
  return o;
}
IS3D_HD long hist_counts(const Bins& b, int npart) { return part_offset(b, npart, H_PARTS); }
IS3D_HD long hist_vn(const Bins& b, int npart) { return 2L * kVnMax * npart * b.pT_bins; }

// floor((v - lo) / width) when it is in [0, n), else -1 (dropped)
IS3D_HD int bin_index(double v, double lo, double width, int n) {
  const double f = floor((v - lo) / width);
  return (f >= 0.0 && f < (double)n) ? (int)f : -1;
}

// a^2 + b^2, each operation rounded once
IS3D_HD double sum_squares(double a, double b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double a2 = a * a, b2 = b * b;
  return a2 + b2;
}

// atan2(b, a) in [0, 2 pi]
IS3D_HD double wrapped_angle(double b, double a) {
  double phi = atan2(b, a);
  if (phi < 0.0) phi += kTwoPi;
  return phi;
}

// rapidity of a particle: the drawn one in 2+1D (candidate() hands it out), from (E, pz) in 3+1D
IS3D_HD double particle_rapidity(int dim, double drawn, double E, double pz) {
  return dim == 2 ? drawn : 0.5 * log((E + pz) / (E - pz));
}

// cos(k phi), sin(k phi), k = 1..7, phi = the direction of (px, py); pT = sqrt(sum_squares(px, py))
IS3D_HD void harmonics(double px, double py, double pT, double* re, double* im) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double c1 = pT > 0.0 ? px / pT : 1.0, s1 = pT > 0.0 ? py / pT : 0.0;
  double c = c1, s = s1;
  re[0] = c; im[0] = s;
#if defined(__clang__)
#pragma unroll
#endif
  for (int k = 1; k < kVnMax; k++) {
    const double cc = c * c1, ss = s * s1, sc = s * c1, cs = c * s1;
    c = cc - ss;
    s = sc + cs;
    re[k] = c; im[k] = s;
  }
}

// v (|v| <= 1 to rounding) as a multiple of q, round to nearest even
IS3D_HD long long vn_quantise(double v) { return (long long)llrint(v * kVnScale); }
IS3D_HD double vn_value(long long sum) { return (double)sum * kVnQuantum; }

// where one particle lands: the index in each count part (-1: dropped) and its quantised harmonics
struct Landing {
  int idx[H_PARTS];
  long long re[kVnMax], im[kVnMax];
};

IS3D_HD Landing bin_particle(const Bins& b, double rapidity, double eta, double px, double py, double tau, double x, double y) {
  Landing l;
  l.idx[H_Y] = bin_index(rapidity, -b.y_cut, b.y_width, b.y_bins);
  l.idx[H_ETA] = bin_index(eta, -b.eta_cut, b.eta_width, b.eta_bins);
  l.idx[H_PHIP] = bin_index(wrapped_angle(py, px), 0.0, b.phip_width, b.phip_bins);
  const double pT = sqrt(sum_squares(px, py));
  l.idx[H_PT] = bin_index(pT, b.pT_min, b.pT_width, b.pT_bins);
  l.idx[H_TAU] = bin_index(tau, b.tau_min, b.tau_width, b.tau_bins);
  l.idx[H_R] = bin_index(sqrt(sum_squares(x, y)), b.r_min, b.r_width, b.r_bins);
  l.idx[H_PHIS] = bin_index(wrapped_angle(y, x), 0.0, b.phip_width, b.phip_bins);
  double re[kVnMax], im[kVnMax];             // unconditional: a few dozen flops, and the landing stays in registers
  harmonics(px, py, pT, re, im);
#if defined(__clang__)
#pragma unroll
#endif
  for (int k = 0; k < kVnMax; k++) { l.re[k] = vn_quantise(re[k]); l.im[k] = vn_quantise(im[k]); }
  return l;
}

// adds the landing of a particle of species sp: add(word, value) for every histogram word it touches
template <class Add>
IS3D_HD void hist_accumulate(const Bins& b, int npart, int sp, const Landing& l, Add add) {
  long o = 0;
  const int nbs[H_PARTS] = {b.y_bins, b.eta_bins, b.phip_bins, b.pT_bins, b.tau_bins, b.r_bins, b.phip_bins};
#if defined(__clang__)
#pragma unroll
#endif
  for (int part = 0; part < H_PARTS; part++) {     // unrolled: the landing stays in registers
    if (l.idx[part] >= 0) add(o + (long)sp * nbs[part] + l.idx[part], 1LL);
    o += (long)npart * nbs[part];
  }
  if (l.idx[H_PT] >= 0) {
    const long stride = (long)npart * b.pT_bins, at = o + (long)sp * b.pT_bins + l.idx[H_PT];
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 0; k < kVnMax; k++) {
      add(at + (long)k * stride, l.re[k]);
      add(at + (long)(kVnMax + k) * stride, l.im[k]);
    }
  }
}

}  // namespace sampler
}  // namespace is3d
