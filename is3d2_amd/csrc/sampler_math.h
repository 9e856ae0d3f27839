// sampler_math.h -- host/device math of the operation = 2 particle sampler (df_mode 1-4; df_mode 5 at the end), shared by the sampling
// kernels (sampler.hip) and the CPU emulator (tests/native/sampler_emulator.cpp).
//
// Reference: EmissionFunctionArray::sample_dN_pTdpTdphidy (ParticleSampler.cpp:638-1134) with sample_momentum
// (:243-405), rescale_momentum (:407-426), the species weights max_particle_number / fast_max_particle_number
// (:122-239), does_feqmod_breakdown (EmissionFunction.cpp:65-109) and the lab boost (Momentum.cpp:14-31).
//
// Random numbers.  The reference draws from four serial std::default_random_engine streams (poisson, type, momentum,
// rapidity); a parallel sampler cannot share them.  Here every draw comes from Philox4x32-10 (Salmon et al., SC'11)
// with key = the 64-bit seed and the 128-bit counter
//     c0 = block | purpose << 22 | (cell >> 32) << 24,   c1 = cell & 0xffffffff,   c2 = event,   c3 = candidate
// so the stream of a draw is a pure function of (seed, purpose, global cell, event, candidate, draw counter): the
// sampled list cannot depend on the launch geometry, the event batch, the cell window or the number of shards.  One
// block gives two 53-bit uniforms in [0, 1); a stream holds at most 2^22 blocks, which the iteration caps below keep
// out of reach.  The streams do not depend on df_mode (PTM's breakdown cells reproduce RTA-CE's list bit for bit).
//
// No unbounded loops: the momentum rejection loop ends after kMomentumCap proposals, the Poisson inversion after
// kPoissonCap terms per part and kPoissonParts parts; a draw that reaches a cap is reported (the candidate is dropped
// and counted in the stats field `capped`), never silently truncated.
//
// Rejection weights are written in the overflow-safe forms exp(pbar - Ebar) / (1 + sign exp(-Ebar)) (= feq / (r1 r2
// r3), :292) and (pbar / Ebar) / (1 + sign exp(chem - Ebar)) (= pbar / Ebar boltz feq, :380).
//
// The transverse mass of a 2+1D particle is sqrt(m^2 + px^2 + py^2), the same number as the reference's
// sqrt(ptau^2 - (tau pn)^2) without the cancellation, so E^2 - p^2 = m^2 holds to a few ulp of E^2.
//
// Two places where the reference leaves the behaviour open: a species weight below zero (possible for PTM's
// linearised density) is undefined for std::discrete_distribution -- here it enters the Poisson mean as it does in
// the reference's dn_tot but counts as zero in the species draw; and a proposal with l1 + l2 = 0 (probability
// 2^-106), where the reference divides by zero, is drawn again.
#pragma once
#include <cmath>
#include <cstdint>

#include "cf_math.h"

namespace is3d {
namespace sampler {

// ---------------------------------------------------------------------------------------------------------
// Philox4x32-10
// ---------------------------------------------------------------------------------------------------------
struct U4 { uint32_t v[4]; };

IS3D_HD U4 philox4x32_10(U4 ctr, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * ctr.v[0], p1 = (uint64_t)0xCD9E8D57u * ctr.v[2];
    const U4 n{{(uint32_t)(p1 >> 32) ^ ctr.v[1] ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ ctr.v[3] ^ k1, (uint32_t)p0}};
    ctr = n;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return ctr;
}

// 53 bits of (hi, lo) -> [0, 1)
IS3D_HD double u53(uint32_t hi, uint32_t lo) {
  return (double)(((uint64_t)hi << 21) | (uint64_t)(lo >> 11)) * (1.0 / 9007199254740992.0);
}

enum Purpose : int { P_POISSON = 0, P_TYPE = 1, P_MOMENTUM = 2, P_RAPIDITY = 3 };

struct Stream {
  uint32_t k0, k1, c0, c1, c2, c3;
  uint32_t block;
  int have;
  double spare;
};

IS3D_HD Stream stream_open(uint64_t seed, int purpose, long cell, long event, long candidate) {
  Stream s;
  s.k0 = (uint32_t)seed; s.k1 = (uint32_t)(seed >> 32);
  s.c0 = ((uint32_t)purpose << 22) | ((uint32_t)(((uint64_t)cell >> 32) & 0xffu) << 24);
  s.c1 = (uint32_t)((uint64_t)cell & 0xffffffffu);
  s.c2 = (uint32_t)event; s.c3 = (uint32_t)candidate;
  s.block = 0; s.have = 0; s.spare = 0.0;
  return s;
}

IS3D_HD double stream_next(Stream& s) {
  if (s.have) { s.have = 0; return s.spare; }
  const U4 r = philox4x32_10(U4{{s.c0 | (s.block & 0x3fffffu), s.c1, s.c2, s.c3}}, s.k0, s.k1);
  s.block++;
  s.spare = u53(r.v[2], r.v[3]);
  s.have = 1;
  return u53(r.v[0], r.v[1]);
}

// ---------------------------------------------------------------------------------------------------------
// Poisson: exact for every mean.  A mean above kPoissonPart is split into equal parts of at most that size, each drawn
// by inversion, and the draws are added (Poisson additivity).
// ---------------------------------------------------------------------------------------------------------
static constexpr double kPoissonPart = 16.0;
static constexpr int kPoissonCap = 512;          // terms of one inversion: P(N > 512 | mean <= 16) < 1e-500
static constexpr long kPoissonParts = 1L << 20;  // means up to 1.6e7 per (cell, event)

IS3D_HD long poisson_draw(Stream& s, double mean, int* capped) {
  if (!(mean > 0.0)) return 0;
  const double want = ceil(mean / kPoissonPart);
  long parts = want < (double)kPoissonParts ? (long)want : kPoissonParts;
  if (want > (double)kPoissonParts) *capped = 1;
  if (parts < 1) parts = 1;
  const double m = mean / (double)parts, p0 = exp(-m);
  long total = 0;
  for (long k = 0; k < parts; k++) {
    const double u = stream_next(s);
    double p = p0, cum = p0;
    int n = 0;
    while (u >= cum && n < kPoissonCap) {
      n++;
      p *= m / (double)n;
      const double next = cum + p;
      if (next == cum && (double)n > m) break;   // the tail below the rounding of cum: u sits in the last ulps under 1
      cum = next;
    }
    if (n >= kPoissonCap) *capped = 1;
    total += n;
  }
  return total;
}

// species draw: index of the first cumulative weight above u x total (cum: running sum of max(weight, 0))
IS3D_HD int species_draw(const double* cum, int n, double u) {
  const double t = u * cum[n - 1];
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cum[mid] > t) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// ---------------------------------------------------------------------------------------------------------
// LRF momentum from the thermal distribution (ParticleSampler.cpp:243-405)
// ---------------------------------------------------------------------------------------------------------
struct LrfP { double E, px, py, pz, feq; };

static constexpr int kMomentumCap = 4096;
static constexpr double kTwoPi = 6.283185307179586476925286766559;

// rational fit of the local maximum of the pion weight for m / T < 0.8554 (ParticleSampler.cpp:41-70)
IS3D_HD double pion_weight_max(double x) {
  const double x2 = x * x, x3 = x2 * x, x4 = x3 * x;
  const double num = 143206.88623164667 - 95956.76008684626 * x - 21341.937407169076 * x2 + 14388.446116867359 * x3 - 6083.775788504437 * x4;
  const double den = -0.3541350577684533 + 143218.69233952634 * x - 24516.803600065778 * x2 - 115811.59391199696 * x3 + 35814.36403387459 * x4;
  return 1.00001 * num / den;
}

// branch taken by the accepted proposal: 0 light (mbar < 1.008), 1..3 the K-distributions (heavy, moderate, light
// kinetic energy), +4 when the pion maximum rescaled the weight.  Returns false when the cap was reached.
IS3D_HD bool sample_momentum(Stream& s, double mass, double sign, double T, double chem, LrfP* out, long* proposals, int* branch) {
  const double mbar = mass / T, mbar2 = mbar * mbar;
  double pbar = 0, Ebar = 0, phi_over_2pi = 0, costheta = 0, feq = 0;
  bool ok = false;
  if (mbar < 1.008) {
    double wmax = 1.0;
    const bool rescaled = mbar < 0.8554 && sign == -1.0;
    if (rescaled) wmax = pion_weight_max(mbar);
    for (int it = 0; it < kMomentumCap && !ok; it++) {
      (*proposals)++;
      const double l1 = log(1.0 - stream_next(s)), l2 = log(1.0 - stream_next(s)), l3 = log(1.0 - stream_next(s));
      pbar = -(l1 + l2 + l3);
      Ebar = sqrt(pbar * pbar + mbar2);
      const double em = exp(-Ebar);
      const double w = exp(pbar - Ebar) / (1.0 + sign * em) / wmax;
      const double u = stream_next(s);
      if (u < w && l1 + l2 != 0.0) {
        feq = em / (1.0 + sign * em);
        phi_over_2pi = (l1 + l2) * (l1 + l2) / (pbar * pbar);
        costheta = (l1 - l2) / (l1 + l2);
        ok = true;
      }
    }
    *branch = rescaled ? 4 : 0;
  } else {
    const double w0 = mbar2, w1 = 2.0 * mbar, wsum = w0 + w1 + 2.0;
    int kd = 0;
    for (int it = 0; it < kMomentumCap && !ok; it++) {
      (*proposals)++;
      const double uk = stream_next(s) * wsum;
      kd = uk < w0 ? 0 : uk < w0 + w1 ? 1 : 2;
      double kbar;
      bool good = true;
      if (kd == 0) {
        kbar = -log(1.0 - stream_next(s));
        phi_over_2pi = stream_next(s);
        costheta = 2.0 * stream_next(s) - 1.0;
      } else if (kd == 1) {
        const double l1 = log(1.0 - stream_next(s)), l2 = log(1.0 - stream_next(s));
        kbar = -(l1 + l2);
        good = kbar != 0.0;
        phi_over_2pi = good ? -l1 / kbar : 0.0;
        costheta = 2.0 * stream_next(s) - 1.0;
      } else {
        const double l1 = log(1.0 - stream_next(s)), l2 = log(1.0 - stream_next(s)), l3 = log(1.0 - stream_next(s));
        kbar = -(l1 + l2 + l3);
        good = l1 + l2 != 0.0;
        phi_over_2pi = good ? (l1 + l2) * (l1 + l2) / (kbar * kbar) : 0.0;
        costheta = good ? (l1 - l2) / (l1 + l2) : 0.0;
      }
      Ebar = kbar + mbar;
      pbar = sqrt(kbar * (kbar + 2.0 * mbar));     // = sqrt(Ebar^2 - mbar^2)
      const double ex = exp(chem - Ebar);
      const double w = pbar / Ebar / (1.0 + sign * ex);
      const double u = stream_next(s);
      if (u < w && good) {
        feq = ex / (1.0 + sign * ex);
        ok = true;
      }
    }
    *branch = 1 + kd;
  }
  if (!ok) return false;
  const double p = pbar * T, phi = phi_over_2pi * kTwoPi;
  double st2 = 1.0 - costheta * costheta;
  const double sintheta = sqrt(st2 > 0.0 ? st2 : 0.0);
  out->E = Ebar * T;
  out->px = p * sintheta * cos(phi);
  out->py = p * sintheta * sin(phi);
  out->pz = p * costheta;
  out->feq = feq;
  return true;
}

// ---------------------------------------------------------------------------------------------------------
// per-cell context (ParticleSampler.cpp:680-915)
// ---------------------------------------------------------------------------------------------------------
struct Cell {
  double live;                     // 0: u.dsigma <= 0 or dn_tot <= 0 (no candidates)
  double tau, x, y, eta, sinheta, cosheta;
  double ut, ux, uy, un;
  Milne b;
  double dst, dsx, dsy, dsz, ds_max;
  PiLRF pi;
  double Vx, Vy, Vz;
  double T, alphaB, T_mod, alphaB_mod, bulkPi, ber;
  DfCoef df;
  double shear_mod, iso_scale, diff_mod;
  double breaks;                   // feqmod breaks down (modes 3, 4)
  double dn_tot;                   // Poisson mean of one event
};

// what the whole run shares
struct Run {
  PrepConsts k;
  int fast;
  double y_max;                    // 0.5 in 3+1D, y_cut in 2+1D
  double Tavg, F_avg, betabulk_avg;  // fast = 1, PTM: the breakdown test at the Plasma averages
};

// the prologue of one cell up to the breakdown test; s = the 25 surface fields.  DF_OK with c.live = 0 for a
// skipped cell; c.dn_tot is filled by cell_finish once the species weights are summed.
IS3D_HD int cell_setup(const Run& R, const DfTables& tb, const double* s, Cell& c) {
  const PrepConsts& k = R.k;
  c = Cell{};
  const double tau = s[S_TAU], tau2 = tau * tau;
  const double dat = s[S_DAT], dax = s[S_DAX], day = s[S_DAY], dan = s[S_DAN];
  const double ux = s[S_UX], uy = s[S_UY], un = s[S_UN];
  const double ut = sqrt(1.0 + ux * ux + uy * uy + tau2 * un * un);
  if (ut * dat + ux * dax + uy * day + un * dan <= 0.0) return DF_OK;
  const double ut2 = ut * ut, ux2 = ux * ux, uy2 = uy * uy;
  const double uperp = sqrt(ux2 + uy2), utperp = sqrt(1.0 + ux2 + uy2);
  const double T = s[S_T], P = s[S_P], E = s[S_E];
  double pitt = 0, pitx = 0, pity = 0, pitn = 0, pixx = 0, pixy = 0, pixn = 0, piyy = 0, piyn = 0, pinn = 0;
  if (k.include_shear) {
    pixx = s[S_PIXX]; pixy = s[S_PIXY]; pixn = s[S_PIXN]; piyy = s[S_PIYY]; piyn = s[S_PIYN];
    pinn = (pixx * (ux2 - ut2) + piyy * (uy2 - ut2) + 2.0 * (pixy * ux * uy + tau2 * un * (pixn * ux + piyn * uy))) / (tau2 * utperp * utperp);
    pitn = (pixn * ux + piyn * uy + tau2 * pinn * un) / ut;
    pity = (pixy * ux + piyy * uy + tau2 * piyn * un) / ut;
    pitx = (pixx * ux + pixy * uy + tau2 * pixn * un) / ut;
    pitt = (pitx * ux + pity * uy + tau2 * pitn * un) / ut;
  }
  double bulkPi = k.include_bulk ? s[S_BULKPI] : 0.0;
  double muB = 0, alphaB = 0, nB = 0, Vt = 0, Vx = 0, Vy = 0, Vn = 0, ber = 0;
  if (k.include_baryon && k.include_diff) {
    muB = s[S_MUB]; nB = s[S_NB]; Vx = s[S_VX]; Vy = s[S_VY]; Vn = s[S_VN];
    Vt = (Vx * ux + Vy * uy + tau2 * Vn * un) / ut;
    alphaB = muB / T;
    ber = nB / (E + P);
  }
  if (k.df_mode == PTB) {          // :770-776
    if (bulkPi <= -P) bulkPi = -(1.0 - 1.e-5) * P;
    else if (bulkPi / P >= tb.bulk_over_P_max) bulkPi = P * (tb.bulk_over_P_max - 1.e-5);
  }
  const int err = df_eval(tb, T, muB, E, P, bulkPi, c.df);
  if (err) return err;
  c.b = milne_basis(ut, ux, uy, un, uperp, utperp, tau);
  const Milne& b = c.b;
  c.dst = dat * ut + dax * ux + day * uy + dan * un;
  c.dsx = -(dat * b.Xt + dax * b.Xx + day * b.Xy + dan * b.Xn);
  c.dsy = -(dax * b.Yx + day * b.Yy);
  c.dsz = -(dat * b.Zt + dan * b.Zn);
  c.ds_max = fabs(c.dst) + sqrt(c.dsx * c.dsx + c.dsy * c.dsy + c.dsz * c.dsz);
  c.pi = boost_pi(b, tau2, pitt, pitx, pity, pitn, pixx, pixy, pixn, piyy, piyn, pinn);
  c.Vx = -Vt * b.Xt + Vx * b.Xx + Vy * b.Xy + tau2 * Vn * b.Xn;
  c.Vy = Vx * b.Yx + Vy * b.Yy;
  c.Vz = -Vt * b.Zt + tau2 * Vn * b.Zn;
  c.T = T; c.alphaB = alphaB; c.T_mod = T; c.alphaB_mod = alphaB; c.bulkPi = bulkPi; c.ber = ber;
  double bulk_mod = 0.0;
  if (k.df_mode == PTM) {
    c.T_mod = T + bulkPi * c.df.F / c.df.betabulk;
    c.alphaB_mod = alphaB + bulkPi * c.df.G / c.df.betabulk;
    c.shear_mod = 0.5 / c.df.betapi;
    bulk_mod = bulkPi / (3.0 * c.df.betabulk);
    c.diff_mod = T / c.df.betaV;
  } else if (k.df_mode == PTB) {
    c.shear_mod = 0.5 / c.df.betapi;
    bulk_mod = c.df.lambda;
  }
  c.iso_scale = 1.0 + bulk_mod;
  bool breaks = false;
  if (k.df_mode == PTM || k.df_mode == PTB) {
    const double Axx = 1.0 + c.pi.xx * c.shear_mod + bulk_mod, Axy = c.pi.xy * c.shear_mod, Axz = c.pi.xz * c.shear_mod;
    const double Ayy = 1.0 + c.pi.yy * c.shear_mod + bulk_mod, Ayz = c.pi.yz * c.shear_mod, Azz = 1.0 + c.pi.zz * c.shear_mod + bulk_mod;
    const double detA = Axx * (Ayy * Azz - Ayz * Ayz) - Axy * (Axy * Azz - Ayz * Axz) + Axz * (Axy * Ayz - Ayy * Axz);
    if (k.df_mode == PTM) {        // EmissionFunction.cpp:65-97; fast: at the Plasma averages
      const double Tb = R.fast ? R.Tavg : T, Fb = R.fast ? R.F_avg : c.df.F, bb = R.fast ? R.betabulk_avg : c.df.betabulk;
      const double mbar = k.mass_pion0 / Tb;
      const double neq_fact = Tb * Tb * Tb / k.two_pi2_hbarC3, J20_fact = Tb * neq_fact;
      const double neq = neq_fact * gt_neq(k.gla_r1, k.gla_w1, k.gla_pts, mbar, 0., 0., -1.);
      const double J20 = J20_fact * gt_J20(k.gla_r2, k.gla_w2, k.gla_pts, mbar, 0., 0., -1.);
      const double dn = bulkPi * (neq + J20 * Fb / Tb / Tb) / bb;
      breaks = detA <= k.deta_min || neq + dn < 0.0;
    } else {
      breaks = detA <= k.deta_min || c.df.z < 0.0;
    }
  }
  c.breaks = breaks ? 1.0 : 0.0;
  c.tau = tau; c.x = s[S_X]; c.y = s[S_Y]; c.eta = s[S_ETA];
  c.sinheta = sinh(c.eta);
  c.cosheta = sqrt(1.0 + c.sinheta * c.sinheta);
  c.ut = ut; c.ux = ux; c.uy = uy; c.un = un;
  c.live = 1.0;
  return DF_OK;
}

// species weight, fast = 0 (max_particle_number, :164-239)
IS3D_HD double species_weight(const Run& R, const Cell& c, double mass, double degeneracy, double sign, double baryon) {
  const PrepConsts& k = R.k;
  const double T = c.T, mbar = mass / T;
  const double neq_fact = T * T * T / k.two_pi2_hbarC3, J20_fact = T * neq_fact;
  const bool linear = k.df_mode == GRAD || k.df_mode == CE || c.breaks != 0.0;
  if (linear) return 2.0 * (neq_fact * degeneracy * gt_neq(k.gla_r1, k.gla_w1, k.gla_pts, mbar, c.alphaB, baryon, sign));
  if (k.df_mode == PTM) {
    const double neq = neq_fact * degeneracy * gt_neq(k.gla_r1, k.gla_w1, k.gla_pts, mbar, c.alphaB, baryon, sign);
    double J10 = 0.0;
    if (k.include_baryon) J10 = neq_fact * degeneracy * gt_J10(k.gla_r1, k.gla_w1, k.gla_pts, mbar, c.alphaB, baryon, sign);
    const double J20 = J20_fact * degeneracy * gt_J20(k.gla_r2, k.gla_w2, k.gla_pts, mbar, c.alphaB, baryon, sign);
    const double bulk_density = (neq + baryon * J10 * c.df.G + J20 * c.df.F / T / T) / c.df.betabulk;
    return neq + c.bulkPi * bulk_density;
  }
  return c.df.z * (neq_fact * degeneracy * gt_neq(k.gla_r1, k.gla_w1, k.gla_pts, mbar, 0.0, 0.0, sign));
}

// species weight, fast = 1 (fast_max_particle_number, :122-161) from the Plasma-average densities
IS3D_HD double species_weight_fast(const Run& R, const Cell& c, double equilibrium_density, double bulk_density) {
  const int m = R.k.df_mode;
  if (m == GRAD || m == CE || c.breaks != 0.0) return 2.0 * equilibrium_density;
  if (m == PTM) return equilibrium_density + c.bulkPi * bulk_density;
  return c.df.z * equilibrium_density;
}

// dn_sum = the plain sum of the species weights
IS3D_HD void cell_finish(const Run& R, Cell& c, double dn_sum) {
  c.dn_tot = dn_sum * (2.0 * R.y_max * c.ds_max);
  if (!(dn_sum > 0.0)) { c.live = 0.0; c.dn_tot = 0.0; }
}

// ---------------------------------------------------------------------------------------------------------
// one candidate (ParticleSampler.cpp:929-1130)
// ---------------------------------------------------------------------------------------------------------
// the plain 96-byte record of include/is3d_amd.h (is3d_particle)
struct Particle {
  int32_t species, event;
  int64_t cell;
  double tau, x, y, eta, t, z, E, px, py, pz;
};

struct Tally { long proposals, acceptances, capped, clamped; };

IS3D_HD LrfP rescale_momentum(const Cell& c, const LrfP& q, double mass2, double baryon, bool with_diffusion) {
  const double dm = with_diffusion ? c.diff_mod * (q.E * c.ber + baryon) : 0.0;
  const double vx = with_diffusion ? c.Vx : 0.0, vy = with_diffusion ? c.Vy : 0.0, vz = with_diffusion ? c.Vz : 0.0;
  LrfP r;
  r.px = c.iso_scale * q.px + c.shear_mod * (c.pi.xx * q.px + c.pi.xy * q.py + c.pi.xz * q.pz) + dm * vx;
  r.py = c.iso_scale * q.py + c.shear_mod * (c.pi.xy * q.px + c.pi.yy * q.py + c.pi.yz * q.pz) + dm * vy;
  r.pz = c.iso_scale * q.pz + c.shear_mod * (c.pi.xz * q.px + c.pi.yz * q.py + c.pi.zz * q.pz) + dm * vz;
  r.E = sqrt(mass2 + r.px * r.px + r.py * r.py + r.pz * r.pz);
  r.feq = q.feq;
  return r;
}

IS3D_HD double clamp_df(double df, Tally& t) {
  if (df > 1.0 || df < -1.0) t.clamped++;
  return fmax(-1.0, fmin(1.0, df));
}

// the kept LRF momentum p of species sp (mass^2 = m2) as the particle record: lab boost (Momentum.cpp:14-31), the
// rapidity draw of a 2+1D surface (:1079-1098) and the cell's position.  The tail of candidate() below, word for word,
// for candidate_famod: candidate() keeps its own copy, because calling this from it moved k_sample<binned only> from
// 231 to 233 VGPRs, and the df_mode 1-4 kernels are to compile to what they were.
IS3D_HD void lab_record(const Run& R, const Cell& c, const LrfP& p, double m2, int sp, uint64_t seed, long cell, long event,
                        long n, Particle* out, double& drawn) {
  const Milne& b = c.b;
  const double ptau = p.E * c.ut + p.px * b.Xt + p.pz * b.Zt;
  const double lpx = p.E * c.ux + p.px * b.Xx + p.py * b.Yx;
  const double lpy = p.E * c.uy + p.px * b.Xy + p.py * b.Yy;
  const double pn = p.E * c.un + p.px * b.Xn + p.pz * b.Zn;
  double eta = c.eta, sinheta = c.sinheta, cosheta = c.cosheta, E, pz;
  if (R.k.dim == 2) {              // :1079-1098
    Stream sr = stream_open(seed, P_RAPIDITY, cell, event, n);
    const double rapidity = R.y_max * (2.0 * stream_next(sr) - 1.0);
    drawn = rapidity;
    const double sinhy = sinh(rapidity), coshy = sqrt(1.0 + sinhy * sinhy);
    const double tau_pn = c.tau * pn;
    const double mT = sqrt(m2 + lpx * lpx + lpy * lpy);   // = sqrt(ptau^2 - (tau pn)^2) of :1088, without its cancellation
    sinheta = (ptau * sinhy - tau_pn * coshy) / mT;
    eta = asinh(sinheta);
    cosheta = sqrt(1.0 + sinheta * sinheta);
    pz = mT * sinhy;
    E = mT * coshy;
  } else {
    pz = c.tau * pn * cosheta + ptau * sinheta;
    E = sqrt(m2 + lpx * lpx + lpy * lpy + pz * pz);
  }
  out->species = sp; out->event = (int32_t)event; out->cell = cell;
  out->tau = c.tau; out->x = c.x; out->y = c.y; out->eta = eta;
  out->t = c.tau * cosheta; out->z = c.tau * sinheta;
  out->E = E; out->px = lpx; out->py = lpy; out->pz = pz;
}

// Draws species, momentum and the keep decision of candidate n of (cell, event); true = kept, *out filled.
// cum[npart]: the cell's running species weights; mass / sign / baryon: the chosen species in their original order.
// drawn: the drawn rapidity of a kept 2+1D particle (the binned distributions take it as drawn; untouched in 3+1D).
IS3D_HD bool candidate(const Run& R, const Cell& c, uint64_t seed, long cell, long event, long n, const double* cum,
                       int npart, const double* mass, const double* sign, const double* baryon_, Particle* out, Tally& t,
                       int* branch_out, double& drawn) {
  const int mode = R.k.df_mode;
  Stream st = stream_open(seed, P_TYPE, cell, event, n);
  const int sp = species_draw(cum, npart, stream_next(st));
  const double m = mass[sp], m2 = m * m, sg = sign[sp], baryon = baryon_[sp];
  const double chem = baryon * c.alphaB, chem_mod = baryon * c.alphaB_mod;
  Stream sm = stream_open(seed, P_MOMENTUM, cell, event, n);
  LrfP p;
  double w_visc = 1.0;
  int branch = 0;
  const bool modified = (mode == PTM || mode == PTB) && c.breaks == 0.0;
  bool ok;
  if (mode == PTM && modified) ok = sample_momentum(sm, m, sg, c.T_mod, chem_mod, &p, &t.proposals, &branch);
  else if (mode == PTB) ok = sample_momentum(sm, m, sg, c.T, 0.0, &p, &t.proposals, &branch);
  else ok = sample_momentum(sm, m, sg, c.T, chem, &p, &t.proposals, &branch);
  if (branch_out) *branch_out = branch;
  if (!ok) { t.capped++; return false; }
  t.acceptances++;
  if (modified) {
    p = rescale_momentum(c, p, m2, mode == PTM ? baryon : 0.0, mode == PTM);
  } else {
    const double E = p.E, px = p.px, py = p.py, pz = p.pz;
    const double feqbar = 1.0 - sg * p.feq;
    const double pipp = px * px * c.pi.xx + py * py * c.pi.yy + pz * pz * c.pi.zz + 2.0 * (px * py * c.pi.xy + px * pz * c.pi.xz + py * pz * c.pi.yz);
    const double Vp = -(px * c.Vx + py * c.Vy + pz * c.Vz);
    const DfCoef& df = c.df;
    double dfv;
    if (mode == GRAD) {
      const double shear = pipp / df.shear14;
      const double bulk = ((df.c0 - df.c2) * m2 + (baryon * df.c1 + (4.0 * df.c2 - df.c0) * E) * E) * c.bulkPi;
      const double diff = (baryon * df.c3 + df.c4 * E) * Vp;
      dfv = feqbar * (shear + bulk + diff);
    } else if (mode == PTB) {      // breakdown of PTB (:1030-1047)
      const double shear = feqbar * pipp / (2.0 * df.betapi * c.T * E);
      const double bulk = (df.dz - 3.0 * df.dlambda) + feqbar * (df.dlambda / c.T) * (E - m2 / E);
      dfv = shear + bulk;
    } else {                       // RTA-CE, and PTM's breakdown
      const double shear = pipp / (2.0 * df.betapi * c.T * E);
      const double bulk = (baryon * df.G + df.F / (c.T * c.T) * E + (E - m2 / E) / (3.0 * c.T)) * (c.bulkPi / df.betabulk);
      const double diff = (c.ber - baryon / E) * Vp / df.betaV;
      dfv = feqbar * (shear + bulk + diff);
    }
    w_visc = 0.5 * (1.0 + clamp_df(dfv, t));
  }
  const double w_flux = fmax(0.0, p.E * c.dst - p.px * c.dsx - p.py * c.dsy - p.pz * c.dsz) / (p.E * c.ds_max);
  if (!(stream_next(sm) < w_flux * w_visc)) return false;
  // lab frame (Momentum.cpp:14-31)
  const Milne& b = c.b;
  const double ptau = p.E * c.ut + p.px * b.Xt + p.pz * b.Zt;
  const double lpx = p.E * c.ux + p.px * b.Xx + p.py * b.Yx;
  const double lpy = p.E * c.uy + p.px * b.Xy + p.py * b.Yy;
  const double pn = p.E * c.un + p.px * b.Xn + p.pz * b.Zn;
  double eta = c.eta, sinheta = c.sinheta, cosheta = c.cosheta, E, pz;
  if (R.k.dim == 2) {              // :1079-1098
    Stream sr = stream_open(seed, P_RAPIDITY, cell, event, n);
    const double rapidity = R.y_max * (2.0 * stream_next(sr) - 1.0);
    drawn = rapidity;
    const double sinhy = sinh(rapidity), coshy = sqrt(1.0 + sinhy * sinhy);
    const double tau_pn = c.tau * pn;
    const double mT = sqrt(m2 + lpx * lpx + lpy * lpy);   // = sqrt(ptau^2 - (tau pn)^2) of :1088, without its cancellation
    sinheta = (ptau * sinhy - tau_pn * coshy) / mT;
    eta = asinh(sinheta);
    cosheta = sqrt(1.0 + sinheta * sinheta);
    pz = mT * sinhy;
    E = mT * coshy;
  } else {
    pz = c.tau * pn * cosheta + ptau * sinheta;
    E = sqrt(m2 + lpx * lpx + lpy * lpy + pz * pz);
  }
  out->species = sp; out->event = (int32_t)event; out->cell = cell;
  out->tau = c.tau; out->x = c.x; out->y = c.y; out->eta = eta;
  out->t = c.tau * cosheta; out->z = c.tau * sinheta;
  out->E = E; out->px = lpx; out->py = lpy; out->pz = pz;
  return true;
}

IS3D_HD bool candidate(const Run& R, const Cell& c, uint64_t seed, long cell, long event, long n, const double* cum,
                       int npart, const double* mass, const double* sign, const double* baryon_, Particle* out, Tally& t,
                       int* branch_out) {
  double drawn = 0.0;
  return candidate(R, c, seed, cell, event, n, cum, npart, mass, sign, baryon_, out, t, branch_out, drawn);
}

// ---------------------------------------------------------------------------------------------------------
// df_mode 5 (PTMA): sample_dN_pTdpTdphidy_famod (ParticleSampler.cpp:1138-1627)
// ---------------------------------------------------------------------------------------------------------
// The method has no delta-f, no diffusion and no fast branch, so its Cell reuses fields it would leave empty:
//   pi = the symmetric momentum transformation B (the identity on breakdown), T_mod = lambda, iso_scale = det A,
//   shear_mod = det B = det C det A (as computed, breakdown or not), alphaB_mod = alphaB (upsilonB, :1328);
// df, V*, diff_mod and ber stay zero.  The df_mode 1-4 record is unchanged.
//
// The prologue (:1181-1461) of one cell; s = the 25 surface fields, sol = the cell's row of the Newton prepass
// (lambda, aT, aL, broken, beta_pi_perp, beta_W_perp; aniso_math.h aniso_cell with the sampler's rule), read only for
// a cell with u.dsigma > 0.  pi and Pi enter pl / pt whatever the delta-f flags say, and muB is read under
// include_baryon alone (:1215-1248).  Breakdown: pl / pt < 0 or a failed reconstruction (sol[3]) or det B <= deta_min;
// lambda and det A stay what the cell ends with -- (T, 1, 1) for the first two causes, the solution for the third.
IS3D_HD void cell_setup_famod(const Run& R, const double* s, const double* sol, Cell& c) {
  const PrepConsts& k = R.k;
  c = Cell{};
  const double tau = s[S_TAU], tau2 = tau * tau;
  const double dat = s[S_DAT], dax = s[S_DAX], day = s[S_DAY], dan = s[S_DAN];
  const double ux = s[S_UX], uy = s[S_UY], un = s[S_UN];
  const double ut = sqrt(1.0 + ux * ux + uy * uy + tau2 * un * un);
  if (ut * dat + ux * dax + uy * day + un * dan <= 0.0) return;
  const double ut2 = ut * ut, ux2 = ux * ux, uy2 = uy * uy;
  const double uperp = sqrt(ux2 + uy2), utperp = sqrt(1.0 + ux2 + uy2);
  const double T = s[S_T];
  const double pixx = s[S_PIXX], pixy = s[S_PIXY], pixn = s[S_PIXN], piyy = s[S_PIYY], piyn = s[S_PIYN];
  const double pinn = (pixx * (ux2 - ut2) + piyy * (uy2 - ut2) + 2.0 * (pixy * ux * uy + tau2 * un * (pixn * ux + piyn * uy))) / (tau2 * utperp * utperp);
  const double pitn = (pixn * ux + piyn * uy + tau2 * pinn * un) / ut;
  const double pity = (pixy * ux + piyy * uy + tau2 * piyn * un) / ut;
  const double pitx = (pixx * ux + pixy * uy + tau2 * pixn * un) / ut;
  const double pitt = (pitx * ux + pity * uy + tau2 * pitn * un) / ut;
  const double muB = k.include_baryon ? s[S_MUB] : 0.0;
  c.b = milne_basis(ut, ux, uy, un, uperp, utperp, tau);
  const Milne& b = c.b;
  c.dst = dat * ut + dax * ux + day * uy + dan * un;
  c.dsx = -(dat * b.Xt + dax * b.Xx + day * b.Xy + dan * b.Xn);
  c.dsy = -(dax * b.Yx + day * b.Yy);
  c.dsz = -(dat * b.Zt + dan * b.Zn);
  c.ds_max = fabs(c.dst) + sqrt(c.dsx * c.dsx + c.dsy * c.dsy + c.dsz * c.dsz);
  const PiLRF pl_ = boost_pi(b, tau2, pitt, pitx, pity, pitn, pixx, pixy, pixn, piyy, piyn, pinn);
  double piTxx = 0, piTxy = 0, piTyy = 0, WTzx = 0, WTzy = 0;
  if (k.include_shear) {
    piTxx = (pl_.xx - pl_.yy) / 2.; piTxy = pl_.xy; piTyy = -(piTxx);
    WTzx = pl_.xz; WTzy = pl_.yz;
  }
  const double lambda = sol[0], aT = sol[1], aL = sol[2];
  bool breaks = sol[3] != 0.0;
  const double shear_coeff = 0.5 / sol[4], diff_coeff = 1. / sol[5];
  const double detA = aT * aT * aL;
  const double Cxx = 1. + shear_coeff * piTxx, Cxy = shear_coeff * piTxy, Cxz = diff_coeff * WTzx * aT / (aT + aL);
  const double Cyx = Cxy, Cyy = 1. + shear_coeff * piTyy, Cyz = diff_coeff * WTzy * aT / (aT + aL);
  const double Czx = diff_coeff * WTzx * aL / (aT + aL), Czy = diff_coeff * WTzy * aL / (aT + aL), Czz = 1.;
  const double detC = Cxx * (Cyy * Czz - Cyz * Czy) - Cxy * (Cyx * Czz - Cyz * Czx) + Cxz * (Cyx * Czy - Cyy * Czx);
  const double detB = detC * detA;
  if (detB <= k.deta_min) breaks = true;
  c.pi = PiLRF{1.0, 0.0, 0.0, 1.0, 0.0, 1.0};
  if (!breaks) {
    c.pi.xx = aT + aT * shear_coeff * piTxx; c.pi.xy = aT * shear_coeff * piTxy; c.pi.xz = diff_coeff * WTzx * aT * aL / (aT + aL);
    c.pi.yy = aT + aT * shear_coeff * piTyy; c.pi.yz = diff_coeff * WTzy * aT * aL / (aT + aL); c.pi.zz = aL;
  }
  c.T = T; c.alphaB = muB / T; c.T_mod = lambda; c.alphaB_mod = c.alphaB; c.bulkPi = s[S_BULKPI];
  c.iso_scale = detA; c.shear_mod = detB;
  c.breaks = breaks ? 1.0 : 0.0;
  c.tau = tau; c.x = s[S_X]; c.y = s[S_Y]; c.eta = s[S_ETA];
  c.sinheta = sinh(c.eta);
  c.cosheta = sqrt(1.0 + c.sinheta * c.sinheta);
  c.ut = ut; c.ux = ux; c.uy = uy; c.un = un;
  c.live = 1.0;
}

// species weight (:1467-1499): the anisotropic density n_a = g lambda^3 det A / (2 pi^2 hbarc^3) I_100 from the
// alpha = 1 Gauss-Laguerre row.  The reference adds the chemical term to Ebar (exp(Ebar + chem), :1493, "should be
// zero atm") where every other density subtracts it; that is reproduced.
IS3D_HD double species_weight_famod(const Run& R, const Cell& c, double mass, double degeneracy, double sign, double baryon) {
  const PrepConsts& k = R.k;
  const double lambda = c.T_mod, mbar = mass / lambda, mbar2 = mbar * mbar, chem = baryon * c.alphaB_mod;
  const double na_fact = lambda * lambda * lambda * c.iso_scale / k.two_pi2_hbarC3;
  double I_100 = 0.0;
  for (int i = 0; i < k.gla_pts; i++) {
    const double pbar = k.gla_r1[i], Ebar = sqrt(pbar * pbar + mbar2);
    I_100 += pbar * k.gla_w1[i] * exp(pbar) / (exp(Ebar + chem) + sign);
  }
  return degeneracy * na_fact * I_100;
}

// rescale_momentum_famod (:428-444): p = B p', E from the mass
IS3D_HD LrfP rescale_momentum_famod(const Cell& c, const LrfP& q, double mass2) {
  LrfP r;
  r.px = c.pi.xx * q.px + c.pi.xy * q.py + c.pi.xz * q.pz;
  r.py = c.pi.xy * q.px + c.pi.yy * q.py + c.pi.yz * q.pz;
  r.pz = c.pi.xz * q.px + c.pi.yz * q.py + c.pi.zz * q.pz;
  r.E = sqrt(mass2 + r.px * r.px + r.py * r.py + r.pz * r.pz);
  r.feq = q.feq;
  return r;
}

// one candidate (:1519-1618): the streams and purposes of candidate(); kept with the flux weight alone
IS3D_HD bool candidate_famod(const Run& R, const Cell& c, uint64_t seed, long cell, long event, long n, const double* cum,
                             int npart, const double* mass, const double* sign, const double* baryon_, Particle* out,
                             Tally& t, double& drawn) {
  Stream st = stream_open(seed, P_TYPE, cell, event, n);
  const int sp = species_draw(cum, npart, stream_next(st));
  const double m = mass[sp], m2 = m * m;
  Stream sm = stream_open(seed, P_MOMENTUM, cell, event, n);
  LrfP p;
  int branch = 0;
  if (!sample_momentum(sm, m, sign[sp], c.T_mod, baryon_[sp] * c.alphaB_mod, &p, &t.proposals, &branch)) { t.capped++; return false; }
  t.acceptances++;
  p = rescale_momentum_famod(c, p, m2);
  const double w_flux = fmax(0.0, p.E * c.dst - p.px * c.dsx - p.py * c.dsy - p.pz * c.dsz) / (p.E * c.ds_max);
  if (!(stream_next(sm) < w_flux)) return false;
  lab_record(R, c, p, m2, sp, seed, cell, event, n, out, drawn);
  return true;
}

}  // namespace sampler
}  // namespace is3d
