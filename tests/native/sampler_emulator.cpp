// sampler_emulator.cpp -- host build of the particle sampler's math (test-only).
//
// Runs is3d2_amd/csrc/sampler_math.h -- the functions k_cells / k_count / k_sample (sampler.hip) call on the device --
// serially: the Philox generator and its streams, the Poisson draw, sample_momentum, and whole cells (prologue,
// species weights, Poisson count per event, candidates).  Built with g++ by tests/test_sampler_cpu.py.
#include <cmath>
#include <cstring>
#include <vector>

#include "../../is3d2_amd/csrc/sampler_math.h"
#include "../../is3d2_amd/csrc/spline_host.h"
#include "../../oracle/is3d_oracle.h"

using namespace is3d;
using namespace is3d::sampler;

namespace {

// delta-f tables and prepass constants on the host (as engine.hip's finalize_tables / make_consts)
struct Tables {
  DfTables tb{};
  PrepConsts k{};
  std::vector<std::vector<double>> sy, sc;
  std::vector<double> jl2, jz, jx, jl2c, jzc;
  Tables(const orc_params* p, const orc_setup* su) : sy(NSPL), sc(NSPL) {
    const int mode = p->df_mode;
    tb.df_mode = mode; tb.include_baryon = p->include_baryon;
    tb.nT = su->nT; tb.nmuB = p->include_baryon ? su->nmuB : 1;
    tb.T = su->Tarr; tb.muB = su->muBarr; tb.tab = su->dftab;
    tb.T_min = su->Tarr[0]; tb.muB_min = su->muBarr[0];
    tb.dT = fabs(su->Tarr[1] - su->Tarr[0]);
    tb.dmuB = su->nmuB > 1 ? fabs(su->muBarr[1] - su->muBarr[0]) : 0.0;
    const int col[NSPL] = {0, 2, 3, 5, 7, 8, 9};
    if (!p->include_baryon) {
      for (int i = 0; i < NSPL; i++) {
        const double* yv = su->dftab + (size_t)col[i] * su->nmuB * su->nT;
        sy[i].assign(yv, yv + su->nT);
        cspline_coeffs(su->Tarr, yv, su->nT, sc[i]);
        tb.sy[i] = sy[i].data(); tb.sc[i] = sc[i].data();
      }
    }
    double bpmax = -1.0;
    if (!p->include_baryon && mode == PTB) {
      jonah_table(su->T_avg, su->npdg, su->pdg_mass, su->pdg_degen, su->pdg_sign, su->gla_root + 2 * su->gla_points,
                  su->gla_weight + 2 * su->gla_points, su->gla_points, jl2, jz, jx, bpmax);
      cspline_coeffs(jx.data(), jl2.data(), 301, jl2c);
      cspline_coeffs(jx.data(), jz.data(), 301, jzc);
      tb.nj = 301; tb.jx = jx.data(); tb.jl2 = jl2.data(); tb.jl2c = jl2c.data(); tb.jz = jz.data(); tb.jzc = jzc.data();
    }
    tb.bulk_over_P_max = bpmax;
    k.operation = 1;
    k.df_mode = mode; k.dim = p->dimension; k.include_baryon = p->include_baryon; k.include_bulk = p->include_bulk_deltaf;
    k.include_shear = p->include_shear_deltaf; k.include_diff = p->include_baryondiff_deltaf;
    k.deta_min = p->deta_min; k.mass_pion0 = p->mass_pion0; k.gla_pts = su->gla_points;
    k.gla_r1 = su->gla_root + su->gla_points; k.gla_r2 = su->gla_root + 2 * su->gla_points;
    k.gla_w1 = su->gla_weight + su->gla_points; k.gla_w2 = su->gla_weight + 2 * su->gla_points;
    k.two_pi2_hbarC3 = 2.0 * pow(M_PI, 2) * pow(kHbarC, 3);
  }
};

// what a run shares, as sampler::run sets it up on the host: the constants, and for fast = 1 the Plasma-average
// densities [3][npart] and PTM's breakdown test at the averages
struct Setup {
  Tables et;
  Run R{};
  std::vector<double> dens;
  int err = 0;
  Setup(const orc_params* p, const orc_setup* su, const double* plasma, double y_cut, int fast) : et(p, su) {
    const int np = su->npart, pts = su->gla_points;
    R.k = et.k; R.fast = fast; R.y_max = p->dimension == 2 ? y_cut : 0.5;
    R.Tavg = plasma[0]; R.F_avg = 0.0; R.betabulk_avg = 1.0;
    dens.assign(3 * (size_t)np, 0.0);
    if (!fast) return;
    DfCoef df;
    err = df_eval(et.tb, plasma[0], plasma[3], plasma[1], plasma[2], 0.0, df);
    if (err) return;
    static const int kAlpha[6] = {1, 1, 1, 2, 3, 3};
    for (int s = 0; s < np; s++) {
      const double T = plasma[0], mbar = su->mass[s] / T, chem = su->baryon[s] * (plasma[3] / T);
      double J[6];
      for (int q = 0; q < 6; q++) {
        double v = 0.0;
        for (int i = 0; i < pts; i++) {
          const long o = (long)kAlpha[q] * pts + i;
          v += su->gla_weight[o] * gt_term(q, su->gla_root[o], mbar, chem, su->sign[s]);
        }
        J[q] = v;
      }
      double d3[3];
      species_densities(p->df_mode, df, T, plasma[4] / (plasma[1] + plasma[2]), su->mass[s], su->degen[s], su->baryon[s], J,
                        et.k.two_pi2_hbarC3, d3);
      for (int i = 0; i < 3; i++) dens[(size_t)i * np + s] = d3[i];
    }
    if (p->df_mode == PTM) {
      DfCoef a;
      err = df_eval(et.tb, plasma[0], plasma[3], 0.0, 0.0, 0.0, a);
      if (err) return;
      R.F_avg = a.F; R.betabulk_avg = a.betabulk;
    }
  }
  // cell c with its running species weights in w[npart]: the df error, or DF_OK with cell.live = 0 for a skipped cell
  int cell(const orc_setup* su, const orc_surface* S, long c, Cell& cell, std::vector<double>& w) const {
    const double* fields[NSURF] = {S->tau, S->x, S->y, S->eta, S->dat, S->dax, S->day, S->dan, S->ux, S->uy, S->un,
                                   S->E, S->T, S->P, S->pixx, S->pixy, S->pixn, S->piyy, S->piyn, S->bulkPi,
                                   S->muB, S->nB, S->Vx, S->Vy, S->Vn};
    const int np = su->npart;
    double sv[NSURF];
    for (int f = 0; f < NSURF; f++) sv[f] = fields[f] ? fields[f][c] : 0.0;
    const int e = cell_setup(R, et.tb, sv, cell);
    if (e || cell.live == 0.0) return e;
    double sum = 0.0, run = 0.0;
    for (int s = 0; s < np; s++) {
      const double v = R.fast ? species_weight_fast(R, cell, dens[s], dens[(size_t)np + s])
                              : species_weight(R, cell, su->mass[s], su->degen[s], su->sign[s], su->baryon[s]);
      sum += v;
      run += v > 0.0 ? v : 0.0;
      w[s] = run;
    }
    cell_finish(R, cell, sum);
    return DF_OK;
  }
};

}  // namespace

extern "C" void smp_philox(const unsigned* ctr, const unsigned* key, unsigned* out) {
  const U4 r = philox4x32_10(U4{{ctr[0], ctr[1], ctr[2], ctr[3]}}, key[0], key[1]);
  for (int i = 0; i < 4; i++) out[i] = r.v[i];
}

extern "C" void smp_uniforms(long seed, int purpose, long cell, long event, long candidate, int n, double* out) {
  Stream s = stream_open((uint64_t)seed, purpose, cell, event, candidate);
  for (int i = 0; i < n; i++) out[i] = stream_next(s);
}

// n draws with the given mean, draw i from the poisson stream of cell i; returns the draws that hit a cap
extern "C" long smp_poisson(long seed, double mean, long n, long* out) {
  long capped = 0;
  for (long i = 0; i < n; i++) {
    Stream s = stream_open((uint64_t)seed, P_POISSON, i, 0, 0);
    int cap = 0;
    out[i] = poisson_draw(s, mean, &cap);
    capped += cap;
  }
  return capped;
}

// n LRF momenta at T = 1 (mass = mbar): out[i] = pbar, costheta, phi, branch, proposals; returns the capped draws
extern "C" long smp_momentum(long seed, double mbar, double sign, double chem, long n, double* out) {
  long capped = 0;
  for (long i = 0; i < n; i++) {
    Stream s = stream_open((uint64_t)seed, P_MOMENTUM, 0, 0, i);
    LrfP p;
    long prop = 0;
    int branch = -1;
    double* o = out + 5 * i;
    if (!sample_momentum(s, mbar, sign, 1.0, chem, &p, &prop, &branch)) { capped++; o[0] = o[1] = o[2] = 0.0; o[3] = -1; o[4] = (double)prop; continue; }
    const double pb = sqrt(p.px * p.px + p.py * p.py + p.pz * p.pz);
    double phi = atan2(p.py, p.px);
    if (phi < 0.0) phi += kTwoPi;
    o[0] = pb; o[1] = p.pz / pb; o[2] = phi; o[3] = (double)branch; o[4] = (double)prop;
  }
  return capped;
}

// The sampler over cells [lo, hi) of a surface for n_events events, cell by cell (the reference's loop nest).
// counts[npart]: kept particles per species; stats[8] = cells with candidates, breakdown cells, candidates, kept,
// proposals, acceptances, capped, clamped; parts (optional, capacity cap records, in (cell, event, candidate) order).
extern "C" int smp_sample(const orc_params* p, const orc_setup* su, const orc_surface* S, const double* plasma, long seed,
                          long n_events, double y_cut, int fast, long lo, long hi, long* counts, long* stats,
                          Particle* parts, long cap) {
  const Setup U(p, su, plasma, y_cut, fast);
  if (U.err) return 100 + U.err;
  const Run& R = U.R;
  const int np = su->npart;
  for (int s = 0; s < np; s++) counts[s] = 0;
  for (int i = 0; i < 8; i++) stats[i] = 0;
  Tally t{0, 0, 0, 0};
  std::vector<double> w(np);
  long nparts = 0;
  for (long c = lo; c < hi; c++) {
    Cell cell;
    const int err = U.cell(su, S, c, cell, w);
    if (err) return 100 + err;
    if (cell.live == 0.0) continue;
    stats[0]++;
    if (cell.breaks != 0.0) stats[1]++;
    for (long ev = 0; ev < n_events; ev++) {
      Stream ps = stream_open((uint64_t)seed, P_POISSON, c, ev, 0);
      int capped = 0;
      const long N = poisson_draw(ps, cell.dn_tot, &capped);
      t.capped += capped;
      stats[2] += N;
      for (long n = 0; n < N; n++) {
        Particle q;
        if (!candidate(R, cell, (uint64_t)seed, c, ev, n, w.data(), np, su->mass, su->sign, su->baryon, &q, t, nullptr)) continue;
        counts[q.species]++;
        if (parts && nparts < cap) parts[nparts] = q;
        nparts++;
      }
    }
  }
  stats[3] = nparts; stats[4] = t.proposals; stats[5] = t.acceptances; stats[6] = t.capped; stats[7] = t.clamped;
  return 0;
}

// Diagnostic of tests/test_gpu_sampler_emulator.py: the candidates of one (cell, event).  out[6 i ..] = species, kept
// (candidate()'s decision), the keep draw u, the keep weight w_flux x w_visc, proposals, and 1 where u < weight is not
// that decision.  u is the momentum stream's draw after a replayed sample_momentum; the weight restates
// candidate()'s own lines (sampler_math.h keeps them inline for the kernels' register count) and is for the message only.
// Returns the number of candidates N (rows beyond cap are not written), or -1 - err.
extern "C" long smp_trace(const orc_params* p, const orc_setup* su, const orc_surface* S, const double* plasma, long seed,
                          double y_cut, int fast, long c, long ev, double* out, long cap) {
  const Setup U(p, su, plasma, y_cut, fast);
  if (U.err) return -1 - U.err;
  const Run& R = U.R;
  const int np = su->npart, mode = R.k.df_mode;
  std::vector<double> w(np);
  Cell cell;
  const int err = U.cell(su, S, c, cell, w);
  if (err) return -1 - err;
  if (cell.live == 0.0) return 0;
  Stream ps = stream_open((uint64_t)seed, P_POISSON, c, ev, 0);
  int capped = 0;
  const long N = poisson_draw(ps, cell.dn_tot, &capped);
  for (long n = 0; n < N && n < cap; n++) {
    Particle q;
    Tally t{0, 0, 0, 0};
    const bool kept = candidate(R, cell, (uint64_t)seed, c, ev, n, w.data(), np, su->mass, su->sign, su->baryon, &q, t, nullptr);
    Stream st = stream_open((uint64_t)seed, P_TYPE, c, ev, n);
    const int sp = species_draw(w.data(), np, stream_next(st));
    const double m = su->mass[sp], m2 = m * m, sg = su->sign[sp], baryon = su->baryon[sp];
    const bool modified = (mode == PTM || mode == PTB) && cell.breaks == 0.0;
    Stream sm = stream_open((uint64_t)seed, P_MOMENTUM, c, ev, n);
    LrfP l;
    long prop = 0;
    int branch = 0;
    const bool ok = mode == PTM && modified ? sample_momentum(sm, m, sg, cell.T_mod, baryon * cell.alphaB_mod, &l, &prop, &branch)
                    : mode == PTB ? sample_momentum(sm, m, sg, cell.T, 0.0, &l, &prop, &branch)
                                  : sample_momentum(sm, m, sg, cell.T, baryon * cell.alphaB, &l, &prop, &branch);
    double u = -1.0, wk = -1.0;
    if (ok) {
      double w_visc = 1.0;
      if (modified) {
        l = rescale_momentum(cell, l, m2, mode == PTM ? baryon : 0.0, mode == PTM);
      } else {
        const double E = l.E, px = l.px, py = l.py, pz = l.pz, feqbar = 1.0 - sg * l.feq;
        const PiLRF& pi = cell.pi;
        const DfCoef& df = cell.df;
        const double pipp = px * px * pi.xx + py * py * pi.yy + pz * pz * pi.zz + 2.0 * (px * py * pi.xy + px * pz * pi.xz + py * pz * pi.yz);
        const double Vp = -(px * cell.Vx + py * cell.Vy + pz * cell.Vz);
        double dfv;
        if (mode == GRAD)
          dfv = feqbar * (pipp / df.shear14 + ((df.c0 - df.c2) * m2 + (baryon * df.c1 + (4.0 * df.c2 - df.c0) * E) * E) * cell.bulkPi +
                          (baryon * df.c3 + df.c4 * E) * Vp);
        else if (mode == PTB)
          dfv = feqbar * pipp / (2.0 * df.betapi * cell.T * E) + (df.dz - 3.0 * df.dlambda) + feqbar * (df.dlambda / cell.T) * (E - m2 / E);
        else
          dfv = feqbar * (pipp / (2.0 * df.betapi * cell.T * E) +
                          (baryon * df.G + df.F / (cell.T * cell.T) * E + (E - m2 / E) / (3.0 * cell.T)) * (cell.bulkPi / df.betabulk) +
                          (cell.ber - baryon / E) * Vp / df.betaV);
        w_visc = 0.5 * (1.0 + fmax(-1.0, fmin(1.0, dfv)));
      }
      wk = fmax(0.0, l.E * cell.dst - l.px * cell.dsx - l.py * cell.dsy - l.pz * cell.dsz) / (l.E * cell.ds_max) * w_visc;
      u = stream_next(sm);
    }
    double* o = out + 6 * n;
    o[0] = sp; o[1] = kept ? 1.0 : 0.0; o[2] = u; o[3] = wk; o[4] = (double)prop; o[5] = (ok && (u < wk)) != kept ? 1.0 : 0.0;
  }
  return N;
}
