// sampler_famod_emulator.cpp -- host build of the df_mode 5 particle sampler's math (test-only).
//
// Runs the functions the GPU path calls -- aniso_math.h's aniso_cell under either chain rule (k_aniso, k_chain_pass),
// sampler_math.h's cell_setup_famod, species_weight_famod and candidate_famod (k_cells / k_sample famod variants) --
// serially over a surface.  Built with g++ by tests/sampler_famod_ref.py.
#include <cmath>
#include <vector>

#include "../../is3d2_amd/csrc/aniso_math.h"
#include "../../is3d2_amd/csrc/sampler_math.h"
#include "../../oracle/is3d_oracle.h"

using namespace is3d;
using namespace is3d::sampler;

namespace {

PrepConsts consts(const orc_params* p, const orc_setup* su) {
  PrepConsts k{};
  k.operation = 1;
  k.df_mode = p->df_mode; k.dim = p->dimension; k.include_baryon = p->include_baryon; k.include_bulk = p->include_bulk_deltaf;
  k.include_shear = p->include_shear_deltaf; k.include_diff = p->include_baryondiff_deltaf;
  k.deta_min = p->deta_min; k.mass_pion0 = p->mass_pion0; k.gla_pts = su->gla_points;
  k.gla_r1 = su->gla_root + su->gla_points; k.gla_r2 = su->gla_root + 2 * su->gla_points;
  k.gla_w1 = su->gla_weight + su->gla_points; k.gla_w2 = su->gla_weight + 2 * su->gla_points;
  k.two_pi2_hbarC3 = 2.0 * pow(M_PI, 2) * pow(kHbarC, 3);
  return k;
}

struct Fields {
  const double* f[NSURF];
  explicit Fields(const orc_surface* S)
      : f{S->tau, S->x, S->y, S->eta, S->dat, S->dax, S->day, S->dan, S->ux, S->uy, S->un, S->E, S->T, S->P, S->pixx,
          S->pixy, S->pixn, S->piyy, S->piyn, S->bulkPi, S->muB, S->nB, S->Vx, S->Vy, S->Vn} {}
  void cell(long c, double* s) const {
    for (int i = 0; i < NSURF; i++) s[i] = f[i] ? f[i][c] : 0.0;
  }
};

// The Newton prepass over every cell: `chains` strided chains (0: every cell cold).  sol[n][6], and per cell the
// chain state after it (sta[n][4]), its Newton iterations (-1: not in the chain) and flags (1: pl/pt < 0,
// 2: reconstruction failure); cnt[3] = pl/pt < 0, failures, iterations.
void solve(const PrepConsts& k, const orc_setup* su, const orc_surface* S, int chains, int srule, double* sol, double* sta,
           int* iters, int* flags, long* cnt) {
  const long n = S->n;
  const Fields F(S);
  const int nh = su->npdg < 320 ? su->npdg : 320;
  const Hadrons h{nh, su->pdg_mass, su->pdg_sign, su->pdg_degen};
  const double fp2 = 4.0 * pow(M_PI, 2) * pow(kHbarC, 3);
  auto id = [](double v) { return v; };
  const long C = chains > 0 ? (chains < n ? chains : n) : n;
  for (int i = 0; i < 3; i++) cnt[i] = 0;
  for (long ch = 0; ch < C; ch++) {
    double state[4] = {0, 0, 0, 0};
    for (long c = ch; c < n; c += C) {
      double s[NSURF], R[NREC], ain[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      F.cell(c, s);
      long one[3] = {0, 0, 0};
      iters[c] = -1; flags[c] = 0;
      for (int i = 0; i < 6; i++) sol[6 * c + i] = 0.0;
      if (prep_famod_a(k, s, R, ain)) {
        aniso_cell(ain, h, 0, 1, id, fp2, state, sol + 6 * c, one, srule);
        iters[c] = (int)one[2];
        flags[c] = (one[0] ? 1 : 0) | (one[1] ? 2 : 0);
        for (int i = 0; i < 3; i++) cnt[i] += one[i];
      }
      for (int i = 0; i < 4; i++) sta[4 * c + i] = state[i];
    }
  }
}

}  // namespace

extern "C" void smpf_chain(const orc_params* p, const orc_setup* su, const orc_surface* S, int chains, int srule, double* sol,
                           double* sta, int* iters, int* flags, long* cnt) {
  solve(consts(p, su), su, S, chains, srule, sol, sta, iters, flags, cnt);
}

// The prologue of every cell from the sampler-rule prepass: out[n][12] = live, breaks, Bxx, Bxy, Bxz, Byy, Byz, Bzz,
// det B, lambda, det A, dn_tot (the Poisson mean of one event)
extern "C" void smpf_cells(const orc_params* p, const orc_setup* su, const orc_surface* S, int chains, double y_cut,
                           double* out) {
  const long n = S->n;
  const Fields F(S);
  Run R{};
  R.k = consts(p, su); R.y_max = p->dimension == 2 ? y_cut : 0.5;
  std::vector<double> sol(6 * (size_t)n), sta(4 * (size_t)n);
  std::vector<int> it((size_t)n), fl((size_t)n);
  long cnt[3];
  solve(R.k, su, S, chains, 1, sol.data(), sta.data(), it.data(), fl.data(), cnt);
  for (long c = 0; c < n; c++) {
    double s[NSURF];
    F.cell(c, s);
    Cell cell;
    cell_setup_famod(R, s, &sol[6 * (size_t)c], cell);
    double sum = 0.0;
    if (cell.live != 0.0) {
      for (int a = 0; a < su->npart; a++) sum += species_weight_famod(R, cell, su->mass[a], su->degen[a], su->sign[a], su->baryon[a]);
      cell_finish(R, cell, sum);
    }
    const double o[12] = {cell.live, cell.breaks, cell.pi.xx, cell.pi.xy, cell.pi.xz, cell.pi.yy, cell.pi.yz, cell.pi.zz,
                          cell.shear_mod, cell.T_mod, cell.iso_scale, cell.dn_tot};
    for (int i = 0; i < 12; i++) out[12 * c + i] = o[i];
  }
}

// The sampler over cells [lo, hi), cell by cell (the reference's loop nest).  counts[npart]: kept per species;
// stats[8] = live cells, breakdown cells, candidates, kept, proposals, acceptances, capped, 0; fam[3] = the prepass
// counters; parts (optional, capacity cap, (cell, event, candidate) order).
extern "C" int smpf_sample(const orc_params* p, const orc_setup* su, const orc_surface* S, int chains, long seed,
                           long n_events, double y_cut, long lo, long hi, long* counts, long* stats, long* fam,
                           Particle* parts, long cap) {
  const long n = S->n;
  const int np = su->npart;
  const Fields F(S);
  Run R{};
  R.k = consts(p, su); R.y_max = p->dimension == 2 ? y_cut : 0.5;
  std::vector<double> sol(6 * (size_t)n), sta(4 * (size_t)n);
  std::vector<int> it((size_t)n), fl((size_t)n);
  solve(R.k, su, S, chains, 1, sol.data(), sta.data(), it.data(), fl.data(), fam);
  for (int s = 0; s < np; s++) counts[s] = 0;
  for (int i = 0; i < 8; i++) stats[i] = 0;
  Tally t{0, 0, 0, 0};
  std::vector<double> w(np);
  long nparts = 0;
  for (long c = lo; c < hi; c++) {
    double sv[NSURF];
    F.cell(c, sv);
    Cell cell;
    cell_setup_famod(R, sv, &sol[6 * (size_t)c], cell);
    if (cell.live == 0.0) continue;
    double sum = 0.0, run = 0.0;
    for (int s = 0; s < np; s++) {
      const double v = species_weight_famod(R, cell, su->mass[s], su->degen[s], su->sign[s], su->baryon[s]);
      sum += v;
      run += v > 0.0 ? v : 0.0;
      w[s] = run;
    }
    cell_finish(R, cell, sum);
    if (cell.live == 0.0) continue;
    stats[0]++;
    if (cell.breaks != 0.0) stats[1]++;
    for (long ev = 0; ev < n_events; ev++) {
      Stream ps = stream_open((uint64_t)seed, P_POISSON, c, ev, 0);
      int capped = 0;
      const long N = poisson_draw(ps, cell.dn_tot, &capped);
      t.capped += capped;
      stats[2] += N;
      for (long k = 0; k < N; k++) {
        Particle q;
        double drawn = 0.0;
        if (!candidate_famod(R, cell, (uint64_t)seed, c, ev, k, w.data(), np, su->mass, su->sign, su->baryon, &q, t, drawn)) continue;
        counts[q.species]++;
        if (parts && nparts < cap) parts[nparts] = q;
        nparts++;
      }
    }
  }
  stats[3] = nparts; stats[4] = t.proposals; stats[5] = t.acceptances; stats[6] = t.capped;
  return 0;
}
