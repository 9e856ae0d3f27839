// engine_sample.hip -- operation = 2 of the engine (engine.h): the oversampling estimate (is3d_total_yield), the particle
// sampler with its bins, histogram and list getters, and the Monte Carlo decays of a particle list.  The sampler's
// kernels are in sampler.hip and the list decays' in decay_list.hip; this unit's own are the plasma-average densities
// and the yield sum (engine_sample_kernels.h).  What a call leaves behind lives in one SampledList (sampled_list.h):
// the engine's, or for a device-list engine the group's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/is3d_amd.h"
#include "cf_math.h"
#include "kernels.h"
#include "group.h"
#include "engine.h"
#include "sample_decay_plan.h"

using namespace is3d;
using namespace is3d::kern;

#include "engine_sample_kernels.h"   // this unit's device code (k_densities, k_yield)

// operation 2: the plasma-average densities (DeltafData.cpp:555-690) into dens[3 npart], synchronously.  Returns the
// device error word (df_error maps it), or -1 after a HIP failure (the engine's error is set)
static int plasma_densities(is3d_engine* e, const double* plasma, double* dens) {
  const int np = (int)e->in.mass.size();
  DensArgs da{};
  da.tb = e->tbl.dtb; da.gla = e->tbl.d_gla; da.gla_alpha = e->in.gla_alpha; da.gla_pts = e->in.gla_pts;
  da.T = plasma[0]; da.E = plasma[1]; da.P = plasma[2]; da.muB = plasma[3]; da.nB = plasma[4];
  da.smass = e->tbl.d_smass; da.ssign = e->tbl.d_ssign; da.sdegen = e->tbl.d_sdegen; da.sbaryon = e->tbl.d_sbaryon; da.sorig = e->tbl.d_sorig;
  da.npart = np; da.df_mode = e->in.p.df_mode; da.two_pi2_hbarC3 = 2.0 * std::pow(M_PI, 2) * std::pow(kHbarC, 3);
  da.dens = dens; da.err = e->ws.d_err.get();
  int derr = 0;
  hipError_t h = hipMemset(e->ws.d_err.get(), 0, sizeof(int));
  if (h == hipSuccess) {
    hipLaunchKernelGGL(k_densities, dim3((unsigned)np), dim3(64), 0, 0, da);
    h = hipGetLastError();
  }
  if (h == hipSuccess) h = hipDeviceSynchronize();
  if (h == hipSuccess) h = hipMemcpy(&derr, e->ws.d_err.get(), sizeof(int), hipMemcpyDeviceToHost);
  if (h != hipSuccess) { hip_fail(e, h, "plasma densities"); return -1; }
  return derr;
}

extern "C" int is3d_total_yield(is3d_engine* e, const double* plasma, double y_cut, double* n_total,
                                double* densities) {
  if (e && e->grp) return is3d::group_total_yield(e->grp, plasma, y_cut, n_total, densities);
  if (!e || !plasma || !n_total) return IS3D_ERR_ARG;
  int rc = finalize_tables(e);
  if (rc) return rc;
  if (!e->in.have_gla || e->in.gla_alpha < 4) return e->fail(IS3D_ERR_STATE, "is3d_set_gauss_laguerre: alpha = 1..3 tables needed");
  if (e->in.gla_pts > 64) return e->fail(IS3D_ERR_ARG, "Gauss-Laguerre table longer than 64 points");
  HIPCHK(e, hipSetDevice(e->device));
  const int np = (int)e->in.mass.size();
  const long n = e->sf.ncell;
  const long nb = (n + 255) / 256;
  DevBuf<double> buf;       // densities [3 np] | k_yield's partial sums [nb]
  if (!buf.reserve(3L * np + std::max(nb, 1L) + 1)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc failed");
  double* const d = buf.get();
  int derr = plasma_densities(e, plasma, d);
  if (derr < 0) return IS3D_ERR_DEVICE;
  std::vector<double> part((size_t)std::max(nb, 1L), 0.0);
  if (!derr && n > 0) {     // k_yield reports through the same error word
    YieldArgs ya{};
    ya.k = make_consts(e); ya.tb = e->tbl.dtb; ya.surf = e->sf.d_surf; ya.n = n; ya.dens = d; ya.npart = np;
    ya.partial = d + 3 * (size_t)np; ya.err = e->ws.d_err.get();
    hipLaunchKernelGGL(k_yield, dim3((unsigned)nb), dim3(256), 0, 0, ya);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipDeviceSynchronize());
    HIPCHK(e, hipMemcpy(&derr, e->ws.d_err.get(), sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(e, hipMemcpy(part.data(), d + 3 * (size_t)np, nb * sizeof(double), hipMemcpyDeviceToHost));
  }
  if (densities) HIPCHK(e, hipMemcpy(densities, d, 3 * (size_t)np * sizeof(double), hipMemcpyDeviceToHost));
  if (derr) return df_error(e, derr, "df coefficient error");
  double Ntot = 0.0;
  for (long b = 0; b < nb; b++) Ntot += part[b];
  if (e->in.p.dimension == 2) Ntot *= 2.0 * y_cut;     // :628-631
  *n_total = Ntot;
  return IS3D_OK;
}

// ------------------------------------------------------------------------------------------
// operation = 2 particle sampler (ParticleSampler.cpp:638-1134; kernels in sampler.hip)
// ------------------------------------------------------------------------------------------
static is3d::sampler::Bins sampler_bins(const is3d_sample_bins& b) {
  return is3d::sampler::make_bins(b.pT_min, b.pT_max, b.pT_bins, b.y_cut, b.y_bins, b.phip_bins, b.eta_cut, b.eta_bins,
                                  b.tau_min, b.tau_max, b.tau_bins, b.r_min, b.r_max, b.r_bins);
}

// the list a getter reads: the group's merged one for a device-list engine
static const SampledList& list_of(const is3d_engine* e) { return e->grp ? is3d::group_list(e->grp) : e->smp.list; }
const is3d::SampledList& is3d_internal_sampled_list(const is3d_engine* e) { return e->smp.list; }

// The histogram of a binned call, from the engine's bins: hist_begin sizes it, reserves and zeroes d_hist (the kernels
// add to H.d); hist_end copies it back into `to` in integer form.  The caller commits `to`.  nomem: the message of a
// failed allocation
struct HistRun {
  is3d::sampler::Bins bins{};
  unsigned long long* d = nullptr;
  long nc = 0, nv = 0;
};
static int hist_begin(is3d_engine* e, HistRun& H, const std::string& nomem) {
  const int np = (int)e->in.mass.size();
  H.bins = sampler_bins(e->smp.bins);
  H.nc = is3d::sampler::hist_counts(H.bins, np);
  H.nv = is3d::sampler::hist_vn(H.bins, np);
  if (!e->smp.d_hist.reserve(H.nc + H.nv)) return e->fail(IS3D_ERR_DEVICE, nomem);
  H.d = e->smp.d_hist.get();
  HIPCHK(e, hipMemset(H.d, 0, (size_t)(H.nc + H.nv) * sizeof(unsigned long long)));
  return IS3D_OK;
}
static int hist_end(is3d_engine* e, const HistRun& H, SampledList& to) {
  to.hist.assign((size_t)(H.nc + H.nv), 0);
  to.hist_nc = H.nc; to.hist_nv = H.nv;
  HIPCHK(e, hipMemcpy(to.hist.data(), H.d, to.hist.size() * sizeof(long long), hipMemcpyDeviceToHost));
  return IS3D_OK;
}

// the plan's Monte Carlo tables on the device, rebuilt when the channels or the species changed
static int decay_tables(is3d_engine* e, const std::string& w) {
  if (!e->is_stale(D_DECAY_LIST)) return IS3D_OK;
  const std::string m = is3d::decay_list::tables_build(e->dl.tables, e->fd.plan, e->in.mass);
  if (!m.empty()) return e->fail(IS3D_ERR_DEVICE, w + m);
  e->rebuilt(D_DECAY_LIST);
  return IS3D_OK;
}

// is3d_sample_decayed: what the list decays need next to the sampler's arguments
struct FusedDecay {
  long seed;
  int list, bin;
};

// The body of is3d_sample_decayed once sample_any has checked the arguments and filled the sampler's Config: every
// compacted batch of the sampler is decayed where it lies.  The sampler plans its batches within half
// of "sample_bytes"; the decay stage's records take what a batch leaves of the whole bound, in sub-ranges of the
// batch when they need more.  Neither bound changes a byte of the result.
static int sample_decayed_batches(is3d_engine* e, is3d::sampler::Config c, bool famod, const FusedDecay& f) {
  namespace dl = is3d::decay_list;
  namespace sm = is3d::sampler;
  const std::string w = "is3d_sample_decayed: ";
  SampledList& out = e->smp.list;
  int rc = decay_tables(e, w);
  if (rc) return rc;
  const long bound = std::max(e->smp.sample_bytes, 1L);
  c.sample_bytes = std::max(bound / 2, 1L);
  c.bound_note = " (the sampler's half of the bound, the other is the decays')";
  dl::Config dc;
  dc.seed = (uint64_t)f.seed;
  dc.sample_bytes = bound;
  HistRun H;
  if (f.bin) {
    rc = hist_begin(e, H, w + "hipMalloc(histogram) failed");
    if (rc) return rc;
    dc.bins = &H.bins; dc.hist = H.d;
  }
  SampledList d;      // the decayed list, built beside the engine's
  std::vector<long> prim_off((size_t)c.n_events + 1, 0);     // the primaries' offsets: the list the two calls would hold
  dl::Stats ds;
  ds.passes = e->dl.tables.levels;
  dl::Stage stage;
  DevBuf<long> d_bounds;
  std::vector<long> bounds;
  sdp::Carry carry;
  long running = 0;     // primaries of the batches before this one: the origin of its first record
  const sm::Consumer consume = [&](const sm::Batch& b, std::string& m) -> int {
    bounds.assign((size_t)b.nev + 1, 0);
    hipError_t h = d_bounds.reserve(b.nev + 1) ? hipSuccess : hipErrorOutOfMemory;
    if (h == hipSuccess) h = dl::batch_bounds(b.slots, b.pos, b.nev, b.c1 - b.c0, d_bounds.get());
    if (h == hipSuccess) h = hipMemcpy(bounds.data(), d_bounds.get(), bounds.size() * sizeof(long), hipMemcpyDeviceToHost);
    if (h != hipSuccess) { m = std::string("the event bounds of a batch: ") + hipGetErrorString(h); return sm::S_DEVICE; }
    const uint64_t cy = carry.before(b.e0, b.nev);
    for (long k = 0; k < b.nev; k++) {
      const long cnt = bounds[(size_t)k + 1] - bounds[(size_t)k];
      if (!sdp::event_fits(k == 0 ? cy : 0ull, cnt)) { m = "event " + std::to_string(b.e0 + k) + " has 2^32 or more primaries"; return sm::S_BUDGET; }
      prim_off[(size_t)(b.e0 + k) + 1] += cnt;
    }
    sdp::SubRanges R(b.kept, sdp::first_guess(bound - b.batch_bytes, 0, dl::kRecBytes));
    while (!R.done()) {
      dl::Source src;
      src.d = b.d + R.at; src.n = R.len; src.origin0 = running + R.at;
      src.bounds = d_bounds.get(); src.nev = b.nev; src.first = R.at; src.carry = cy;
      long finals = 0, need = 0;
      int s = stage.decay(e->dl.tables, dc, src, b.batch_bytes, f.list != 0, ds, finals, need, m);
      if (s == dl::S_BUDGET) {
        if (R.halve()) continue;
        m = dl::too_big_message(running + R.at, need, bound);
        return sm::S_BUDGET;
      }
      if (s == dl::S_OK && f.list) s = dl::download(stage, finals, d.particles, d.origins, ds, m);
      if (s != dl::S_OK) return sm::S_DEVICE;
      R.accept();
    }
    carry.after(b.e0, b.nev, b.kept);
    running += b.kept;
    return sm::S_OK;
  };
  sm::Stats st;
  int derr = 0;
  std::string msg;
  const int s = sm::run(e->smp.tables, c, consume, st, derr, msg);
  e->smp.list_d2h = ds.list_d2h;
  if (s == sm::S_DF) return df_error(e, derr, "df coefficient error");
  if (s == sm::S_DEVICE) return e->fail(IS3D_ERR_DEVICE, w + msg);
  if (s == sm::S_BUDGET) return e->fail(IS3D_ERR_ARG, w + msg);
  for (long k = 0; k < c.n_events; k++) prim_off[(size_t)k + 1] += prim_off[(size_t)k];
  ds.primaries = running;
  if (f.bin) {
    rc = hist_end(e, H, d);
    if (rc) return rc;
  }
  // the offsets of the decayed list: origins are non-decreasing, so event k ends where the origins reach its end
  d.offsets.assign((size_t)c.n_events + 1, 0);
  size_t j = 0;
  for (long k = 0; k < c.n_events && f.list; k++) {
    while (j < d.origins.size() && d.origins[j] < prim_off[(size_t)k + 1]) j++;
    d.offsets[(size_t)k + 1] = (long)j;
  }
  d.decay_stats = is3d_decay_list_stats{ds.primaries, ds.decays, ds.undecayed, ds.dropped_daughters, ds.capped,
                                      ds.final_particles, ds.passes, ds.batches, ds.ms_total};
  out.stats = is3d_sample_stats{st.cells, st.breakdown, st.candidates, st.kept, st.proposals, st.acceptances, st.capped,
                             st.clamped, st.batches};
  out.commit_sample_decayed(d, famod, f.list != 0, f.bin != 0);
  return IS3D_OK;
}

// cell_base: global index of this engine's cell 0 (a shard of a device-list engine holds only its window)
// famod: the df_mode 5 method (is3d_sample_famod; plasma unused, fast ignored): the Newton prepass under the sampler's
// chain rule first, then the same sampler with the k_cells / k_sample famod variants reading d_sol
// fused: is3d_sample_decayed -- the same checks and setup, then the batches are decayed on the device
static int sample_any(is3d_engine* e, const is3d_sample_params* sp, const double* plasma, long cell_base, int binned,
                      bool famod, const FusedDecay* fused = nullptr) {
  if (!e || e->grp) return IS3D_ERR_ARG;
  SampledList& out = e->smp.list;
  out.begin_sample();
  e->smp.list_h2d = e->smp.list_d2h = 0;
  if (fused) {
    const std::string w = "is3d_sample_decayed: ";
    if (!fused->list && !fused->bin) return e->fail(IS3D_ERR_ARG, w + "list = 0 and bin = 0 leave nothing to return");
    if (!e->have_decays()) return e->fail(IS3D_ERR_STATE, w + "no decay channels set (is3d_set_decays)");
    if (fused->bin && !e->smp.have_bins) return e->fail(IS3D_ERR_STATE, w + "is3d_set_sample_bins not called");
    if (fused->seed < 0) return e->fail(IS3D_ERR_ARG, w + "the seed must be non-negative");
    const std::string plan_err = is3d::decay_mc::check_plan(e->fd.plan);
    if (!plan_err.empty()) return e->fail(IS3D_ERR_ARG, w + plan_err);
  }
  if (!sp || (!famod && !plasma)) return e->fail(IS3D_ERR_ARG, "is3d_sample: null argument");
  if (!famod && e->in.have_params && e->in.p.df_mode == PTMA)
    return e->fail(IS3D_ERR_UNSUPPORTED, "is3d_sample: df_mode 5 has its own method (sample_dN_pTdpTdphidy_famod): call is3d_sample_famod");
  if (famod && (!e->in.have_params || e->in.p.df_mode != PTMA))
    return e->fail(IS3D_ERR_STATE, "is3d_sample_famod: needs params with df_mode 5 (df_mode 1-4: is3d_sample)");
  if (famod && e->in.pdg_mass.empty()) return e->fail(IS3D_ERR_STATE, "is3d_sample_famod: no PDG table set (is3d_set_pdg)");
  if (famod && e->sf.chain_q1 >= 0) return e->fail(IS3D_ERR_STATE, "is3d_sample_famod: a chain range is set (is3d_set_chain_range); the sampler solves the whole chain");
  if (sp->n_events < 1) return e->fail(IS3D_ERR_ARG, "is3d_sample: n_events must be >= 1");
  if (!(sp->y_cut > 0.0)) return e->fail(IS3D_ERR_ARG, "is3d_sample: y_cut must be positive");
  if (sp->seed < 0) return e->fail(IS3D_ERR_ARG, "is3d_sample: the seed must be non-negative (a negative sampler_seed takes the clock on the host)");
  if (binned && !e->smp.have_bins) return e->fail(IS3D_ERR_STATE, "is3d_sample_binned: is3d_set_sample_bins not called");
  int rc = finalize_tables(e);
  if (rc) return rc;
  if (!e->sf.have_surf) return e->fail(IS3D_ERR_STATE, "is3d_sample: no surface set");
  const int fast = (sp->fast && !famod) ? 1 : 0;
  if (!e->in.have_gla || e->in.gla_alpha < (fast ? 4 : 3)) return e->fail(IS3D_ERR_STATE, "is3d_set_gauss_laguerre: alpha = 1..3 tables needed");
  if (e->in.gla_pts > 64) return e->fail(IS3D_ERR_ARG, "Gauss-Laguerre table longer than 64 points");
  HIPCHK(e, hipSetDevice(e->device));
  if (e->is_stale(D_SAMPLER)) {
    const std::string m = is3d::sampler::tables_build(e->smp.tables, e->in.mass, e->in.sign, e->in.degen, e->in.baryon);
    if (!m.empty()) return e->fail(IS3D_ERR_DEVICE, "is3d_sample: " + m);
    e->rebuilt(D_SAMPLER);
  }
  const int np = (int)e->in.mass.size();
  is3d::sampler::Config c;
  c.run.k = make_consts(e);
  c.run.fast = fast;
  c.run.y_max = e->in.p.dimension == 2 ? sp->y_cut : 0.5;
  c.run.Tavg = famod ? 0.0 : plasma[0]; c.run.F_avg = 0.0; c.run.betabulk_avg = 1.0;
  c.tb = e->tbl.dtb; c.surf = e->sf.d_surf; c.n = e->sf.ncell;
  cell_window(e, c.lo, c.hi);
  c.cell_base = cell_base; c.seed = (uint64_t)sp->seed; c.n_events = sp->n_events; c.sample_bytes = e->smp.sample_bytes;
  DevBuf<double> dens;
  if (fast) {     // Plasma-average densities (DeltafData.cpp:555-690) and PTM's average df coefficients (:664-673)
    if (!dens.reserve(3L * np)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc failed");
    const int derr = plasma_densities(e, plasma, dens.get());
    if (derr) return derr < 0 ? IS3D_ERR_DEVICE : df_error(e, derr, "df coefficient error");
    if (e->in.p.df_mode == PTM) {
      double o[15];
      rc = is3d_evaluate_df_coefficients(e, plasma[0], plasma[3], 0.0, 0.0, 0.0, o);
      if (rc) return rc;
      c.run.F_avg = o[6]; c.run.betabulk_avg = o[8];
    }
    c.dens = dens.get();
  }
  if (famod && c.hi > c.lo) {
    // (lambda, aT, aL) of the cells: the whole surface along the chains, or the window cold (famod_chains = 0)
    rc = run_prepass(e, nullptr, 1, 1);
    if (rc) return rc;
    HIPCHK(e, hipStreamSynchronize(nullptr));
    rc = read_counters(e);
    if (rc) return rc;
    out.famod_stats = is3d_sample_famod_stats{e->ws.st.pl_negative, e->ws.st.recon_fail, e->ws.st.iterations};
    c.sol = e->ws.d_sol.get();
  } else if (famod) {
    out.famod_stats = is3d_sample_famod_stats{};
  }
  if (fused) return sample_decayed_batches(e, c, famod, *fused);
  HistRun H;
  if (binned) {
    rc = hist_begin(e, H, "hipMalloc(sampler histogram) failed");
    if (rc) return rc;
    c.bins = &H.bins; c.hist = H.d; c.keep_list = binned == 2;
  }
  is3d::sampler::Stats st;
  int derr = 0;
  std::string msg;
  const int s = is3d::sampler::run(e->smp.tables, c, out.particles, out.offsets, st, derr, msg);
  e->smp.list_d2h = st.list_d2h;
  if (s == is3d::sampler::S_DF) return df_error(e, derr, "df coefficient error");
  if (s == is3d::sampler::S_DEVICE) return e->fail(IS3D_ERR_DEVICE, "is3d_sample: " + msg);
  if (s == is3d::sampler::S_BUDGET) return e->fail(IS3D_ERR_ARG, "is3d_sample: " + msg);
  out.stats = is3d_sample_stats{st.cells, st.breakdown, st.candidates, st.kept, st.proposals, st.acceptances, st.capped,
                             st.clamped, st.batches};
  if (binned) {
    rc = hist_end(e, H, out);
    if (rc) return rc;
  }
  out.commit_sample(famod, binned != 0);
  return IS3D_OK;
}

int is3d_internal_sample(is3d_engine* e, const is3d_sample_params* sp, const double* plasma, long cell_base, int binned) {
  return sample_any(e, sp, plasma, cell_base, binned, false);
}
int is3d_internal_sample_famod(is3d_engine* e, const is3d_sample_params* sp, long cell_base, int binned) {
  return sample_any(e, sp, nullptr, cell_base, binned, true);
}

extern "C" int is3d_sample_famod(is3d_engine* e, const is3d_sample_params* sp, int binned) {
  if (e && e->grp) return is3d::group_sample_famod(e->grp, sp, binned);
  if (e && (binned < 0 || binned > 2)) return e->fail(IS3D_ERR_ARG, "is3d_sample_famod: binned must be 0, 1 or 2");
  return is3d_internal_sample_famod(e, sp, 0, binned);
}

extern "C" int is3d_get_sample_famod_stats(const is3d_engine* e, is3d_sample_famod_stats* out) {
  return e ? list_of(e).get_famod_stats(out) : IS3D_ERR_ARG;
}

extern "C" int is3d_sample(is3d_engine* e, const is3d_sample_params* sp, const double* plasma) {
  if (e && e->grp) return is3d::group_sample(e->grp, sp, plasma, 0);
  return is3d_internal_sample(e, sp, plasma, 0, 0);
}

extern "C" int is3d_sample_decayed(is3d_engine* e, const is3d_sample_params* sp, const double* plasma, long decay_seed,
                                   int list, int bin) {
  if (e && e->grp) return is3d::group_sample_decayed(e->grp, sp, plasma, decay_seed, list, bin);
  if (!e) return IS3D_ERR_ARG;
  const FusedDecay f{decay_seed, list ? 1 : 0, bin ? 1 : 0};
  const bool famod = e->in.have_params && e->in.p.df_mode == PTMA;
  return sample_any(e, sp, famod ? nullptr : plasma, 0, 0, famod, &f);
}

extern "C" int is3d_set_sample_bins(is3d_engine* e, const is3d_sample_bins* b) {
  if (e && e->grp) return b ? is3d::group_set_sample_bins(e->grp, b) : IS3D_ERR_ARG;
  if (!e || !b) return IS3D_ERR_ARG;
  if (b->pT_bins < 1 || b->y_bins < 1 || b->phip_bins < 1 || b->eta_bins < 1 || b->tau_bins < 1 || b->r_bins < 1)
    return e->fail(IS3D_ERR_ARG, "is3d_set_sample_bins: every bin count must be >= 1");
  if (!(b->pT_max > b->pT_min) || !(b->tau_max > b->tau_min) || !(b->r_max > b->r_min))
    return e->fail(IS3D_ERR_ARG, "is3d_set_sample_bins: pT, tau and r ranges must be increasing");
  if (!(b->y_cut > 0.0) || !(b->eta_cut > 0.0)) return e->fail(IS3D_ERR_ARG, "is3d_set_sample_bins: y_cut and eta_cut must be positive");
  e->smp.bins = *b;
  e->smp.have_bins = true;
  e->smp.list.bins_changed();
  return IS3D_OK;
}

extern "C" int is3d_sample_binned(is3d_engine* e, const is3d_sample_params* sp, const double* plasma, int keep_list) {
  if (e && e->grp) return is3d::group_sample(e->grp, sp, plasma, keep_list ? 2 : 1);
  return is3d_internal_sample(e, sp, plasma, 0, keep_list ? 2 : 1);
}

extern "C" long is3d_sample_hist_size(const is3d_engine* e, long* n_counts, long* n_vn) {
  if (e && e->grp) return is3d::group_sample_hist_size(e->grp, n_counts, n_vn);
  if (!e || !e->smp.have_bins || e->in.mass.empty()) return -1;
  const is3d::sampler::Bins sb = sampler_bins(e->smp.bins);
  const long nc = is3d::sampler::hist_counts(sb, (int)e->in.mass.size()), nv = is3d::sampler::hist_vn(sb, (int)e->in.mass.size());
  if (n_counts) *n_counts = nc;
  if (n_vn) *n_vn = nv;
  return nc + nv;
}

extern "C" int is3d_get_sample_hist(const is3d_engine* e, long* counts, double* vn) {
  return e ? list_of(e).get_hist(counts, vn) : IS3D_ERR_ARG;
}

extern "C" long is3d_sample_count(const is3d_engine* e) {
  return e ? list_of(e).count() : -1;
}

extern "C" int is3d_sample_offsets(const is3d_engine* e, long* offsets) {
  return e ? list_of(e).get_offsets(offsets) : IS3D_ERR_ARG;
}

extern "C" int is3d_get_particles(const is3d_engine* e, long first, long count, is3d_particle* out) {
  return e ? list_of(e).get_particles(first, count, out) : IS3D_ERR_ARG;
}

extern "C" int is3d_get_sample_stats(const is3d_engine* e, is3d_sample_stats* out) {
  return e ? list_of(e).get_stats(out) : IS3D_ERR_ARG;
}

extern "C" int is3d_sample_uniforms(is3d_engine* e, long seed, int purpose, long cell, long event, long candidate, int n,
                                    double* out) {
  if (e && e->grp) return is3d::group_fail(e->grp, IS3D_ERR_UNSUPPORTED, "is3d_sample_uniforms: a one-device test hook");
  if (!e || !out || n < 0 || seed < 0 || purpose < 0 || purpose > 3 || cell < 0 || event < 0 || candidate < 0)
    return e ? e->fail(IS3D_ERR_ARG, "is3d_sample_uniforms: bad argument") : IS3D_ERR_ARG;
  HIPCHK(e, hipSetDevice(e->device));
  HIPCHK(e, is3d::sampler::uniforms((uint64_t)seed, purpose, cell, event, candidate, n, out));
  return IS3D_OK;
}

// ------------------------------------------------------------------------------------------
// Monte Carlo decays of a particle list (do_resonance_decays with operation = 2; method in decay_mc_math.h, kernels in
// decay_list.hip)
// ------------------------------------------------------------------------------------------
// in may be the engine's own list: nothing of the engine changes before the call has succeeded
static int decay_list_any(is3d_engine* e, long seed, int n_events, const long* offsets, const is3d_particle* in, int bin,
                          const char* who) {
  const std::string w = std::string(who) + ": ";
  if (!e->have_decays()) return e->fail(IS3D_ERR_STATE, w + "no decay channels set (is3d_set_decays)");
  if (bin && !e->smp.have_bins) return e->fail(IS3D_ERR_STATE, w + "is3d_set_sample_bins not called");
  if (seed < 0) return e->fail(IS3D_ERR_ARG, w + "the seed must be non-negative");
  if (n_events < 0 || !offsets) return e->fail(IS3D_ERR_ARG, w + "bad event offsets");
  const std::string plan_err = is3d::decay_mc::check_plan(e->fd.plan);
  if (!plan_err.empty()) return e->fail(IS3D_ERR_ARG, w + plan_err);
  const int np = (int)e->in.mass.size();
  const long i0 = offsets[0], n = offsets[n_events] - i0;
  if (i0 < 0 || n < 0 || (n > 0 && !in)) return e->fail(IS3D_ERR_ARG, w + "bad event offsets");
  for (int k = 0; k < n_events; k++)
    if (offsets[k + 1] < offsets[k]) return e->fail(IS3D_ERR_ARG, w + "the event offsets decrease at event " + std::to_string(k));
  std::vector<uint32_t> prim((size_t)n);
  long last_event = 0;
  bool seen = false;
  for (int k = 0; k < n_events; k++) {
    const long a = offsets[k], b = offsets[k + 1];
    if (b - a > 0xffffffffL) return e->fail(IS3D_ERR_ARG, w + "event " + std::to_string(k) + " has 2^32 or more primaries");
    for (long i = a; i < b; i++) {
      if (in[i].species < 0 || in[i].species >= np)
        return e->fail(IS3D_ERR_ARG, w + "record " + std::to_string(i) + ": species index out of range");
      if (in[i].event != in[a].event)
        return e->fail(IS3D_ERR_ARG, w + "record " + std::to_string(i) + ": the events are not contiguous");
      prim[(size_t)(i - i0)] = (uint32_t)(i - a);
    }
    if (b > a) {
      // equal values would give two events one set of streams (primary index, event, path)
      if (seen && in[a].event <= last_event)
        return e->fail(IS3D_ERR_ARG, w + "record " + std::to_string(a) + ": the event field does not increase from event to event");
      last_event = in[a].event;
      seen = true;
    }
  }
  HIPCHK(e, hipSetDevice(e->device));
  e->smp.list_h2d = e->smp.list_d2h = 0;
  const int trc = decay_tables(e, w);
  if (trc) return trc;
  is3d::decay_list::Config c;
  c.seed = (uint64_t)seed;
  c.sample_bytes = e->smp.sample_bytes;
  HistRun H;
  if (bin) {
    const int rc = hist_begin(e, H, w + "hipMalloc(histogram) failed");
    if (rc) return rc;
    c.bins = &H.bins; c.hist = H.d;
  }
  SampledList d;      // the decayed list, built beside the engine's
  std::vector<long>& origin = d.origins;
  is3d::decay_list::Stats st;
  std::string msg;
  const int s = is3d::decay_list::run(e->dl.tables, c, n, reinterpret_cast<const is3d::sampler::Particle*>(in) + i0, prim.data(),
                                      d.particles, origin, st, msg);
  e->smp.list_h2d = st.list_h2d;
  e->smp.list_d2h = st.list_d2h;
  if (s == is3d::decay_list::S_DEVICE) return e->fail(IS3D_ERR_DEVICE, w + msg);
  if (s == is3d::decay_list::S_BUDGET) return e->fail(IS3D_ERR_ARG, w + msg);
  if (bin) {
    const int rc = hist_end(e, H, d);
    if (rc) return rc;
  }
  // the offsets of the decayed list: origins are non-decreasing, so event k ends where the origins reach its end
  std::vector<long>& off = d.offsets;
  off.assign((size_t)n_events + 1, 0);
  size_t j = 0;
  for (int k = 0; k < n_events; k++) {
    while (j < origin.size() && origin[j] < offsets[k + 1] - i0) j++;
    off[(size_t)k + 1] = (long)j;
  }
  for (long& o : origin) o += i0;
  d.decay_stats = is3d_decay_list_stats{st.primaries, st.decays, st.undecayed, st.dropped_daughters, st.capped,
                                      st.final_particles, st.passes, st.batches, st.ms_total};
  e->smp.list.replace_decayed(d, bin != 0);
  return IS3D_OK;
}

extern "C" int is3d_decay_particles(is3d_engine* e, long seed, int n_events, const long* offsets, const is3d_particle* in, int bin) {
  if (e && e->grp) return is3d::group_decay_particles(e->grp, seed, n_events, offsets, in, bin);
  if (!e) return IS3D_ERR_ARG;
  const int rc = decay_list_any(e, seed, n_events, offsets, in, bin, "is3d_decay_particles");
  if (!rc) e->smp.list.famod = false;     // a caller's list
  return rc;
}

extern "C" int is3d_decay_sampled(is3d_engine* e, long seed, int bin) {
  if (e && e->grp) return is3d::group_decay_sampled(e->grp, seed, bin);
  if (!e) return IS3D_ERR_ARG;
  if (!e->have_decays()) return e->fail(IS3D_ERR_STATE, "is3d_decay_sampled: no decay channels set (is3d_set_decays)");
  if (!e->smp.list.has_list())
    return e->fail(IS3D_ERR_STATE, "is3d_decay_sampled: no sampled list (is3d_sample, or a binned call that keeps the list)");
  return decay_list_any(e, seed, (int)e->smp.list.offsets.size() - 1, e->smp.list.offsets.data(),
                        reinterpret_cast<const is3d_particle*>(e->smp.list.particles.data()), bin, "is3d_decay_sampled");
}

extern "C" int is3d_get_particle_origins(const is3d_engine* e, long first, long count, long* origin) {
  return e ? list_of(e).get_origins(first, count, origin) : IS3D_ERR_ARG;
}

extern "C" int is3d_get_decay_list_stats(const is3d_engine* e, is3d_decay_list_stats* out) {
  return e ? list_of(e).get_decay_stats(out) : IS3D_ERR_ARG;
}
