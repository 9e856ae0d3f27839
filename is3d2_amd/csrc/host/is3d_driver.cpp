// is3d_driver.cpp -- IS3D / EmissionFunctionArray facades over the engine's C ABI.
#include "is3d_driver.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "../../../include/is3d_amd.h"
#include "../../../include/is3d_host.h"

namespace is3d {
namespace host {

static void check(bool ok, const std::string& msg) {
  if (!ok) throw std::runtime_error(msg);
}

EmissionFunctionArray::EmissionFunctionArray(const ParameterReader& params, const Table& chosen, const Table& pT,
                                             const Table& phi, const Table& y, const Table& eta,
                                             const std::vector<Particle>& particles, const Surface& surf,
                                             const DfTablesData& df, const Averages& plasma,
                                             const std::vector<double>& gla_roots, const std::vector<double>& gla_weights,
                                             int gla_alpha, int gla_points)
    : p_(params), pT_(pT), phi_(phi), y_(y), eta_(eta), surf_(surf), df_(df), plasma_(plasma), gr_(gla_roots),
      gw_(gla_weights), galpha_(gla_alpha), gpts_(gla_points) {
  dimension_ = (int)p_.get("dimension");
  check(dimension_ == 2 || dimension_ == 3, "EmissionFunctionArray error: need to set dimension = (2,3)");
  const int df_mode = (int)p_.get("df_mode");
  check(df_mode >= 1 && df_mode <= 5, "EmissionFunctionArray error: need to set df_mode = (1,2,3,4,5)");
  // chosen particles -> PDG indices, first match (EmissionFunction.cpp:356-372)
  std::vector<int> idx;
  for (long m = 0; m < chosen.rows(); m++) {
    const long mc = (long)chosen.get(1, m + 1);
    int hit = -1;
    for (size_t n = 0; n < particles.size(); n++)
      if (particles[n].mcid == mc) { hit = (int)n; break; }
    check(hit >= 0, "chosen particle " + std::to_string(mc) + " is not in the PDG list");
    idx.push_back(hit);
  }
  if ((int)p_.get("group_particles", 0.0) == 1) {   // bubble sort by mass (:375-390)
    const int nc = (int)idx.size();
    for (int m = 0; m < nc; m++)
      for (int n = 0; n < nc - m - 1; n++)
        if (particles[idx[n]].mass > particles[idx[n + 1]].mass) std::swap(idx[n], idx[n + 1]);
  }
  for (int i : idx) {
    mass_.push_back(particles[i].mass); sign_.push_back(particles[i].sign); degen_.push_back(particles[i].gspin);
    baryon_.push_back(particles[i].baryon); mcid_.push_back(particles[i].mcid);
  }
  for (const auto& q : particles) {
    pdg_mass_.push_back(q.mass); pdg_sign_.push_back(q.sign); pdg_degen_.push_back(q.gspin); pdg_baryon_.push_back(q.baryon);
  }
  // the decay rows of the chosen species as the engine's channel table: indices into the chosen list (first match,
  // -1 for a daughter that is not chosen), masses and widths from the PDG list; |n_body| (the UrQMD table flags some
  // rows with a negative count); lightest_particle is read and not used, as in the reference.  Operations 1
  // (the feed-down of the spectra) and 2 (the Monte Carlo decays of the sampled list) use the table: under operation 0
  // the key changes nothing, so a row it could not resolve must not fail the run.  four_body_decays = 1 (ours; absent
  // or 0: as before) builds the rows with four daughter slots for is3d_set_decays4, which keeps the open 4-body channels
  const int op_key = (int)p_.get("operation", 1.0);
  const bool four_body = (int)p_.get("four_body_decays", 0.0) == 1;
  if ((int)p_.get("do_resonance_decays", 0.0) == 1 && (op_key == 1 || op_key == 2)) {
    auto find = [&](long mc) {
      for (size_t n = 0; n < particles.size(); n++) if (particles[n].mcid == mc) return (int)n;
      return -1;
    };
    auto chosen_index = [&](long mc) {
      for (size_t k = 0; k < mcid_.size(); k++) if (mcid_[k] == mc) return (int)k;
      return -1;
    };
    for (size_t k = 0; k < idx.size(); k++) {
      const Particle& par = particles[idx[k]];
      if (chosen_index(par.mcid) != (int)k) continue;       // a repeated chosen entry: the first carries the channels
      for (const DecayRow& r : par.decays) {
        is3d_decay_channel c{};
        c.parent = (int)k; c.n_body = std::abs(r.n_body); c.branching = r.branching;
        c.mass_parent = par.mass; c.width_parent = par.width;
        for (int d = 0; d < 3; d++) c.daughter[d] = -1;
        for (int d = 0; d < std::min(c.n_body, 3); d++) {
          const int at = find(r.daughter[d]);
          check(at >= 0, "decay row of " + std::to_string(par.mcid) + ": daughter " + std::to_string(r.daughter[d]) + " is not in the PDG list");
          c.daughter[d] = chosen_index(r.daughter[d]);
          c.mass[d] = particles[at].mass; c.width[d] = particles[at].width;
        }
        decays_.push_back(c);
        if (four_body) {
          is3d_decay_channel4 w{};
          w.parent = c.parent; w.n_body = c.n_body; w.branching = c.branching;
          w.mass_parent = c.mass_parent; w.width_parent = c.width_parent;
          for (int d = 0; d < 4; d++) w.daughter[d] = -1;
          for (int d = 0; d < 3; d++) { w.daughter[d] = c.daughter[d]; w.mass[d] = c.mass[d]; w.width[d] = c.width[d]; }
          if (c.n_body >= 4) {
            const int at = find(r.daughter[3]);
            check(at >= 0, "decay row of " + std::to_string(par.mcid) + ": daughter " + std::to_string(r.daughter[3]) + " is not in the PDG list");
            w.daughter[3] = chosen_index(r.daughter[3]);
            w.mass[3] = particles[at].mass; w.width[3] = particles[at].width;
          }
          decays4_.push_back(w);
        }
      }
    }
  }
}

// the channel table of the run: four slots (is3d_set_decays4) under four_body_decays = 1, else three
int EmissionFunctionArray::set_run_decays(is3d_engine* e) const {
  if ((int)p_.get("four_body_decays", 0.0) == 1) return is3d_set_decays4(e, (int)decays4_.size(), decays4_.data());
  return is3d_set_decays(e, (int)decays_.size(), decays_.data());
}

static void set_or_throw(is3d_engine* e, int rc) {
  if (rc != IS3D_OK) throw EngineError(rc, std::string("is3d engine: ") + is3d_last_error(e));
}

static is3d_params engine_params(const ParameterReader& p, int operation, int dimension) {
  is3d_params prm{};
  prm.operation = operation;
  prm.dimension = dimension;
  prm.df_mode = (int)p.get("df_mode");
  prm.include_baryon = (int)p.get("include_baryon");
  prm.include_bulk_deltaf = (int)p.get("include_bulk_deltaf");
  prm.include_shear_deltaf = (int)p.get("include_shear_deltaf");
  prm.include_baryondiff_deltaf = (int)p.get("include_baryondiff_deltaf");
  prm.regulate_deltaf = (int)p.get("regulate_deltaf");
  prm.outflow = (int)p.get("outflow");
  prm.deta_min = p.get("deta_min");
  prm.mass_pion0 = p.get("mass_pion0");
  // PTMA warm-start chains: the reference as shipped is serial (CORES = 1, EmissionFunction.cpp:131-135), one
  // chain over every cell (MomentumSpectra.cpp:1308-1364); iS3D_parameters.dat has no such key, so the drop-in
  // default is 1.  famod_chains = C reproduces an OpenMP build with C threads, 0 solves every cell cold.
  prm.famod_chains = (int)p.get("famod_chains", 1.0);
  return prm;
}

// operation = 0 binning from the parameter file (EmissionFunction.cpp:232-247); spacetime_threads (ours,
// default 0) = the reference run's OpenMP thread count to reproduce its memset carry (is3d_amd.h)
static is3d_spacetime_bins spacetime_bins(const ParameterReader& p) {
  is3d_spacetime_bins b{};
  b.tau_min = p.get("tau_min", 0.0); b.tau_max = p.get("tau_max", 12.0); b.tau_bins = (int)p.get("tau_bins", 120.0);
  b.r_min = p.get("r_min", 0.0); b.r_max = p.get("r_max", 12.0); b.r_bins = (int)p.get("r_bins", 60.0);
  b.phip_bins = (int)p.get("phip_bins", 100.0);
  b.threads = (int)p.get("spacetime_threads", 0.0);
  return b;
}

// test_sampler = 1 binning from the parameter file (EmissionFunction.cpp:223-247; the reference's defaults)
static is3d_sample_bins read_sample_bins(const ParameterReader& p) {
  is3d_sample_bins b{};
  b.pT_min = p.get("pT_min", 0.0); b.pT_max = p.get("pT_max", 3.0); b.pT_bins = (int)p.get("pT_bins", 100.0);
  b.y_cut = p.get("y_cut", 5.0); b.y_bins = (int)p.get("y_bins", 100.0);
  b.phip_bins = (int)p.get("phip_bins", 100.0);
  b.eta_cut = p.get("eta_cut", 7.0); b.eta_bins = (int)p.get("eta_bins", 140.0);
  b.tau_min = p.get("tau_min", 0.0); b.tau_max = p.get("tau_max", 12.0); b.tau_bins = (int)p.get("tau_bins", 120.0);
  b.r_min = p.get("r_min", 0.0); b.r_max = p.get("r_max", 12.0); b.r_bins = (int)p.get("r_bins", 60.0);
  return b;
}

// One engine over every requested device (is3d_create_devices): the library splits the cells into
// cost-balanced windows, runs the devices concurrently and sums their spectra on the devices (RCCL
// all-reduce over distinct GPUs), replacing the reference's OpenMP fan-out and thread reduction
// (MomentumSpectra.cpp:98-107, 383-411).
void EmissionFunctionArray::run_sharded(const RunOptions& opt, int operation) {
  // operation < 0: the polarization alone, on an engine of its own, so that the caller can write the operation's
  // files before it runs (a polarization error then costs none of them)
  const bool polzn_only = operation < 0;
  if (polzn_only && !((int)p_.get("mode") == 5 && surf_.has_vorticity()))
    throw EngineError(IS3D_ERR_STATE, "polarization needs a mode = 5 surface (thermal vorticity columns)");
  const is3d_params prm = engine_params(p_, polzn_only ? 1 : std::min(operation, 2), dimension_);
  const is3d_spacetime_bins bins = spacetime_bins(p_);
  const int ndev = opt.devices.empty() ? std::max(1, opt.num_devices) : (int)opt.devices.size();
  std::vector<int> devs(ndev);
  for (int k = 0; k < ndev; k++) devs[k] = opt.devices.empty() ? opt.device + k : opt.devices[k];
  std::vector<double> pTv(pT_.cols[0]), phiv(phi_.cols[0]), yv(y_.cols[0]), etav(eta_.cols[0]), etaw(eta_.cols[1]);
  std::vector<double> pTw(pT_.ncols() > 1 ? pT_.cols[1] : std::vector<double>(pTv.size(), 0.0));
  std::vector<double> phiw(phi_.ncols() > 1 ? phi_.cols[1] : std::vector<double>(phiv.size(), 0.0));
  const long n = surf_.size();
  const int np = (int)mass_.size();
  auto t0 = std::chrono::steady_clock::now();
  is3d_engine* e = ndev == 1 ? is3d_create(devs[0]) : is3d_create_devices(ndev, devs.data());
  if (!e) throw EngineError(IS3D_ERR_DEVICE, "is3d_create on device " + std::to_string(devs[0]) + " failed");
  try {
    set_or_throw(e, is3d_set_params(e, &prm));
    set_or_throw(e, is3d_set_species(e, np, mass_.data(), sign_.data(), degen_.data(), baryon_.data()));
    set_or_throw(e, is3d_set_momentum_grid(e, (int)pTv.size(), pTv.data(), (int)phiv.size(), phiv.data(), (int)yv.size(),
                                           yv.data(), (int)etav.size(), etav.data(), etaw.data()));
    if (!polzn_only) {
      set_or_throw(e, is3d_set_pdg(e, (int)pdg_mass_.size(), pdg_mass_.data(), pdg_sign_.data(), pdg_degen_.data(), pdg_baryon_.data()));
      set_or_throw(e, is3d_set_gauss_laguerre(e, galpha_, gpts_, gr_.data(), gw_.data()));
      set_or_throw(e, is3d_set_df_tables(e, df_.nT, df_.nmuB, df_.T.data(), df_.muB.data(), df_.tab.data(), plasma_.T));
    }
    auto fp = [&](const std::vector<double>& v) { return v.empty() ? nullptr : v.data(); };
    is3d_surface s{fp(surf_.tau), fp(surf_.x), fp(surf_.y), fp(surf_.eta), fp(surf_.dat), fp(surf_.dax), fp(surf_.day),
                   fp(surf_.dan), fp(surf_.ux), fp(surf_.uy), fp(surf_.un), fp(surf_.E), fp(surf_.T), fp(surf_.P),
                   fp(surf_.pixx), fp(surf_.pixy), fp(surf_.pixn), fp(surf_.piyy), fp(surf_.piyn), fp(surf_.bulkPi),
                   fp(surf_.muB), fp(surf_.nB), fp(surf_.Vx), fp(surf_.Vy), fp(surf_.Vn)};
    set_or_throw(e, is3d_set_surface(e, n, &s));
    if (operation == 1) {
      dN_.assign(is3d_output_size(e), 0.0);
      set_or_throw(e, is3d_calculate_spectra(e, dN_.data()));
      if ((int)p_.get("do_resonance_decays", 0.0) == 1) {     // between the spectra and the writers
        set_or_throw(e, set_run_decays(e));
        set_or_throw(e, is3d_decay_feeddown(e, dN_.data()));
        set_or_throw(e, is3d_get_decay_stats(e, &decay_stats_));
        if (!opt.quiet) {
          const is3d_decay_stats& d = decay_stats_;
          std::printf("\nResonance decays: %ld channels, %ld kept (%ld opened by the mass adjustment), %ld with %d or more "
                      "bodies and %ld closed skipped (summed branching %g), %ld levels, %g ms\n",
                      d.channels, d.kept, d.adjusted, d.skipped_many_body, (int)p_.get("four_body_decays", 0.0) == 1 ? 5 : 4, d.skipped_closed, d.branching_skipped, d.levels,
                      d.ms_total);
        }
      }
    } else if (operation == 2) {
      const double plasma[5] = {plasma_.T, plasma_.E, plasma_.P, plasma_.muB, plasma_.nB};
      set_or_throw(e, is3d_total_yield(e, plasma, p_.get("y_cut", 0.5), &ntotal_, nullptr));
    } else if (operation == 3 || operation == 4) {
      const double plasma[5] = {plasma_.T, plasma_.E, plasma_.P, plasma_.muB, plasma_.nB};
      is3d_sample_params sp{};
      sp.seed = sample_seed_; sp.n_events = (int)sample_events_; sp.fast = (int)p_.get("fast", 0.0);
      sp.y_cut = p_.get("y_cut", 0.5);
      // df_mode 5 has a method of its own (EmissionFunction.cpp:1255-1275): sample_dN_pTdpTdphidy_famod
      const bool famod = prm.df_mode == 5;
      // do_resonance_decays = 1: the sampled hadrons are decayed down their chains on the device, batch by batch
      // (is3d_sample_decayed, the sampler's seed), so the lists, the offsets and the binned files carry the final hadrons
      const bool decays = (int)p_.get("do_resonance_decays", 0.0) == 1;
      if (decays) set_or_throw(e, set_run_decays(e));
      if (operation == 4) {      // test_sampler = 1: binned only, no list (EmissionFunction.cpp:1279-1291)
        sbins_ = read_sample_bins(p_);
        set_or_throw(e, is3d_set_sample_bins(e, &sbins_));
        if (decays) {            // the final hadrons are binned where they are made: no list reaches the host
          set_or_throw(e, is3d_sample_decayed(e, &sp, plasma, sample_seed_, 0, 1));
        } else {
          set_or_throw(e, famod ? is3d_sample_famod(e, &sp, 1) : is3d_sample_binned(e, &sp, plasma, 0));
        }
        long nc = 0, nv = 0;
        if (is3d_sample_hist_size(e, &nc, &nv) < 0) throw EngineError(IS3D_ERR_STATE, "is3d_sample_hist_size failed");
        hist_counts_.assign((size_t)nc, 0);
        hist_vn_.assign((size_t)nv, 0.0);
        set_or_throw(e, is3d_get_sample_hist(e, hist_counts_.data(), hist_vn_.data()));
      } else {
        if (decays) set_or_throw(e, is3d_sample_decayed(e, &sp, plasma, sample_seed_, 1, 0));
        else set_or_throw(e, famod ? is3d_sample_famod(e, &sp, 0) : is3d_sample(e, &sp, plasma));
      }
      famod_sampled_ = famod;
      if (famod) set_or_throw(e, is3d_get_sample_famod_stats(e, &famod_stats_));
      records_.assign((size_t)is3d_sample_count(e), is3d_particle{});
      sample_offsets_.assign((size_t)sample_events_ + 1, 0);
      set_or_throw(e, is3d_sample_offsets(e, sample_offsets_.data()));
      set_or_throw(e, is3d_get_particles(e, 0, (long)records_.size(), records_.data()));
      set_or_throw(e, is3d_get_sample_stats(e, &sample_stats_));     // the sampler's, decays or not
      origins_.clear();
      decay_list_stats_ = is3d_decay_list_stats{};
      if (decays) {
        origins_.assign(records_.size(), 0);
        set_or_throw(e, is3d_get_particle_origins(e, 0, (long)origins_.size(), origins_.data()));
        set_or_throw(e, is3d_get_decay_list_stats(e, &decay_list_stats_));
      }
    } else if (operation == 0) {
      set_or_throw(e, is3d_set_momentum_weights(e, pTw.data(), phiw.data()));
      set_or_throw(e, is3d_set_spacetime_bins(e, &bins));
      bins_ = bins;
      dNtau_.assign((size_t)np * bins.tau_bins, 0.0);
      dNr_.assign((size_t)np * bins.r_bins, 0.0);
      dNphi_.assign((size_t)np * bins.phip_bins, 0.0);
      // df_mode 5: the reference has no routine; the engine's is the per-cell decomposition of the PTMA spectra
      set_or_throw(e, prm.df_mode == 5 ? is3d_calculate_dN_dX_famod(e, dNtau_.data(), dNr_.data(), dNphi_.data())
                                       : is3d_calculate_dN_dX(e, dNtau_.data(), dNr_.data(), dNphi_.data()));
    }
    if (polzn_only) {   // EmissionFunction.cpp:1305-1310: T = QGP->temperature
      const is3d_vorticity w{surf_.w[0].data(), surf_.w[1].data(), surf_.w[2].data(), surf_.w[3].data(),
                             surf_.w[4].data(), surf_.w[5].data()};
      set_or_throw(e, is3d_set_vorticity(e, n, &w));
      S_.assign(is3d_polarization_size(e), 0.0);
      set_or_throw(e, is3d_calculate_polarization(e, plasma_.T, S_.data()));
    }
  } catch (...) {
    is3d_destroy(e);
    throw;
  }
  is3d_destroy(e);
  seconds_ = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

void EmissionFunctionArray::calculate_spectra(const RunOptions& opt) { run_sharded(opt, 1); }

void EmissionFunctionArray::calculate_dN_dX(const RunOptions& opt) { run_sharded(opt, 0); }

double EmissionFunctionArray::estimate_total_yield(const RunOptions& opt) {
  run_sharded(opt, 2);
  return ntotal_;
}

void EmissionFunctionArray::calculate_polarization(const RunOptions& opt) { run_sharded(opt, -1); }

void EmissionFunctionArray::sample_particles(const RunOptions& opt, long seed, long n_events) {
  sample_seed_ = seed;
  sample_events_ = n_events;
  run_sharded(opt, 3);
  sampled_.resize(records_.size());
  for (size_t i = 0; i < records_.size(); i++) {
    const is3d_particle& r = records_[i];
    sampled_[i] = SampledParticle{mcid_[(size_t)r.species], mass_[(size_t)r.species], r.tau, r.x, r.y, r.eta, r.t, r.z,
                                  r.E, r.px, r.py, r.pz};
  }
}

void EmissionFunctionArray::sample_binned(const RunOptions& opt, long seed, long n_events) {
  sample_seed_ = seed;
  sample_events_ = n_events;
  run_sharded(opt, 4);
  sampled_.clear();
}

void EmissionFunctionArray::write_sampled_files(const std::string& dir) const {
  const is3d_sample_bins& b = sbins_;
  SampledHistView v{hist_counts_.data(), hist_vn_.data(), (int)mass_.size(), sample_events_, b.pT_min, b.pT_max, b.pT_bins,
                    b.y_cut, b.y_bins, b.phip_bins, b.eta_cut, b.eta_bins, b.tau_min, b.tau_max, b.tau_bins, b.r_min, b.r_max,
                    b.r_bins, &mcid_};
  const std::string err = host::write_sampled_files(dir, v);
  if (!err.empty()) throw std::runtime_error(err);
}

void EmissionFunctionArray::write_polzn_files(const std::string& dir) const {
  const int ny = (dimension_ == 3) ? (int)y_.rows() : 1;
  PolznView v{S_.data(), (int)mass_.size(), (int)pT_.rows(), (int)phi_.rows(), ny, dimension_, &pT_, &phi_, &y_};
  const std::string err = host::write_polzn_files(dir, v);
  if (!err.empty()) throw std::runtime_error(err);
}

void EmissionFunctionArray::write_spacetime_files(const std::string& dir) const {
  SpacetimeView v{dNtau_.data(), dNr_.data(), dNphi_.data(), (int)mass_.size(), bins_.tau_min, bins_.tau_max,
                  bins_.tau_bins, bins_.r_min, bins_.r_max, bins_.r_bins, bins_.phip_bins, &mcid_};
  const std::string err = host::write_spacetime_files(dir, v);
  if (!err.empty()) throw std::runtime_error(err);
}

void EmissionFunctionArray::write_files(const std::string& dir) const {
  const int ny = (dimension_ == 3) ? (int)y_.rows() : 1;
  SpectraView v{dN_.data(), (int)mass_.size(), (int)pT_.rows(), (int)phi_.rows(), ny, dimension_, &pT_, &phi_, &y_, &mcid_};
  const std::string err = write_spectra_files(dir, v);
  if (!err.empty()) throw std::runtime_error(err);
}

void IS3D::read_fo_surf_from_memory(std::vector<double> tau, std::vector<double> x, std::vector<double> y,
                                   std::vector<double> eta, std::vector<double> dsigma_tau,
                                   std::vector<double> dsigma_x, std::vector<double> dsigma_y,
                                   std::vector<double> dsigma_eta, std::vector<double> E, std::vector<double> T,
                                   std::vector<double> P, std::vector<double> ux, std::vector<double> uy,
                                   std::vector<double> un, std::vector<double> pixx, std::vector<double> pixy,
                                   std::vector<double> pixn, std::vector<double> piyy, std::vector<double> piyn,
                                   std::vector<double> pinn, std::vector<double> Pi) {
  (void)pinn;   // reconstructed from orthogonality/tracelessness, as in the reference
  const long n = (long)tau.size();
  mem_.resize(n);
  mem_.tau = tau; mem_.x = x; mem_.y = y; mem_.eta = eta; mem_.dat = dsigma_tau; mem_.dax = dsigma_x;
  mem_.day = dsigma_y; mem_.dan = dsigma_eta; mem_.E = E; mem_.T = T; mem_.P = P; mem_.ux = ux; mem_.uy = uy;
  mem_.un = un; mem_.pixx = pixx; mem_.pixy = pixy; mem_.pixn = pixn; mem_.piyy = piyy; mem_.piyn = piyn;
  mem_.bulkPi = Pi;
}

static std::string path_in(const std::string& dir, const std::string& rel) {
  return (dir.empty() || dir == ".") ? rel : dir + "/" + rel;
}

// generate_df_coefficients = 1 | 2: the delta-f tables of the run's PDG list from the engine (is3d_generate_df_tables)
// on the shipped grid (T 0.1 .. 0.2 GeV, 101 points; muB 0 .. 0.8 GeV, 81 points) or the df_T_* / df_muB_* keys', with
// the 64-point Gauss-Laguerre table tables/gla_roots_weights_64_points.txt (the generator's own), or, where the run
// directory has none, the run's tables/gauss/gla_roots_weights.txt
static void generate_df_tables(const std::string& dir, const ParameterReader& prm, const std::vector<Particle>& parts,
                               const RunOptions& opt, DfTablesData& df) {
  df.nT = (int)prm.get("df_T_points", 101.0);
  df.nmuB = (int)prm.get("df_muB_points", 81.0);
  check(df.nT >= 1 && df.nmuB >= 1, "generate_df_coefficients: df_T_points and df_muB_points must be at least 1");
  const double T0 = prm.get("df_T_min", 0.1), T1 = prm.get("df_T_max", 0.2);
  const double B0 = prm.get("df_muB_min", 0.0), B1 = prm.get("df_muB_max", 0.8);
  // deltaf_table.cpp:58-71
  const double dT = df.nT > 1 ? (T1 - T0) / (double)(df.nT - 1) : 0.0, dB = df.nmuB > 1 ? (B1 - B0) / (double)(df.nmuB - 1) : 0.0;
  df.T.assign(df.nT, T0);
  df.muB.assign(df.nmuB, B0);
  for (int i = 1; i < df.nT; i++) df.T[i] = T0 + (double)i * dT;
  for (int i = 1; i < df.nmuB; i++) df.muB[i] = B0 + (double)i * dB;
  df.tab.assign((size_t)10 * df.nmuB * df.nT, 0.0);
  int galpha = 0, gpts = 0;
  std::vector<double> gr, gw;
  std::string err = read_gauss_laguerre(path_in(dir, "tables/gla_roots_weights_64_points.txt"), galpha, gpts, gr, gw);
  if (!err.empty()) err = read_gauss_laguerre(path_in(dir, "tables/gauss/gla_roots_weights.txt"), galpha, gpts, gr, gw);
  check(err.empty(), err);
  std::vector<double> mass, sign, degen, baryon;
  for (const auto& q : parts) { mass.push_back(q.mass); sign.push_back(q.sign); degen.push_back(q.gspin); baryon.push_back(q.baryon); }
  const int dev = opt.devices.empty() ? opt.device : opt.devices[0];
  is3d_engine* e = is3d_create(dev);
  if (!e) throw EngineError(IS3D_ERR_DEVICE, "is3d_create on device " + std::to_string(dev) + " failed");
  int rc = is3d_set_pdg(e, (int)mass.size(), mass.data(), sign.data(), degen.data(), baryon.data());
  if (!rc) rc = is3d_set_gauss_laguerre(e, galpha, gpts, gr.data(), gw.data());
  if (!rc) rc = is3d_generate_df_tables(e, df.nT, df.nmuB, df.T.data(), df.muB.data(), df.tab.data());
  const std::string msg = rc ? std::string("is3d engine: ") + is3d_last_error(e) : "";
  is3d_destroy(e);
  if (rc) throw EngineError(rc, msg);
}

void IS3D::run_particlization(int fo_from_file, const RunOptions& opt) {
  ParameterReader prm;
  check(prm.read_file(path_in(dir_, "iS3D_parameters.dat")), "ParameterReader::readFromFile error: file iS3D_parameters.dat does not exist.");
  const int operation = (int)prm.get("operation");
  check(operation == 0 || operation == 1 || operation == 2, "calculate_spectra error: need to set operation = (0, 1, 2)");
  const int mode = (int)prm.get("mode"), dimension = (int)prm.get("dimension"), hrg = (int)prm.get("hrg_eos");
  const int include_baryon = (int)prm.get("include_baryon");
  Surface file_surf;
  Averages avg{};
  const Surface* surf = &mem_;
  if (fo_from_file == 1) {
    const std::string err = read_surface(dir_, mode, dimension, include_baryon, file_surf, avg, true);
    check(err.empty(), err);
    surf = &file_surf;
  } else {
    avg = surface_averages(mem_, 0);            // JETSCAPE path: muB, nB not considered (iS3D.cpp:174-176)
    const std::string err = write_averages_file(dir_, avg);
    check(err.empty(), err);
  }
  if (!opt.quiet) std::printf("Number of freezeout cells = %ld\n", surf->size());
  std::vector<Particle> parts;
  std::string err = read_pdg(dir_, hrg, parts);
  check(err.empty(), err);
  Table chosen, pT, phi, y, eta;
  check(load_table(path_in(dir_, "PDG/chosen_particles.dat"), chosen), "cannot read PDG/chosen_particles.dat");
  DfTablesData df;          // the polarization alone uses neither the df tables nor the Gauss-Laguerre roots
  if (!opt.polarization_only) {
    const int gen = (int)prm.get("generate_df_coefficients", 0.0);
    if (gen == 1 || gen == 2) {           // deltaf_coefficients/ is not read
      generate_df_tables(dir_, prm, parts, opt, df);
      if (gen == 2 && opt.write_files) err = write_df_tables(dir_, df);
    } else {
      err = read_df_tables(dir_, hrg, df);
    }
    check(err.empty(), err);
  }
  check(load_table(path_in(dir_, "tables/momentum/pT_table.dat"), pT), "cannot read tables/momentum/pT_table.dat");
  check(load_table(path_in(dir_, "tables/momentum/phi_table.dat"), phi), "cannot read tables/momentum/phi_table.dat");
  check(load_table(path_in(dir_, "tables/momentum/y_table.dat"), y), "cannot read tables/momentum/y_table.dat");
  check(load_table(path_in(dir_, "tables/spacetime_rapidity/eta_table.dat"), eta),
        "cannot read tables/spacetime_rapidity/eta_table.dat");
  int galpha = 0, gpts = 0;
  std::vector<double> gr, gw;
  if (!opt.polarization_only) {
    err = read_gauss_laguerre(path_in(dir_, "tables/gauss/gla_roots_weights.txt"), galpha, gpts, gr, gw);
    check(err.empty(), err);
  }
  EmissionFunctionArray efa(prm, chosen, pT, phi, y, eta, parts, *surf, df, avg, gr, gw, galpha, gpts);
  S_.clear();
  if (opt.polarization_only) {
    efa.calculate_polarization(opt);
    if (opt.write_files) efa.write_polzn_files(dir_);
    S_ = efa.polarization();
    dN_.clear();
    return;
  }
  if (operation == 2) {        // EmissionFunction.cpp:1235-1249: the oversampling estimate
    nevents_ = 1;
    if ((int)prm.get("oversample", 0.0)) {
      ntotal_ = efa.estimate_total_yield(opt);
      if (!opt.quiet) std::printf("\nEstimated total particle yield = %ld particles\n", (long)ntotal_);
      nevents_ = (long)std::min(std::ceil(prm.get("min_num_hadrons", 1.0e5) / ntotal_), prm.get("max_num_samples", 1.0e3));
      if (!opt.quiet) std::printf("\nSampling %ld particlization events...\n\n", nevents_);
    } else if (!opt.quiet) {
      std::printf("\nSampling 1 particlization event...\n\n");
    }
    dN_.clear();
    final_particles_.clear(); particle_offsets_.clear(); particle_records_.clear(); particle_origins_.clear();
    decay_list_stats_ = is3d_decay_list_stats{};
    hist_counts_.clear(); hist_vn_.clear();
    if (opt.sample) {            // EmissionFunction.cpp:1251-1301: sample, then write the lists
      // sampler_seed < 0: the clock, as the reference (ParticleSampler.cpp:646-648); the engine sees a seed >= 0
      seed_ = (long)prm.get("sampler_seed", -1.0);
      if (seed_ < 0) seed_ = (long)(std::chrono::system_clock::now().time_since_epoch().count() & 0x7fffffffffffffffLL);
      // test_sampler = 1 (EmissionFunction.cpp:1279-1291): the particles are binned, never listed
      const bool binned = (int)prm.get("test_sampler", 0.0) != 0;
      if (binned) efa.sample_binned(opt, seed_, nevents_);
      else efa.sample_particles(opt, seed_, nevents_);
      final_particles_ = efa.sampled();
      particle_offsets_ = efa.sample_offsets();
      particle_records_ = efa.sampled_records();
      particle_origins_ = efa.sample_origins();
      decay_list_stats_ = efa.decay_list_stats();
      sample_stats_ = efa.sample_stats();
      if (!opt.quiet) {
        const is3d_sample_stats& st = sample_stats_;
        std::printf("\nMomentum sampling efficiency = %f %%\n", st.proposals ? 100.0 * (double)st.acceptances / (double)st.proposals : 0.0);
        if (efa.famod_sampled()) {       // the closing lines of sample_dN_pTdpTdphidy_famod (ParticleSampler.cpp:1625-1626)
          std::printf("pl went negative for %ld / %ld cells\n\n", efa.famod_stats().plpt_negative, (long)surf->size());
          std::printf("Number of reconstruction failures = %ld\n", efa.famod_stats().reconstruction_fail);
        }
        std::printf("Sampled %ld particles in %ld events (%ld candidates, %ld dropped at an iteration cap)\n", st.kept, nevents_,
                    st.candidates, st.capped);
        if ((int)prm.get("do_resonance_decays", 0.0) == 1) {
          const is3d_decay_list_stats& d = decay_list_stats_;
          std::printf("Resonance decays: %ld decays of %ld primaries in %ld passes -> %ld final hadrons (%ld undecayed, %ld daughters "
                      "dropped, %ld capped), %.3f ms\n", d.decays, d.primaries, d.passes, d.final_particles, d.undecayed,
                      d.dropped_daughters, d.capped, d.ms_total);
        }
      }
      if (binned) {
        hist_counts_ = efa.hist_counts();
        hist_vn_ = efa.hist_vn();
        sample_bins_ = efa.sample_bins();
        if (opt.write_files) {
          if (!opt.quiet) {
            std::printf("Writing event-averaged dN/dy of each species to file...\n");
            std::printf("Writing event-averaged dN/deta of each species to file...\n");
            std::printf("Writing event-averaged dN/2pipTdpTdy of each species to file...\n");
            std::printf("Writing event-averaged dN/dphipdy of each species to file...\n");
            std::printf("Writing event-averaged vn(pT) of each species to file...\n");
            std::printf("Writing event-averaged boost invariant spacetime distributions dN_dX of each species to file...\n");
          }
          efa.write_sampled_files(dir_);
        }
      } else if (opt.write_files) {
        if (!opt.quiet) std::printf("Writing sampled particles list to OSCAR File...\n");
        std::string werr = write_particle_list_osc(dir_, final_particles_, particle_offsets_);
        if (werr.empty() && opt.particle_list_csv) werr = write_particle_list_csv(dir_, final_particles_, particle_offsets_);
        check(werr.empty(), werr);
      }
    }
  } else if (operation == 1) {
    efa.calculate_spectra(opt);
    if (opt.write_files) efa.write_files(dir_);
    if (!opt.quiet) std::printf("\nSpectra calculation took %g seconds\n\n", efa.seconds());
    dN_ = efa.spectra();
  } else {
    efa.calculate_dN_dX(opt);
    if (opt.write_files) efa.write_spacetime_files(dir_);
    if (!opt.quiet) std::printf("\nSpacetime distributions took %g seconds\n\n", efa.seconds());
    const int np = (int)efa.mcid().size();
    const is3d_spacetime_bins b = efa.bins();
    dN_.clear();
    for (int k = 0; k < np; k++) {   // per species [tau bins | r bins | phip bins]
      dN_.insert(dN_.end(), efa.dN_taudtaudy().begin() + (long)k * b.tau_bins, efa.dN_taudtaudy().begin() + (long)(k + 1) * b.tau_bins);
      dN_.insert(dN_.end(), efa.dN_2pirdrdy().begin() + (long)k * b.r_bins, efa.dN_2pirdrdy().begin() + (long)(k + 1) * b.r_bins);
      dN_.insert(dN_.end(), efa.dN_dphidy().begin() + (long)k * b.phip_bins, efa.dN_dphidy().begin() + (long)(k + 1) * b.phip_bins);
    }
  }
  // mode = 5 (EmissionFunction.cpp:1305-1310): after the chosen operation, whichever it is, and after its files
  if (mode == 5 && surf->has_vorticity()) {
    if (!opt.quiet) std::printf("\nComputing spin polarization...\n");
    efa.calculate_polarization(opt);
    if (opt.write_files) efa.write_polzn_files(dir_);
    S_ = efa.polarization();
  }
}

}  // namespace host
}  // namespace is3d

// ------------------------------------------------------------------------------------------------
// C ABI of the host layer (include/is3d_host.h)
// ------------------------------------------------------------------------------------------------
using namespace is3d::host;

static void put_err(char* buf, int len, const std::string& msg) {
  if (buf && len > 0) { std::strncpy(buf, msg.c_str(), (size_t)len - 1); buf[len - 1] = 0; }
}

static int run_particlization_opt(const char* workdir, RunOptions opt, double* dN_out, long out_capacity, char* err,
                                  int errlen) {
  try {
    IS3D run(workdir ? workdir : ".");
    opt.quiet = true;
    run.run_particlization(1, opt);
    const auto& dN = run.spectra();
    if (dN_out) {
      if ((long)dN.size() > out_capacity) { put_err(err, errlen, "output buffer too small"); return IS3D_ERR_ARG; }
      std::copy(dN.begin(), dN.end(), dN_out);
    }
    return IS3D_OK;
  } catch (const EngineError& ex) {
    put_err(err, errlen, ex.what());
    return ex.code;
  } catch (const std::exception& ex) {
    put_err(err, errlen, ex.what());
    return IS3D_ERR_ARG;
  }
}

extern "C" int is3d_host_run_particlization(const char* workdir, int device, int num_devices, double* dN_out,
                                            long out_capacity, char* err, int errlen) {
  RunOptions opt;
  opt.device = device;
  opt.num_devices = num_devices;
  return run_particlization_opt(workdir, opt, dN_out, out_capacity, err, errlen);
}

extern "C" int is3d_host_run_particlization_devices(const char* workdir, const int* devices, int num_devices,
                                                    double* dN_out, long out_capacity, char* err, int errlen) {
  if (!devices || num_devices <= 0) { put_err(err, errlen, "empty device list"); return IS3D_ERR_ARG; }
  RunOptions opt;
  opt.devices.assign(devices, devices + num_devices);
  return run_particlization_opt(workdir, opt, dN_out, out_capacity, err, errlen);
}

extern "C" int is3d_host_total_yield(const char* workdir, int device, int num_devices, double* n_total,
                                     long* n_events, char* err, int errlen) {
  try {
    IS3D run(workdir ? workdir : ".");
    RunOptions opt;
    opt.device = device;
    opt.num_devices = num_devices;
    opt.quiet = true;
    run.run_particlization(1, opt);
    if (n_total) *n_total = run.total_yield();
    if (n_events) *n_events = run.events();
    return IS3D_OK;
  } catch (const std::exception& ex) {
    put_err(err, errlen, ex.what());
    return IS3D_ERR_ARG;
  }
}

extern "C" int is3d_host_sample(const char* workdir, const int* devices, int num_devices, int write_files, int write_csv,
                                is3d_particle* out, long* mcid_out, long capacity, long* offsets, long offsets_capacity,
                                long* n_particles, long* n_events, double* n_total, long* seed, char* err, int errlen) {
  return is3d_host_sample_decays(workdir, devices, num_devices, write_files, write_csv, out, mcid_out, capacity, offsets,
                                 offsets_capacity, n_particles, n_events, n_total, seed, nullptr, nullptr, err, errlen);
}

extern "C" int is3d_host_sample_decays(const char* workdir, const int* devices, int num_devices, int write_files, int write_csv,
                                       is3d_particle* out, long* mcid_out, long capacity, long* offsets, long offsets_capacity,
                                       long* n_particles, long* n_events, double* n_total, long* seed, long* origins,
                                       is3d_decay_list_stats* decay_stats, char* err, int errlen) {
  if (!devices || num_devices <= 0) { put_err(err, errlen, "empty device list"); return IS3D_ERR_ARG; }
  try {
    IS3D run(workdir ? workdir : ".");
    RunOptions opt;
    opt.devices.assign(devices, devices + num_devices);
    opt.quiet = true;
    opt.sample = true;
    opt.write_files = write_files != 0;
    opt.particle_list_csv = write_csv != 0;
    run.run_particlization(1, opt);
    if (run.particle_offsets().empty()) { put_err(err, errlen, "is3d_host_sample: operation = 2 expected in iS3D_parameters.dat"); return IS3D_ERR_ARG; }
    const long n = (long)run.final_particles().size(), nev = run.events();
    if (n_particles) *n_particles = n;
    if (n_events) *n_events = nev;
    if (n_total) *n_total = run.total_yield();
    if (seed) *seed = run.sampler_seed();
    if ((out && n > capacity) || (offsets && nev + 1 > offsets_capacity)) { put_err(err, errlen, "output buffer too small"); return IS3D_ERR_ARG; }
    if (out) std::copy(run.particle_records().begin(), run.particle_records().end(), out);
    if (mcid_out) {
      if (n > capacity) { put_err(err, errlen, "output buffer too small"); return IS3D_ERR_ARG; }
      for (long i = 0; i < n; i++) mcid_out[i] = run.final_particles()[(size_t)i].mcid;
    }
    if (offsets) std::copy(run.particle_offsets().begin(), run.particle_offsets().end(), offsets);
    if (origins) {
      if ((long)run.particle_origins().size() > capacity) { put_err(err, errlen, "output buffer too small"); return IS3D_ERR_ARG; }
      std::copy(run.particle_origins().begin(), run.particle_origins().end(), origins);
    }
    if (decay_stats) *decay_stats = run.decay_list_stats();
    return IS3D_OK;
  } catch (const EngineError& ex) {
    put_err(err, errlen, ex.what());
    return ex.code;
  } catch (const std::exception& ex) {
    put_err(err, errlen, ex.what());
    return IS3D_ERR_ARG;
  }
}

extern "C" int is3d_host_sample_hist_size(const char* workdir, is3d_sample_bins* bins, int* npart, long* n_counts, long* n_vn) {
  const std::string dir = workdir ? workdir : ".";
  ParameterReader prm;
  Table chosen;
  if (!prm.read_file(path_in(dir, "iS3D_parameters.dat")) || !load_table(path_in(dir, "PDG/chosen_particles.dat"), chosen)) return -1;
  const is3d_sample_bins b = read_sample_bins(prm);
  const long np = chosen.rows();
  if (bins) *bins = b;
  if (npart) *npart = (int)np;
  if (n_counts) *n_counts = np * ((long)b.y_bins + b.eta_bins + 2L * b.phip_bins + b.pT_bins + b.tau_bins + b.r_bins);
  if (n_vn) *n_vn = 14L * np * b.pT_bins;
  return 0;
}

extern "C" int is3d_host_sample_binned(const char* workdir, const int* devices, int num_devices, int write_files, long* counts,
                                       long counts_capacity, double* vn, long vn_capacity, long* n_events, double* n_total,
                                       long* seed, is3d_sample_stats* stats, char* err, int errlen) {
  return is3d_host_sample_binned_decays(workdir, devices, num_devices, write_files, counts, counts_capacity, vn, vn_capacity,
                                        n_events, n_total, seed, stats, nullptr, err, errlen);
}

extern "C" int is3d_host_sample_binned_decays(const char* workdir, const int* devices, int num_devices, int write_files,
                                              long* counts, long counts_capacity, double* vn, long vn_capacity, long* n_events,
                                              double* n_total, long* seed, is3d_sample_stats* stats,
                                              is3d_decay_list_stats* decay_stats, char* err, int errlen) {
  if (!devices || num_devices <= 0) { put_err(err, errlen, "empty device list"); return IS3D_ERR_ARG; }
  try {
    IS3D run(workdir ? workdir : ".");
    RunOptions opt;
    opt.devices.assign(devices, devices + num_devices);
    opt.quiet = true;
    opt.sample = true;
    opt.write_files = write_files != 0;
    run.run_particlization(1, opt);
    if (run.hist_counts().empty()) { put_err(err, errlen, "is3d_host_sample_binned: operation = 2 and test_sampler = 1 expected in iS3D_parameters.dat"); return IS3D_ERR_ARG; }
    if (n_events) *n_events = run.events();
    if (n_total) *n_total = run.total_yield();
    if (seed) *seed = run.sampler_seed();
    if (stats) *stats = run.sample_stats();
    if (decay_stats) *decay_stats = run.decay_list_stats();
    if ((counts && (long)run.hist_counts().size() > counts_capacity) || (vn && (long)run.hist_vn().size() > vn_capacity)) {
      put_err(err, errlen, "output buffer too small");
      return IS3D_ERR_ARG;
    }
    if (counts) std::copy(run.hist_counts().begin(), run.hist_counts().end(), counts);
    if (vn) std::copy(run.hist_vn().begin(), run.hist_vn().end(), vn);
    return IS3D_OK;
  } catch (const EngineError& ex) {
    put_err(err, errlen, ex.what());
    return ex.code;
  } catch (const std::exception& ex) {
    put_err(err, errlen, ex.what());
    return IS3D_ERR_ARG;
  }
}

extern "C" int is3d_host_write_particle_lists(const char* workdir, long n_events, const long* offsets, const is3d_particle* list,
                                              const long* mcid, const double* mass, int write_csv, char* err, int errlen) {
  if (!offsets || n_events < 0 || (offsets[n_events] > 0 && (!list || !mcid || !mass))) { put_err(err, errlen, "bad particle list"); return IS3D_ERR_ARG; }
  std::vector<long> off(offsets, offsets + n_events + 1);
  std::vector<SampledParticle> v((size_t)offsets[n_events]);
  for (size_t i = 0; i < v.size(); i++) {
    const is3d_particle& r = list[i];
    v[i] = SampledParticle{mcid[i], mass[i], r.tau, r.x, r.y, r.eta, r.t, r.z, r.E, r.px, r.py, r.pz};
  }
  std::string w = write_particle_list_osc(workdir ? workdir : ".", v, off);
  if (w.empty() && write_csv) w = write_particle_list_csv(workdir ? workdir : ".", v, off);
  if (!w.empty()) { put_err(err, errlen, w); return IS3D_ERR_ARG; }
  return IS3D_OK;
}

extern "C" int is3d_host_polarization(const char* workdir, const int* devices, int num_devices, double* S_out,
                                      long out_capacity, char* err, int errlen) {
  if (!devices || num_devices <= 0) { put_err(err, errlen, "empty device list"); return IS3D_ERR_ARG; }
  try {
    IS3D run(workdir ? workdir : ".");
    RunOptions opt;
    opt.devices.assign(devices, devices + num_devices);
    opt.quiet = true;
    opt.polarization_only = true;
    run.run_particlization(1, opt);
    const auto& S = run.polarization();
    if (S_out) {
      if ((long)S.size() > out_capacity) { put_err(err, errlen, "output buffer too small"); return IS3D_ERR_ARG; }
      std::copy(S.begin(), S.end(), S_out);
    }
    return IS3D_OK;
  } catch (const EngineError& ex) {
    put_err(err, errlen, ex.what());
    return ex.code;
  } catch (const std::exception& ex) {
    put_err(err, errlen, ex.what());
    return IS3D_ERR_ARG;
  }
}

extern "C" long is3d_host_read_vorticity(const char* workdir, int dimension, int include_baryon, double* w6) {
  Surface s;
  Averages a{};
  if (!read_surface(workdir ? workdir : ".", 5, dimension, include_baryon, s, a, false).empty()) return -1;
  const long n = s.size();
  if (w6)
    for (int k = 0; k < 6; k++) std::copy(s.w[k].begin(), s.w[k].end(), w6 + (size_t)k * n);
  return n;
}

extern "C" long is3d_host_read_surface(const char* workdir, int mode, int dimension, int include_baryon, double* fields,
                                       double* avg5) {
  Surface s;
  Averages a{};
  if (!read_surface(workdir ? workdir : ".", mode, dimension, include_baryon, s, a, false).empty()) return -1;
  const long n = s.size();
  if (fields) {
    const std::vector<double>* f[25] = {&s.tau, &s.x, &s.y, &s.eta, &s.dat, &s.dax, &s.day, &s.dan, &s.ux, &s.uy, &s.un,
                                        &s.E, &s.T, &s.P, &s.pixx, &s.pixy, &s.pixn, &s.piyy, &s.piyn, &s.bulkPi,
                                        &s.muB, &s.nB, &s.Vx, &s.Vy, &s.Vn};
    for (int k = 0; k < 25; k++) std::copy(f[k]->begin(), f[k]->end(), fields + (size_t)k * n);
  }
  if (avg5) { avg5[0] = a.T; avg5[1] = a.E; avg5[2] = a.P; avg5[3] = a.muB; avg5[4] = a.nB; }
  return n;
}

extern "C" int is3d_host_read_pdg(const char* workdir, int hrg_eos, int capacity, long* mcid, double* mass, int* gspin,
                                  int* baryon, int* sign) {
  std::vector<Particle> p;
  if (!read_pdg(workdir ? workdir : ".", hrg_eos, p).empty()) return -1;
  const int n = (int)p.size();
  if (mcid) {
    if (n > capacity) return -2;
    for (int i = 0; i < n; i++) { mcid[i] = p[i].mcid; mass[i] = p[i].mass; gspin[i] = p[i].gspin; baryon[i] = p[i].baryon; sign[i] = p[i].sign; }
  }
  return n;
}

extern "C" long is3d_host_read_decays(const char* workdir, int hrg_eos, long capacity, long* parent, int* n_body,
                                      double* branching, long* daughters) {
  std::vector<Particle> p;
  if (!read_pdg(workdir ? workdir : ".", hrg_eos, p).empty()) return -1;
  long n = 0;
  for (const auto& q : p) n += (long)q.decays.size();
  if (parent) {
    if (n > capacity) return -2;
    long i = 0;
    for (const auto& q : p)
      for (const auto& r : q.decays) {
        parent[i] = q.mcid; n_body[i] = r.n_body; branching[i] = r.branching;
        for (int k = 0; k < 5; k++) daughters[5 * i + k] = r.daughter[k];
        i++;
      }
  }
  return n;
}

extern "C" int is3d_host_read_df_tables(const char* table_dir, int* nT, int* nmuB, long capacity, double* T, double* muB,
                                        double* tables) {
  DfTablesData d;
  if (!table_dir || !nT || !nmuB || !read_df_table_dir(table_dir, d).empty()) return -1;
  *nT = d.nT; *nmuB = d.nmuB;
  if (T && muB && tables) {
    if ((long)d.tab.size() > capacity) return -1;
    std::copy(d.T.begin(), d.T.end(), T);
    std::copy(d.muB.begin(), d.muB.end(), muB);
    std::copy(d.tab.begin(), d.tab.end(), tables);
  }
  return 0;
}

extern "C" int is3d_host_param(const char* path, const char* key, double* value) {
  ParameterReader r;
  if (!r.read_file(path) || !r.has(key)) return -1;
  *value = r.get(key);
  return 0;
}
