// is3d_driver.h -- drop-in C++ facade of iS3D2's particlization plug-in surface for
// operations 1 (continuous spectra) and 0 (spacetime distributions), running the MI355X engine
// (libis3d_amd.so) underneath.
//
//   class IS3D                (iS3D.h:25-104)   read_fo_surf_from_memory + run_particlization
//   class EmissionFunctionArray (EmissionFunction.h:135-140) ctor + calculate_spectra
//
// Same inputs (iS3D_parameters.dat, input/surface.dat, PDG/, deltaf_coefficients/, tables/
// relative to a working directory) and the same outputs (results/continuous/*.dat).
// Differences from the reference: errors are returned / thrown instead of exit(); operation = 2 gives the
// oversampling estimate (Ntotal, Nevents) and, with RunOptions::sample, the sampled particle lists of df_mode 1-5
// (the engine's counter-based streams, not the reference's serial random engine) or, with test_sampler = 1, the
// binned results/sampled files instead of the lists; cells may be sharded over several GPUs in one process.
#pragma once
#include <string>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/is3d_amd.h"
#include "host_io.h"

namespace is3d {
namespace host {

// engine failure with the is3d_amd.h return code (IS3D_ERR_DF_RANGE for the reference's GSL abort, ...)
struct EngineError : std::runtime_error {
  int code;
  EngineError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

struct RunOptions {
  int device = 0;          // first HIP device
  int num_devices = 1;     // cells sharded over devices [device, device + num_devices)
  std::vector<int> devices;  // if not empty: shard k runs on devices[k] (an index may repeat)
  bool write_files = true;
  bool quiet = false;
  bool polarization_only = false;   // mode = 5: run only calculate_spin_polzn and its writer, not the operation
  // operation = 2: after the estimate, sample Nevents events (sample_dN_pTdpTdphidy) and write
  // results/particle_list_osc_<event>.dat -- or, test_sampler = 1, bin them and write results/sampled/*; off: the estimate only, no files (is3d_host_total_yield and
  // is3d_host_run_particlization); the iS3D_amd executable and is3d_host_sample set it
  bool sample = false;
  bool particle_list_csv = false;   // also write results/particle_list_<event>.dat (write_particle_list_toFile)
};

// EmissionFunctionArray(paraRdr, chosen, pT, phi, y, eta, particles, Nparticles, surface, FO_length, df tables)
class EmissionFunctionArray {
 public:
  EmissionFunctionArray(const ParameterReader& params, const Table& chosen, const Table& pT, const Table& phi,
                        const Table& y, const Table& eta, const std::vector<Particle>& particles, const Surface& surf,
                        const DfTablesData& df, const Averages& plasma, const std::vector<double>& gla_roots,
                        const std::vector<double>& gla_weights, int gla_alpha, int gla_points);
  // operation = 1: dN/(pT dpT dphi dy) [species][pT][phi][y]; throws std::runtime_error on failure
  void calculate_spectra(const RunOptions& opt);
  void write_files(const std::string& dir) const;
  const std::vector<double>& spectra() const { return dN_; }
  // operation = 0 (SpacetimeDistribution.cpp): dN/(tau dtau dy), dN/(2 pi r dr dy), dN/(dphi dy) [species][bins]
  void calculate_dN_dX(const RunOptions& opt);
  void write_spacetime_files(const std::string& dir) const;
  const std::vector<double>& dN_taudtaudy() const { return dNtau_; }
  const std::vector<double>& dN_2pirdrdy() const { return dNr_; }
  const std::vector<double>& dN_dphidy() const { return dNphi_; }
  is3d_spacetime_bins bins() const { return bins_; }
  const std::vector<long>& mcid() const { return mcid_; }
  // operation = 2 oversampling estimate (ParticleSampler.cpp:447-636): the reference's Ntotal
  double estimate_total_yield(const RunOptions& opt);
  // operation = 2, the sampler (ParticleSampler.cpp:638-1134, df_mode 1-4; :1138-1627, df_mode 5): n_events events with the given
  // non-negative seed; sampled() = the list with the chosen table's mcID and mass filled, sample_offsets() its
  // n_events + 1 event offsets, sampled_records() the engine's records (species index, event, cell)
  void sample_particles(const RunOptions& opt, long seed, long n_events);
  const std::vector<SampledParticle>& sampled() const { return sampled_; }
  const std::vector<is3d_particle>& sampled_records() const { return records_; }
  const std::vector<long>& sample_offsets() const { return sample_offsets_; }
  const is3d_sample_stats& sample_stats() const { return sample_stats_; }
  // df_mode 5: both went through is3d_sample_famod (sample_dN_pTdpTdphidy_famod, ParticleSampler.cpp:1138-1627);
  // famod_stats() = its reconstruction counters
  bool famod_sampled() const { return famod_sampled_; }
  const is3d_sample_famod_stats& famod_stats() const { return famod_stats_; }
  // ... with test_sampler = 1 (ParticleSampler.cpp:1112-1121): the same events binned on the device with the parameter
  // file's bins and no list; hist_counts() / hist_vn() = is3d_get_sample_hist's arrays, write_sampled_files the
  // results/sampled/* tree (EmissionFunction.cpp:685-975)
  void sample_binned(const RunOptions& opt, long seed, long n_events);
  const std::vector<long>& hist_counts() const { return hist_counts_; }
  const std::vector<double>& hist_vn() const { return hist_vn_; }
  is3d_sample_bins sample_bins() const { return sbins_; }
  void write_sampled_files(const std::string& dir) const;
  // mode = 5 (EmissionFunction.cpp:1305-1310): calculate_spin_polzn at T = the Plasma average temperature, on an
  // engine of its own that holds only params, species, grid, surface and vorticity.  IS3D::run_particlization calls
  // it after the chosen operation (0, 1 or 2) and after that operation's files are written.
  // polarization() = the raw sums [5][species][pT][phi][y] (S_t S_x S_y S_n Snorm), write_polzn_files the four
  // results/S*.dat (S_c / Snorm)
  void calculate_polarization(const RunOptions& opt);
  bool has_polarization() const { return !S_.empty(); }
  const std::vector<double>& polarization() const { return S_; }
  void write_polzn_files(const std::string& dir) const;
  double seconds() const { return seconds_; }
  // do_resonance_decays = 1 with operation = 1: the decay rows of the PDG file over the chosen species
  // (decay_channels()), applied to the spectra by is3d_decay_feeddown before the writers run; decay_stats() = the
  // engine's bookkeeping (zero when the key is 0 or absent)
  const std::vector<is3d_decay_channel>& decay_channels() const { return decays_; }
  const is3d_decay_stats& decay_stats() const { return decay_stats_; }
  // do_resonance_decays = 1 with operation = 2: the sampled hadrons are decayed on the device as they are sampled
  // (is3d_sample_decayed, the sampler's seed); sampled(), sample_offsets() and sampled_records() then hold the final hadrons,
  // sample_origins() the index in the sampled list of the primary each descends from and decay_list_stats() the
  // engine's counters (empty / zero when the key is 0 or absent).  With test_sampler = 1 the final hadrons are binned
  const std::vector<long>& sample_origins() const { return origins_; }
  const is3d_decay_list_stats& decay_list_stats() const { return decay_list_stats_; }

 private:
  std::vector<long> origins_;
  is3d_decay_list_stats decay_list_stats_{};
  std::vector<is3d_decay_channel> decays_;
  std::vector<is3d_decay_channel4> decays4_;       // four_body_decays = 1: the same rows with four daughter slots
  int set_run_decays(is3d_engine* e) const;
  is3d_decay_stats decay_stats_{};
  const ParameterReader& p_;
  const Table &pT_, &phi_, &y_, &eta_;
  const Surface& surf_;
  const DfTablesData& df_;
  Averages plasma_;
  const std::vector<double>&gr_, &gw_;
  int galpha_, gpts_;
  int dimension_ = 2;
  std::vector<double> mass_, sign_, degen_, baryon_;
  std::vector<double> pdg_mass_, pdg_sign_, pdg_degen_, pdg_baryon_;
  std::vector<long> mcid_;
  std::vector<double> dN_;
  std::vector<double> dNtau_, dNr_, dNphi_;
  std::vector<double> S_;
  is3d_spacetime_bins bins_{};
  double seconds_ = 0.0;
  double ntotal_ = 0.0;
  long sample_seed_ = 0, sample_events_ = 1;
  std::vector<SampledParticle> sampled_;
  std::vector<is3d_particle> records_;
  std::vector<long> sample_offsets_;
  is3d_sample_stats sample_stats_{};
  is3d_sample_famod_stats famod_stats_{};
  bool famod_sampled_ = false;
  is3d_sample_bins sbins_{};
  std::vector<long> hist_counts_;
  std::vector<double> hist_vn_;
  // operation 3: the sampler (engine operation 2), 4: its binned-only form; 2: the yield estimate; -1: the polarization alone (an engine without PDG, Gauss-Laguerre and df tables)
  void run_sharded(const RunOptions& opt, int operation);
};

class IS3D {
 public:
  explicit IS3D(std::string workdir = ".") : dir_(std::move(workdir)) {}
  // iS3D.cpp:33-78 (units: reader-converted, GeV / fm)
  void read_fo_surf_from_memory(std::vector<double> tau, std::vector<double> x, std::vector<double> y,
                                std::vector<double> eta, std::vector<double> dsigma_tau, std::vector<double> dsigma_x,
                                std::vector<double> dsigma_y, std::vector<double> dsigma_eta, std::vector<double> E,
                                std::vector<double> T, std::vector<double> P, std::vector<double> ux,
                                std::vector<double> uy, std::vector<double> un, std::vector<double> pixx,
                                std::vector<double> pixy, std::vector<double> pixn, std::vector<double> piyy,
                                std::vector<double> piyn, std::vector<double> pinn, std::vector<double> Pi);
  // iS3D.cpp:81-282 for operation = 1, 0 and the estimate of 2; throws std::runtime_error.  spectra() = the momentum
  // spectra (operation 1) or, per species, [dN_taudtaudy | dN_2pirdrdy | dN_dphidy] bins (operation 0)
  void run_particlization(int fo_from_file, const RunOptions& opt = RunOptions());
  const std::vector<double>& spectra() const { return dN_; }
  // mode = 5: the raw polarization sums [5][species][pT][phi][y] of the run (empty otherwise)
  const std::vector<double>& polarization() const { return S_; }
  // operation = 2: Ntotal and Nevents = min(ceil(min_num_hadrons / Ntotal), max_num_samples) if
  // oversample, else 1 (EmissionFunction.cpp:1237-1249)
  double total_yield() const { return ntotal_; }
  long events() const { return nevents_; }
  // operation = 2 with RunOptions::sample: the sampled list, events contiguous (the reference's final_particles_ /
  // particle_event_list for in-memory callers), its events() + 1 offsets and the engine's records and stats
  const std::vector<SampledParticle>& final_particles() const { return final_particles_; }
  const std::vector<long>& particle_offsets() const { return particle_offsets_; }
  const std::vector<is3d_particle>& particle_records() const { return particle_records_; }
  const is3d_sample_stats& sample_stats() const { return sample_stats_; }
  // do_resonance_decays = 1: the lists above are the decayed ones; particle_origins()[i] = the sampled primary record
  // i descends from, decay_list_stats() the counters of the decays
  const std::vector<long>& particle_origins() const { return particle_origins_; }
  const is3d_decay_list_stats& decay_list_stats() const { return decay_list_stats_; }
  long sampler_seed() const { return seed_; }
  // ... with test_sampler = 1: no list (the offsets are zero); the histograms of is3d_get_sample_hist and their bins
  const std::vector<long>& hist_counts() const { return hist_counts_; }
  const std::vector<double>& hist_vn() const { return hist_vn_; }
  const is3d_sample_bins& sample_bins() const { return sample_bins_; }

 private:
  std::string dir_;
  double ntotal_ = 0.0;
  long nevents_ = 0;
  Surface mem_;
  std::vector<double> dN_;
  std::vector<double> S_;
  std::vector<SampledParticle> final_particles_;
  std::vector<long> particle_offsets_;
  std::vector<is3d_particle> particle_records_;
  std::vector<long> particle_origins_;
  is3d_decay_list_stats decay_list_stats_{};
  is3d_sample_stats sample_stats_{};
  std::vector<long> hist_counts_;
  std::vector<double> hist_vn_;
  is3d_sample_bins sample_bins_{};
  long seed_ = 0;
};

}  // namespace host
}  // namespace is3d
