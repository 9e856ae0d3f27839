// host_io.h -- C++ host services for the iS3D2 drop-in workflow (reference file
// formats on both sides of the continuous-spectra hot path).  Clean-room
// implementations of the reference's readers/writers; each function cites the
// reference code whose behaviour it reproduces.
#pragma once
#include <string>
#include <vector>

namespace is3d {
namespace host {

// ParameterReader (ParameterReader.cpp:28-155): "key = value # comment", keys
// lower-cased and trimmed, values parsed as double, later keys overwrite earlier.
class ParameterReader {
 public:
  bool read_file(const std::string& path);            // false if the file cannot be opened
  bool has(const std::string& key) const;
  double get(const std::string& key) const;           // throws std::runtime_error if missing
  double get(const std::string& key, double fallback) const;
  void set(const std::string& key, double v);
 private:
  std::vector<std::string> names_;
  std::vector<double> values_;
  long find(const std::string& key) const;
};

// Table (Table.cpp:141-162 + Arsenal.cpp:86-121): whitespace columns; a row is a line
// terminated by '\n' (a final unterminated line is not read, as in readBlockData).
struct Table {
  std::vector<std::vector<double>> cols;              // cols[c][r]
  long rows() const { return cols.empty() ? 0 : (long)cols[0].size(); }
  long ncols() const { return (long)cols.size(); }
  double get(long col1, long row1) const { return cols[col1 - 1][row1 - 1]; }   // 1-based like the reference
};
bool load_table(const std::string& path, Table& t);

// Freeze-out surface, SoA in reader units (GeV, fm), field order of include/is3d_amd.h.
struct Surface {
  std::vector<double> tau, x, y, eta, dat, dax, day, dan, ux, uy, un, E, T, P, pixx, pixy, pixn, piyy, piyn, bulkPi,
      muB, nB, Vx, Vy, Vn;
  // mode 5 only: thermal vorticity wbar^{tx ty tn xy xn yn}, no unit conversion (readindata.cpp:298-306); else empty
  std::vector<double> w[6];
  bool has_vorticity() const { return size() > 0 && (long)w[0].size() == size(); }
  long size() const { return (long)tau.size(); }
  void resize(long n);
};

// Plasma averages (readindata.cpp:316-366): ds_max-weighted T, E, P, muB, nB.
struct Averages { double T, E, P, muB, nB; };

// FO_data_reader::read_freezeout_surface for mode 1/5 (CPU VH, readindata.cpp:167-367),
// 6 (MUSIC, :372-567) and 7 (HIC-EventGen, :570-731).  Reads <dir>/input/surface.dat,
// returns the averages after the reference's setprecision(15) text round trip and (like the
// reference) writes them to <dir>/tables/thermodynamic/average_thermodynamic_quantities.dat
// when write_averages is set.  Returns an empty string on success, else an error message.
std::string read_surface(const std::string& dir, int mode, int dimension, int include_baryon, Surface& s,
                         Averages& avg, bool write_averages);
// averages for a surface handed over in memory (iS3D.cpp:126-220)
Averages surface_averages(const Surface& s, int include_baryon);
std::string write_averages_file(const std::string& dir, const Averages& a);

// PDG_Data::read_resonances (readindata.cpp:973-1252): hrg_eos 1 UrQMD, 2 SMASH
// (conventional format, antibaryons inserted), 3 SMASH box (mcid-decoded).
// Conventional format: the decay rows are kept (n_body as written: the UrQMD table flags some rows with a negative
// count), and an antibaryon's rows repeat the baryon's with every daughter negated except neutral non-strange mesons
// (readindata.cpp:1035-1056; a daughter is looked up in the whole file).  The box format has no decay rows.
struct DecayRow { int n_body; double branching; long daughter[5]; };
struct Particle {
  long mcid; std::string name; double mass, width; int gspin, baryon, sign;
  int strange = 0, charge = 0;
  std::vector<DecayRow> decays;
};
std::string read_pdg(const std::string& dir, int hrg_eos, std::vector<Particle>& out);
void decode_mcid(long mcid, int& gspin, int& baryon, int& sign, bool& has_antiparticle);   // read_mcid

// Deltaf_Data::load_df_coefficient_data (DeltafData.cpp:65-217): 10 tables
// c0 c1 c2 c3 c4 F G betabulk betaV betapi from <dir>/deltaf_coefficients/vh/<hrg>/.
struct DfTablesData { int nT = 0, nmuB = 0; std::vector<double> T, muB, tab; };   // tab[10][nmuB][nT]
std::string read_df_tables(const std::string& dir, int hrg_eos, DfTablesData& d);
// ... from the ten files c0.dat .. betapi.dat of one directory
std::string read_df_table_dir(const std::string& table_dir, DfTablesData& d);
// generate_df_coefficients = 2: the ten files under <dir>/results/deltaf_coefficients/ in the format of the
// reference's generator (deltaf_table.cpp:122-133, 240-244: nT, nmuB, the label line, rows "T  muB  value" with muB
// outer and T inner, fixed with six decimals), which read_df_table_dir and the reference read
std::string write_df_tables(const std::string& dir, const DfTablesData& d);

// Gauss_Laguerre::load_roots_and_weights (readindata.cpp:26-61)
std::string read_gauss_laguerre(const std::string& path, int& alpha, int& points, std::vector<double>& roots,
                                std::vector<double>& weights);

// EmissionFunctionArray writers (EmissionFunction.cpp:406-558, 804-878): dN_pTdpTdphidy_<mcid>.dat,
// vn_, dN_2pipTdpTdy_, dN_dphidy_, dN_dy_ under <dir>/results/continuous/.
struct SpectraView {
  const double* dN;                 // [species][pT][phi][y]
  int npart, npT, nphi, ny, dimension;
  const Table *pT, *phi, *y;
  const std::vector<long>* mcid;
};
std::string write_spectra_files(const std::string& dir, const SpectraView& v);

// write_polzn_vector_toFile (EmissionFunction.cpp:561-609): <dir>/results/St.dat, Sx.dat, Sy.dat, Sn.dat with rows
// "y \t phi \t pT \t S_c / Snorm" (scientific, 8 digits), species -> y -> phi -> pT, a blank line after each pT run.
// Departure from the reference: each row holds the value its labels name (the reference reads index
// iy + ny (iphi + nphi (ipT + npT ipart)) from arrays filled at ipart + npart (ipT + npT (iphi + nphi iy)), and in
// 2+1D loops y_tab_length rows over one filled y slot); 2+1D writes one y = 0 block.
struct PolznView {
  const double* S;                  // [5][species][pT][phi][y]: S_t S_x S_y S_n Snorm
  int npart, npT, nphi, ny, dimension;
  const Table *pT, *phi, *y;
};
std::string write_polzn_files(const std::string& dir, const PolznView& v);

// operation = 0 writers (SpacetimeDistribution.cpp:138-145, 407-440): dN_taudtaudy_<mcid>.dat,
// dN_2pirdrdy_<mcid>.dat, dN_dphidy_<mcid>.dat under <dir>/results/continuous/, opened in append mode,
// "bin midpoint \t value" with setprecision(6) scientific.
struct SpacetimeView {
  const double *dN_taudtaudy, *dN_2pirdrdy, *dN_dphidy;   // [species][bins], bin-normalised
  int npart;
  double tau_min, tau_max; int tau_bins;
  double r_min, r_max; int r_bins;
  int phip_bins;
  const std::vector<long>* mcid;
};
std::string write_spacetime_files(const std::string& dir, const SpacetimeView& v);

// Sampled particle lists of operation = 2, one file per event (numbered from 1):
//   write_particle_list_osc  results/particle_list_osc_<event>.dat  (write_particle_list_OSC, EmissionFunction.cpp:645-678)
//       header "n pid px py pz E m x y z t", rows "index mcid" then the nine values, scientific with 16 digits
//   write_particle_list_csv  results/particle_list_<event>.dat      (write_particle_list_toFile, :611-642)
//       header "mcid,tau,x,y,eta,E,px,py,pz", rows: the mcid right-aligned in 5 columns, the values with 8 digits
// offsets: n_events + 1 positions into the list (events contiguous).
struct SampledParticle { long mcid; double mass, tau, x, y, eta, t, z, E, px, py, pz; };
std::string write_particle_list_osc(const std::string& dir, const std::vector<SampledParticle>& list, const std::vector<long>& offsets);
std::string write_particle_list_csv(const std::string& dir, const std::vector<SampledParticle>& list, const std::vector<long>& offsets);


// test_sampler = 1 writers (EmissionFunction.cpp:685-975), all under <dir>/results/sampled/, one file per species;
// the sub-directories are created when missing (the reference relies on a prepared tree).  Byte for byte what the
// reference's streams produce:
//   dN_dy/dN_dy_<mcid>_test.dat                   "midpoint \t count / (width Nevents)", both %.6g
//   dN_dy/dN_dy_<mcid>_average_test.dat           one %.6g line: sum of counts / (2 y_cut Nevents)
//   dN_deta/dN_deta_<mcid>_test.dat               as dN_dy, with the eta bins
//   dN_2pipTdpTdy/dN_2pipTdpTdy_<mcid>_test.dat   %.6e: count / (2 pi 2 y_cut width pT_mid Nevents)
//   dN_dphipdy/dN_dphipdy_<mcid>_test.dat         %.6e: count / (2 y_cut width Nevents)
//   vn/vn_<mcid>_test.dat                         %.6e: pT midpoint, then seven |re + i im| / pT_count (NaN, inf -> 0)
//   dN_taudtaudy/dN_taudtaudy_<mcid>_test.dat     %.6e: count / (tau_mid width Nevents 2 y_cut)
//   dN_2pirdrdy/dN_2pirdrdy_<mcid>_test.dat       %.6e: count / (2 pi r_mid width Nevents 2 y_cut)
//   dN_dphisdy/dN_dphisdy_<mcid>_test.dat         %.6e: count / (width Nevents 2 y_cut)
struct SampledHistView {
  const long* counts;       // is3d_get_sample_hist: dN_dy | dN_deta | dN_dphipdy | pT | tau | r | phis, each [npart][bins]
  const double* vn;         // [2][7][npart][pT_bins] raw sums
  int npart;
  long n_events;
  double pT_min, pT_max; int pT_bins;
  double y_cut; int y_bins;
  int phip_bins;
  double eta_cut; int eta_bins;
  double tau_min, tau_max; int tau_bins;
  double r_min, r_max; int r_bins;
  const std::vector<long>* mcid;
};
std::string write_sampled_files(const std::string& dir, const SampledHistView& v);

}  // namespace host
}  // namespace is3d
