/*
 * is3d_host.h -- C ABI of the C++ host layer (libis3d_host.so): the iS3D2 drop-in
 * workflow around the engine (include/is3d_amd.h).
 *
 *   is3d_host_run_particlization   IS3D::run_particlization(1) for operation = 1 or 0 (iS3D.cpp:81-282)
 *                                  reading <workdir>/iS3D_parameters.dat, input/surface.dat, PDG/,
 *                                  deltaf_coefficients/, tables/ and writing results/continuous/
 *   is3d_host_run_particlization_devices   the same with an explicit device per cell shard
 *   is3d_host_total_yield          IS3D::run_particlization(1) for operation = 2: the oversampling
 *                                  estimate Ntotal / Nevents (EmissionFunction.cpp:1235-1249)
 *   is3d_host_sample               ... and the sampler: sample_dN_pTdpTdphidy + write_particle_list_OSC
 *                                  (ParticleSampler.cpp:638-1134, EmissionFunction.cpp:1251-1301, 611-678)
 *   is3d_host_sample_binned        ... with test_sampler = 1: the binned distributions and the results/sampled
 *                                  files instead of the lists (BinSampledParticle.cpp, EmissionFunction.cpp:685-975)
 *   is3d_host_read_surface         FO_data_reader::read_freezeout_surface modes 1/5/6/7 (readindata.cpp:149-731)
 *   is3d_host_read_vorticity       the thermal-vorticity columns of a mode-5 surface    (readindata.cpp:298-306)
 *   is3d_host_polarization         calculate_spin_polzn + write_polzn_vector_toFile     (Polarization.cpp:25-263,
 *                                                                                        EmissionFunction.cpp:561-609)
 *   is3d_host_read_pdg             PDG_Data::read_resonances                            (readindata.cpp:1217-1252)
 *   is3d_host_read_decays          ... its decay rows, with the antibaryon rule         (readindata.cpp:997-1007, 1035-1056)
 *   is3d_host_read_df_tables       Deltaf_Data::load_df_coefficient_data of one directory (DeltafData.cpp:65-217)
 *   is3d_host_param                ParameterReader::getVal                             (ParameterReader.cpp:142-155)
 */
#ifndef IS3D_HOST_H
#define IS3D_HOST_H
#include "is3d_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* generate_df_coefficients = 1 in iS3D_parameters.dat (ours; 0 or absent: nothing changes): deltaf_coefficients/ is not
 * read; the delta-f tables are generated on the GPU from the run's PDG list (is3d_generate_df_tables, is3d_amd.h) on
 * the shipped grid -- T 0.1 .. 0.2 GeV in 101 points, muB 0 .. 0.8 GeV in 81 -- or on the grid of the optional keys
 * df_T_min, df_T_max, df_T_points, df_muB_min, df_muB_max, df_muB_points, and installed.  The Gauss-Laguerre table is
 * tables/gla_roots_weights_64_points.txt (the generator's own 64-point file, the reference's layout), or, where the
 * run directory has none, tables/gauss/gla_roots_weights.txt.  = 2: the ten files are also written to
 * results/deltaf_coefficients/ in the reference's format (six decimals).  Every operation of the run uses the tables.
 *
 * do_resonance_decays = 1 in iS3D_parameters.dat with operation = 1: the decay rows of the PDG file are applied to the
 * spectra (is3d_set_decays + is3d_decay_feeddown, include/is3d_amd.h) between the spectra and the writers, so
 * results/continuous and dN_out hold thermal + feed-down, and the channel counts are printed.  With the key 0 or
 * absent, or under another operation, nothing changes.  lightest_particle is read and not used, as in the reference.
 * four_body_decays = 1 (ours; absent or 0: as before) next to it, for operations 1 and 2: the rows are built with four
 * daughter slots and set with is3d_set_decays4, which keeps the open 4-body channels; the printed line then counts the
 * rows with 5 or more bodies.
 *
 * Runs the whole workflow on HIP devices [device, device + num_devices) (cells sharded);
 * dN_out (optional, capacity doubles) receives dN/(pT dpT dphi dy)[species][pT][phi][y] (operation 1)
 * or, per species, [dN_taudtaudy (tau_bins) | dN_2pirdrdy (r_bins) | dN_dphidy (phip_bins)] (operation 0). */
int is3d_host_run_particlization(const char *workdir, int device, int num_devices, double *dN_out,
                                 long out_capacity, char *err, int errlen);
/* As is3d_host_run_particlization with cell shard k on HIP device devices[k] (an index may repeat:
 * several engines on one GPU, e.g. to exercise the sharded path on a one-GPU box).  Returns the
 * engine's is3d_amd.h code (IS3D_ERR_DF_RANGE for the reference's GSL spline abort, ...). */
int is3d_host_run_particlization_devices(const char *workdir, const int *devices, int num_devices, double *dN_out,
                                         long out_capacity, char *err, int errlen);
/* operation = 2 in <workdir>/iS3D_parameters.dat: n_total = the estimated total yield (0 unless
 * oversample = 1), n_events = min(ceil(min_num_hadrons / Ntotal), max_num_samples) (1 without
 * oversampling).  Estimate only: nothing is sampled and no file is written, as is3d_host_run_particlization of an
 * operation = 2 directory; is3d_host_sample samples. */
int is3d_host_total_yield(const char *workdir, int device, int num_devices, double *n_total, long *n_events,
                          char *err, int errlen);
/* operation = 2 in <workdir>/iS3D_parameters.dat, df_mode 1-4: the estimate above, then the sampler
 * (is3d_sample: sample_dN_pTdpTdphidy on the GPU) over Nevents events on HIP devices devices[0..num_devices), with
 * the run directory's sampler_seed (< 0: the clock, as the reference; *seed receives the seed used), fast and y_cut.
 * write_files: results/particle_list_osc_<event>.dat for event = 1..Nevents, exactly as write_particle_list_OSC;
 * write_csv: also results/particle_list_<event>.dat (write_particle_list_toFile).  test_sampler = 1: the particles
 * are binned on the device and never listed, as in the reference (EmissionFunction.cpp:1279-1291) -- write_files
 * writes the results/sampled tree and no particle list, n_particles is 0 and the offsets are 0; is3d_host_sample_binned
 * also returns the histograms.  A mode = 5 directory runs the polarization afterwards.
 * out (optional, capacity records): the engine's records, events contiguous and ordered by (cell, candidate) inside
 * an event; mcid_out (optional, capacity): each particle's MCID from the chosen table; offsets (optional,
 * offsets_capacity >= Nevents + 1).  n_particles / n_events / n_total / seed are filled even when the buffers are too
 * small (IS3D_ERR_ARG "output buffer too small"): with a fixed sampler_seed a second call returns the same list. */
int is3d_host_sample(const char *workdir, const int *devices, int num_devices, int write_files, int write_csv,
                     is3d_particle *out, long *mcid_out, long capacity, long *offsets, long offsets_capacity,
                     long *n_particles, long *n_events, double *n_total, long *seed, char *err, int errlen);
/* is3d_host_sample with the bookkeeping of do_resonance_decays = 1 (the sampled hadrons are decayed down their chains
 * on the device by is3d_sample_decayed with the sampler's seed, and every output above is the decayed list's;
 * test_sampler = 1: the final hadrons are binned and no list is made): origins (optional, capacity) = for each record the index, in the sampled list, of the primary it
 * descends from; decay_stats (optional) = is3d_get_decay_list_stats.  With the key 0 or absent nothing is written to
 * origins and the stats are zero. */
int is3d_host_sample_decays(const char *workdir, const int *devices, int num_devices, int write_files, int write_csv,
                            is3d_particle *out, long *mcid_out, long capacity, long *offsets, long offsets_capacity,
                            long *n_particles, long *n_events, double *n_total, long *seed, long *origins,
                            is3d_decay_list_stats *decay_stats, char *err, int errlen);
/* operation = 2 and test_sampler = 1 in <workdir>/iS3D_parameters.dat: as is3d_host_sample, with every kept particle
 * binned on the device (is3d_sample_binned, keep_list = 0) with the parameter file's pT / y / phip / eta / tau / r bins.
 * write_files: the results/sampled tree of write_sampled_*_to_file_test (EmissionFunction.cpp:685-975), nine files per
 * species, sub-directories created when missing; no particle list.  counts / vn (optional): is3d_get_sample_hist's
 * arrays; is3d_host_sample_hist_size gives their sizes, the bins and the number of chosen species from the run
 * directory alone (returns 0, or -1 when the parameter file or PDG/chosen_particles.dat cannot be read). */
int is3d_host_sample_hist_size(const char *workdir, is3d_sample_bins *bins, int *npart, long *n_counts, long *n_vn);
int is3d_host_sample_binned(const char *workdir, const int *devices, int num_devices, int write_files, long *counts,
                            long counts_capacity, double *vn, long vn_capacity, long *n_events, double *n_total,
                            long *seed, is3d_sample_stats *stats, char *err, int errlen);
/* ... with decay_stats (optional) = is3d_get_decay_list_stats of the decays that do_resonance_decays = 1 ran on the kept
 * list before it was binned (zero with the key 0 or absent). */
int is3d_host_sample_binned_decays(const char *workdir, const int *devices, int num_devices, int write_files, long *counts,
                                   long counts_capacity, double *vn, long vn_capacity, long *n_events, double *n_total,
                                   long *seed, is3d_sample_stats *stats, is3d_decay_list_stats *decay_stats, char *err,
                                   int errlen);
/* The two writers alone, for a list the caller holds: offsets[n_events + 1], list / mcid / mass per particle. */
int is3d_host_write_particle_lists(const char *workdir, long n_events, const long *offsets, const is3d_particle *list,
                                   const long *mcid, const double *mass, int write_csv, char *err, int errlen);
/* Returns the number of cells (or < 0); fields (optional) receives [25][n] in is3d_surface order,
 * avg5 the Plasma averages T, E, P, muB, nB after the 15-digit round trip. */
long is3d_host_read_surface(const char *workdir, int mode, int dimension, int include_baryon, double *fields,
                            double *avg5);
/* The six thermal-vorticity columns of a mode-5 <workdir>/input/surface.dat (wbar^{tx ty tn xy xn yn}, no unit
 * conversion, readindata.cpp:298-306): returns the number of cells (or < 0); w6 (optional) receives [6][n]. */
long is3d_host_read_vorticity(const char *workdir, int dimension, int include_baryon, double *w6);
/* mode = 5 only: EmissionFunctionArray::calculate_spin_polzn (Polarization.cpp:25-263) of the run directory on
 * HIP devices devices[0..num_devices), at T = the Plasma average temperature, without running the operation:
 * writes results/St.dat, Sx.dat, Sy.dat, Sn.dat (rows y, phi, pT, S_c / Snorm) and returns the raw sums
 * S_out[5][species][pT][phi][y] (S_t S_x S_y S_n Snorm; optional, capacity doubles).
 * is3d_host_run_particlization[_devices] of a mode = 5 directory runs the same after the chosen operation
 * (EmissionFunction.cpp:1305-1310) and writes the same four files. */
int is3d_host_polarization(const char *workdir, const int *devices, int num_devices, double *S_out, long out_capacity,
                           char *err, int errlen);
/* Returns the number of particles (or < 0); arrays optional (capacity entries). */
int is3d_host_read_pdg(const char *workdir, int hrg_eos, int capacity, long *mcid, double *mass, int *gspin,
                       int *baryon, int *sign);
/* The decay rows of a conventional PDG file (hrg_eos 1, 2) in particle order, antibaryon rows generated
 * (readindata.cpp:997-1007, 1035-1056): returns their number (or < 0); arrays optional (capacity rows):
 * parent mcid, n_body as written, branching, daughters[n][5]. */
long is3d_host_read_decays(const char *workdir, int hrg_eos, long capacity, long *parent, int *n_body,
                           double *branching, long *daughters);
/* The ten delta-f coefficient files c0.dat .. betapi.dat of one directory (a run directory's
 * deltaf_coefficients/vh/<list>/, results/deltaf_coefficients/, or what hrg.write_df_tables wrote): returns 0 (or -1) and
 * the grid sizes; T[nT], muB[nmuB], tables[10][nmuB][nT] are optional (capacity = doubles in tables). */
int is3d_host_read_df_tables(const char *table_dir, int *nT, int *nmuB, long capacity, double *T, double *muB,
                             double *tables);
int is3d_host_param(const char *path, const char *key, double *value);

#ifdef __cplusplus
}
#endif
#endif
