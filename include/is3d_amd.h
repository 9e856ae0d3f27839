/*
 * is3d_amd.h -- C ABI of the MI355X Cooper-Frye continuous-spectra engine
 * (libis3d_amd.so).  Plain pointers and sizes only; no torch / HIP types.
 *
 * This is the drop-in boundary for iS3D2's operation = 1 hot path.  Each entry
 * point replaces one piece of the reference's EmissionFunctionArray /
 * Deltaf_Data / IS3D plug-in surface (reference = xyw2016/iS3D2 @ 2025-01-17):
 *
 *   is3d_create / is3d_destroy        EmissionFunctionArray ctor / dtor        (EmissionFunction.cpp:114-399)
 *   is3d_set_params                   ParameterReader flags read by the ctor   (EmissionFunction.cpp:140-205)
 *   is3d_set_species                  chosen particle arrays                    (EmissionFunction.cpp:997-1021, 339-390)
 *   is3d_set_pdg                      full PDG arrays (PTMA, PTB Jonah table)   (EmissionFunction.cpp:1025-1036)
 *   is3d_set_momentum_grid            pT/phi/y/eta Tables                      (iS3D.cpp:254-257, MomentumSpectra.cpp:49-91)
 *   is3d_set_gauss_laguerre           Gauss_Laguerre::load_roots_and_weights   (readindata.cpp:26-61)
 *   is3d_set_df_tables                Deltaf_Data::load_df_coefficient_data +  (DeltafData.cpp:65-321)
 *                                     construct_cubic_splines + compute_jonah_coefficients
 *   is3d_set_surface                  FO_surf[] -> SoA unpack                  (EmissionFunction.cpp:1049-1161)
 *   is3d_calculate_spectra            calculate_spectra, operation = 1         (EmissionFunction.cpp:1198-1226)
 *   is3d_set_momentum_weights         pT/phi Table weight columns              (SpacetimeDistribution.cpp:57-79)
 *   is3d_set_spacetime_bins           tau/r/phip bin parameters                (EmissionFunction.cpp:232-247)
 *   is3d_calculate_dN_dX              calculate_spectra, operation = 0         (EmissionFunction.cpp:1165-1196)
 *   is3d_calculate_dN_dX_famod        operation = 0 for df_mode 5: no reference routine; the per-cell decomposition of
 *                                     calculate_dN_pTdpTdphidy_famod           (MomentumSpectra.cpp:1517-1621)
 *   is3d_get_cell_yields              dN_dy_cell of each freeze-out cell       (SpacetimeDistribution.cpp:374)
 *   is3d_evaluate_df_coefficients     Deltaf_Data::evaluate_df_coefficients    (DeltafData.cpp:501-519)
 *   is3d_generate_df_tables           the offline generator of deltaf_coefficients/vh/<list>/<name>.dat
 *                                     (generate_delta_f_coefficients/<list>/df_vh_dimensionless/src/deltaf_table.cpp)
 *   is3d_surface_averages             ds_max-weighted averages (Plasma)        (readindata.cpp:316-366, iS3D.cpp:184-219)
 *   is3d_total_yield                  calculate_total_yield (operation 2       (ParticleSampler.cpp:447-636,
 *                                     oversampling) + particle densities        DeltafData.cpp:555-690)
 *   is3d_set_vorticity                thermal vorticity columns of a mode-5 surface (readindata.cpp:298-306)
 *   is3d_calculate_polarization       calculate_spin_polzn, mode = 5            (Polarization.cpp:25-263,
 *                                                                                EmissionFunction.cpp:1305-1310)
 *   is3d_sample / is3d_get_particles  sample_dN_pTdpTdphidy, operation = 2      (ParticleSampler.cpp:638-1134)
 *   is3d_sample_binned                ... with test_sampler = 1: the binned     (BinSampledParticle.cpp:9-133,
 *                                     distributions of the kept particles        ParticleSampler.cpp:1112-1121)
 *   is3d_sample_famod                 sample_dN_pTdpTdphidy_famod, df_mode 5    (ParticleSampler.cpp:1138-1627)
 *   is3d_set_decays / is3d_decay_feeddown   do_resonance_decays: no live reference routine (the key is read at
 *                                     EmissionFunction.cpp:204-205; src/cpp/jail/emissionfunction_resonance_decays.cpp
 *                                     is dead code): the decay feed-down of the spectra, defined in DESIGN.md 7.6
 *
 * Conventions: caller-owned host buffers in and out; the engine owns its HBM
 * buffers.  Errors are return codes (never exit()); is3d_last_error() gives the
 * message the reference would have printed before aborting.  One engine per
 * host thread per GPU; an engine is not re-entrant.  Output layout is the
 * reference's dN_pTdpTdphidy[ipart][ipT][iphi][iy] (MomentumSpectra.cpp:252-295).
 */
#ifndef IS3D_AMD_H
#define IS3D_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

#define IS3D_ABI_VERSION 5

enum {
  IS3D_OK = 0,
  IS3D_ERR_ARG = 1,          /* bad argument / inconsistent setup */
  IS3D_ERR_STATE = 2,        /* missing setup step */
  IS3D_ERR_DEVICE = 3,       /* HIP runtime error */
  IS3D_ERR_DF_RANGE = 4,     /* df coefficient spline/table evaluated out of range (reference: GSL abort / exit) */
  IS3D_ERR_UNSUPPORTED = 5   /* combination the reference rejects (e.g. PTB + baryon) */
};

typedef struct is3d_engine is3d_engine;

typedef struct {
  int operation;                  /* 1 continuous spectra, 0 spacetime distributions, 2 the particle sampler;
                                     informs the host facade -- each compute entry point fixes its own semantics */
  int dimension;                  /* 2 = boost-invariant (eta quadrature), 3 = 3+1d (y grid) */
  int df_mode;                    /* 1 Grad, 2 RTA-CE, 3 PTM, 4 PTB, 5 PTMA */
  int include_baryon;
  int include_bulk_deltaf;
  int include_shear_deltaf;
  int include_baryondiff_deltaf;
  int regulate_deltaf;
  int outflow;
  int famod_chains;               /* PTMA warm-start chains (= reference OpenMP thread count);
                                     0 = every cell solved independently (= threads >= cells) */
  double deta_min;
  double mass_pion0;
} is3d_params;

/* Freeze-out surface as structure-of-arrays, reference units after the reader's
 * conversion (GeV, fm): tau x y eta | dsigma_mu (covariant) | u^x u^y u^eta |
 * E T P | pi^xx pi^xy pi^xeta pi^yy pi^yeta | Pi | muB nB V^x V^y V^eta.
 * The baryon arrays may be NULL when include_baryon = 0.  (readindata.h:79-91) */
typedef struct {
  const double *tau, *x, *y, *eta;
  const double *dat, *dax, *day, *dan;
  const double *ux, *uy, *un;
  const double *E, *T, *P;
  const double *pixx, *pixy, *pixn, *piyy, *piyn;
  const double *bulkPi;
  const double *muB, *nB, *Vx, *Vy, *Vn;
} is3d_surface;

/* operation = 0 binning (iS3D_parameters.dat tau_min/tau_max/tau_bins, r_min/r_max/r_bins, phip_bins;
 * EmissionFunction.cpp:232-247).  threads = the reference's OpenMP thread count CORES:
 *   0      every species is binned from zero (the evident intent of the reference);
 *   C >= 1 reproduce a reference run with OMP_NUM_THREADS = C, whose per-species reset
 *          memset(all, 0, CORES * bins) clears BYTES, so thread-slice entries past the first
 *          CORES*bins/8 doubles carry the previous species' sums (SpacetimeDistribution.cpp:165-167). */
typedef struct {
  double tau_min, tau_max;
  int tau_bins;
  double r_min, r_max;
  int r_bins;
  int phip_bins;
  int threads;
} is3d_spacetime_bins;

typedef struct {
  long cells;                     /* cells processed in the last call */
  long breakdown;                 /* feqmod / famod breakdown cells */
  long pl_negative;               /* cells with p_L < 0 (p_L or p_T < 0 for PTMA) */
  long recon_fail;                /* PTMA reconstruction failures */
  long iterations;                /* PTMA total Newton iterations */
  double ms_prepass, ms_spectra, ms_total;   /* device time of the last call (HIP events) */
} is3d_stats;

int is3d_abi_version(void);
/* Build identity: a hash of the sources and compiler flags this library was built from (Makefile SRC_ID).
 * The committed rocprofv3 counter summaries (profiles/pmc_*.json) record it; bench.py reports their
 * roofline figures only for the identical build. */
const char *is3d_build_id(void);
is3d_engine *is3d_create(int device);
/* One engine over several GPUs of this process (the multi-GPU fan-out inside the compute
 * call).  Every setter goes to one engine per listed device; is3d_set_surface splits the cells into
 * contiguous windows of ~equal estimated cost (cells with u.dsigma <= 0 are nearly free); one
 * is3d_calculate_spectra / is3d_launch runs all devices concurrently and sums their spectra with one
 * RCCL ncclAllReduce (float64, sum) of the device-resident outputs -- or, when the list repeats a device,
 * with peer copies and a fixed-order add on devices[0].  is3d_launch's dev_out and stream belong to
 * devices[0].  PTMA with warm-start chains (famod_chains > 0): every device holds the whole surface and
 * walks the chains (set the params before the surface).  Replaces the reference's OpenMP fan-out
 * (MomentumSpectra.cpp:98-107) and its thread reduction (:383-411). */
is3d_engine *is3d_create_devices(int n_devices, const int *devices);
void is3d_destroy(is3d_engine *e);
const char *is3d_last_error(const is3d_engine *e);

int is3d_set_params(is3d_engine *e, const is3d_params *p);
/* Engine tuning knobs (no reference counterpart; a device-list engine forwards them to every shard).
 *   "phitab_one_bytes"    F_TS scalar tables (Grad / RTA-CE, one phi block) of the whole window up to this size are
 *                         written and integrated in one chunk (default 8 GiB)
 *   "phitab_chunk_bytes"  larger ones in chunks of whole cell splits of about this size, alternating over two streams
 *                         (default 2 GiB; BASELINE config 4 runs 29 chunks)
 *   "max_splits"          cap on k_spectra's cell splits, one output-sized partial slab each (default 1024)
 *   "slab_bytes"          cap on those slabs' memory (default 48 GiB; also at most half the device's free memory)
 *   "split_bytes"         record bytes per cell split the plan aims for (default 512 KiB: a split stays in an XCD's L2)
 *   "sample_bytes"        bound on the working buffers of one is3d_sample batch of events (default 1 GiB)
 * A negative value restores the default.  is3d_get_tuning also reads "phitab_chunks": the F_TS chunks of the last
 * launch (0: not an F_TS launch), "splits": the cell splits of the last launch, and "slabs": the output-sized partial
 * slabs it held (several 3+1D F_TS chunks fold theirs into one accumulator as they finish: 1 + 2 x splits per chunk);
 * -1 = unknown key. */
int is3d_set_tuning(is3d_engine *e, const char *key, long value);
long is3d_get_tuning(const is3d_engine *e, const char *key);
int is3d_set_species(is3d_engine *e, int n, const double *mass, const double *sign,
                     const double *degeneracy, const double *baryon);
/* Integrand classes (no reference counterpart: an engine option, default on).  The momentum integrals see a
 * species only through its (mass, sign, baryon) -- and, for PTM, its degeneracy, which enters the
 * renormalisation (MomentumSpectra.cpp:800-808) -- while the degeneracy multiplies the result
 * (MomentumSpectra.cpp:365).  With classes on, chosen species with identical keys are integrated once and the
 * reduction writes every member (prefactor x its degeneracy x the shared cell sum): the spectra are
 * equal to rounding (< 1e-9 relative, tests/test_gpu_classes.py) to integrating each species separately (on = 0):
 * the two launches group different lanes into their wavefronts and can pick other cell splits, and they are
 * bit-identical only when the per-wavefront Boltzmann-tail decisions coincide as well.
 * is3d_species_integrated counts the integrand classes under that documented key (SMASH 444 -> 193, UrQMD 305 -> 124;
 * the species count with classes off), whatever the run's flags.
 * The kernels integrate the *lane classes*, which is3d_lanes_integrated counts.  They are the integrand classes, or
 * fewer when the run is baryon-blind: with include_baryon = 0 the baryon number of a species multiplies only per-cell
 * quantities that are zero (alphaB, V^mu, and the delta-f coefficients c1 / G, which the engine checks to be zero on
 * the table row such a run uses), so a baryon and its antibaryon of equal (mass, sign) are one integrand and share a
 * lane (SMASH 193 -> 135, UrQMD 124 -> 75); the reduction writes every member with its own degeneracy.  With
 * include_baryon = 1, a table that fails the check, or classes off, the two counts are equal.
 * Both return minus an IS3D_ERR_* code when the tables cannot be finalised (is3d_last_error says why). */
int is3d_set_species_classes(is3d_engine *e, int on);
int is3d_species_integrated(is3d_engine *e);
int is3d_lanes_integrated(is3d_engine *e);
int is3d_set_pdg(is3d_engine *e, int n, const double *mass, const double *sign,
                 const double *degeneracy, const double *baryon);
int is3d_set_momentum_grid(is3d_engine *e, int npT, const double *pT, int nphi, const double *phi,
                           int ny, const double *y, int neta, const double *eta, const double *eta_weight);
/* roots/weights[alpha][points], as in tables/gauss/gla_roots_weights.txt */
int is3d_set_gauss_laguerre(is3d_engine *e, int alpha, int points, const double *roots, const double *weights);
/* tables[10][nmuB][nT] in file order c0 c1 c2 c3 c4 F G betabulk betaV betapi;
 * T_avg = Plasma::temperature (surface average after the 15-digit file round trip),
 * used only for the PTB (Jonah) table. */
int is3d_set_df_tables(is3d_engine *e, int nT, int nmuB, const double *T, const double *muB,
                       const double *tables, double T_avg);

/* Copies n_cells cells (host pointers) into engine-owned HBM. */
int is3d_set_surface(is3d_engine *e, long n_cells, const is3d_surface *s);
/* Same, but the 25 field arrays are already in device memory on the engine's GPU
 * (field-major: dev[f * n_cells + c], f in is3d_surface order).  Not copied. */
int is3d_set_surface_device(is3d_engine *e, long n_cells, const double *dev_fields);

/* Integrate only cells [lo, hi) of the surface set last (lo = hi = -1: every cell; setting a surface clears
 * it).  For one process per GPU: every rank holds the whole surface and integrates its window; the PTMA
 * warm-start chains (famod_chains > 0) still walk every cell, so each window sees the serial chain's
 * solutions (MomentumSpectra.cpp:1308-1364), which cell shards could not. */
int is3d_set_cell_window(is3d_engine *e, long lo, long hi);

/* Estimated k_spectra cost of every cell of the surface set last, relative to a live cell of the mode's main
 * launch (no reference counterpart: the shard cost model of SURVEY.md 8(e), used by is3d_create_devices' windows
 * and by one-process-per-GPU callers): 0.02 for u.dsigma <= 0 (skipped by every kernel,
 * MomentumSpectra.cpp:132; its record prep only); PTM / PTB cells that break down or have narrow rapidity
 * windows take the separable fallback launch (MomentumSpectra.cpp:863-929) at 1.4 / 1.8 (measured on MI355X,
 * tools/fb_cost_probe.py); every other cell 1 (PTMA's breakdowns are only known after its Newton solves).
 * Runs the record prepass on the engine's GPU (synchronous); cost holds n_cells doubles. */
int is3d_cell_costs(is3d_engine *e, double *cost);

/* PTMA warm-start chains split over processes (one process per GPU; SURVEY.md 8(e) "partition by chain and keep
 * chain order").  The reference warm-starts each Newton solve from the previous successful cell of its OpenMP thread
 * (MomentumSpectra.cpp:1132-1135, 1308-1364): chain c = cells c, c + C, c + 2C, ... with C = famod_chains.  Every
 * process holds the whole surface; is3d_set_chain_range(e, q0, q1) makes this engine solve chain positions
 * [q0, q1) of every chain and integrate cells [q0 C, min(n, q1 C)) (q0 = q1 = -1: off; setting a surface or a cell
 * window clears it).  The staged launch then lets the caller move the boundary states between processes:
 *   is3d_launch_begin                        prepass of the range (on `stream`)
 *   for pass j < is3d_chain_passes(e):
 *     [q0 > 0, j > 0]  is3d_chain_boundary_put(e, (j - 1) & 1, buf)   the predecessor's pass j - 1 end states
 *     is3d_chain_pass(e, j)
 *     [successor]      is3d_chain_boundary_get(e, j & 1, buf)         this range's pass j end states, to send
 *   [q0 > 0]  is3d_chain_boundary_put(e, 2, buf)   the predecessor's final states (after its is3d_chain_end)
 *   is3d_chain_end(e)
 *   [successor]  is3d_chain_boundary_get(e, 2, buf)
 *   is3d_launch_end(e)   ...   is3d_finish(e)
 * Buffers hold is3d_chain_boundary_size(e) doubles, in device memory (or host memory: the copies are asynchronous
 * on the launch stream, so the caller synchronises it before reading a host buffer it got).
 * At the fixed point each range's solutions are the one-chain solutions bit for bit (engine_kernels.h k_chain_pass), so
 * the per-process Newton iteration counts (is3d_get_stats) add up to the serial chain's.  is3d_launch refuses an
 * engine with a chain range. */
int is3d_set_chain_range(is3d_engine *e, long q0, long q1);
int is3d_launch_begin(is3d_engine *e, double *dev_out, void *stream);
int is3d_chain_passes(const is3d_engine *e);
int is3d_chain_pass(is3d_engine *e, int pass);
int is3d_chain_end(is3d_engine *e);
int is3d_launch_end(is3d_engine *e);
long is3d_chain_boundary_size(const is3d_engine *e);
int is3d_chain_boundary_get(is3d_engine *e, int slot, double *dev_buf);
int is3d_chain_boundary_put(is3d_engine *e, int slot, const double *dev_buf);

/* Full call: kernels + device->host copy of dN/(pT dpT dphi dy) into dN_out. */
int is3d_calculate_spectra(is3d_engine *e, double *dN_out);

/* Split call for resident benchmarking / multi-GPU reduction: launch the whole
 * hot path on `stream` (a hipStream_t, NULL = default) writing the spectra into
 * the device buffer dev_out (npart*npT*nphi*ny doubles on the engine's GPU);
 * is3d_finish() synchronises and reports device-side errors. */
int is3d_launch(is3d_engine *e, double *dev_out, void *stream);
int is3d_finish(is3d_engine *e);
int is3d_get_stats(const is3d_engine *e, is3d_stats *out);
long is3d_output_size(const is3d_engine *e);

/* operation = 0, spacetime distributions dN/dX (EmissionFunction.cpp:1165-1196 ->
 * calculate_dN_dX / calculate_dN_dX_feqmod, SpacetimeDistribution.cpp:31-1250; df_mode 1-4, PTMA is
 * rejected as in the reference).  Needs the pT / phi quadrature weights (Table column 2) and the bins.
 * Outputs [species][bins] are the values the reference writes to results/continuous/dN_taudtaudy_<MCID>.dat,
 * dN_2pirdrdy_<MCID>.dat and dN_dphidy_<MCID>.dat (already divided by tau dtau, 2 pi r dr, dphi). */
int is3d_set_momentum_weights(is3d_engine *e, const double *pT_weight, const double *phi_weight);
int is3d_set_spacetime_bins(is3d_engine *e, const is3d_spacetime_bins *bins);
int is3d_calculate_dN_dX(is3d_engine *e, double *dN_taudtaudy, double *dN_2pirdrdy, double *dN_dphidy);
/* operation = 0 for df_mode 5 (PTMA).  The reference has no routine (it prints "no spacetime distribution routine for
 * famod yet" and exits, EmissionFunction.cpp:1184-1189; is3d_calculate_dN_dX returns that sentence as
 * IS3D_ERR_UNSUPPORTED), so this entry defines one: dN_dy_cell[s][c] is cell c's term of
 * calculate_dN_pTdpTdphidy_famod (MomentumSpectra.cpp:1517-1621) folded with the pT / phi weights and summed over the
 * y table (3+1D) or taken at y = 0 over the eta nodes with their weights (2+1D), so that
 *   sum_c dN_dy_cell[s][c] = sum_ipT,iphi,iy w_pT w_phi dN_pTdpTdphidy[s][ipT][iphi][iy]
 * holds to rounding against is3d_calculate_spectra; the (lambda, aT, aL) of a cell are the spectra's (their chain rule,
 * famod_chains as for the spectra).  Bins, thread slices, the per-species reset and the normalisation are
 * is3d_calculate_dN_dX's.  is3d_get_cell_yields works after it; is3d_get_stats carries the breakdown cells and the
 * Newton iterations.  Every call solves the chains again.  Honours is3d_set_cell_window as the spectra do (the chains
 * walk every cell, the arrays and is3d_get_cell_yields' [species][hi - lo] cover the window); a chain range
 * (is3d_set_chain_range) is refused.  df_mode 1-4: IS3D_ERR_UNSUPPORTED (is3d_calculate_dN_dX). */
int is3d_calculate_dN_dX_famod(is3d_engine *e, double *dN_taudtaudy, double *dN_2pirdrdy, double *dN_dphidy);
/* dN_dy_cell[species][cell] of the last is3d_calculate_dN_dX / is3d_calculate_dN_dX_famod call
 * (SpacetimeDistribution.cpp:374). */
int is3d_get_cell_yields(const is3d_engine *e, double *dN_dy_cell);

/* Test hooks mirroring reference services. out[15] = c0 c1 c2 c3 c4 shear14 F G
 * betabulk betaV betapi lambda z delta_lambda delta_z (evaluated on the GPU). */
int is3d_evaluate_df_coefficients(is3d_engine *e, double T, double muB, double E, double P,
                                  double bulkPi, double *out15);
/* The ten delta-f coefficient tables of the PDG list on a (T, muB) grid, computed on the GPU: the reference's offline
 * generator (generate_delta_f_coefficients/<list>/df_vh_dimensionless: deltaf_table.cpp, thermal_integrands.cpp,
 * gauss_integration.cpp) with its prefactors, its closing algebra ("update 3/25" bulk form, alphaB form of G, F and
 * betabulk, hbarc = 0.197327053) and its scaling by powers of T, so that the shipped files are these values rounded to
 * six decimals.
 * tables[10][nmuB][nT] in the order of is3d_set_df_tables, from the PDG set with is3d_set_pdg and the
 * Gauss-Laguerre table set with is3d_set_gauss_laguerre (alpha >= 5: rows 1..4 are used).
 * Reads engine inputs only: it installs nothing and invalidates nothing; pass the result to is3d_set_df_tables.
 * A value is a pure function of (PDG list, Gauss-Laguerre table, T, muB): repeats and other grids holding the same
 * point give the same bits.  A device-list engine runs it on devices[0].
 * Errors: IS3D_ERR_STATE without a PDG or with fewer than five Gauss-Laguerre rows; IS3D_ERR_ARG for a null pointer,
 * nT < 1, nmuB < 1, T <= 0 or a grid that is not strictly ascending; IS3D_ERR_DF_RANGE when a value is not finite or
 * one of the reference's exit(-1) checks fires -- is3d_last_error then holds the reference's message ("Bulk
 * denominator is zero", "Diffusion denominator is zero", "Shear denominator is zero") and the first (T, muB) it
 * occurs at, in the reference's loop order; a list without baryons is such a case. */
int is3d_generate_df_tables(is3d_engine *e, int nT, int nmuB, const double *T, const double *muB, double *tables);
/* out[5] = T, E, P, muB, nB averages (after the setprecision(15) round trip). */
int is3d_surface_averages(long n_cells, const is3d_surface *s, int include_baryon, double *out5);
/* Jonah table the engine built: lambda^2, z, bulkPi/P (301 each) and the max. */
/* operation = 2 oversampling estimate: the reference's Ntotal (ParticleSampler.cpp:447-636
 * calculate_total_yield, EmissionFunction.cpp:1237-1242), with the per-species densities of
 * Deltaf_Data::compute_particle_densities (DeltafData.cpp:555-690) evaluated on the device at the
 * Plasma averages plasma = (T, E, P, muB, nB) (is3d_surface_averages).  Like the reference, the
 * densities use the alpha = 1, 2, 3 rows of tables/gauss/gla_roots_weights.txt: set that 32-point
 * table with is3d_set_gauss_laguerre.  2+1D: multiplied by 2 y_cut.  densities (optional, [3][npart]):
 * equilibrium, bulk and diffusion densities of the chosen species.  Nevents =
 * min(ceil(min_num_hadrons / Ntotal), max_num_samples) is the caller's (EmissionFunction.cpp:1242). */
int is3d_total_yield(is3d_engine *e, const double *plasma, double y_cut, double *n_total, double *densities);

int is3d_get_jonah_table(const is3d_engine *e, double *lambda2, double *z, double *bulk_over_P,
                         double *bulk_over_P_max);

/* mode = 5, spin polarization from thermal vorticity (EmissionFunctionArray::calculate_spin_polzn,
 * Polarization.cpp:25-263, run after the chosen operation at EmissionFunction.cpp:1305-1310).  The six
 * thermal-vorticity components wbar^{tx ty tn xy xn yn} of every cell are the last six columns of a mode-5
 * input/surface.dat (no unit conversion, readindata.cpp:298-306); host pointers, copied.  Set them after the
 * surface: n_cells must equal the surface's, and setting a surface again clears them.
 * S_out[c][ipart][ipT][iphi][iy], c = 0..4: the raw cell sums S_t, S_x, S_y, S_n, Snorm of the reference (the files
 * hold S_c / Snorm), each in the spectra layout; 2+1D: one y = 0 slot, summed over the eta table with weights
 * eta_weight x (eta_2 - eta_1) as in the reference.  T_avg = Plasma::temperature: one temperature for the whole
 * surface, no chemical potential, no degeneracy, no (2 pi hbarc)^-3, every cell counted (no u.dsigma test).
 * Needs params (dimension), species, momentum grid, surface and vorticity -- no delta-f tables, Gauss-Laguerre
 * table or PDG set.  Honours is3d_set_cell_window, is3d_set_species_classes (classes by (mass, sign)) and the
 * "max_splits" / "split_bytes" / "slab_bytes" knobs; sums in a fixed order (bit-reproducible).
 * Two deliberate departures from the reference: the vorticity is indexed by the global cell (Polarization.cpp:131-136
 * uses the index inside its 10 000-cell chunk: identical up to 10 000 cells), and the layout above is the one the
 * row labels of the reference's files name (its writer, EmissionFunction.cpp:591, reads another index than its loop
 * filled).  Errors: IS3D_ERR_STATE for a missing setup step, IS3D_ERR_ARG for T_avg <= 0 or a vorticity length
 * other than the surface's.  is3d_launch_polarization + is3d_finish is the resident form (dev_out: device buffer of
 * is3d_polarization_size doubles); is3d_get_stats then holds the cells and device times of the call. */
typedef struct { const double *wtx, *wty, *wtn, *wxy, *wxn, *wyn; } is3d_vorticity;
int is3d_set_vorticity(is3d_engine *e, long n_cells, const is3d_vorticity *w);
long is3d_polarization_size(const is3d_engine *e);      /* 5 * is3d_output_size */
int is3d_calculate_polarization(is3d_engine *e, double T_avg, double *S_out);
int is3d_launch_polarization(is3d_engine *e, double T_avg, double *dev_out, void *stream);

/* operation = 2, the particle sampler (EmissionFunctionArray::sample_dN_pTdpTdphidy, ParticleSampler.cpp:638-1134):
 * df_mode 1-4, 2+1D and 3+1D, fast = 0 / 1, with and without baryon diffusion, n_events >= 1 sampled events.
 * plasma = (T, E, P, muB, nB) averages (is3d_surface_averages), used by fast = 1: the species weights come from the
 * Plasma-average densities of is3d_total_yield and PTM's breakdown test from the average temperature.  Needs what
 * is3d_total_yield needs (params, species, df tables, the 32-point Gauss-Laguerre table, a surface); honours
 * is3d_set_cell_window; a device-list engine samples each shard's window and concatenates the shard lists per event.
 *
 * Random numbers: Philox4x32-10; the stream of every draw is a pure function of (seed, purpose, global cell index,
 * event, candidate index, draw counter) with the reference's four purposes (poisson, type, momentum, rapidity), so
 * the list is bit-identical for every launch geometry, event batch, cell window split and number of shards -- that
 * replaces the reference's "same seed, same list" (its serial std::default_random_engine stream is not reproduced).
 * The engine takes a non-negative seed; the reference's "seed < 0: take the clock" is the host layer's.
 * The Poisson draw is exact (inversion over equal parts of the mean of at most 16).  The momentum rejection loop and
 * the Poisson search are capped; a candidate that reaches a cap is dropped and counted in `capped` (0 in practice).
 *
 * Output: within an event particles are ordered by (cell, candidate index) -- the reference's loop order -- and
 * events are contiguous: offsets[n_events + 1].  The list stays in the engine until the next is3d_sample /
 * is3d_destroy; is3d_sample_count and is3d_sample_offsets read its size, is3d_get_particles copies records
 * [first, first + count) into caller-owned memory.  `species` is the index into the chosen species (the caller maps
 * it to an MCID), `cell` the global cell index.
 *
 * Memory: the working buffers of one batch of events (12 bytes per (event, cell) plus 204 per candidate) stay below
 * the "sample_bytes" knob of is3d_set_tuning (default 1 GiB); the batches do not change the result.  One event that
 * alone exceeds the bound is sampled in batches of cells; a single (cell, event) that exceeds it is an error
 * (IS3D_ERR_ARG with the size needed), never a truncation.  is3d_get_tuning("sample_batches") is the number of
 * batches of the last call.
 *
 * df_mode 5 has a method of its own, as in the reference (EmissionFunction.cpp:1255-1275): is3d_sample and
 * is3d_sample_binned return IS3D_ERR_UNSUPPORTED for it, is3d_sample_famod (below) samples it.  Not covered: bit
 * parity with the reference's serial random stream.  Errors: IS3D_ERR_STATE for a missing setup step, IS3D_ERR_ARG for n_events < 1,
 * y_cut <= 0 or a negative seed, IS3D_ERR_DF_RANGE as elsewhere. */
typedef struct {
  long seed;                      /* >= 0 */
  int n_events;                   /* >= 1 */
  int fast;                       /* 1: species weights from the Plasma-average densities */
  double y_cut;                   /* 2+1D: rapidity window [-y_cut, y_cut) and volume factor 2 y_cut; 3+1D: unused (> 0) */
} is3d_sample_params;
typedef struct {                  /* 96 bytes */
  int species;
  int event;
  long cell;
  double tau, x, y, eta, t, z, E, px, py, pz;
} is3d_particle;
typedef struct {
  long cells;                     /* cells of the window */
  long breakdown;                 /* PTM / PTB cells that fall back to the linear delta-f */
  long candidates;                /* Poisson candidates over all events */
  long kept;                      /* particles in the list */
  long proposals, acceptances;    /* momentum rejection loop (the reference prints acceptances / proposals) */
  long capped;                    /* candidates dropped at an iteration cap (expected 0) */
  long clamped;                   /* linear delta-f corrections cut to [-1, 1] */
  long batches;                   /* memory-bound batches the call ran */
} is3d_sample_stats;
int is3d_sample(is3d_engine *e, const is3d_sample_params *p, const double *plasma);
long is3d_sample_count(const is3d_engine *e);
int is3d_sample_offsets(const is3d_engine *e, long *offsets);
int is3d_get_particles(const is3d_engine *e, long first, long count, is3d_particle *out);
int is3d_get_sample_stats(const is3d_engine *e, is3d_sample_stats *out);

/* test_sampler = 1: the sampler bins every kept particle on the device (BinSampledParticle.cpp:9-133) instead of --
 * keep_list = 0 -- or next to -- keep_list = 1 -- listing it.  is3d_set_sample_bins takes the reference's bin
 * parameters (widths as EmissionFunction.cpp:223-247: (max - min) / bins, 2 cut / bins, 2 pi / bins); y_cut is the
 * binning window of dN_dy (in 2+1D pass the sampler's y_cut).  A particle outside a histogram's range is dropped from
 * that histogram only.  Rapidity is 0.5 log((E + pz) / (E - pz)) in 3+1D and the drawn rapidity in 2+1D; eta is the
 * particle record's.
 *
 * is3d_sample_binned samples like is3d_sample (same arguments, streams, cell window, device list, errors) and leaves
 * the histograms in the engine until the next sampling call:
 *   counts  one block of n_counts integers, each part [npart][bins] in chosen-species order:
 *           dN_dy | dN_deta | dN_dphipdy | pT | tau | r | phis          (the pT part is both dN_2pipTdpTdy_count
 *           and pT_count of the reference; phis uses phip_bins)
 *   vn      n_vn = 2 x 7 x npart x pT_bins doubles, [2][7][npart][pT_bins]: the sums of cos(k phi), then of sin(k phi),
 *           k = 1..7, over the particles of a pT bin.  Raw sums: the normalisation belongs to the writer.
 * The counts are exact.  The vn sums are accumulated in fixed point -- every term rounded to a multiple of
 * q = 2^-32 and added as a 64-bit integer, converted to double once -- so they carry at most q / 2 per particle and,
 * like the counts, are bit-identical for every event batch, cell batch, cell window split, launch geometry and number
 * of shards (a device-list engine adds its shards' integer histograms).  A bin holds up to 2^31 particles.
 *
 * keep_list = 0: no candidate slots, no compaction, no list -- a batch needs 12 bytes per (event, cell) whatever the
 * number of candidates, so no (cell, event) can exceed "sample_bytes"; is3d_sample_count is 0, the offsets are 0 and
 * is3d_get_sample_stats holds the true candidates, kept, ... and batches.  keep_list = 1: the list entry points
 * behave exactly as after is3d_sample with the same arguments.
 *
 * Errors: IS3D_ERR_STATE when no bins are set; is3d_set_sample_bins: IS3D_ERR_ARG for a bin count < 1, a max <= min or
 * a cut <= 0; IS3D_ERR_UNSUPPORTED for df_mode 5; otherwise what is3d_sample returns.  is3d_sample_hist_size returns
 * n_counts + n_vn (either pointer may be null), -1 before the bins and the species are set. */
typedef struct {
  double pT_min, pT_max;   int pT_bins;
  double y_cut;            int y_bins;
  int phip_bins;
  double eta_cut;          int eta_bins;
  double tau_min, tau_max; int tau_bins;
  double r_min, r_max;     int r_bins;
} is3d_sample_bins;
int is3d_set_sample_bins(is3d_engine *e, const is3d_sample_bins *b);
int is3d_sample_binned(is3d_engine *e, const is3d_sample_params *p, const double *plasma, int keep_list);
long is3d_sample_hist_size(const is3d_engine *e, long *n_counts, long *n_vn);
int is3d_get_sample_hist(const is3d_engine *e, long *counts, double *vn);
/* Test hook: the first n uniforms in [0, 1) of the stream (seed, purpose 0 poisson / 1 type / 2 momentum /
 * 3 rapidity, cell, event, candidate), generated on the device (tests compare them with sampler_math.h on the host). */
int is3d_sample_uniforms(is3d_engine *e, long seed, int purpose, long cell, long event, long candidate, int n, double *out);

/* df_mode 5 (PTMA): sample_dN_pTdpTdphidy_famod (ParticleSampler.cpp:1138-1627).  binned = 0: the list (as
 * is3d_sample); 1: binned only, 2: binned with the list (as is3d_sample_binned with keep_list = 0 / 1; both need
 * is3d_set_sample_bins).  The method uses no Plasma averages and has no fast branch: p->fast is ignored.  Results
 * come through the getters above (is3d_sample_count / _offsets, is3d_get_particles, is3d_get_sample_stats,
 * is3d_get_sample_hist); streams, order, batches, cell window and device list behave as for is3d_sample.
 *
 * Each call first reconstructs (lambda, aT, aL) of every cell along the reference's serial chain under the sampler's
 * rule (:1330-1399: unlike the spectra's, a failed cold solve with no previous success breaks the cell down and counts
 * a failure).  famod_chains means what it means for the spectra: C >= 1 strided chains (1: the reference's loop), each
 * walking every cell of the surface whatever cell window is sampled; 0: every cell cold.  A device-list engine with
 * famod_chains > 0 solves the whole chain on every shard, with 0 each shard solves its window.  A broken-down cell
 * (pl or pt < 0, a failed reconstruction, det B <= deta_min) samples feq at the (lambda, aT, aL) it ends with, B = 1;
 * is3d_sample_stats.breakdown counts the live ones of the window.  The species weights carry the reference's
 * exp(Ebar + chem) (:1493).  is3d_get_sample_famod_stats: the counters of the reference's closing lines, over the
 * cells the reconstruction covered (the surface; the cell window when famod_chains = 0).
 *
 * Errors: IS3D_ERR_STATE when df_mode is not 5, no PDG table is set, no bins are set for binned != 0, or a chain
 * range (is3d_set_chain_range) is set; otherwise the argument and budget errors of is3d_sample. */
typedef struct {
  long plpt_negative;             /* cells with pl < 0 or pt < 0 */
  long reconstruction_fail;       /* failed reconstructions, the sampler's rule */
  long iterations;                /* Newton iterations */
} is3d_sample_famod_stats;
int is3d_sample_famod(is3d_engine *e, const is3d_sample_params *p, int binned);
int is3d_get_sample_famod_stats(const is3d_engine *e, is3d_sample_famod_stats *out);

/* do_resonance_decays: feed-down of the continuous spectra from resonance decays.  The reference reads the key
 * (EmissionFunction.cpp:204-205) but has no working routine (src/cpp/jail/emissionfunction_resonance_decays.cpp is in
 * no makefile and starts with exit(-1)); the method here is defined in is3d2_amd/csrc/decay_math.h and DESIGN.md 7.6
 * (Sollfrank, Koch and Heinz, Z. Phys. C 52 (1991) 593; 2- and 3-body channels, 12-point Gauss-Legendre rules).
 *
 * is3d_set_decays takes the channel table (after the species and the momentum grid; setting either again clears it):
 * parent and daughter[] are indices into the chosen species (-1: a daughter that is not chosen receives nothing),
 * masses and widths in GeV (the widths only open closed 2-body channels, the jail file's rule :239-256).  1-body rows
 * (the stability marker) are ignored; rows with >= 4 bodies and closed channels are skipped and counted.
 * is3d_set_decays4 takes the same table in rows of four daughter slots and replaces the plan exactly as is3d_set_decays
 * does (same state rules, same errors, same device-list path), but keeps open 4-body channels too: the feed-down of a
 * slot is the flat four-body marginal of the invariant mass^2 recoiling against it, a 12-node rule like the 3-body
 * one (decay_math.h), and the list decays below draw flat four-body phase space (decay_mc_math.h).  After it `kept`
 * includes the open 4-body channels, skipped_many_body counts the rows with >= 5 bodies and a 4-body row that is not
 * open counts in skipped_closed (the width adjustment stays a 2-body rule).
 * is3d_decay_feeddown updates a host array in the spectra layout [species][pT][phi][y] in place (any such array, not
 * only the last is3d_calculate_spectra result): every species then holds thermal + feed-down; a decaying parent keeps
 * its own spectrum.  is3d_launch_feeddown is the resident form (dev_inout on the engine's GPU, is3d_finish
 * synchronises).  Every output element sums its terms in a fixed order: the result is bit-identical across repeats
 * and does not depend on the order the channels were listed in.  A device-list engine runs it on devices[0].
 * Errors: IS3D_ERR_STATE when no decays / species / grid / params are set; IS3D_ERR_ARG for a pT <= 0 or a pT table that
 * is not ascending, a phi table that is not ascending in [0, 2 pi), an index out of range, n_body < 1, a cycle. */
typedef struct {
  int parent;
  int n_body;
  int daughter[3];                /* chosen index, -1: not a chosen species */
  double branching, mass_parent, width_parent, mass[3], width[3];
} is3d_decay_channel;
typedef struct {
  int parent;
  int n_body;
  int daughter[4];                /* chosen index, -1: not a chosen species */
  double branching, mass_parent, width_parent, mass[4], width[4];
} is3d_decay_channel4;
typedef struct {
  long channels;                  /* rows given */
  long kept;                      /* open 2- and 3-body channels (is3d_set_decays4: and 4-body channels) */
  long skipped_many_body;         /* rows with >= 4 bodies (is3d_set_decays4: >= 5 bodies) */
  long skipped_closed;            /* closed 3-body (and 4-body) channels, 2-body channels the mass adjustment cannot open */
  long adjusted;                  /* 2-body channels the mass adjustment opened (among kept) */
  long levels;                    /* topological levels = launches */
  double branching_skipped;       /* summed branching of the skipped rows (many-body and closed) */
  double ms_total;                /* device time of the last feed-down (HIP events) */
} is3d_decay_stats;
int is3d_set_decays(is3d_engine *e, int n, const is3d_decay_channel *channels);
int is3d_set_decays4(is3d_engine *e, int n, const is3d_decay_channel4 *channels);
int is3d_decay_feeddown(is3d_engine *e, double *dN_inout);
int is3d_launch_feeddown(is3d_engine *e, double *dev_inout, void *stream);
int is3d_get_decay_stats(const is3d_engine *e, is3d_decay_stats *out);

/* do_resonance_decays for operation = 2: Monte Carlo decays of a particle list, the counterpart of the feed-down above
 * with the same channel plan (is3d_set_decays; method in is3d2_amd/csrc/decay_mc_math.h and DESIGN.md 7.7).  Every
 * particle whose species has a kept channel decays down its chains on the GPU: 2-body isotropic, 3-body flat Dalitz,
 * 4-body (is3d_set_decays4) flat four-body phase space;
 * zero lifetime, so daughters inherit the parent's position and cell; a daughter that is not a chosen species (-1) is
 * dropped and counted.  A particle stays in the list as a residual when the channel draw falls on the branching of
 * skipped rows (counted in undecayed) or a 3- or 4-body rejection loop reaches its cap (capped).  Primaries keep their
 * order; each is replaced by its leaves in depth-first daughter-slot order.  The list is a pure function of (seed,
 * input list): bit-identical for every "sample_bytes" batching, and for a sub-range of events decayed alone.
 *
 * is3d_decay_particles decays a caller's list in[offsets[0] .. offsets[n_events]): event k is in[offsets[k] ..
 * offsets[k + 1]), its records carry one value of `event`, and that value increases from one non-empty event to the next
 * (two events with one value would share their random streams).
 * is3d_decay_sampled decays the engine's last sampled list (is3d_sample, is3d_sample_binned with keep_list = 1,
 * is3d_sample_famod with binned = 0 or 2) in place of it.  After either call is3d_sample_count, is3d_sample_offsets
 * and is3d_get_particles return the decayed list and is3d_get_particle_origins the index, in the input list, of the
 * primary each record descends from.  bin = 1 (needs is3d_set_sample_bins): is3d_get_sample_hist then returns the
 * histograms of the decayed list; the rapidity binned is 0.5 log((E + pz) / (E - pz)) in both dimensions.
 * A device-list engine runs the call on devices[0] over the merged list.
 * Errors: IS3D_ERR_STATE without is3d_set_decays, without a sampled list (is3d_decay_sampled), or without bins for
 * bin = 1; IS3D_ERR_ARG for a negative seed, a species index out of range, events that are not contiguous and
 * increasing, a plan of more than 16 levels (15 when it holds a 4-body channel), an event of 2^32 or more primaries, or a primary whose decay
 * products alone exceed the "sample_bytes" bound (with the size needed). */
typedef struct {
  long primaries, decays, undecayed, dropped_daughters, capped, final_particles, passes, batches;
  double ms_total;                /* device time, HIP events: every batch attempt, the halved ones included */
} is3d_decay_list_stats;
int is3d_decay_particles(is3d_engine *e, long seed, int n_events, const long *offsets, const is3d_particle *in, int bin);
int is3d_decay_sampled(is3d_engine *e, long seed, int bin);
int is3d_get_particle_origins(const is3d_engine *e, long first, long count, long *origin);
int is3d_get_decay_list_stats(const is3d_engine *e, is3d_decay_list_stats *out);

/* Sample and decay in one device-resident pass: every compacted batch of the sampler is decayed where
 * it lies, so no primary is downloaded or uploaded.  The result is, byte for byte, that of the two calls above:
 * is3d_sample (df_mode 1-4) or is3d_sample_famod(.., 0) (df_mode 5: plasma and p->fast are ignored, plasma may be
 * null, and is3d_get_sample_famod_stats is valid afterwards) followed by is3d_decay_sampled(e, decay_seed, bin).
 *   list = 1: is3d_sample_count, is3d_sample_offsets, is3d_get_particles and is3d_get_particle_origins return the
 *     decayed list (origins index the primary list the two calls would have held), is3d_get_sample_hist the
 *     histograms of the final hadrons when bin = 1, and both stats getters their values; only `batches` and
 *     `ms_total` of the stats depend on how the work was cut.
 *   list = 0, bin = 1: the histograms of the final hadrons only.  No particle record reaches the host: the count and
 *     the offsets are 0 as after a binned-only sample, is3d_get_particle_origins accepts only count = 0, and the
 *     sample stats and the decay-list stats are the true ones.
 * The sampler plans its batches within half of "sample_bytes" and the decay stage's records take the rest; a batch
 * whose products need more is decayed in sub-ranges (halved, never sampled again).  No bound changes the result.
 * is3d_get_tuning(e, "list_h2d_bytes") / "list_d2h_bytes": the bytes of particle records, stream keys and origins
 * that the last sampling or list-decay call (this one, or any of those above) copied to / from the device.
 * A device-list engine runs the two-call sequence underneath (the shards sample, the merged list decays on
 * devices[0]); decaying per shard is out of scope, since a primary's index inside its event depends on the other
 * shards' counts.
 * Errors: IS3D_ERR_ARG for list = 0 and bin = 0; IS3D_ERR_STATE without is3d_set_decays or, for bin = 1, without bins;
 * otherwise the errors of the two calls it replaces.  A failed call leaves no list (is3d_sample_count is -1). */
int is3d_sample_decayed(is3d_engine *e, const is3d_sample_params *p, const double *plasma, long decay_seed, int list,
                        int bin);

#ifdef __cplusplus
}
#endif
#endif
