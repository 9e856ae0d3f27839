// engine.hip -- MI355X (gfx950) Cooper-Frye continuous-spectra engine behind the
// C ABI of include/is3d_amd.h.  This file is the host side; the kernels named below are in engine_kernels.h (the
// prepass, the reductions, operations 0 and 2) and kernels.h (the momentum integrals).
//
// Hot path (reference MomentumSpectra.cpp:32-1682, dispatched from
// EmissionFunction.cpp:1198-1226):
//   k_prep_*      one thread per freeze-out cell: u^tau, pi^{mu nu} reconstruction,
//                 delta-f coefficients (GSL-equivalent spline / bilinear table on
//                 device), LRF basis, A^{-1} (PTM/PTB), breakdown tests -> cell record
//   k_aniso       PTMA only: one wavefront per warm-start chain (or per cell),
//                 Newton solve for (lambda, aT, aL) + famod coefficients
//   k_renorm      PTM only: per (cell, species) renormalisation n_linear / n_mod
//   k_spectra     the (cell x species x pT x phi x y [x eta]) integral: workgroup =
//                 one pT value x 256 (species, y) lanes x a cell range; each lane keeps
//                 32 phi accumulators in VGPRs; per cell tile the per-(cell,phi) and
//                 per-(cell,y/eta) factors are built cooperatively in LDS (see
//                 cf_math.h for the factorisation); no atomics, fixed summation order
//   k_reduce      sum of the cell-split partial slabs x (2 pi hbarc)^-3 x g
#ifndef IS3D_LDS_QROW_LIMIT
#define IS3D_LDS_QROW_LIMIT (80 * 1024)   // above this k_spectra takes the F_LY launch (per-lane y-term rows)
#endif
#ifndef IS3D_FILL_WGS
#define IS3D_FILL_WGS 8192    // k_spectra workgroups the cell splits aim for (>= 8k fills the chip evenly)
#endif
#ifndef IS3D_FILL_WGS_MP
#define IS3D_FILL_WGS_MP 2048 // the same for F_MP launches
#endif
#ifndef IS3D_CHAIN_L
#define IS3D_CHAIN_L 32       // PTMA warm-start chains: positions per segment (k_chain_pass), at least
#endif
#ifndef IS3D_CHAIN_SLOTS
#define IS3D_CHAIN_SLOTS 16384   // PTMA chain segments per pass (one wavefront each)
#endif
#ifndef IS3D_CHAIN_W
#define IS3D_CHAIN_W 4        // PTMA chain segments: wavefronts per segment sharing each Newton evaluation's terms
#endif
#ifndef IS3D_MAX_SPLITS
#define IS3D_MAX_SPLITS 1024  // cap on k_spectra's cell splits (one output-sized slab each)
#endif
#ifndef IS3D_SLAB_BYTES
#define IS3D_SLAB_BYTES (48L << 30)   // ... and on their slabs' memory: config 4 (10^6 cells, 50 MB slabs) runs 880 splits
                                      // of 0.5 MB of records (44 GB of slabs): 2569 ms per pass, 512 splits 2679 ms,
                                      // 256 splits 2751 ms (profiles/round4_r4a_ab_ts.log)
#endif
#ifndef IS3D_SAMPLE_BYTES
#define IS3D_SAMPLE_BYTES (1L << 30)  // bound on the working buffers of one is3d_sample batch of events
#endif
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <map>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/is3d_amd.h"
#include "aniso_math.h"
#include "cf_math.h"
#include "spline_host.h"
#include "kernels.h"
#include "group.h"
#include "polzn.h"
#include "sampler.h"
#include "decay.h"
#include "decay_list.h"
#include "devbuf.h"

using namespace is3d;
using namespace is3d::kern;

#include "engine_kernels.h"   // this unit's device code (k_prep ... k_df_eval)

// ------------------------------------------------------------------------------------------
// engine
// ------------------------------------------------------------------------------------------
// one launch's state between the stages of a staged launch (launch_begin .. launch_end)
struct LaunchCtx {
  hipStream_t st = nullptr;
  double* dev_out = nullptr;
  long wlo = 0, whi = 0, nw = 0, p0 = 0, p1 = 0;
  bool chained = false, empty = false;
  PrepArgs pa{};
  ChainArgs ca{};
};

struct is3d_engine {
  int device = 0;
  std::string err;
  // is3d_create_devices: the shard engines and their reduction (group.hip); every entry point forwards
  is3d::Group* grp = nullptr;
  // cell window [win_lo, win_hi) of the held surface that k_spectra integrates (-1: every cell); set by a
  // group whose shards hold the whole surface for the PTMA warm-start chains
  long win_lo = -1, win_hi = -1;
  // is3d_set_chain_range: PTMA warm-start chain positions [chain_q0, chain_q1) this engine solves (-1: all), for the
  // staged launch of one process per GPU
  long chain_q0 = -1, chain_q1 = -1;
  bool have_params = false, have_species = false, have_pdg = false, have_grid = false, have_gla = false, have_df = false;
  is3d_params p{};
  // species (original order) and mass-sorted permutation
  std::vector<double> mass, sign, degen, baryon;
  std::vector<int> order;
  std::vector<double> pdg_mass, pdg_sign, pdg_degen, pdg_baryon;
  std::vector<double> pT, phi, y, eta, eta_w;
  std::vector<double> pT_w, phi_w;       // operation 0 quadrature weights
  bool have_weights = false, have_bins = false;
  is3d_spacetime_bins bins{};
  int gla_alpha = 0, gla_pts = 0;
  std::vector<double> gla_r, gla_w;
  int nT = 0, nmuB = 0;
  std::vector<double> Tarr, muBarr, tab;
  double T_avg = 0.0;
  // derived host tables
  std::vector<double> jl2, jz, jx, jl2c, jzc;
  double bp_max = -1.0;
  bool tables_dirty = true;
  // device: every allocation, stream and event is a DevBuf / DevStream / DevEvent member (devbuf.h); the raw pointers
  // below are views into d_tables / d_const
  DevBuf<double> d_tables;
  DfTables dtb{};
  DevBuf<double> d_const;    // species, grids, gla, pdg
  const double *d_smass = nullptr, *d_ssign = nullptr, *d_sbaryon = nullptr, *d_sdegen = nullptr, *d_degen_orig = nullptr;
  const double* d_csg = nullptr;   // [npT][nphp] {pT cos, pT sin}
  const double *d_pT = nullptr, *d_cphi = nullptr, *d_sphi = nullptr, *d_y = nullptr, *d_eta = nullptr, *d_etaw = nullptr;
  const double *d_pTw = nullptr, *d_phiw = nullptr;
  const double *d_gla = nullptr;
  const double *d_pdg = nullptr;
  const double* d_aniso_h = nullptr;   // [3][n_aniso_h] merged (mass, sign, degeneracy) of the PTMA hadrons
  int n_aniso_h = 0;
  int* d_sorig = nullptr;
  // PTM renormalisation classes: sorted species with identical (mass, sign, baryon) and a zero / nonzero degeneracy
  // share one n_linear / n_mod per cell (ptm_renorm depends on nothing else, ptm_gkey): d_rcls[s] = class of sorted species s,
  // d_rrep[k] = a representative sorted species of class k (SMASH 444 -> nrcls classes)
  int* d_rcls = nullptr;
  int* d_rrep = nullptr;
  int nrcls = 0;
  // integrand classes (is3d_set_species_classes, default on): the momentum integrals see a species only through
  // its (mass, sign, baryon) -- plus, in PTM, whether its degeneracy is zero (ptm_gkey) -- and the engine applies the degeneracy once, to the cell sum, in k_reduce (the reference
  // multiplies every cell's term by prefactor x degeneracy, MomentumSpectra.cpp:365: the same product up to
  // rounding), so sorted species with identical keys have bit-identical cell sums: k_spectra / k_dndx integrate one lane species per class (SMASH 444 -> 193, UrQMD 305 -> 124) and the
  // reduction writes every member.  d_cmass/d_csign/d_cbaryon: class values, d_crcls: class -> renorm class,
  // d_cmem[d_cmem_off[c] ..]: member sorted species of class c, d_scls: sorted species -> class.
  bool classes = true;
  int ncls = 0;
  std::vector<int> scls;   // host copy of d_scls
  const double *d_cmass = nullptr, *d_csign = nullptr, *d_cbaryon = nullptr;
  int *d_crcls = nullptr, *d_cmem_off = nullptr, *d_cmem = nullptr, *d_scls = nullptr;
  // the surface [NSURF][ncell]: a view of surf_own (an uploaded or copied surface) or of the caller's device memory
  // (is3d_set_surface_device; surf_own is then empty)
  double* d_surf = nullptr; long ncell = 0;
  DevBuf<double> surf_own;
  DevBuf<double> d_chain;     // PTMA warm-start chain segments (k_chain_pass)
  DevBuf<double> d_rec, d_aux, d_sol, d_renorm, d_slab, d_out;
  DevBuf<int> d_fb;           // modified modes: [0] fallback cell count, [1..] k_fbwrite's cell list
  DevBuf<double> d_phtab;     // F_TS launches: k_phitab's per-(cell, pT, phi) rows of one chunk of cells
  DevBuf<double> d_phtab2;    // ... and of the next chunk, integrated on the side stream meanwhile
  // the streams and events of the chunked F_TS launches are made by the first launch that needs them
  DevStream side;             // F_TS chunks alternate between the launch stream and this one
  DevEvent fork, join;
  // folded F_TS chunks: k_fold runs on its own stream, in chunk order, after each chunk's k_spectra
  // (ev_spec); a chunk reusing a slab buffer waits for the fold that emptied it (ev_fold)
  DevStream fold_st;
  DevEvent ev_spec[2], ev_fold[2], fold_join;
  // is3d_set_tuning: F_TS table chunking (defaults IS3D_PHITAB_ONE / IS3D_PHITAB_BYTES): tables of the whole window
  // up to phitab_one bytes are one chunk, larger ones chunks of whole cell splits of about phitab_chunk bytes
  long phitab_one = IS3D_PHITAB_ONE, phitab_chunk = IS3D_PHITAB_BYTES;
  long last_nchunk = 0;       // F_TS chunks of the last launch (0: not an F_TS launch)
  // is3d_set_tuning: k_spectra's cell splits (defaults IS3D_MAX_SPLITS / IS3D_SLAB_BYTES / IS3D_SPLIT_BYTES)
  long max_splits = IS3D_MAX_SPLITS, slab_bytes = IS3D_SLAB_BYTES, split_bytes = IS3D_SPLIT_BYTES;
  long last_nsplit = 0;       // cell splits of the last launch's main plan
  long last_nslab = 0;        // ... and the output-sized partial slabs it held (folded F_TS chunks: 1 + 2 spc)
  // operation 0
  DevBuf<double> d_ycell, d_part;
  DevBuf<int> d_keys, d_perm;
  DevBuf<long> d_offs;
  long ycell_n = -1;
  DevBuf<int> d_err;                  // the device error word (cf_math.h DF_*)
  DevBuf<unsigned long long> d_cnt;   // [8] counters (PrepArgs::cnt)
  DevEvent ev[4];             // timing events of a launch's stages
  LaunchCtx lc;               // the launch in flight (staged launches)
  // spin polarization (mode 5, polzn.hip): thermal vorticity [6][ncell] of the surface set last (a new surface
  // clears it) and the kernels' constants, rebuilt after a species / classes / grid / params change
  DevBuf<double> d_vort; bool have_vort = false;
  bool have_surf = false;    // a surface was set (an empty one set from device memory has no d_surf)
  is3d::polzn::Tables pz;
  bool pz_dirty = true;
  // particle sampler (operation 2, sampler.hip): species tables in the original order, the "sample_bytes" bound on
  // a batch's working buffers, and the list / stats of the last is3d_sample
  is3d::sampler::Tables smp;
  bool smp_dirty = true;
  long sample_bytes = IS3D_SAMPLE_BYTES;
  std::vector<is3d::sampler::Particle> particles;
  std::vector<long> particle_offsets;
  is3d_sample_stats sst{};
  is3d_sample_famod_stats sfst{};   // is3d_sample_famod: the reconstruction counters of the last call
  bool sampled = false, sampled_famod = false;
  // test_sampler = 1: the bins, the device histogram of a binned call (zeroed at its start) and its host copy in
  // integer form (hist_nc counts, then hist_nv fixed-point vn sums)
  is3d_sample_bins sbins{};
  bool have_sbins = false;
  DevBuf<unsigned long long> d_hist;
  std::vector<long long> hist;
  long hist_nc = 0, hist_nv = 0;
  bool binned = false;
  is3d_stats st{};
  bool launched = false;
  // resonance-decay feed-down (decay.hip): the channel table as given, its plan (built by is3d_set_decays; a new
  // species list or momentum grid clears it), the packed tables (rebuilt after a params change: ny) and the log slabs
  std::vector<is3d_decay_channel> dk_ch;
  bool have_decays = false, dk_dirty = true, dk_launched = false;
  is3d::decay::Rule dk_rule{};
  is3d::decay::Plan dk_plan;
  is3d::decay::Packed dk_pack;
  DevBuf<double> d_dk_d, d_dk_log, d_dk_io;
  DevBuf<int> d_dk_i;
  DevEvent dk_ev[2];
  is3d_decay_stats dk_stats{};
  // Monte Carlo decays of a particle list (decay_list.hip): the plan's tables on the device (rebuilt after
  // is3d_set_decays), and the origins and stats of the last decayed list (a new sample clears them)
  is3d::decay_list::Tables dl;
  bool dl_dirty = true, decayed = false;
  std::vector<long> origins;
  is3d_decay_list_stats dl_stats{};

  int fail(int code, const std::string& msg) { err = msg; return code; }
};

static int hip_fail(is3d_engine* e, hipError_t h, const char* what) {
  return e->fail(IS3D_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(h));
}
#define HIPCHK(e, x)                                           \
  do {                                                         \
    hipError_t h_ = (x);                                       \
    if (h_ != hipSuccess) return hip_fail((e), h_, #x);        \
  } while (0)

// The device error word (cf_math.h DfErr) as the IS3D_ERR_* code and message of every entry point that reads one; the
// table errors carry the reference's printed messages.  other: the caller's message for any other nonzero word
static int df_error(is3d_engine* e, int derr, const char* other) {
  switch (derr) {
    case DF_OK: return IS3D_OK;
    case DF_SPLINE_RANGE: return e->fail(IS3D_ERR_DF_RANGE, "gsl: interp.c: interpolation error (df coefficient spline evaluated outside its table)");
    case DF_TABLE_RANGE: return e->fail(IS3D_ERR_DF_RANGE, "Error: (T,muB) outside df coefficient table. Exiting...");
    case DF_PTB_BARYON: return e->fail(IS3D_ERR_UNSUPPORTED, "Bilinear interpolation error: Jonah df doesn't work for nonzero muB. Exiting..");
    case DF_TS_SLOW: return e->fail(IS3D_ERR_DEVICE, "internal: a scalar-table (F_TS) lane left the fast path (sep_slow_cell bound)");
    default: return e->fail(IS3D_ERR_ARG, other);
  }
}

extern "C" int is3d_abi_version(void) { return IS3D_ABI_VERSION; }

#ifndef IS3D_BUILD_ID
#define IS3D_BUILD_ID "unknown"
#endif
extern "C" const char* is3d_build_id(void) { return IS3D_BUILD_ID; }

extern "C" is3d_engine* is3d_create(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return nullptr;
  if (hipSetDevice(device) != hipSuccess) return nullptr;
  is3d_engine* e = new is3d_engine();
  e->device = device;
  if (!e->d_err.reserve(1) || !e->d_cnt.reserve(8)) {
    delete e;
    return nullptr;
  }
  for (auto& v : e->ev) (void)v.create(hipEventDefault);
  for (auto& v : e->dk_ev) (void)v.create(hipEventDefault);
  return e;
}

extern "C" void is3d_destroy(is3d_engine* e) {
  if (!e) return;
  if (e->grp) {
    is3d::group_destroy(e->grp);
    delete e;
    return;
  }
  (void)hipSetDevice(e->device);
  (void)hipDeviceSynchronize();     // before the buffers, streams and events die with *e
  delete e;
}

extern "C" const char* is3d_last_error(const is3d_engine* e) {
  if (!e) return "null engine";
  return e->grp ? is3d::group_error(e->grp) : e->err.c_str();
}

extern "C" is3d_engine* is3d_create_devices(int n, const int* devices) {
  std::string err;
  is3d::Group* g = is3d::group_create(n, devices, err);
  if (!g) return nullptr;
  is3d_engine* e = new is3d_engine();
  e->device = devices[0];
  e->grp = g;
  return e;
}

extern "C" int is3d_set_cell_window(is3d_engine* e, long lo, long hi) {
  if (!e) return IS3D_ERR_ARG;
  if (e->grp) return is3d::group_fail(e->grp, IS3D_ERR_UNSUPPORTED, "a device-list engine places its own windows");
  e->chain_q0 = e->chain_q1 = -1;
  if (lo < 0 || hi < 0) { e->win_lo = e->win_hi = -1; return IS3D_OK; }
  if (lo > hi || hi > e->ncell) return e->fail(IS3D_ERR_ARG, "cell window outside the surface");
  e->win_lo = lo; e->win_hi = hi;
  return IS3D_OK;
}

extern "C" int is3d_set_tuning(is3d_engine* e, const char* key, long value) {
  if (e && e->grp) return key ? is3d::group_set_tuning(e->grp, key, value) : IS3D_ERR_ARG;
  if (!e || !key) return IS3D_ERR_ARG;
  if (!std::strcmp(key, "phitab_one_bytes")) e->phitab_one = value < 0 ? (long)IS3D_PHITAB_ONE : value;
  else if (!std::strcmp(key, "phitab_chunk_bytes")) e->phitab_chunk = value <= 0 ? (long)IS3D_PHITAB_BYTES : value;
  else if (!std::strcmp(key, "max_splits")) e->max_splits = value <= 0 ? (long)IS3D_MAX_SPLITS : value;
  else if (!std::strcmp(key, "slab_bytes")) e->slab_bytes = value <= 0 ? (long)IS3D_SLAB_BYTES : value;
  else if (!std::strcmp(key, "split_bytes")) e->split_bytes = value <= 0 ? (long)IS3D_SPLIT_BYTES : value;
  else if (!std::strcmp(key, "sample_bytes")) e->sample_bytes = value <= 0 ? (long)IS3D_SAMPLE_BYTES : value;
  else return e->fail(IS3D_ERR_ARG, std::string("is3d_set_tuning: unknown key ") + key);
  return IS3D_OK;
}

extern "C" long is3d_get_tuning(const is3d_engine* e, const char* key) {
  if (!e || !key) return -1;
  if (e->grp) return is3d::group_get_tuning(e->grp, key);
  if (!std::strcmp(key, "phitab_one_bytes")) return e->phitab_one;
  if (!std::strcmp(key, "phitab_chunk_bytes")) return e->phitab_chunk;
  if (!std::strcmp(key, "phitab_chunks")) return e->last_nchunk;
  if (!std::strcmp(key, "max_splits")) return e->max_splits;
  if (!std::strcmp(key, "slab_bytes")) return e->slab_bytes;
  if (!std::strcmp(key, "split_bytes")) return e->split_bytes;
  if (!std::strcmp(key, "splits")) return e->last_nsplit;
  if (!std::strcmp(key, "slabs")) return e->last_nslab;
  if (!std::strcmp(key, "sample_bytes")) return e->sample_bytes;
  if (!std::strcmp(key, "sample_batches")) return e->sst.batches;
  return -1;
}

extern "C" int is3d_set_params(is3d_engine* e, const is3d_params* p) {
  if (e && e->grp) return p ? is3d::group_set_params(e->grp, p) : IS3D_ERR_ARG;
  if (!e || !p) return IS3D_ERR_ARG;
  // operation 2: the oversampling estimate (is3d_total_yield) and the particle sampler (is3d_sample)
  if (p->operation < 0 || p->operation > 2)
    return e->fail(IS3D_ERR_ARG, "calculate_spectra error: need to set operation = (0, 1, 2)");
  if (p->dimension != 2 && p->dimension != 3) return e->fail(IS3D_ERR_ARG, "EmissionFunctionArray error: need to set dimension = (2,3)");
  if (p->df_mode < 1 || p->df_mode > 5) return e->fail(IS3D_ERR_ARG, "EmissionFunctionArray error: need to set df_mode = (1,2,3,4,5)");
  if (p->df_mode == PTB && p->include_baryon) return e->fail(IS3D_ERR_UNSUPPORTED, "Bilinear interpolation error: Jonah df doesn't work for nonzero muB. Exiting..");
  if (p->famod_chains < 0) return e->fail(IS3D_ERR_ARG, "famod_chains must be >= 0");
  e->p = *p;
  e->have_params = true;
  e->tables_dirty = true;
  e->pz_dirty = true;
  e->dk_dirty = true;
  return IS3D_OK;
}

extern "C" int is3d_set_species(is3d_engine* e, int n, const double* mass, const double* sign, const double* degeneracy,
                                const double* baryon) {
  if (e && e->grp) return is3d::group_set_species(e->grp, n, mass, sign, degeneracy, baryon);
  if (!e || n <= 0 || !mass || !sign || !degeneracy || !baryon) return e ? e->fail(IS3D_ERR_ARG, "bad species arrays") : IS3D_ERR_ARG;
  e->mass.assign(mass, mass + n); e->sign.assign(sign, sign + n); e->degen.assign(degeneracy, degeneracy + n);
  e->baryon.assign(baryon, baryon + n);
  e->order.resize(n);
  for (int i = 0; i < n; i++) e->order[i] = i;
  // lanes of a wavefront take consecutive species: sort by mass so that whole wavefronts hit the
  // exp-underflow early-out together (output order is unchanged)
  std::stable_sort(e->order.begin(), e->order.end(), [&](int a, int b) { return e->mass[a] < e->mass[b]; });
  e->have_species = true;
  e->tables_dirty = true;
  e->pz_dirty = true;
  e->smp_dirty = true;
  e->have_decays = false;     // the channels index the species
  e->dk_ch.clear();
  return IS3D_OK;
}

static int finalize_tables(is3d_engine* e);

extern "C" int is3d_set_species_classes(is3d_engine* e, int on) {
  if (e && e->grp) return is3d::group_set_species_classes(e->grp, on);
  if (!e) return IS3D_ERR_ARG;
  e->classes = on != 0;
  e->tables_dirty = true;
  e->pz_dirty = true;
  return IS3D_OK;
}

extern "C" int is3d_species_integrated(is3d_engine* e) {
  if (e && e->grp) return is3d::group_species_integrated(e->grp);
  if (!e) return -IS3D_ERR_ARG;
  const int rc = finalize_tables(e);
  return rc ? -rc : e->ncls;       // an error as minus its IS3D_ERR_* code (a count is >= 1)
}

extern "C" int is3d_set_pdg(is3d_engine* e, int n, const double* mass, const double* sign, const double* degeneracy,
                            const double* baryon) {
  if (e && e->grp) return is3d::group_set_pdg(e->grp, n, mass, sign, degeneracy, baryon);
  if (!e || n <= 0 || !mass || !sign || !degeneracy || !baryon) return e ? e->fail(IS3D_ERR_ARG, "bad pdg arrays") : IS3D_ERR_ARG;
  e->pdg_mass.assign(mass, mass + n); e->pdg_sign.assign(sign, sign + n); e->pdg_degen.assign(degeneracy, degeneracy + n);
  e->pdg_baryon.assign(baryon, baryon + n);
  e->have_pdg = true;
  e->tables_dirty = true;
  return IS3D_OK;
}

extern "C" int is3d_set_momentum_grid(is3d_engine* e, int npT, const double* pT, int nphi, const double* phi, int ny,
                                      const double* y, int neta, const double* eta, const double* eta_weight) {
  if (e && e->grp) return is3d::group_set_momentum_grid(e->grp, npT, pT, nphi, phi, ny, y, neta, eta, eta_weight);
  if (!e) return IS3D_ERR_ARG;
  if (npT <= 0 || nphi <= 0 || !pT || !phi) return e->fail(IS3D_ERR_ARG, "empty pT/phi table");
  e->pT.assign(pT, pT + npT); e->phi.assign(phi, phi + nphi);
  e->y.assign(y ? y : pT, y ? y + std::max(ny, 0) : pT);
  e->eta.assign(eta ? eta : pT, eta ? eta + std::max(neta, 0) : pT);
  e->eta_w.assign(eta_weight ? eta_weight : pT, eta_weight ? eta_weight + std::max(neta, 0) : pT);
  e->have_grid = true;
  e->tables_dirty = true;
  e->pz_dirty = true;
  e->have_decays = false;     // is3d_set_decays checked the grid it saw
  e->dk_ch.clear();
  return IS3D_OK;
}

extern "C" int is3d_set_momentum_weights(is3d_engine* e, const double* pT_weight, const double* phi_weight) {
  if (e && e->grp) return is3d::group_set_momentum_weights(e->grp, pT_weight, phi_weight);
  if (!e) return IS3D_ERR_ARG;
  if (!e->have_grid) return e->fail(IS3D_ERR_STATE, "is3d_set_momentum_grid not called");
  if (!pT_weight || !phi_weight) return e->fail(IS3D_ERR_ARG, "null pT/phi weights");
  e->pT_w.assign(pT_weight, pT_weight + e->pT.size());
  e->phi_w.assign(phi_weight, phi_weight + e->phi.size());
  e->have_weights = true;
  e->tables_dirty = true;
  return IS3D_OK;
}

extern "C" int is3d_set_spacetime_bins(is3d_engine* e, const is3d_spacetime_bins* b) {
  if (e && e->grp) return b ? is3d::group_set_spacetime_bins(e->grp, b) : IS3D_ERR_ARG;
  if (!e || !b) return IS3D_ERR_ARG;
  if (b->tau_bins <= 0 || b->r_bins <= 0 || b->phip_bins <= 0) return e->fail(IS3D_ERR_ARG, "spacetime bins must be positive");
  if (!(b->tau_max > b->tau_min) || !(b->r_max > b->r_min)) return e->fail(IS3D_ERR_ARG, "spacetime bin ranges must be increasing");
  if (b->threads < 0) return e->fail(IS3D_ERR_ARG, "spacetime threads must be >= 0");
  e->bins = *b;
  e->have_bins = true;
  return IS3D_OK;
}

extern "C" int is3d_set_gauss_laguerre(is3d_engine* e, int alpha, int points, const double* roots, const double* weights) {
  if (e && e->grp) return is3d::group_set_gauss_laguerre(e->grp, alpha, points, roots, weights);
  if (!e) return IS3D_ERR_ARG;
  if (alpha < 3 || points <= 0 || !roots || !weights) return e->fail(IS3D_ERR_ARG, "Gauss-Laguerre table needs alpha >= 3");
  e->gla_alpha = alpha; e->gla_pts = points;
  e->gla_r.assign(roots, roots + (size_t)alpha * points);
  e->gla_w.assign(weights, weights + (size_t)alpha * points);
  e->have_gla = true;
  e->tables_dirty = true;
  return IS3D_OK;
}

extern "C" int is3d_set_df_tables(is3d_engine* e, int nT, int nmuB, const double* T, const double* muB,
                                  const double* tables, double T_avg) {
  if (e && e->grp) return is3d::group_set_df_tables(e->grp, nT, nmuB, T, muB, tables, T_avg);
  if (!e) return IS3D_ERR_ARG;
  if (nT < 3 || nmuB < 1 || !T || !muB || !tables) return e->fail(IS3D_ERR_ARG, "bad df coefficient tables");
  e->nT = nT; e->nmuB = nmuB;
  e->Tarr.assign(T, T + nT); e->muBarr.assign(muB, muB + nmuB);
  e->tab.assign(tables, tables + (size_t)10 * nmuB * nT);
  e->T_avg = T_avg;
  e->have_df = true;
  e->tables_dirty = true;
  return IS3D_OK;
}

// Build the derived tables (splines, Jonah) and upload everything read-only to HBM.
// PTB Jonah table on the device (k_jonah_terms + k_jonah_sum) into e->jl2 / jz / jx / bp_max; the
// host keeps only the two 301-point spline solves
static int device_jonah_table(is3d_engine* e, const double* r2, const double* w2) {
  const int npdg = (int)e->pdg_mass.size(), pts = e->gla_pts;
  if (npdg == 0) return e->fail(IS3D_ERR_STATE, "PTB needs the PDG (is3d_set_pdg)");
  std::vector<double> in;
  in.insert(in.end(), e->pdg_mass.begin(), e->pdg_mass.end());
  in.insert(in.end(), e->pdg_degen.begin(), e->pdg_degen.end());
  in.insert(in.end(), e->pdg_sign.begin(), e->pdg_sign.end());
  in.insert(in.end(), r2, r2 + pts);
  in.insert(in.end(), w2, w2 + pts);
  const size_t nterms = (size_t)(kJonahN + 1) * 2 * npdg, nout = 3 * (size_t)kJonahN;
  DevBuf<double> buf;
  if (!buf.reserve((long)(in.size() + nterms + nout))) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(Jonah table) failed");
  double* const d = buf.get();
  JonahArgs ja{};
  ja.T = e->T_avg; ja.npdg = npdg; ja.pts = pts;
  ja.mass = d; ja.degen = d + npdg; ja.sign = d + 2 * npdg; ja.r2 = d + 3 * npdg; ja.w2 = d + 3 * npdg + pts;
  ja.terms = d + in.size();
  ja.l2 = ja.terms + nterms; ja.z = ja.l2 + kJonahN; ja.bp = ja.z + kJonahN;
  std::vector<double> out(nout);
  HIPCHK(e, hipMemcpy(d, in.data(), in.size() * sizeof(double), hipMemcpyHostToDevice));
  const long nthr = (long)(kJonahN + 1) * npdg;
  hipLaunchKernelGGL(k_jonah_terms, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, 0, ja);
  hipLaunchKernelGGL(k_jonah_sum, dim3((kJonahN + 63) / 64), dim3(64), 0, 0, ja);
  HIPCHK(e, hipGetLastError());
  HIPCHK(e, hipMemcpy(out.data(), ja.l2, nout * sizeof(double), hipMemcpyDeviceToHost));
  e->jl2.assign(out.begin(), out.begin() + kJonahN);
  e->jz.assign(out.begin() + kJonahN, out.begin() + 2 * kJonahN);
  e->jx.assign(out.begin() + 2 * kJonahN, out.end());
  e->bp_max = -1.0;
  for (int i = 0; i < kJonahN; i++) e->bp_max = std::fmax(e->bp_max, e->jx[i]);
  return IS3D_OK;
}

// k_spectra launch shape for this engine's species / grids (shared by the launch and by the {pT cos,
// pT sin} table finalize_tables builds for KJ-padded phi rows)
struct SpectraPlan {
  int KJ, njb, nq, nqmax, tb, ly, t8, tile;
  int ts;                     // F_TS: the F_TB launch with the per-(cell, phi) operands from k_phitab's table
  int by;                     // F_BY: ... with include_baryon (T3 rows)
  int mp, npw;                // F_MP: pT values per workgroup (1 otherwise)
  size_t shmem;
  size_t shmem_fb;            // modified modes: the F_FB launch (8-cell tiles, per-lane y-term rows, no q tables)
};
static SpectraPlan spectra_plan(const is3d_engine* e, bool allow_ts = true) {
  SpectraPlan P{};
  P.npw = 1;
  const int mode = e->p.df_mode, dim = e->p.dimension;
  const int np = e->ncls, nphi = (int)e->phi.size();     // lane species: the integrand classes
  const int npT = (int)e->pT.size();
  const int nk = (dim == 3) ? (int)e->y.size() : 1, nl = (dim == 3) ? 1 : (int)e->eta.size();
  P.nq = nk * nl;
  auto shape = [&](int KJ) {
    P.KJ = KJ;
    P.njb = (nphi + KJ - 1) / KJ;
    // rows (r = q + nq jb) one workgroup's 256 consecutive tasks can span: a contiguous range of at most
    // (kBlock - 1) / np + 2 of the nq njb rows
    P.nqmax = (int)std::min<long>((long)P.nq * P.njb, (kBlock - 1) / np + 2);
    // Grad {PD, T1} table (F_TB, sep_quad_tb_t): exact only without baryon terms (R_SCB = R_SSB = 0:
    // V^mu and alphaB are only packed when include_baryon && include_baryondiff_deltaf (prep_grad_ce), and
    // df_eval leaves c1 = c3 = 0 without baryons); needs phi blocks of fours and at most kTbQ rows per
    // workgroup
    // with include_baryon only as F_TS + F_BY (one phi block of 24 or 32 points: the baryon part of the linear
    // coefficients comes from the table as T3)
    const bool ts_shape = allow_ts && P.njb == 1 && (KJ == 24 || KJ == 32);
    P.tb = ((mode == GRAD || mode == CE) && (!e->p.include_baryon || ts_shape) &&
            KJ % 4 == 0 && P.nqmax <= kTbQ) ? F_TB : 0;
  };
  int kTile = (mode >= PTM) ? IS3D_KTILE_MOD : is3d::kern::kTile;   // spectra_tile<MODE, FLAGS>()
  // k_spectra's LDS layout (kernels.h): record tiles x kRecBufs, per-tile tables x kTabBufs
  // F_TS (kernels.h TS): an F_TB launch with one phi block of 24 or 32 points
  auto ts_ok = [&]() { return allow_ts && P.tb && P.njb == 1 && (P.KJ == 24 || P.KJ == 32); };
  bool fb_layout = false;               // sizing the F_FB launch (separable lanes of a modified mode)
  auto lds_bytes = [&](int qrows) {     // qrows = 0: F_LY layout (one y-term row per lane)
    const size_t nphp = (size_t)P.njb * P.KJ, tile = (size_t)kTile;
    // modified launches (kernels.h MODMAIN): no {b', Phi} rows
    const bool modmain = mode >= PTM && !fb_layout;
    const size_t etab = kExpTabN;
    const size_t bprows = modmain ? 0 : 1;
    if (ts_ok()) {
      // records x 3, trig + {pc, ps}, grid, y-term rows x 2, exp table, T1 rows [tile][qrows][KJ + 2] (+ 1: alignment)
      return sizeof(double) * (3 * tile * NREC + 4 * nphp + (size_t)(nk + 2 * nl) +
                               2 * tile * std::min(qrows, P.nq) * kYRow + kExpTabN + tile * qrows * (P.KJ + 2) + 1 +
                               128);     // + 128: the landing rows of the k_phitab L2 prefetch
    }
    // pipelined launches (F_TB, the modified path's 16-cell tiles): 3 record tiles, 2 table buffers
    const bool pipe = (P.tb || (mode >= PTM && qrows && !P.t8 && !P.ly));
    const size_t rb = pipe ? 3 : 2, tb = pipe ? 2 : 1, qvf = (mode >= PTM || !pipe) ? 2 : 1;
    const size_t w = (size_t)P.npw;     // F_MP: pT blocks of {pc, ps} and of the per-(cell, phi) tables
    return sizeof(double) * (rb * tile * NREC + (2 + 2 * w) * nphp + bprows * tb * 2 * w * tile * nphp + tb * qvf * w * tile * nphp +
                             (size_t)(nk + 2 * nl) +
                             (qrows ? tb * tile * std::min(qrows, P.nq) * kYRow : (size_t)kBlock * kYRowLY) + etab +
                             (P.tb ? 2 * tile * qrows * (P.KJ + 1) + 1 : 0) +
                             (P.tb && mode == CE ? tb * 2 * tile * nphp : 0) +
                             // the per-lane RTA-CE launch's {TE, T2} table (kernels.h PDE)
                             // (+ 1: s_pe starts at the 16-byte-aligned end of the y-term rows)
                             (mode == CE && !P.tb && !P.mp && qrows && P.KJ % 4 == 0 ? tb * 2 * tile * nphp + 1 : 0) +
                             (mode >= PTM && qrows ? tile * qrows * (P.KJ + 1) + 1 : 0));
  };
  shape(spectra_kj_fill(nphi, (long)np * P.nq));
  P.ly = 0;
  P.shmem = lds_bytes(P.nqmax);
  // RTA-CE's table launch adds {TE, T2} to the {PD, T1} rows: where that costs the third workgroup per CU
  // (LDS above 160 KB / 3 -- SMASH as 193 integrand classes spans 3 q rows per workgroup: 54.5 KB) the
  // per-lane launch is faster (config 2 RTA-CE 349.7 -> 324.3 ms, profiles/round3_r3h_ab_ce_tb.log; with
  // 444 species, 2 rows, 47.8 KB, the table launch had won 723 -> 676 ms in round 1)
  if (P.tb && mode == CE && 3 * P.shmem > 160 * 1024) {
    P.tb = 0;
    P.shmem = lds_bytes(P.nqmax);
  }
  // the modified path's 16-cell tiles fall back to 8 (F_T8) before giving up the q-row tables
  if (P.shmem > IS3D_LDS_QROW_LIMIT && mode >= PTM && kTile != is3d::kern::kTile) {
    kTile = is3d::kern::kTile;
    P.t8 = F_T8;
    const size_t s8 = lds_bytes(P.nqmax);
    if (s8 <= IS3D_LDS_QROW_LIMIT) P.shmem = s8;
    else { kTile = IS3D_KTILE_MOD; P.t8 = 0; }
  }
  // grids whose q rows do not fit (large y / eta tables with few species; np >= 86 keeps nqmax <= 4) run
  // the F_LY launch (KJ = 8, per-lane y-term rows, no q-row tables) instead of failing: the reference has
  // no grid limit
  if (P.shmem > IS3D_LDS_QROW_LIMIT && !P.tb) {
    shape(8);
    P.tb = 0;
    P.t8 = 0;
    P.ly = F_LY;
    kTile = is3d::kern::kTile;     // spectra_tile<MODE, F_LY | ...>
    P.shmem = lds_bytes(0);
  }
  // F_MP (Grad / RTA-CE, no table launch): when one pT's tasks with a single phi block of KJ >= nphi fill at
  // most half a workgroup (pikp 2+1D: 3 x 24 = 72), a workgroup takes npw = 256 / tasks pT values and every
  // lane a whole phi row -- the lane setup (~4.5 points' work) is paid once per row instead of once per
  // 8-point block; chosen by the same cost model as spectra_kj_fill (lane slots x (KJ + 4.5))
  if (mode <= CE && !P.tb && !P.ly && nphi <= 32) {
    const long tpp = (long)np * P.nq;
    const int kjm = nphi <= 24 ? 24 : 32;
    if (tpp * 2 <= kBlock) {
      const long slots = (tpp * P.njb + kBlock - 1) / kBlock * kBlock;
      const double cost_now = (double)slots * (P.KJ + 4.5);
      const int npw = (int)std::min<long>(kBlock / tpp, npT);
      const double cost_mp = (double)kBlock / npw * (kjm + 4.5);
      if (cost_mp < cost_now) {
        SpectraPlan Q = P;
        shape(kjm);
        P.tb = 0;
        P.nqmax = P.nq;
        P.mp = F_MP;
        P.npw = npw;
        const size_t sm = lds_bytes(P.nqmax);
        if (sm <= IS3D_LDS_QROW_LIMIT) P.shmem = sm;
        else P = Q;
      }
    }
  }
  P.ts = ts_ok() ? F_TS : 0;
  P.by = (P.ts && e->p.include_baryon) ? F_BY : 0;
  if (P.ts && kTile != IS3D_KTILE_TS) {     // spectra_tile<MODE, F_TB | F_TS>()
    kTile = IS3D_KTILE_TS;
    P.shmem = lds_bytes(P.nqmax);
    // the F_TS tile's LDS past the limit (a y / eta grid of thousands of nodes): the plan without F_TS
    if (P.shmem > IS3D_LDS_QROW_LIMIT) return spectra_plan(e, false);
  }
  P.tile = kTile;
  if (mode >= PTM) {
    const int t = kTile, ly = P.ly, tb = P.tb, t8 = P.t8;
    kTile = is3d::kern::kTile;
    P.ly = F_LY; P.tb = 0; P.t8 = 0;
    fb_layout = true;
    P.shmem_fb = lds_bytes(0);
    fb_layout = false;
    kTile = t; P.ly = ly; P.tb = tb; P.t8 = t8;
  }
  return P;
}

// PTM's renormalisation n_linear / n_mod (MomentumSpectra.cpp:790-832) is a ratio of two sums that both carry the
// degeneracy as a factor, so it depends on (mass, sign, baryon) alone -- except g = 0, where it is 0 / 0 = NaN and the
// species is skipped.  The renormalisation classes and PTM's integrand classes therefore key on whether g is zero
// (SMASH 205 -> 193 PTM lane classes, the same as the other modes; the class representative's g cancels to rounding,
// ~1e-16; rounds 3 / 4 keyed on g itself)
static uint64_t ptm_gkey(double g) { return (uint64_t)(g == 0.0 ? 1 : 0); }

static int finalize_tables(is3d_engine* e) {
  if (!e->have_params) return e->fail(IS3D_ERR_STATE, "is3d_set_params not called");
  if (!e->have_species) return e->fail(IS3D_ERR_STATE, "is3d_set_species not called");
  if (!e->have_grid) return e->fail(IS3D_ERR_STATE, "is3d_set_momentum_grid not called");
  if (!e->have_df) return e->fail(IS3D_ERR_STATE, "is3d_set_df_tables not called");
  const int mode = e->p.df_mode;
  if ((mode == PTM || mode == PTB) && !e->have_gla) return e->fail(IS3D_ERR_STATE, "is3d_set_gauss_laguerre not called");
  if ((mode == PTB || mode == PTMA) && !e->have_pdg) return e->fail(IS3D_ERR_STATE, "is3d_set_pdg not called");
  if (e->p.dimension == 3 && e->y.empty()) return e->fail(IS3D_ERR_ARG, "dimension = 3 needs a y table");
  if (e->p.dimension == 2 && e->eta.empty()) return e->fail(IS3D_ERR_ARG, "dimension = 2 needs an eta table");
  if (!e->tables_dirty) return IS3D_OK;
  HIPCHK(e, hipSetDevice(e->device));
  const int nT = e->nT, nmuB_used = e->p.include_baryon ? e->nmuB : 1;
  // --- delta-f blob: T | muB | tab | 7 x (y, c) | jonah x, l2, l2c, z, zc
  std::vector<double> blob;
  auto put = [&](const double* v, size_t n) { size_t off = blob.size(); blob.insert(blob.end(), v, v + n); return off; };
  const size_t oT = put(e->Tarr.data(), nT);
  const size_t omu = put(e->muBarr.data(), e->nmuB);
  const size_t otab = put(e->tab.data(), e->tab.size());
  size_t osy[NSPL] = {0}, osc[NSPL] = {0};
  const int spl_col[NSPL] = {0, 2, 3, 5, 7, 8, 9};   // c0 c2 c3 F betabulk betaV betapi
  if (!e->p.include_baryon) {
    for (int k = 0; k < NSPL; k++) {
      const double* yv = e->tab.data() + (size_t)spl_col[k] * e->nmuB * nT;   // muB row 0
      std::vector<double> c;
      if (!cspline_coeffs(e->Tarr.data(), yv, nT, c)) return e->fail(IS3D_ERR_ARG, "gsl: x values must be strictly increasing (T table)");
      osy[k] = put(yv, nT);
      osc[k] = put(c.data(), nT);
    }
  }
  size_t ojx = 0, ojl = 0, ojlc = 0, ojz = 0, ojzc = 0;
  int nj = 0;
  if (!e->p.include_baryon && mode == PTB) {
    const double* r2 = e->gla_r.data() + 2 * e->gla_pts;
    const double* w2 = e->gla_w.data() + 2 * e->gla_pts;
    const int rc = device_jonah_table(e, r2, w2);
    if (rc) return rc;
    if (!cspline_coeffs(e->jx.data(), e->jl2.data(), 301, e->jl2c) || !cspline_coeffs(e->jx.data(), e->jz.data(), 301, e->jzc))
      return e->fail(IS3D_ERR_DF_RANGE, "gsl: x values must be strictly increasing (Jonah bulkPi/P table)");
    nj = 301;
    ojx = put(e->jx.data(), 301); ojl = put(e->jl2.data(), 301); ojlc = put(e->jl2c.data(), 301);
    ojz = put(e->jz.data(), 301); ojzc = put(e->jzc.data(), 301);
  }
  e->d_tables.reset();      // a new blob every time, as large as it needs to be
  if (!e->d_tables.reserve((long)blob.size())) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(tables) failed");
  const double* const dt = e->d_tables.get();
  HIPCHK(e, hipMemcpy(e->d_tables.get(), blob.data(), blob.size() * sizeof(double), hipMemcpyHostToDevice));
  DfTables& tb = e->dtb;
  tb.df_mode = mode; tb.include_baryon = e->p.include_baryon;
  tb.nT = nT; tb.nmuB = nmuB_used;
  tb.T = dt + oT; tb.muB = dt + omu; tb.tab = dt + otab;
  tb.T_min = e->Tarr[0]; tb.muB_min = e->muBarr[0];
  tb.dT = std::fabs(e->Tarr[1] - e->Tarr[0]);
  tb.dmuB = e->nmuB > 1 ? std::fabs(e->muBarr[1] - e->muBarr[0]) : 0.0;
  for (int k = 0; k < NSPL; k++) { tb.sy[k] = dt + osy[k]; tb.sc[k] = dt + osc[k]; }
  tb.nj = nj; tb.jx = dt + ojx; tb.jl2 = dt + ojl; tb.jl2c = dt + ojlc;
  tb.jz = dt + ojz; tb.jzc = dt + ojzc;
  tb.bulk_over_P_max = e->bp_max;
  // tab is laid out [10][nmuB][nT]; with include_baryon = 0 only muB row 0 is used (nmuB_used = 1)
  // but the stride must stay the file's nmuB
  if (!e->p.include_baryon) tb.nmuB = 1;
  // --- constants blob: sorted species, original degeneracy, grids, gla, pdg
  const int np = (int)e->mass.size();
  std::vector<double> cb;
  auto cput = [&](const double* v, size_t n) { size_t off = cb.size(); cb.insert(cb.end(), v, v + n); return off; };
  std::vector<double> sm(np), ss(np), sb(np), sd(np);
  for (int i = 0; i < np; i++) { const int o = e->order[i]; sm[i] = e->mass[o]; ss[i] = e->sign[o]; sb[i] = e->baryon[o]; sd[i] = e->degen[o]; }
  const size_t osm = cput(sm.data(), np), oss = cput(ss.data(), np), osb = cput(sb.data(), np), osd = cput(sd.data(), np);
  const size_t odg = cput(e->degen.data(), np);
  const size_t opt = cput(e->pT.data(), e->pT.size());
  std::vector<double> cph(e->phi.size()), sph(e->phi.size());
  for (size_t j = 0; j < e->phi.size(); j++) { cph[j] = std::cos(e->phi[j]); sph[j] = std::sin(e->phi[j]); }
  const size_t oc = cput(cph.data(), cph.size()), os = cput(sph.data(), sph.size());
  const size_t oy = cput(e->y.data(), e->y.size()), oe = cput(e->eta.data(), e->eta.size()), ow = cput(e->eta_w.data(), e->eta_w.size());
  std::vector<double> pTw(e->pT.size(), 0.0), phiw(e->phi.size(), 0.0);
  if (e->have_weights) { pTw = e->pT_w; phiw = e->phi_w; }
  const size_t opw = cput(pTw.data(), pTw.size()), ophw = cput(phiw.data(), phiw.size());
  // integrand classes of the sorted species (first occurrence order, so the class list stays mass-sorted)
  std::vector<int> scls(np), crep, cmem_off, cmem;
  {
    std::map<std::array<uint64_t, 4>, int> cls;
    for (int i = 0; i < np; i++) {
      const std::array<uint64_t, 4> key{__builtin_bit_cast(uint64_t, sm[i]), __builtin_bit_cast(uint64_t, ss[i]),
                                        __builtin_bit_cast(uint64_t, sb[i]), mode == PTM ? ptm_gkey(sd[i]) : (uint64_t)0};
      int c = (int)crep.size();
      if (e->classes) {
        auto it = cls.find(key);
        if (it == cls.end()) it = cls.emplace(key, c).first;
        c = it->second;
      }
      if (c == (int)crep.size()) crep.push_back(i);
      scls[i] = c;
    }
    const int nc = (int)crep.size();
    cmem_off.assign(nc + 1, 0);
    for (int i = 0; i < np; i++) cmem_off[scls[i] + 1]++;
    for (int c = 0; c < nc; c++) cmem_off[c + 1] += cmem_off[c];
    cmem.resize(np);
    std::vector<int> fill(cmem_off.begin(), cmem_off.end() - 1);
    for (int i = 0; i < np; i++) cmem[fill[scls[i]]++] = i;
    e->ncls = nc;
    e->scls = scls;
  }
  std::vector<double> cm(e->ncls), csn(e->ncls), cby(e->ncls);
  for (int c = 0; c < e->ncls; c++) { cm[c] = sm[crep[c]]; csn[c] = ss[crep[c]]; cby[c] = sb[crep[c]]; }
  const size_t ocm = cput(cm.data(), e->ncls), ocs_ = cput(csn.data(), e->ncls), ocb = cput(cby.data(), e->ncls);
  // {pT cos phi, pT sin phi} per (pT, padded phi slot) for k_spectra's scalar loads (same products as
  // its LDS copy s_cs); 16-byte aligned
  if (cb.size() & 1) cb.push_back(0.0);
  const int kj_cs = spectra_plan(e).KJ;
  const int nphp_cs = (int)((e->phi.size() + kj_cs - 1) / kj_cs) * kj_cs;
  std::vector<double> csv((size_t)e->pT.size() * nphp_cs * 2, 0.0);
  for (size_t i = 0; i < e->pT.size(); i++)
    for (size_t j = 0; j < e->phi.size(); j++) {
      csv[(i * nphp_cs + j) * 2] = e->pT[i] * cph[j];
      csv[(i * nphp_cs + j) * 2 + 1] = e->pT[i] * sph[j];
    }
  const size_t ocs = cput(csv.data(), csv.size());
  const size_t og = cput(e->gla_r.data(), e->gla_r.size());
  cput(e->gla_w.data(), e->gla_w.size());
  const size_t opd = cput(e->pdg_mass.data(), e->pdg_mass.size());
  cput(e->pdg_sign.data(), e->pdg_sign.size());
  cput(e->pdg_degen.data(), e->pdg_degen.size());
  // PTMA Newton solve / famod coefficients: the reference sums its first min(320, N) PDG hadrons
  // (MomentumSpectra.cpp:1295); the integrands depend on a hadron's (mass, sign) only, times its
  // degeneracy, so hadrons with identical (mass, sign) are merged with summed degeneracies (SMASH:
  // 320 -> 92, UrQMD: 320 -> 83; first-occurrence order).  Only the FP summation order changes, as it
  // already does in the lane-strided sums.  Checked on the breakdown-heavy chain (bulk x10, one chain,
  // tests/test_gpu_configs.py::test_modified_fallback_launch): the merged GPU solve and the unmerged
  // oracle take the same 894 Newton steps and agree to 3e-13; tests/test_kernel_math_cpu.py compares
  // merged and per-hadron sums of the same device math directly (cf_emulator variant bit 8).
  std::vector<double> am, as, ag;
  {
    const int nh = std::min(320, (int)e->pdg_mass.size());
    for (int i = 0; i < nh; i++) {
      int k = -1;
      for (size_t u = 0; u < am.size(); u++)
        if (am[u] == e->pdg_mass[i] && as[u] == e->pdg_sign[i]) { k = (int)u; break; }
      if (k < 0) { am.push_back(e->pdg_mass[i]); as.push_back(e->pdg_sign[i]); ag.push_back(e->pdg_degen[i]); }
      else ag[k] += e->pdg_degen[i];
    }
    if (am.empty()) { am.push_back(0.0); as.push_back(0.0); ag.push_back(0.0); }
  }
  e->n_aniso_h = e->pdg_mass.empty() ? 0 : (int)am.size();
  const size_t oah = cput(am.data(), am.size());
  cput(as.data(), as.size());
  cput(ag.data(), ag.size());
  std::vector<int> rcls(np), rrep;
  {
    std::map<std::array<uint64_t, 4>, int> cls;
    for (int i = 0; i < np; i++) {
      const std::array<uint64_t, 4> key{__builtin_bit_cast(uint64_t, sm[i]), __builtin_bit_cast(uint64_t, ss[i]),
                                        ptm_gkey(sd[i]), __builtin_bit_cast(uint64_t, sb[i])};
      auto it = cls.find(key);
      if (it == cls.end()) { it = cls.emplace(key, (int)rrep.size()).first; rrep.push_back(i); }
      rcls[i] = it->second;
    }
  }
  e->nrcls = (int)rrep.size();
  const int nc = e->ncls;
  std::vector<int> crcls(nc);
  for (int c = 0; c < nc; c++) crcls[c] = rcls[crep[c]];
  // ints after the doubles: sorig[np] | rcls[np] | rrep[np] | crcls[nc] | cmem_off[nc + 1] | cmem[np] | scls[np]
  std::vector<int> ib;
  for (int i = 0; i < np; i++) ib.push_back(e->order[i]);
  ib.insert(ib.end(), rcls.begin(), rcls.end());
  rrep.resize(np, 0);
  ib.insert(ib.end(), rrep.begin(), rrep.end());
  ib.insert(ib.end(), crcls.begin(), crcls.end());
  ib.insert(ib.end(), cmem_off.begin(), cmem_off.end());
  ib.insert(ib.end(), cmem.begin(), cmem.end());
  ib.insert(ib.end(), scls.begin(), scls.end());
  e->d_const.reset();
  if (!e->d_const.reserve((long)(cb.size() + (ib.size() + 1) / 2))) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(constants) failed");
  double* const dc = e->d_const.get();
  HIPCHK(e, hipMemcpy(dc, cb.data(), cb.size() * sizeof(double), hipMemcpyHostToDevice));
  int* const di = (int*)(dc + cb.size());
  HIPCHK(e, hipMemcpy(di, ib.data(), ib.size() * sizeof(int), hipMemcpyHostToDevice));
  e->d_sorig = di;
  e->d_rcls = di + np;
  e->d_rrep = di + 2 * (size_t)np;
  e->d_crcls = di + 3 * (size_t)np;
  e->d_cmem_off = e->d_crcls + nc;
  e->d_cmem = e->d_cmem_off + nc + 1;
  e->d_scls = e->d_cmem + np;
  e->d_cmass = dc + ocm; e->d_csign = dc + ocs_; e->d_cbaryon = dc + ocb;
  e->d_smass = dc + osm; e->d_ssign = dc + oss; e->d_sbaryon = dc + osb; e->d_sdegen = dc + osd;
  e->d_degen_orig = dc + odg; e->d_pT = dc + opt; e->d_cphi = dc + oc; e->d_sphi = dc + os;
  e->d_y = dc + oy; e->d_eta = dc + oe; e->d_etaw = dc + ow;
  e->d_gla = dc + og; e->d_pdg = dc + opd; e->d_aniso_h = dc + oah;
  e->d_pTw = dc + opw; e->d_phiw = dc + ophw;
  e->d_csg = dc + ocs;
  e->tables_dirty = false;
  return IS3D_OK;
}

// What every surface setter does on taking a surface of n cells.  owned: d_surf becomes the engine's own buffer --
// reallocated when too small, or more than twice the size (a device group's cost prepass uploads the whole surface
// to shard 0 before its own window); otherwise that buffer is dropped and the caller points d_surf at its memory.
// The vorticity, the cell window and the chain range belonged to the previous surface.
static int adopt_surface(is3d_engine* e, long n, bool owned) {
  if (!owned || e->surf_own.capacity() > (long)NSURF * (2 * n + 4096)) e->surf_own.reset();
  const bool ok = !owned || e->surf_own.reserve((long)NSURF * std::max(n, 1L));
  e->d_surf = e->surf_own.get();
  if (!ok) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(surface) failed");
  e->ncell = n;
  e->have_surf = true;
  e->have_vort = false;
  e->win_lo = e->win_hi = -1;
  e->chain_q0 = e->chain_q1 = -1;
  return IS3D_OK;
}

extern "C" int is3d_set_surface(is3d_engine* e, long n, const is3d_surface* s) {
  if (e && e->grp) return is3d::group_set_surface(e->grp, n, s);
  if (!e || !s || n < 0) return e ? e->fail(IS3D_ERR_ARG, "bad surface") : IS3D_ERR_ARG;
  HIPCHK(e, hipSetDevice(e->device));
  const double* fields[NSURF] = {s->tau, s->x, s->y, s->eta, s->dat, s->dax, s->day, s->dan, s->ux, s->uy, s->un,
                                 s->E, s->T, s->P, s->pixx, s->pixy, s->pixn, s->piyy, s->piyn, s->bulkPi,
                                 s->muB, s->nB, s->Vx, s->Vy, s->Vn};
  for (int f = 0; f < S_MUB; f++)
    if (!fields[f] && n > 0) return e->fail(IS3D_ERR_ARG, "surface field missing");
  const int rc = adopt_surface(e, n, true);
  if (rc || n == 0) return rc;
  for (int f = 0; f < NSURF; f++) {
    double* dst = e->d_surf + (size_t)f * n;
    if (fields[f]) HIPCHK(e, hipMemcpy(dst, fields[f], n * sizeof(double), hipMemcpyHostToDevice));
    else HIPCHK(e, hipMemset(dst, 0, n * sizeof(double)));
  }
  return IS3D_OK;
}

extern "C" int is3d_set_surface_device(is3d_engine* e, long n, const double* dev_fields) {
  if (e && e->grp) return is3d::group_set_surface_device(e->grp, n, dev_fields);
  if (!e || n < 0 || (!dev_fields && n > 0)) return e ? e->fail(IS3D_ERR_ARG, "bad device surface") : IS3D_ERR_ARG;
  (void)adopt_surface(e, n, false);
  e->d_surf = const_cast<double*>(dev_fields);
  return IS3D_OK;
}

extern "C" int is3d_internal_copy_surface(is3d_engine* e, long n, const double* src, long src_n, int src_device, long lo) {
  if (!e || e->grp || n < 0 || lo < 0 || lo + n > src_n || (!src && n > 0)) return e ? e->fail(IS3D_ERR_ARG, "bad surface copy") : IS3D_ERR_ARG;
  HIPCHK(e, hipSetDevice(e->device));
  const int rc = adopt_surface(e, n, true);
  if (rc) return rc;
  for (int f = 0; f < NSURF && n > 0; f++)
    HIPCHK(e, hipMemcpyPeer(e->d_surf + (size_t)f * n, e->device, src + (size_t)f * src_n + lo, src_device, n * sizeof(double)));
  return IS3D_OK;
}

extern "C" long is3d_output_size(const is3d_engine* e) {
  if (e && e->grp) return is3d::group_output_size(e->grp);
  if (!e || !e->have_species || !e->have_grid || !e->have_params) return -1;
  const long ny = (e->p.dimension == 3) ? (long)e->y.size() : 1;
  return (long)e->mass.size() * (long)e->pT.size() * (long)e->phi.size() * ny;
}

static PrepConsts make_consts(const is3d_engine* e) {
  PrepConsts k{};
  k.operation = 1;
  k.df_mode = e->p.df_mode; k.dim = e->p.dimension; k.include_baryon = e->p.include_baryon;
  k.include_bulk = e->p.include_bulk_deltaf; k.include_shear = e->p.include_shear_deltaf;
  k.include_diff = e->p.include_baryondiff_deltaf;
  k.deta_min = e->p.deta_min; k.mass_pion0 = e->p.mass_pion0;
  k.gla_pts = e->gla_pts;
  if (e->have_gla) {
    k.gla_r1 = e->d_gla + 1 * e->gla_pts; k.gla_r2 = e->d_gla + 2 * e->gla_pts;
    const double* w = e->d_gla + (size_t)e->gla_alpha * e->gla_pts;
    k.gla_w1 = w + 1 * e->gla_pts; k.gla_w2 = w + 2 * e->gla_pts;
  }
  k.two_pi2_hbarC3 = 2.0 * std::pow(M_PI, 2) * std::pow(kHbarC, 3);
  k.pT_max = 0.0; k.b_max = 0.0;
  for (double v : e->pT) k.pT_max = std::max(k.pT_max, std::fabs(v));
  for (double v : e->baryon) k.b_max = std::max(k.b_max, std::fabs(v));
  return k;
}

// ---- host sequences the entry points share ---------------------------------------------------------------------
// cells [lo, hi) of the held surface that a launch covers: the cell window, or every cell
static void cell_window(const is3d_engine* e, long& lo, long& hi) {
  lo = e->win_hi >= 0 ? e->win_lo : 0;
  hi = e->win_hi >= 0 ? e->win_hi : e->ncell;
}

// a launch's prologue on its stream: fresh stats, the error word and the counters cleared, ev[0] recorded
static int begin_stats(is3d_engine* e, long cells, hipStream_t st) {
  e->st = is3d_stats{};
  e->st.cells = cells;
  HIPCHK(e, hipMemsetAsync(e->d_err.get(), 0, sizeof(int), st));
  HIPCHK(e, hipMemsetAsync(e->d_cnt.get(), 0, 8 * sizeof(unsigned long long), st));
  HIPCHK(e, hipEventRecord(e->ev[0].get(), st));
  return IS3D_OK;
}

// ... and the stage times between its four events, once ev[3] has completed
static void read_timings(is3d_engine* e) {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, e->ev[0].get(), e->ev[1].get()) == hipSuccess) e->st.ms_prepass = ms;
  if (hipEventElapsedTime(&ms, e->ev[1].get(), e->ev[2].get()) == hipSuccess) e->st.ms_spectra = ms;
  if (hipEventElapsedTime(&ms, e->ev[0].get(), e->ev[3].get()) == hipSuccess) e->st.ms_total = ms;
}

// the prepass of cells [c0, c1) of the held surface into rec / aux (operation 1; a caller for another sets k.operation)
static PrepArgs prep_args(const is3d_engine* e, double* rec, double* aux, long c0, long c1, int* err,
                          unsigned long long* cnt) {
  PrepArgs pa{};
  pa.k = make_consts(e); pa.tb = e->dtb; pa.surf = e->d_surf; pa.rec = rec; pa.aux = aux; pa.n = e->ncell;
  pa.c0 = c0; pa.c1 = c1;
  pa.err = err; pa.cnt = cnt;
  return pa;
}
// f(std::integral_constant<int, MODE>{}) for df_mode `mode`: the one place a templated launcher's mode is chosen.
// FIRST: the lowest mode the site sees (an F_FB launch: PTM), so that it names no launcher for the modes below it
template <int FIRST = GRAD, class F>
static void with_mode(int mode, F f) {
  if constexpr (FIRST <= GRAD) { if (mode == GRAD) return f(std::integral_constant<int, GRAD>{}); }
  if constexpr (FIRST <= CE) { if (mode == CE) return f(std::integral_constant<int, CE>{}); }
  if (mode == PTM) return f(std::integral_constant<int, PTM>{});
  if (mode == PTB) return f(std::integral_constant<int, PTB>{});
  return f(std::integral_constant<int, PTMA>{});
}

static int enqueue_prep(is3d_engine* e, const PrepArgs& pa, hipStream_t st) {
  const dim3 g1((unsigned)std::max(1L, (pa.c1 - pa.c0 + 255) / 256)), b1(256);
  with_mode(e->p.df_mode, [&](auto M) { hipLaunchKernelGGL(k_prep<decltype(M)::value>, g1, b1, 0, st, pa); });
  HIPCHK(e, hipGetLastError());
  return IS3D_OK;
}

// PTM: the renormalisation factors of cells [c0, c0 + n) (records and aux of `stride` cells), one per renorm class
static int enqueue_renorm(is3d_engine* e, const PrepConsts& k, long c0, long n, long stride, hipStream_t st) {
  const long tot = n * (long)e->nrcls;
  if (!e->d_renorm.reserve(tot)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(renorm) failed");
  RenormArgs ra{};
  ra.k = k; ra.rec = e->d_rec.get(); ra.aux = e->d_aux.get(); ra.renorm = e->d_renorm.get();
  ra.mass = e->d_smass; ra.sign = e->d_ssign; ra.degen = e->d_sdegen; ra.baryon = e->d_sbaryon;
  ra.c0 = c0; ra.n = n; ra.stride = stride;
  ra.npart = e->nrcls; ra.rrep = e->d_rrep;
  hipLaunchKernelGGL(k_renorm, dim3((unsigned)std::max(1L, (tot + 255) / 256)), dim3(256), 0, st, ra);
  HIPCHK(e, hipGetLastError());
  return IS3D_OK;
}

// operation 2: the plasma-average densities (DeltafData.cpp:555-690) into dens[3 npart], synchronously.  Returns the
// device error word (df_error maps it), or -1 after a HIP failure (the engine's error is set)
static int plasma_densities(is3d_engine* e, const double* plasma, double* dens) {
  const int np = (int)e->mass.size();
  DensArgs da{};
  da.tb = e->dtb; da.gla = e->d_gla; da.gla_alpha = e->gla_alpha; da.gla_pts = e->gla_pts;
  da.T = plasma[0]; da.E = plasma[1]; da.P = plasma[2]; da.muB = plasma[3]; da.nB = plasma[4];
  da.smass = e->d_smass; da.ssign = e->d_ssign; da.sdegen = e->d_sdegen; da.sbaryon = e->d_sbaryon; da.sorig = e->d_sorig;
  da.npart = np; da.df_mode = e->p.df_mode; da.two_pi2_hbarC3 = 2.0 * std::pow(M_PI, 2) * std::pow(kHbarC, 3);
  da.dens = dens; da.err = e->d_err.get();
  int derr = 0;
  hipError_t h = hipMemset(e->d_err.get(), 0, sizeof(int));
  if (h == hipSuccess) {
    hipLaunchKernelGGL(k_densities, dim3((unsigned)np), dim3(64), 0, 0, da);
    h = hipGetLastError();
  }
  if (h == hipSuccess) h = hipDeviceSynchronize();
  if (h == hipSuccess) h = hipMemcpy(&derr, e->d_err.get(), sizeof(int), hipMemcpyDeviceToHost);
  if (h != hipSuccess) { hip_fail(e, h, "plasma densities"); return -1; }
  return derr;
}

// A launch in stages: launch_begin (prepass up to PTMA's warm-start chains), chain_pass x npass + chain_end (the
// chains), launch_end (PTMA C/B matrices, PTM renormalisation, the integral, the reduction).  is3d_launch runs them
// back to back; a device group whose shards solve their own ranges of the chains (group.hip) interleaves the
// shards' passes with the boundary hand-offs between them.
//
// prepass_begin is launch_begin without an output buffer: it starts the launch context, enqueues the records and, for
// PTMA, the Newton inputs and the (lambda, aT, aL) solution d_sol [6][n] -- cold (k_aniso) or the start of the chains
// that chain_pass x npass + chain_end complete -- with the counters in d_cnt.  srule: the chain rule (aniso_math.h
// aniso_cell), 0 for the spectra, 1 for the particle sampler (is3d_sample_famod).  op: the prep constants' operation
// (1; 0 for is3d_calculate_dN_dX_famod).  L.empty: no cell in the window.
static int prepass_begin(is3d_engine* e, void* stream, long q0, long q1, int has_pred, int srule, int op) {
  HIPCHK(e, hipSetDevice(e->device));
  LaunchCtx& L = e->lc;
  L = LaunchCtx{};
  hipStream_t st = (hipStream_t)stream;
  L.st = st;
  const long n = e->ncell;
  const int mode = e->p.df_mode;
  // cell window (group shards holding the whole surface): k_spectra integrates [wlo, whi); the prepass covers
  // the window too, except for PTMA's warm-start chains, which walk every cell (MomentumSpectra.cpp:1308-1364) --
  // or, when a device group splits the chains (q1 >= 0), the cells of this shard's positions, which are its window
  long wlo, whi;
  cell_window(e, wlo, whi);
  const long nw = whi - wlo;
  const bool chained = mode == PTMA && e->p.famod_chains > 0;
  const bool split_chain = chained && q1 >= 0;
  const long p0 = chained && !split_chain ? 0 : wlo, p1 = chained && !split_chain ? n : whi;
  L.wlo = wlo; L.whi = whi; L.nw = nw; L.p0 = p0; L.p1 = p1; L.chained = chained;
  int rc = begin_stats(e, nw, st);
  if (rc) return rc;
  if (nw == 0) {
    L.empty = true;
    return IS3D_OK;
  }
  if (!e->d_rec.reserve((long)NREC * n)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(records) failed");
  if (!e->d_aux.reserve(9L * n)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(aux) failed");
  if (mode == PTMA && !e->d_sol.reserve(6L * n)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(sol) failed");
  L.pa = prep_args(e, e->d_rec.get(), e->d_aux.get(), p0, p1, e->d_err.get(), e->d_cnt.get());
  L.pa.k.operation = op;
  rc = enqueue_prep(e, L.pa, st);
  if (rc) return rc;
  if (mode == PTMA) {
    AnisoArgs aa{};
    aa.rec = e->d_rec.get(); aa.ain = e->d_aux.get(); aa.sol = e->d_sol.get(); aa.stride = n;
    aa.c0 = p0; aa.n = p1 - p0;
    aa.chains = chained ? std::min<long>(e->p.famod_chains, n) : std::max(1L, p1 - p0);
    const int nh = e->n_aniso_h;
    aa.h = Hadrons{nh, e->d_aniso_h, e->d_aniso_h + nh, e->d_aniso_h + 2 * nh};
    aa.fp2 = 4.0 * std::pow(M_PI, 2) * std::pow(kHbarC, 3);
    aa.cnt = e->d_cnt.get();
    aa.srule = srule;
    if (!chained) {
      hipLaunchKernelGGL(k_aniso, dim3((unsigned)aa.chains), dim3(64), 0, st, aa);
      HIPCHK(e, hipGetLastError());
    } else {
      // warm-start chains in parallel segments (k_chain_pass): ~16k segments of this engine's positions keep the
      // GPU full
      ChainArgs& ca = L.ca;
      ca.rec = e->d_rec.get(); ca.ain = e->d_aux.get(); ca.sol = e->d_sol.get(); ca.n = n; ca.C = aa.chains; ca.h = aa.h; ca.fp2 = aa.fp2;
      ca.srule = srule;
      const long P = (n + ca.C - 1) / ca.C;
      ca.q0 = split_chain ? q0 : 0;
      ca.q1 = split_chain ? std::min(q1, P) : P;
      ca.has_pred = split_chain && has_pred && ca.q0 > 0;
      const long npos = std::max(1L, ca.q1 - ca.q0);
      // ~IS3D_CHAIN_SLOTS segments of at least IS3D_CHAIN_L positions (sized to the GPU's resident k_chain_pass
      // wavefronts instead -- 2048, L = 49 at 10^5 cells -- measured the same: profiles/round4_r4b_ab_newton.log)
      long slots = IS3D_CHAIN_SLOTS;
      if (const char* v = std::getenv("IS3D_CHAIN_SLOTS")) slots = std::max(1L, std::atol(v));   // A/B knob
      const long spc_max = std::max(1L, slots / ca.C);
      ca.L = std::max((long)IS3D_CHAIN_L, (npos + spc_max - 1) / spc_max);
      ca.nspc = (npos + ca.L - 1) / ca.L;
      ca.npass = kChainPasses;
      if (const char* v = std::getenv("IS3D_CHAIN_PASSES")) ca.npass = std::max(1, std::min(kChainPasses, std::atoi(v)));
      const long nseg = ca.C * ca.nspc, bw = 4 * ca.C + 1;
      const long need = 4 * n + (n + 1) / 2 + 12 * nseg + kChainPasses + 2 * kBndSlots * bw;
      if (!e->d_chain.reserve(need)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(chain state) failed");
      ca.sta = e->d_chain.get(); ca.info = (int*)(e->d_chain.get() + 4 * n);
      ca.send = e->d_chain.get() + 4 * n + (n + 1) / 2; ca.sstart = ca.send + 8 * nseg;
      ca.changed = (int*)(ca.sstart + 4 * nseg);
      ca.bin = ca.sstart + 4 * nseg + kChainPasses;
      ca.bout = ca.bin + kBndSlots * bw;
      HIPCHK(e, hipMemsetAsync(ca.changed, 0, kChainPasses * sizeof(int), st));
    }
  }
  return IS3D_OK;
}

static int chain_pass(is3d_engine* e, int pass) {
  LaunchCtx& L = e->lc;
  if (L.empty || !L.chained) return IS3D_OK;
  HIPCHK(e, hipSetDevice(e->device));
  hipLaunchKernelGGL(k_chain_pass, dim3((unsigned)(L.ca.C * L.ca.nspc)), dim3(64 * IS3D_CHAIN_W), 0, L.st, L.ca, pass);
  HIPCHK(e, hipGetLastError());
  return IS3D_OK;
}

static int chain_end(is3d_engine* e) {
  LaunchCtx& L = e->lc;
  if (L.empty || !L.chained) return IS3D_OK;
  HIPCHK(e, hipSetDevice(e->device));
  const long c_lo = L.ca.q0 * L.ca.C, c_hi = std::min(e->ncell, L.ca.q1 * L.ca.C);
  hipLaunchKernelGGL(k_chain_finish, dim3(1), dim3(64 * IS3D_CHAIN_W), 0, L.st, L.ca);
  hipLaunchKernelGGL(k_chain_count, dim3((unsigned)std::min(1024L, std::max(1L, (c_hi - c_lo + 255) / 256))), dim3(256), 0,
                     L.st, (const double*)e->d_rec.get(), (const int*)L.ca.info, c_lo, c_hi, e->d_cnt.get());
  HIPCHK(e, hipGetLastError());
  return IS3D_OK;
}

// the whole prepass of a launch on this engine alone: prepass_begin, every chain pass, chain_end
static int run_prepass(is3d_engine* e, void* stream, int srule, int op) {
  int rc = prepass_begin(e, stream, 0, -1, 0, srule, op);
  for (int pass = 0; !rc && e->lc.chained && pass < e->lc.ca.npass; pass++) rc = chain_pass(e, pass);
  return rc ? rc : chain_end(e);
}

// whole: the chains too (run_prepass: is3d_launch); otherwise the caller stages them (a chain range q0, q1, has_pred)
static int launch_begin(is3d_engine* e, double* dev_out, void* stream, long q0, long q1, int has_pred, bool whole = false) {
  int rc = finalize_tables(e);
  if (rc) return rc;
  if (!dev_out) return e->fail(IS3D_ERR_ARG, "null output buffer");
  rc = whole ? run_prepass(e, stream, 0, 1) : prepass_begin(e, stream, q0, q1, has_pred, 0, 1);
  if (rc) return rc;
  e->lc.dev_out = dev_out;
  if (e->lc.empty) HIPCHK(e, hipMemsetAsync(dev_out, 0, is3d_output_size(e) * sizeof(double), e->lc.st));
  return IS3D_OK;
}

// PTMA: the C / B matrices of cells [p0, p1) of the launch in flight from their (lambda, aT, aL) in d_sol
static int enqueue_famod_b(is3d_engine* e) {
  const LaunchCtx& L = e->lc;
  hipLaunchKernelGGL(k_famod_b, dim3((unsigned)std::max(1L, (L.p1 - L.p0 + 255) / 256)), dim3(256), 0, L.st, L.pa,
                     (const double*)e->d_sol.get());
  HIPCHK(e, hipGetLastError());
  return IS3D_OK;
}

// the prepass counters of a launch whose stream has been waited for: d_cnt -> the stats
static int read_counters(is3d_engine* e) {
  unsigned long long cnt[4] = {0, 0, 0, 0};
  HIPCHK(e, hipMemcpy(cnt, e->d_cnt.get(), sizeof(cnt), hipMemcpyDeviceToHost));
  e->st.breakdown = (long)cnt[0]; e->st.pl_negative = (long)cnt[1]; e->st.recon_fail = (long)cnt[2]; e->st.iterations = (long)cnt[3];
  return IS3D_OK;
}

// Cell splits and slab geometry of one k_spectra plan over a launch window of nw cells.
struct IntegralPlan {
  SpectraPlan P;
  long ntask = 0, bx = 0, wgs = 0, nsplit = 0, cps = 0, sstride = 0, nsplit_fb = 0;
  // F_TS table chunks: spc splits per chunk, nchunk chunks; fold: each chunk's slabs are folded into one accumulator
  // slab as soon as the chunk is integrated (3+1D, several chunks), so the slabs take 1 + 2 spc output sizes of HBM
  // instead of nsplit (config 4: 947 -> 67 slabs, 47 -> 3.4 GB)
  long spc = 0, nchunk = 0, rw = 0;
  bool fold = false;
  long slabs() const { return fold ? 1 + 2 * spc : nsplit + nsplit_fb; }
};

// F_TS chunking of plan I over nw cells: tables of the whole window up to phitab_one bytes in one chunk, larger ones in
// chunks of whole cell splits of about phitab_chunk bytes; both within half the device's free memory (plus the table
// buffers this engine already holds)
static void ts_chunking(is3d_engine* e, IntegralPlan& I) {
  const int npT = (int)e->pT.size();
  I.rw = phitab_row(e->p.df_mode, I.P.KJ, I.P.by != 0);
  const long per_split = I.cps * (long)npT * I.rw;
  const long whole = per_split * I.nsplit * 8;          // bytes of the whole surface's rows
  long one = e->phitab_one, chunk = e->phitab_chunk;
  {
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess && tot > 0) {
      const long avail = (long)(fr / 2) + (e->d_phtab.capacity() + e->d_phtab2.capacity()) * (long)sizeof(double);
      one = std::min(one, avail);
      chunk = std::max(8L * per_split, std::min(chunk, avail / 2));
    }
  }
  const long budget = whole <= one ? whole : chunk;
  I.spc = std::max(1L, std::min(I.nsplit, budget / 8 / per_split));
  I.nchunk = (I.nsplit + I.spc - 1) / I.spc;
  I.fold = I.nchunk > 1 && e->p.dimension == 3 && I.nsplit_fb == 0;
}

static int integral_plan(is3d_engine* e, const SpectraPlan& P, long nw, IntegralPlan& I, long cap_slabs = 0) {
  const int dim = e->p.dimension, mode = e->p.df_mode;
  const int npT = (int)e->pT.size();
  const int nk = (dim == 3) ? (int)e->y.size() : 1, nl = (dim == 3) ? 1 : (int)e->eta.size();
  const int KJ = P.KJ, njb = P.njb;
  if (!spectra_kj_supported(KJ)) return e->fail(IS3D_ERR_ARG, "internal: no k_spectra instantiation for this phi block");
  if (P.shmem > 160 * 1024) return e->fail(IS3D_ERR_ARG, "momentum grid too large for the LDS tile (phi table)");
  const int nc = e->ncls;      // lane species: one per integrand class (the reduction writes the members)
  const long ntask = (long)nc * nk * nl * njb;
  const long bx = (ntask + kBlock - 1) / kBlock;            // lane groups per pT (F_MP: 1, ntask <= 128)
  if (!P.ly) {
    // k_spectra's LDS row tables hold nqmax rows per cell; a lane group spanning more would compute nothing
    // (its slab is NaN-filled, rows_ok), so refuse the launch here instead of returning NaN spectra
    for (long g = 0; g < bx; g++) {
      const long t0 = g * kBlock, t1 = std::min(ntask, t0 + kBlock) - 1;
      if (t1 / nc - t0 / nc + 1 > P.nqmax)
        return e->fail(IS3D_ERR_ARG, "internal: k_spectra lane group spans more q rows than the LDS plan");
    }
  }
  // workgroups per cell split: lane groups x pT values, or F_MP's pT groups of npw
  const long npg = P.mp ? (npT + P.npw - 1) / P.npw : npT;
  const long wgs = bx * npg;
  // cell splits: enough workgroups to fill the chip (>= 8k), and each split's records small enough
  // (~0.5 MB, with the PTM renormalisation rows 2 MB) to stay in one XCD's 4 MB L2 while that XCD's workgroups stream them; a multiple of 8
  // so every XCD owns whole splits; at most IS3D_MAX_SPLITS slabs (each one output-sized)
  const long kTile = P.tile;                              // cells per tile of this mode's k_spectra
  const long max_split = std::max(1L, (nw + kTile - 1) / kTile);
  // (F_MP launches aim for 2k: their 2+1D slabs hold every eta node, and k_reduce_wave's reads across 1k
  // splits cost config 1's shape 0.5 ms of a 4.7 ms pass -- Grad 4.7 -> 4.2 ms, RTA-CE 5.4 -> 5.0 ms with 2k,
  // while the F_LY launch of the modified modes lost 14% with it: profiles/round3_r3p_ab_fill.log)
  const long by_fill = ((P.mp ? IS3D_FILL_WGS_MP : IS3D_FILL_WGS) + wgs - 1) / wgs;
  const long by_l2 = ((long)NREC * 8 * nw + e->split_bytes - 1) / e->split_bytes;
  const long sstride = (long)npT * bx * KJ * kBlock;
  // slab memory: the tuning cap, and at most half of the device's total memory -- deterministic inputs only, since
  // the split count sets the summation order (free memory changes from launch to launch with other engines, ranks
  // and torch's cache; it decides only the F_TS chunking and folding below, which leave the bits unchanged)
  long slab_budget = e->slab_bytes;
  {
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess && tot > 0) slab_budget = std::min(slab_budget, (long)(tot / 2));
  }
  long max_slabs = std::max(8L, std::min(e->max_splits, (slab_budget / 8) / std::max(1L, sstride)));
  if (cap_slabs > 0) max_slabs = std::min(max_slabs, cap_slabs);
  long nsplit = std::max(by_fill, std::min(by_l2, max_slabs));
  if (nsplit >= 8) nsplit = (nsplit + 7) / 8 * 8;
  nsplit = std::max(1L, std::min(nsplit, max_split));
  long cps = std::max(1L, (nw + nsplit - 1) / nsplit);
  cps = ((cps + kTile - 1) / kTile) * kTile;
  nsplit = std::max(1L, (nw + cps - 1) / cps);
  I.P = P; I.ntask = ntask; I.bx = bx; I.wgs = wgs; I.nsplit = nsplit; I.cps = cps; I.sstride = sstride;
  // modified modes: the F_FB launch (separable-fallback lanes, cells listed by k_fbcount / k_fbwrite) writes its own
  // nsplit_fb slabs after the main ones; k_reduce sums both
  I.nsplit_fb = (mode >= PTM) ? std::max(1L, std::min(nsplit, 8L)) : 0;
  if (P.ts) ts_chunking(e, I);
  return IS3D_OK;
}

// the integral of one plan over the launch window (records rec_w, nw cells) into the slabs; gate: launch_end's
// device-side choice between two plans (kernels.h gate_closed), nullptr = unconditional
static int enqueue_spectra(is3d_engine* e, const IntegralPlan& I, const double* rec_w, long nw, hipStream_t st,
                           const unsigned long long* gate, int want) {
  const SpectraPlan& P = I.P;
  const int mode = e->p.df_mode, dim = e->p.dimension;
  const int npT = (int)e->pT.size(), nphi = (int)e->phi.size();
  const int ny_out = (dim == 3) ? (int)e->y.size() : 1;
  const int nk = ny_out, nl = (dim == 3) ? 1 : (int)e->eta.size();
  const int KJ = P.KJ, njb = P.njb, nc = e->ncls;
  const long nsplit = I.nsplit, cps = I.cps, wgs = I.wgs;
  if (mode >= PTM) {
    if (!e->d_fb.reserve(nw + 1 + kFbBlocks)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(fallback list) failed");
    enqueue_fbscan(rec_w, nw, e->d_fb.get(), st);
    HIPCHK(e, hipGetLastError());
  }
  SpecArgs sa{};
  sa.err = e->d_err.get();
  sa.rec = rec_w; sa.n = nw; sa.renorm = e->d_renorm.get(); sa.rcls = e->d_crcls; sa.nrcls = e->nrcls; sa.slab = e->d_slab.get();
  sa.outsize = is3d_output_size(e);
  sa.smass = e->d_cmass; sa.ssign = e->d_csign; sa.sbaryon = e->d_cbaryon; sa.sorig = e->d_sorig;
  sa.csg = e->d_csg;
  sa.pT = e->d_pT; sa.cphi = e->d_cphi; sa.sphi = e->d_sphi; sa.yv = e->d_y; sa.etav = e->d_eta; sa.etaw = e->d_etaw;
  sa.npart = nc; sa.npT = npT; sa.nphi = nphi; sa.ny_out = ny_out; sa.nk = nk; sa.nl = nl; sa.nq = nk * nl; sa.njb = njb;
  sa.nqmax = P.nqmax;
  sa.ntask = I.ntask; sa.cells_per_split = cps; sa.nbx = (int)I.bx; sa.nsplit = (int)nsplit; sa.sstride = I.sstride;
  sa.npw = P.npw;
  sa.regulate = e->p.regulate_deltaf; sa.outflow = e->p.outflow; sa.dim = dim; sa.op = 1;
  sa.gate = gate; sa.gate_want = want;
  const size_t shmem = P.shmem;
  const int tb = P.tb | P.ly | P.t8 | P.mp | P.ts | P.by;
  const int kflags = (e->p.regulate_deltaf ? F_REG : 0) | (e->p.outflow ? F_OUT : 0) | tb;
  if (P.ts) {
    // F_TS: k_phitab writes the per-(cell, pT, phi) rows of a chunk of whole cell splits (at most
    // phitab_chunk bytes, is3d_set_tuning), then k_spectra integrates that chunk's splits; one chunk at config 2
    // (3.7 GB).  Several chunks (config 4: 61 GB of rows) alternate between the launch stream and a side stream
    // with a table buffer each, so the next chunk's k_phitab and the first workgroups of its k_spectra fill the
    // CUs the previous launch's last workgroups leave idle (config 4: 11 chunks ran 2811 ms back to back, one
    // 61 GB chunk 2739 ms)
    const long rw = I.rw, spc = I.spc, nchunk = I.nchunk;
    const long phn = spc * cps;
    e->last_nchunk = nchunk;
    if (!e->d_phtab.reserve(phn * npT * rw)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(phi tables) failed");
    if (nchunk > 1) {
      if (!e->d_phtab2.reserve(phn * npT * rw)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(phi tables) failed");
      if (!e->side) HIPCHK(e, e->side.create(hipStreamNonBlocking));
      if (!e->fork) HIPCHK(e, e->fork.create(hipEventDisableTiming));
      if (!e->join) HIPCHK(e, e->join.create(hipEventDisableTiming));
      HIPCHK(e, hipEventRecord(e->fork.get(), st));
      HIPCHK(e, hipStreamWaitEvent(e->side.get(), e->fork.get(), 0));
    }
    if (I.fold) {
      if (!e->fold_st) HIPCHK(e, e->fold_st.create(hipStreamNonBlocking));
      for (auto* v : {&e->ev_spec[0], &e->ev_spec[1], &e->ev_fold[0], &e->ev_fold[1], &e->fold_join})
        if (!*v) HIPCHK(e, v->create(hipEventDisableTiming));
      HIPCHK(e, hipStreamWaitEvent(e->fold_st.get(), e->fork.get(), 0));
    }
    // folded: slab 0 is the accumulator, chunk ic's splits go to buffer ic & 1 (slabs 1 + (ic & 1) spc ...)
    const int fgrid = (int)std::min(4096L, std::max(1L, (I.sstride + 255) / 256));
    for (long ic = 0; ic < nchunk; ic++) {
      const long s0 = ic * spc, ns = std::min(spc, nsplit - s0);
      const long c0 = s0 * cps, ncc = std::min(nw, (s0 + ns) * cps) - c0;
      hipStream_t cs = (ic & 1) ? e->side.get() : st;
      double* tab = (ic & 1) ? e->d_phtab2.get() : e->d_phtab.get();
      PhiTabArgs ta{};
      ta.rec = rec_w; ta.c0 = c0; ta.nc = ncc; ta.pT = e->d_pT; ta.cphi = e->d_cphi; ta.sphi = e->d_sphi;
      ta.npT = npT; ta.nphi = nphi; ta.nphp = KJ; ta.tab = tab; ta.phn = phn; ta.by = P.by != 0;
      ta.gate = gate; ta.gate_want = want;
      SpecArgs sc = sa;
      sc.split0 = (int)s0; sc.nsplit = (int)ns; sc.phtab = tab; sc.phn = phn; sc.phc0 = c0; sc.phrow = (int)rw;
      double* buf = e->d_slab.get() + (1 + (ic & 1) * spc) * I.sstride;
      if (I.fold) { sc.slab = buf; sc.slab0 = (int)s0; }
      const dim3 grid((unsigned)(wgs * ns));
      if (mode == GRAD) launch_phitab<GRAD>(cs, ta);
      else launch_phitab<CE>(cs, ta);
      // a folded chunk reusing slab buffer ic & 1 waits for the fold of chunk ic - 2, which emptied it
      if (I.fold && ic >= 2) HIPCHK(e, hipStreamWaitEvent(cs, e->ev_fold[ic & 1].get(), 0));
      if (mode == GRAD) launch_spectra<GRAD>(grid, shmem, cs, sc, kflags, KJ);
      else launch_spectra<CE>(grid, shmem, cs, sc, kflags, KJ);
      HIPCHK(e, hipGetLastError());
      if (I.fold) {
        HIPCHK(e, hipEventRecord(e->ev_spec[ic & 1].get(), cs));
        HIPCHK(e, hipStreamWaitEvent(e->fold_st.get(), e->ev_spec[ic & 1].get(), 0));
        hipLaunchKernelGGL(k_fold, dim3((unsigned)fgrid), dim3(256), 0, e->fold_st.get(), e->d_slab.get(), (const double*)buf,
                           I.sstride, (int)ns, ic == 0 ? 1 : 0, gate, want);
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, hipEventRecord(e->ev_fold[ic & 1].get(), e->fold_st.get()));
      }
    }
    if (nchunk > 1) {
      HIPCHK(e, hipEventRecord(e->join.get(), e->side.get()));
      HIPCHK(e, hipStreamWaitEvent(st, e->join.get(), 0));
    }
    if (I.fold) {
      HIPCHK(e, hipEventRecord(e->fold_join.get(), e->fold_st.get()));
      HIPCHK(e, hipStreamWaitEvent(st, e->fold_join.get(), 0));
    }
  } else {
    const dim3 grid((unsigned)(wgs * nsplit));
    with_mode(mode, [&](auto M) { launch_spectra<decltype(M)::value>(grid, shmem, st, sa, kflags, KJ); });
  }
  HIPCHK(e, hipGetLastError());
  if (mode >= PTM) {
    SpecArgs fa = sa;
    fa.slab = e->d_slab.get() + nsplit * I.sstride; fa.nsplit = (int)I.nsplit_fb; fa.cells_per_split = 0;
    fa.fbcells = e->d_fb.get() + 1; fa.fbcount = e->d_fb.get();
    const int fflags = (e->p.regulate_deltaf ? F_REG : 0) | (e->p.outflow ? F_OUT : 0) | F_FB;
    const dim3 gfb((unsigned)(I.bx * npT * I.nsplit_fb));
    with_mode<PTM>(mode, [&](auto M) { launch_spectra<decltype(M)::value>(gfb, P.shmem_fb, st, fa, fflags, KJ); });
    HIPCHK(e, hipGetLastError());
  }
  return IS3D_OK;
}

// sum of one plan's slabs into the reference-layout output (k_reduce / k_reduce_wave), gated as enqueue_spectra
static int enqueue_reduce(is3d_engine* e, const IntegralPlan& I, double* dev_out, hipStream_t st,
                          const unsigned long long* gate, int want) {
  const int dim = e->p.dimension;
  const int npT = (int)e->pT.size(), nphi = (int)e->phi.size();
  const int ny_out = (dim == 3) ? (int)e->y.size() : 1;
  const int nk = ny_out, nl = (dim == 3) ? 1 : (int)e->eta.size();
  const int nc = e->ncls;
  ReduceArgs ra{};
  ra.slab = e->d_slab.get(); ra.sstride = I.sstride; ra.nsplit = I.fold ? 1 : (int)(I.nsplit + I.nsplit_fb);
  ra.nbx = (int)I.bx; ra.npart = nc; ra.npT = npT; ra.nphi = nphi; ra.nk = nk; ra.nl = nl; ra.ny_out = ny_out; ra.kj = I.P.KJ;
  ra.ntask = I.ntask;
  ra.sorig = e->d_sorig; ra.degen_orig = e->d_degen_orig; ra.prefactor = std::pow(2.0 * M_PI * kHbarC, -3);
  ra.cmem_off = e->d_cmem_off; ra.cmem = e->d_cmem;
  ra.out = dev_out;
  ra.gate = gate; ra.gate_want = want;
  // one wavefront per output when each output sums many (eta node, split) terms and there are few outputs
  if ((long)nl * ra.nsplit >= 128 && I.sstride / nl < (1L << 20)) {
    const long nout = (long)nc * npT * nphi * ny_out;
    hipLaunchKernelGGL(k_reduce_wave, dim3((unsigned)((nout + 3) / 4)), dim3(256), 0, st, ra);
  } else {
    hipLaunchKernelGGL(k_reduce, dim3((unsigned)((I.sstride + 255) / 256)), dim3(256), 0, st, ra);
  }
  HIPCHK(e, hipGetLastError());
  return IS3D_OK;
}

static int launch_end(is3d_engine* e) {
  LaunchCtx& L = e->lc;
  hipStream_t st = L.st;
  double* dev_out = L.dev_out;
  HIPCHK(e, hipSetDevice(e->device));
  if (L.empty) {
    HIPCHK(e, hipEventRecord(e->ev[1].get(), st));
    HIPCHK(e, hipEventRecord(e->ev[2].get(), st));
    HIPCHK(e, hipEventRecord(e->ev[3].get(), st));
    e->launched = true;
    return IS3D_OK;
  }
  const long n = e->ncell;
  const int mode = e->p.df_mode;
  const long wlo = L.wlo, nw = L.nw;
  int rc = mode == PTMA ? enqueue_famod_b(e) : mode == PTM ? enqueue_renorm(e, L.pa.k, wlo, nw, n, st) : IS3D_OK;
  if (rc) return rc;
  HIPCHK(e, hipEventRecord(e->ev[1].get(), st));
  // the integral and the reduction see the window only: records from wlo on, nw cells
  const double* rec_w = e->d_rec.get() + wlo * (long)NREC;
  // --- main integral
  // Grad / RTA-CE F_TS: a surface with cells whose lanes may leave the fast path (k_prep counts them in cnt[4]; none
  // in any tabulated delta-f range) needs the kernels that carry the slow loop, which the F_TS ones do not.  The
  // choice is made on the device: both plans are enqueued, each gated on cnt[4] (gate_closed: the other plan's
  // workgroups return at once, ~10 us), so is3d_launch never waits for the prepass (no host round trip)
  const SpectraPlan P = spectra_plan(e, true);
  e->last_nchunk = 0;
  IntegralPlan I{}, J{};
  rc = integral_plan(e, P, nw, I);
  if (rc) return rc;
  e->last_nsplit = I.nsplit;
  e->last_nslab = I.slabs();
  const bool gated = mode <= CE && P.ts;
  if (gated) {
    // the fallback plan shares the slab memory: a folded main plan caps its splits at the same footprint
    rc = integral_plan(e, spectra_plan(e, false), nw, J, I.fold ? I.slabs() : 0);
    if (rc) return rc;
  }
  const long slab_need = std::max(I.slabs() * I.sstride, gated ? J.slabs() * J.sstride : 0L);
  if (!e->d_slab.reserve(slab_need)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(slabs) failed");
  const unsigned long long* gate = gated ? e->d_cnt.get() + 4 : nullptr;
  rc = enqueue_spectra(e, I, rec_w, nw, st, gate, 0);
  if (!rc && gated) rc = enqueue_spectra(e, J, rec_w, nw, st, gate, 1);
  if (rc) return rc;
  HIPCHK(e, hipEventRecord(e->ev[2].get(), st));
  rc = enqueue_reduce(e, I, dev_out, st, gate, 0);
  if (!rc && gated) rc = enqueue_reduce(e, J, dev_out, st, gate, 1);
  if (rc) return rc;
  HIPCHK(e, hipEventRecord(e->ev[3].get(), st));
  e->launched = true;
  return IS3D_OK;
}

extern "C" int is3d_launch(is3d_engine* e, double* dev_out, void* stream) {
  if (e && e->grp) return is3d::group_launch(e->grp, dev_out, stream);
  if (!e) return IS3D_ERR_ARG;
  if (e->chain_q1 >= 0)
    return e->fail(IS3D_ERR_STATE, "a chain range (is3d_set_chain_range) runs through the staged launch: its first "
                                   "positions need the previous range's boundary states");
  const int rc = launch_begin(e, dev_out, stream, 0, -1, 0, true);
  return rc ? rc : launch_end(e);
}

// staged launch for the device group (group.h)
int is3d_internal_launch_begin(is3d_engine* e, double* dev_out, void* stream, long q0, long q1, int has_pred) {
  return launch_begin(e, dev_out, stream, q0, q1, has_pred);
}
int is3d_internal_chain_pass(is3d_engine* e, int pass) { return chain_pass(e, pass); }
int is3d_internal_chain_end(is3d_engine* e) { return chain_end(e); }
int is3d_internal_launch_end(is3d_engine* e) { return launch_end(e); }
int is3d_internal_chain_npass(const is3d_engine* e) { return e->lc.chained && !e->lc.empty ? e->lc.ca.npass : 0; }
// boundary slot k (0, 1: pass parity, 2: final) of this engine's chain range: in (from the previous shard) or out
double* is3d_internal_chain_bnd(is3d_engine* e, int out, int slot) {
  if (!e->lc.chained || e->lc.empty) return nullptr;
  const long bw = 4 * e->lc.ca.C + 1;
  return (out ? e->lc.ca.bout : e->lc.ca.bin) + slot * bw;
}
long is3d_internal_chain_bnd_bytes(const is3d_engine* e) { return (4 * e->lc.ca.C + 1) * (long)sizeof(double); }

// ---- staged launch for PTMA warm-start chains split over processes (include/is3d_amd.h) ----------------------------
extern "C" int is3d_set_chain_range(is3d_engine* e, long q0, long q1) {
  if (!e) return IS3D_ERR_ARG;
  if (e->grp) return is3d::group_fail(e->grp, IS3D_ERR_UNSUPPORTED, "a device-list engine splits its chains itself");
  if (q0 < 0 || q1 < 0) { e->chain_q0 = e->chain_q1 = -1; e->win_lo = e->win_hi = -1; return IS3D_OK; }
  if (!e->have_params || e->p.df_mode != PTMA || e->p.famod_chains <= 0)
    return e->fail(IS3D_ERR_STATE, "a chain range needs PTMA (df_mode 5) with famod_chains > 0 set first");
  const long n = e->ncell, C = std::max(1L, std::min<long>(e->p.famod_chains, std::max(n, 1L))), P = (n + C - 1) / C;
  if (q0 > q1 || q1 > P) return e->fail(IS3D_ERR_ARG, "chain range outside the surface's chain positions");
  e->win_lo = std::min(n, q0 * C);
  e->win_hi = std::min(n, q1 * C);
  e->chain_q0 = q0; e->chain_q1 = q1;
  return IS3D_OK;
}

extern "C" int is3d_launch_begin(is3d_engine* e, double* dev_out, void* stream) {
  if (!e) return IS3D_ERR_ARG;
  if (e->grp) return is3d::group_fail(e->grp, IS3D_ERR_UNSUPPORTED, "the staged launch runs on one-device engines");
  if (e->chain_q1 >= 0 && (e->p.df_mode != PTMA || e->p.famod_chains <= 0))
    return e->fail(IS3D_ERR_STATE, "a chain range needs PTMA with famod_chains > 0 (params changed since)");
  const bool range = e->chain_q1 >= 0;
  if (range) {
    // the integration window follows the chain positions under the current famod_chains C (set_params may have
    // changed C since is3d_set_chain_range): cells [q0 C, q1 C), so the ranks' windows still tile the surface
    const long n = e->ncell, C = std::max(1L, std::min<long>(e->p.famod_chains, std::max(n, 1L))), P = (n + C - 1) / C;
    if (e->chain_q1 > P) return e->fail(IS3D_ERR_ARG, "chain range outside the surface's chain positions (famod_chains changed)");
    e->win_lo = std::min(n, e->chain_q0 * C);
    e->win_hi = std::min(n, e->chain_q1 * C);
  }
  return launch_begin(e, dev_out, stream, range ? e->chain_q0 : 0, range ? e->chain_q1 : -1, range && e->chain_q0 > 0);
}
extern "C" int is3d_chain_passes(const is3d_engine* e) { return e && !e->grp ? is3d_internal_chain_npass(e) : 0; }
extern "C" int is3d_chain_pass(is3d_engine* e, int pass) {
  if (!e || e->grp) return IS3D_ERR_ARG;
  if (pass < 0 || pass >= is3d_internal_chain_npass(e)) return e->fail(IS3D_ERR_ARG, "chain pass out of range");
  return chain_pass(e, pass);
}
extern "C" int is3d_chain_end(is3d_engine* e) { return (!e || e->grp) ? IS3D_ERR_ARG : chain_end(e); }
extern "C" int is3d_launch_end(is3d_engine* e) { return (!e || e->grp) ? IS3D_ERR_ARG : launch_end(e); }
extern "C" long is3d_chain_boundary_size(const is3d_engine* e) {
  return (e && !e->grp && e->lc.chained && !e->lc.empty) ? 4 * e->lc.ca.C + 1 : 0;
}
// boundary slot `slot` (0, 1: pass parity, 2: the finisher's) out of this range into dev_buf / from dev_buf into this
// range's incoming slot, on the launch stream (hipMemcpyDefault: a host buffer works too, read after a stream sync)
extern "C" int is3d_chain_boundary_get(is3d_engine* e, int slot, double* dev_buf) {
  if (!e || e->grp || !dev_buf || slot < 0 || slot >= kBndSlots) return e ? e->fail(IS3D_ERR_ARG, "bad chain boundary slot") : IS3D_ERR_ARG;
  const long nb = is3d_chain_boundary_size(e);
  if (nb == 0) return e->fail(IS3D_ERR_STATE, "no chains in the launch in flight");
  HIPCHK(e, hipSetDevice(e->device));
  HIPCHK(e, hipMemcpyAsync(dev_buf, is3d_internal_chain_bnd(e, 1, slot), nb * sizeof(double), hipMemcpyDefault, e->lc.st));
  return IS3D_OK;
}
extern "C" int is3d_chain_boundary_put(is3d_engine* e, int slot, const double* dev_buf) {
  if (!e || e->grp || !dev_buf || slot < 0 || slot >= kBndSlots) return e ? e->fail(IS3D_ERR_ARG, "bad chain boundary slot") : IS3D_ERR_ARG;
  const long nb = is3d_chain_boundary_size(e);
  if (nb == 0) return e->fail(IS3D_ERR_STATE, "no chains in the launch in flight");
  HIPCHK(e, hipSetDevice(e->device));
  HIPCHK(e, hipMemcpyAsync(is3d_internal_chain_bnd(e, 0, slot), dev_buf, nb * sizeof(double), hipMemcpyDefault, e->lc.st));
  return IS3D_OK;
}

extern "C" int is3d_cell_costs(is3d_engine* e, double* cost) {
  if (e && e->grp) return is3d::group_fail(e->grp, IS3D_ERR_UNSUPPORTED, "is3d_cell_costs: call it on a one-device engine");
  if (!e || !cost) return IS3D_ERR_ARG;
  int rc = finalize_tables(e);
  if (rc) return rc;
  const long n = e->ncell;
  if (n <= 0) return IS3D_OK;
  HIPCHK(e, hipSetDevice(e->device));
  const int mode = e->p.df_mode;
  // private scratch (records, aux, cost, error word, counters), freed on return: a launch in flight keeps its
  // buffers and the error word is3d_finish reports, and a device group's cost prepass over the whole surface
  // (group_set_surface on shard 0) leaves no full-surface-sized buffers behind on that shard
  DevBuf<double> scratch;
  if (!scratch.reserve((long)(NREC + 9 + 1) * n + 9)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(cell cost scratch) failed");
  double* d_rec = scratch.get();
  double* d_aux = d_rec + (size_t)NREC * n;
  double* d_cost = d_aux + 9 * (size_t)n;
  int* d_err = (int*)(d_cost + n);
  unsigned long long* d_cnt = (unsigned long long*)(d_cost + n + 1);
  HIPCHK(e, hipMemsetAsync(d_err, 0, 9 * sizeof(double), nullptr));
  rc = enqueue_prep(e, prep_args(e, d_rec, d_aux, 0, n, d_err, d_cnt), nullptr);
  if (rc) return rc;
  // separable-fallback cells of PTM / PTB relative to a modified cell (config-2 shape, MI355X,
  // tools/fb_cost_probe.py: PTM 1.37-1.43, PTB 1.58-1.80)
  const double fb_cost = mode == PTM ? 1.4 : mode == PTB ? 1.8 : 0.0;
  hipLaunchKernelGGL(k_cell_cost, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, (const double*)d_rec, n, fb_cost, d_cost);
  HIPCHK(e, hipGetLastError());
  HIPCHK(e, hipMemcpy(cost, d_cost, n * sizeof(double), hipMemcpyDeviceToHost));
  return IS3D_OK;
}

extern "C" int is3d_finish(is3d_engine* e) {
  if (e && e->grp) return is3d::group_finish(e->grp);
  if (!e) return IS3D_ERR_ARG;
  if (!e->launched && !e->dk_launched) return e->fail(IS3D_ERR_STATE, "nothing launched");
  HIPCHK(e, hipSetDevice(e->device));
  if (e->dk_launched) {       // is3d_launch_feeddown: no device error word, its own two events
    e->dk_launched = false;
    HIPCHK(e, hipEventSynchronize(e->dk_ev[1].get()));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e->dk_ev[0].get(), e->dk_ev[1].get()) == hipSuccess) e->dk_stats.ms_total = ms;
    if (!e->launched) return IS3D_OK;
  }
  HIPCHK(e, hipEventSynchronize(e->ev[3].get()));
  e->launched = false;
  int derr = 0;
  HIPCHK(e, hipMemcpy(&derr, e->d_err.get(), sizeof(int), hipMemcpyDeviceToHost));
  const int rc = read_counters(e);
  if (rc) return rc;
  read_timings(e);
  return df_error(e, derr, "Error: choose df_mode = (1,2,3,4,5)");
}

// what is3d_calculate_spectra and is3d_calculate_polarization share: launch(d_out) into the engine's output buffer of
// outsize doubles on the null stream, finished and downloaded to `out`
template <class L>
static int calculate(is3d_engine* e, long outsize, double* out, L launch) {
  HIPCHK(e, hipSetDevice(e->device));
  if (!e->d_out.reserve(outsize)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(output) failed");
  int rc = launch(e->d_out.get());
  if (!rc) rc = is3d_finish(e);
  if (rc) return rc;
  HIPCHK(e, hipMemcpy(out, e->d_out.get(), outsize * sizeof(double), hipMemcpyDeviceToHost));
  return IS3D_OK;
}

extern "C" int is3d_calculate_spectra(is3d_engine* e, double* dN_out) {
  if (e && e->grp) return is3d::group_calculate_spectra(e->grp, dN_out);
  if (!e || !dN_out) return e ? e->fail(IS3D_ERR_ARG, "null output") : IS3D_ERR_ARG;
  const int rc = finalize_tables(e);
  if (rc) return rc;
  return calculate(e, is3d_output_size(e), dN_out, [&](double* d) { return is3d_launch(e, d, nullptr); });
}

// operation = 0 (SpacetimeDistribution.cpp:31-1250): device prepass + per-(species, cell) yields + binning
// into thread slices; the host then applies the reference's per-species reset (byte-count memset,
// :165-167 / :628-630) and writes the bin-normalised distributions (:407-440).
//
// dndx_finish is what follows the prepass, shared by is3d_calculate_dN_dX and is3d_calculate_dN_dX_famod: the k_dndx
// launches over cells [wlo, wlo + n) of the held surface (their records in d_rec; the yields go to d_ycell [class][n]),
// the bin keys / CSR / k_stbin and the host epilogue.  The caller has recorded ev[0] and ev[1] on the null stream.
static int dndx_finish(is3d_engine* e, long wlo, long n, const char* df_msg, double* dN_taudtaudy, double* dN_2pirdrdy,
                       double* dN_dphidy) {
  hipStream_t st = nullptr;
  const long nsurf = e->ncell;
  const int mode = e->p.df_mode, dim = e->p.dimension;
  const int np = (int)e->mass.size(), npT = (int)e->pT.size(), nphi = (int)e->phi.size();
  const int nk = (dim == 3) ? (int)e->y.size() : 1, nl = (dim == 3) ? 1 : (int)e->eta.size();
  const is3d_spacetime_bins& B = e->bins;
  const long C = std::max(1, B.threads);
  const int carry = B.threads >= 1;
  const long nb[3] = {B.tau_bins, B.r_bins, B.phip_bins};
  const long nent = C * (nb[0] + nb[1] + nb[2]);
  std::vector<double> part((size_t)np * nent, 0.0);
  if (n > 0) {
    // --- per-(species, cell) yields
    const int KJ = spectra_kj(nphi);
    const int njb = (nphi + KJ - 1) / KJ;
    DndxArgs da{};
    const int nc = e->ncls;    // lane species: the integrand classes (k_stbin scales and writes the members)
    da.ntask = nk * njb * nl;
    da.Sl = std::min(nc, 64);
    da.Yl = 64 / da.Sl;
    da.nbx = (nc + da.Sl - 1) / da.Sl;
    static_assert(is3d::kern::kTile % IS3D_DNDX_TILE_MOD == 0 && is3d::kern::kTile % IS3D_DNDX_TILE == 0,
                  "k_dndx's cells per workgroup (multiples of kTile) hold whole record tiles");
    long cpw = 4L * kTile;
    if ((long)da.nbx * ((n + cpw - 1) / cpw) < 4096) cpw = kTile;
    da.cells_per_wg = cpw;
    da.nchunk = (n + cpw - 1) / cpw;
    if (!e->d_ycell.reserve((long)nc * n)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(cell yields) failed");
    da.rec = e->d_rec.get() + wlo * (long)NREC; da.n = n; da.renorm = e->d_renorm.get(); da.rcls = e->d_crcls; da.nrcls = e->nrcls; da.ycell = e->d_ycell.get();
    da.smass = e->d_cmass; da.ssign = e->d_csign; da.sbaryon = e->d_cbaryon;
    da.pT = e->d_pT; da.pTw = e->d_pTw; da.cphi = e->d_cphi; da.sphi = e->d_sphi; da.phiw = e->d_phiw;
    da.yv = e->d_y; da.etav = e->d_eta; da.etaw = e->d_etaw;
    da.npart = nc; da.npT = npT; da.nphi = nphi; da.nk = nk; da.nl = nl; da.nq = nk * nl; da.njb = njb; da.dim = dim;
    const size_t nphp = (size_t)njb * KJ;
    // kernels.h k_dndx's layout: records, trig / {pc, ps} / phi weights, {b', Phi} rows (not in the modified
    // launch), Qv rows ({PDm, Qv} pairs in the modified launch with phi blocks of fours), per-lane cell sums, grid, y-term rows, exp table, PTM's renorm factors [kTile][Sl]
    auto dndx_lds = [&](bool modmain, bool fb = false) {
      const bool bp = !modmain;
      // kernels.h dndx_tile: the launch's record tile
      const size_t kTile = fb ? is3d::kern::kTile : modmain ? IS3D_DNDX_TILE_MOD : IS3D_DNDX_TILE;
      return sizeof(double) * ((size_t)kTile * NREC + 2 * nphp + 2 * nphp + nphp + (bp ? 2 : 0) * (size_t)kTile * nphp +
                               (modmain && KJ % 4 == 0 ? 2 : 1) * (size_t)kTile * nphp +
                               (size_t)kTile * kBlock + (size_t)(nk + 2 * nl) +
                               (size_t)kTile * da.nq * kYRowLY + (size_t)kExpTabN +
                               (mode == PTM ? (size_t)kTile * da.Sl : 0));
    };
    const size_t shmem = dndx_lds(mode >= PTM), shmem_fb = dndx_lds(false, true);
    if (std::max(shmem, shmem_fb) > 160 * 1024) return e->fail(IS3D_ERR_ARG, "momentum grid too large for the LDS tile");
    const long nwg = (long)da.nbx * da.nchunk;
    if (nwg > 0x7fffffffL) return e->fail(IS3D_ERR_ARG, "surface too large for one dN/dX launch");
    const int kflags = (e->p.regulate_deltaf ? F_REG : 0) | (e->p.outflow ? F_OUT : 0);
    with_mode(mode, [&](auto M) { launch_dndx<decltype(M)::value>(dim3((unsigned)nwg), shmem, st, da, kflags, KJ); });
    HIPCHK(e, hipGetLastError());
    if (mode >= PTM) {
      // the separable-fallback lanes of the cells k_fbwrite lists (breakdown, narrow rapidity windows) in their own
      // launch (kernels.h k_dndx F_FB), added to ycell; the list's length stays on the device, so the grid is sized
      // for the whole surface and the workgroups split whatever the list holds
      if (!e->d_fb.reserve(n + 1 + kFbBlocks)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(fallback list) failed");
      enqueue_fbscan(da.rec, n, e->d_fb.get(), st);
      DndxArgs fa = da;
      fa.fbcells = e->d_fb.get() + 1; fa.fbcount = e->d_fb.get();
      fa.nchunk = std::max(1L, std::min(da.nchunk, (4096L + da.nbx - 1) / da.nbx));
      const long nfw = (long)da.nbx * fa.nchunk;
      with_mode<PTM>(mode, [&](auto M) { launch_dndx<decltype(M)::value>(dim3((unsigned)nfw), shmem_fb, st, fa, kflags | F_FB, KJ); });
      HIPCHK(e, hipGetLastError());
    }
    e->ycell_n = n;
  } else {
    e->ycell_n = 0;
  }
  HIPCHK(e, hipEventRecord(e->ev[2].get(), st));
  if (n > 0) {
    // --- bin keys on the device, CSR (thread slice, bin) -> cells on the host, sums on the device
    if (!e->d_keys.reserve(3 * n)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(keys) failed");
    KeyArgs ka{};
    ka.tau = e->d_surf + wlo; ka.x = e->d_surf + nsurf + wlo; ka.y = e->d_surf + 2 * nsurf + wlo; ka.n = n;
    ka.tau_min = B.tau_min; ka.tau_width = (B.tau_max - B.tau_min) / (double)B.tau_bins;
    ka.r_min = B.r_min; ka.r_width = (B.r_max - B.r_min) / (double)B.r_bins;
    ka.phip_width = 2.0 * M_PI / (double)B.phip_bins;
    ka.tau_bins = B.tau_bins; ka.r_bins = B.r_bins; ka.phip_bins = B.phip_bins; ka.keys = e->d_keys.get();
    hipLaunchKernelGGL(k_stkeys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ka);
    HIPCHK(e, hipGetLastError());
    std::vector<int> keys((size_t)3 * n);
    HIPCHK(e, hipMemcpy(keys.data(), e->d_keys.get(), keys.size() * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<long> offs((size_t)nent + 1, 0);
    long off_d[3] = {0, C * nb[0], C * (nb[0] + nb[1])};
    for (int d = 0; d < 3; d++)
      for (long c = 0; c < n; c++) {
        const int kb = keys[(size_t)d * n + c];
        if (kb >= 0) offs[off_d[d] + ((wlo + c) % C) * nb[d] + kb + 1]++;
      }
    for (long i = 0; i < nent; i++) offs[i + 1] += offs[i];
    std::vector<int> perm((size_t)std::max(offs[nent], 1L));
    std::vector<long> fill(offs.begin(), offs.end() - 1);
    for (int d = 0; d < 3; d++)
      for (long c = 0; c < n; c++) {
        const int kb = keys[(size_t)d * n + c];
        if (kb >= 0) perm[fill[off_d[d] + ((wlo + c) % C) * nb[d] + kb]++] = (int)c;
      }
    if (!e->d_perm.reserve((long)perm.size())) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(perm) failed");
    if (!e->d_offs.reserve(nent + 1)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(offsets) failed");
    if (!e->d_part.reserve((long)np * nent)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(bins) failed");
    HIPCHK(e, hipMemcpy(e->d_perm.get(), perm.data(), perm.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(e->d_offs.get(), offs.data(), offs.size() * sizeof(long), hipMemcpyHostToDevice));
    BinArgs ba{};
    ba.ycell = e->d_ycell.get(); ba.n = n; ba.npart = np;
    ba.perm = e->d_perm.get(); ba.offs = e->d_offs.get(); ba.nent = nent;
    ba.sorig = e->d_sorig; ba.sdegen = e->d_sdegen; ba.prefactor = std::pow(2.0 * M_PI * kHbarC, -3);
    ba.scls = e->d_scls;
    ba.part = e->d_part.get();
    const long nthr = nent * np;
    hipLaunchKernelGGL(k_stbin, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st, ba);
    HIPCHK(e, hipGetLastError());
  }
  HIPCHK(e, hipEventRecord(e->ev[3].get(), st));
  HIPCHK(e, hipEventSynchronize(e->ev[3].get()));
  int derr = 0;
  HIPCHK(e, hipMemcpy(&derr, e->d_err.get(), sizeof(int), hipMemcpyDeviceToHost));
  if (n > 0) HIPCHK(e, hipMemcpy(part.data(), e->d_part.get(), part.size() * sizeof(double), hipMemcpyDeviceToHost));
  read_timings(e);
  if (derr) return df_error(e, derr, df_msg);
  // --- the reference's per-species thread-slice reset and bin normalisation
  const double two_pi = 2.0 * M_PI;
  const double width[3] = {(B.tau_max - B.tau_min) / (double)B.tau_bins, (B.r_max - B.r_min) / (double)B.r_bins,
                           two_pi / (double)B.phip_bins};
  double* outs[3] = {dN_taudtaudy, dN_2pirdrdy, dN_dphidy};
  long off = 0;
  for (int d = 0; d < 3; d++) {
    const long bins = nb[d];
    std::vector<double> all((size_t)C * bins, 0.0);
    for (int k = 0; k < np; k++) {
      if (carry) std::memset(all.data(), 0, (size_t)(C * bins));   // bytes, not doubles (:165-167)
      else std::fill(all.begin(), all.end(), 0.0);
      const double* pk = part.data() + (size_t)k * nent + off;
      for (long t = 0; t < C; t++)
        for (long i = 0; i < bins; i++) all[i + t * bins] += pk[t * bins + i];
      for (long i = 0; i < bins; i++) {
        double acc = 0.0;
        for (long t = 0; t < C; t++) acc += all[i + t * bins];
        double norm = width[d];
        if (d == 0) norm = (B.tau_min + width[0] * ((double)i + 0.5)) * width[0];
        else if (d == 1) norm = two_pi * (B.r_min + width[1] * ((double)i + 0.5)) * width[1];
        outs[d][(size_t)k * bins + i] = acc / norm;
      }
    }
    off += C * bins;
  }
  return IS3D_OK;
}

// the checks the two operation-0 entries share, up to the tables
static int dndx_begin(is3d_engine* e, const double* dN_taudtaudy, const double* dN_2pirdrdy, const double* dN_dphidy) {
  if (!dN_taudtaudy || !dN_2pirdrdy || !dN_dphidy) return e->fail(IS3D_ERR_ARG, "null output");
  if (!e->have_params) return e->fail(IS3D_ERR_STATE, "is3d_set_params not called");
  return IS3D_OK;
}

extern "C" int is3d_calculate_dN_dX(is3d_engine* e, double* dN_taudtaudy, double* dN_2pirdrdy, double* dN_dphidy) {
  if (e && e->grp) return is3d::group_calculate_dN_dX(e->grp, dN_taudtaudy, dN_2pirdrdy, dN_dphidy);
  if (!e) return IS3D_ERR_ARG;
  int rc = dndx_begin(e, dN_taudtaudy, dN_2pirdrdy, dN_dphidy);
  if (rc) return rc;
  if (e->p.df_mode == PTMA)
    return e->fail(IS3D_ERR_UNSUPPORTED, "calculate_spectra error: no spacetime distribution routine for famod yet "
                                         "(the per-cell decomposition of the PTMA spectra: call is3d_calculate_dN_dX_famod)");
  if (!e->have_weights) return e->fail(IS3D_ERR_STATE, "is3d_set_momentum_weights not called");
  if (!e->have_bins) return e->fail(IS3D_ERR_STATE, "is3d_set_spacetime_bins not called");
  rc = finalize_tables(e);
  if (rc) return rc;
  HIPCHK(e, hipSetDevice(e->device));
  hipStream_t st = nullptr;
  const long n = e->ncell;
  rc = begin_stats(e, n, st);
  if (rc) return rc;
  if (n > 0) {
    if (!e->d_rec.reserve((long)NREC * n)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(records) failed");
    if (!e->d_aux.reserve(9L * n)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(aux) failed");
    PrepArgs pa = prep_args(e, e->d_rec.get(), e->d_aux.get(), 0, n, e->d_err.get(), e->d_cnt.get());
    pa.k.operation = 0;
    rc = enqueue_prep(e, pa, st);
    if (!rc && e->p.df_mode == PTM) rc = enqueue_renorm(e, pa.k, 0, n, n, st);
    if (rc) return rc;
  }
  HIPCHK(e, hipEventRecord(e->ev[1].get(), st));
  return dndx_finish(e, 0, n, "Error: set df_mode = (1,2) in parameters.dat", dN_taudtaudy, dN_2pirdrdy, dN_dphidy);
}

// operation = 0 for df_mode 5.  The reference has no routine (EmissionFunction.cpp:1184-1189); this one is the per-cell
// decomposition of calculate_dN_pTdpTdphidy_famod (MomentumSpectra.cpp:1517-1621) binned as the other modes' (DESIGN
// 7.1): the spectra's PTMA prepass (chain rule 0) with operation 0 in the prep constants, then dndx_finish over the
// cell window.  Nothing is kept between calls: every call solves the chains again.
extern "C" int is3d_calculate_dN_dX_famod(is3d_engine* e, double* dN_taudtaudy, double* dN_2pirdrdy, double* dN_dphidy) {
  if (e && e->grp) return is3d::group_calculate_dN_dX_famod(e->grp, dN_taudtaudy, dN_2pirdrdy, dN_dphidy);
  if (!e) return IS3D_ERR_ARG;
  int rc = dndx_begin(e, dN_taudtaudy, dN_2pirdrdy, dN_dphidy);
  if (rc) return rc;
  if (e->p.df_mode != PTMA)
    return e->fail(IS3D_ERR_UNSUPPORTED, "is3d_calculate_dN_dX_famod: needs df_mode 5 (df_mode 1-4: is3d_calculate_dN_dX)");
  if (e->chain_q1 >= 0)
    return e->fail(IS3D_ERR_STATE, "is3d_calculate_dN_dX_famod: a chain range is set (is3d_set_chain_range); this entry solves the whole chain");
  if (!e->have_weights) return e->fail(IS3D_ERR_STATE, "is3d_set_momentum_weights not called");
  if (!e->have_bins) return e->fail(IS3D_ERR_STATE, "is3d_set_spacetime_bins not called");
  rc = finalize_tables(e);
  if (rc) return rc;
  rc = run_prepass(e, nullptr, 0, 0);
  const LaunchCtx& L = e->lc;
  if (!rc && !L.empty) rc = enqueue_famod_b(e);
  if (rc) return rc;
  HIPCHK(e, hipEventRecord(e->ev[1].get(), L.st));
  rc = dndx_finish(e, L.wlo, L.nw, "Error: choose df_mode = (1,2,3,4,5)", dN_taudtaudy, dN_2pirdrdy, dN_dphidy);
  return rc ? rc : read_counters(e);     // dndx_finish has waited for the stream
}

extern "C" int is3d_get_cell_yields(const is3d_engine* e, double* dN_dy_cell) {
  if (e && e->grp) return is3d::group_get_cell_yields(e->grp, dN_dy_cell);
  if (!e || !dN_dy_cell) return IS3D_ERR_ARG;
  if (e->ycell_n < 0) return IS3D_ERR_STATE;
  const long n = e->ycell_n;
  const int np = (int)e->mass.size();
  if (n == 0) return IS3D_OK;
  std::vector<double> y((size_t)e->ncls * n);
  if (hipSetDevice(e->device) != hipSuccess) return IS3D_ERR_DEVICE;
  if (hipMemcpy(y.data(), e->d_ycell.get(), y.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return IS3D_ERR_DEVICE;
  const double pref = std::pow(2.0 * M_PI * kHbarC, -3);
  for (int s = 0; s < np; s++) {
    const int so = e->order[s];
    for (long c = 0; c < n; c++) dN_dy_cell[(size_t)so * n + c] = pref * e->degen[so] * y[(size_t)e->scls[s] * n + c];
  }
  return IS3D_OK;
}

// ------------------------------------------------------------------------------------------
// spin polarization from thermal vorticity (mode 5; Polarization.cpp:25-263, kernels in polzn.hip)
// ------------------------------------------------------------------------------------------
extern "C" int is3d_set_vorticity(is3d_engine* e, long n, const is3d_vorticity* w) {
  if (e && e->grp) return is3d::group_set_vorticity(e->grp, n, w);
  if (!e) return IS3D_ERR_ARG;
  if (!e->have_surf) return e->fail(IS3D_ERR_STATE, "is3d_set_vorticity: set the surface first");
  if (!w || n != e->ncell) return e->fail(IS3D_ERR_ARG, "is3d_set_vorticity: the vorticity must have one entry per surface cell");
  const double* f[6] = {w->wtx, w->wty, w->wtn, w->wxy, w->wxn, w->wyn};
  for (int k = 0; k < 6; k++)
    if (!f[k] && n > 0) return e->fail(IS3D_ERR_ARG, "is3d_set_vorticity: vorticity component missing");
  HIPCHK(e, hipSetDevice(e->device));
  if (!e->d_vort.reserve(6L * n)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(vorticity) failed");
  for (int k = 0; k < 6 && n > 0; k++)
    HIPCHK(e, hipMemcpy(e->d_vort.get() + (size_t)k * n, f[k], n * sizeof(double), hipMemcpyHostToDevice));
  e->have_vort = true;
  return IS3D_OK;
}

extern "C" long is3d_polarization_size(const is3d_engine* e) {
  const long n = is3d_output_size(e);
  return n < 0 ? n : 5 * n;
}

extern "C" int is3d_launch_polarization(is3d_engine* e, double T_avg, double* dev_out, void* stream) {
  if (e && e->grp) return is3d::group_launch_polarization(e->grp, T_avg, dev_out, stream);
  if (!e) return IS3D_ERR_ARG;
  if (!e->have_params || !e->have_species || !e->have_grid)
    return e->fail(IS3D_ERR_STATE, "polarization: params, species and momentum grid must be set");
  if (!e->have_surf) return e->fail(IS3D_ERR_STATE, "polarization: no surface set");
  if (!e->have_vort) return e->fail(IS3D_ERR_STATE, "polarization: no thermal vorticity set for this surface (is3d_set_vorticity)");
  if (!(T_avg > 0.0)) return e->fail(IS3D_ERR_ARG, "polarization: T_avg must be positive");
  if (!dev_out) return e->fail(IS3D_ERR_ARG, "null output buffer");
  HIPCHK(e, hipSetDevice(e->device));
  if (e->pz_dirty) {
    const std::string msg = is3d::polzn::tables_build(e->pz, e->p.dimension, e->classes, e->mass, e->sign, e->pT, e->phi,
                                                      e->y, e->eta, e->eta_w);
    if (!msg.empty()) return e->fail(IS3D_ERR_ARG, "polarization: " + msg);
    e->pz_dirty = false;
  }
  hipStream_t st = (hipStream_t)stream;
  const long n = e->ncell;
  long wlo, whi;
  cell_window(e, wlo, whi);
  const long nw = whi - wlo;
  const int rc = begin_stats(e, nw, st);
  if (rc) return rc;
  HIPCHK(e, hipEventRecord(e->ev[1].get(), st));     // no prepass: k_polzn reads the surface itself
  if (nw == 0) {
    HIPCHK(e, hipMemsetAsync(dev_out, 0, e->pz.out_size() * sizeof(double), st));
    HIPCHK(e, hipEventRecord(e->ev[2].get(), st));
  } else {
    const is3d::polzn::Plan P = is3d::polzn::make_plan(e->pz, nw, e->max_splits, e->split_bytes, e->slab_bytes);
    if (!P.ok) return e->fail(IS3D_ERR_ARG, "polarization: the phi / y / eta tables do not fit a workgroup's LDS tile");
    if (!e->d_slab.reserve(P.nsplit * P.sstride)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(slabs) failed");
    e->last_nchunk = 0;
    e->last_nsplit = P.nsplit;
    e->last_nslab = P.nsplit;
    HIPCHK(e, is3d::polzn::enqueue(e->pz, P, e->d_surf, e->d_vort.get(), n, wlo, whi, T_avg, e->d_slab.get(), dev_out, st, e->ev[2].get()));
  }
  HIPCHK(e, hipEventRecord(e->ev[3].get(), st));
  e->launched = true;
  return IS3D_OK;
}

extern "C" int is3d_calculate_polarization(is3d_engine* e, double T_avg, double* S_out) {
  if (e && e->grp) return is3d::group_calculate_polarization(e->grp, T_avg, S_out);
  if (!e || !S_out) return e ? e->fail(IS3D_ERR_ARG, "null output") : IS3D_ERR_ARG;
  const long outsize = is3d_polarization_size(e);
  if (outsize < 0) return e->fail(IS3D_ERR_STATE, "polarization: params, species and momentum grid must be set");
  return calculate(e, outsize, S_out, [&](double* d) { return is3d_launch_polarization(e, T_avg, d, nullptr); });
}

// ------------------------------------------------------------------------------------------
// resonance-decay feed-down of the continuous spectra (do_resonance_decays; method in decay_math.h, kernels in decay.hip)
// ------------------------------------------------------------------------------------------
extern "C" int is3d_set_decays(is3d_engine* e, int n, const is3d_decay_channel* ch) {
  if (e && e->grp) return is3d::group_set_decays(e->grp, n, ch);
  if (!e) return IS3D_ERR_ARG;
  if (!e->have_species || !e->have_grid) return e->fail(IS3D_ERR_STATE, "is3d_set_decays: set the species and the momentum grid first");
  if (n < 0 || (n > 0 && !ch)) return e->fail(IS3D_ERR_ARG, "is3d_set_decays: bad channel table");
  e->have_decays = false;
  e->dk_ch.clear();
  std::string msg = is3d::decay::check_grid((int)e->pT.size(), e->pT.data(), (int)e->phi.size(), e->phi.data(), 0, nullptr);
  if (!msg.empty()) return e->fail(IS3D_ERR_ARG, "is3d_set_decays: " + msg);
  e->dk_rule = is3d::decay::make_rule();
  msg = is3d::decay::build_plan(e->dk_plan, e->dk_rule, (int)e->mass.size(), e->mass.data(), n, ch);
  if (!msg.empty()) return e->fail(IS3D_ERR_ARG, "is3d_set_decays: " + msg);
  e->dk_ch.assign(ch, ch + n);
  e->dk_stats = e->dk_plan.stats;
  e->have_decays = true;
  e->dk_dirty = true;
  e->dl_dirty = true;
  return IS3D_OK;
}

extern "C" int is3d_get_decay_stats(const is3d_engine* e, is3d_decay_stats* out) {
  if (e && e->grp) return out ? is3d::group_get_decay_stats(e->grp, out) : IS3D_ERR_ARG;
  if (!e || !out) return IS3D_ERR_ARG;
  if (!e->have_decays) return IS3D_ERR_STATE;
  *out = e->dk_stats;
  return IS3D_OK;
}

extern "C" int is3d_launch_feeddown(is3d_engine* e, double* dev_inout, void* stream) {
  if (e && e->grp) return is3d::group_launch_feeddown(e->grp, dev_inout, stream);
  if (!e) return IS3D_ERR_ARG;
  if (!e->have_params || !e->have_species || !e->have_grid)
    return e->fail(IS3D_ERR_STATE, "feed-down: params, species and momentum grid must be set");
  if (!e->have_decays) return e->fail(IS3D_ERR_STATE, "feed-down: no decay channels set (is3d_set_decays)");
  if (!dev_inout) return e->fail(IS3D_ERR_ARG, "null spectra buffer");
  HIPCHK(e, hipSetDevice(e->device));
  const int ny = e->p.dimension == 3 ? (int)e->y.size() : 1;
  if (e->dk_dirty) {
    if (ny < 1) return e->fail(IS3D_ERR_ARG, "feed-down: empty y table");
    const std::string msg = is3d::decay::check_grid((int)e->pT.size(), e->pT.data(), (int)e->phi.size(), e->phi.data(), ny, e->y.data());
    if (!msg.empty()) return e->fail(IS3D_ERR_ARG, "feed-down: " + msg);
    e->dk_pack = is3d::decay::pack(e->dk_plan, e->dk_rule, e->pT, e->phi, ny, e->y);
    const is3d::decay::Packed& K = e->dk_pack;
    if (K.nb < 1 || K.lds > 64 * 1024) return e->fail(IS3D_ERR_ARG, "feed-down: the phi table does not fit a workgroup's LDS");
    if (!e->d_dk_d.reserve((long)K.d.size()) || !e->d_dk_i.reserve((long)K.i.size()))
      return e->fail(IS3D_ERR_DEVICE, "hipMalloc(decay tables) failed");
    HIPCHK(e, hipMemcpy(e->d_dk_d.get(), K.d.data(), K.d.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(e->d_dk_i.get(), K.i.data(), K.i.size() * sizeof(int), hipMemcpyHostToDevice));
    e->dk_dirty = false;
  }
  const long per = (long)e->pT.size() * ny;
  for (int l = 0; l < e->dk_plan.levels(); l++)
    if ((long)(e->dk_plan.lvl_r0[l + 1] - e->dk_plan.lvl_r0[l]) * per > 0x7fffffffL)
      return e->fail(IS3D_ERR_ARG, "feed-down: a level has more than 2^31 workgroups");
  if (!e->d_dk_log.reserve(is3d_output_size(e))) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(decay logs) failed");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(e, hipEventRecord(e->dk_ev[0].get(), st));
  HIPCHK(e, is3d::decay::enqueue(e->dk_plan, e->dk_pack, e->d_dk_d.get(), e->d_dk_i.get(), dev_inout, e->d_dk_log.get(), st));
  HIPCHK(e, hipEventRecord(e->dk_ev[1].get(), st));
  e->dk_launched = true;
  return IS3D_OK;
}

extern "C" int is3d_decay_feeddown(is3d_engine* e, double* dN) {
  if (e && e->grp) return is3d::group_decay_feeddown(e->grp, dN);
  if (!e || !dN) return e ? e->fail(IS3D_ERR_ARG, "null spectra array") : IS3D_ERR_ARG;
  const long n = is3d_output_size(e);
  if (n < 0) return e->fail(IS3D_ERR_STATE, "feed-down: params, species and momentum grid must be set");
  if (!e->have_decays) return e->fail(IS3D_ERR_STATE, "feed-down: no decay channels set (is3d_set_decays)");
  HIPCHK(e, hipSetDevice(e->device));
  if (!e->d_dk_io.reserve(n)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(spectra) failed");
  HIPCHK(e, hipMemcpy(e->d_dk_io.get(), dN, n * sizeof(double), hipMemcpyHostToDevice));
  int rc = is3d_launch_feeddown(e, e->d_dk_io.get(), nullptr);
  if (rc) return rc;
  rc = is3d_finish(e);
  if (rc) return rc;
  HIPCHK(e, hipMemcpy(dN, e->d_dk_io.get(), n * sizeof(double), hipMemcpyDeviceToHost));
  return IS3D_OK;
}

extern "C" int is3d_get_stats(const is3d_engine* e, is3d_stats* out) {
  if (e && e->grp) return out ? is3d::group_get_stats(e->grp, out) : IS3D_ERR_ARG;
  if (!e || !out) return IS3D_ERR_ARG;
  *out = e->st;
  return IS3D_OK;
}

extern "C" int is3d_evaluate_df_coefficients(is3d_engine* e, double T, double muB, double E, double P, double bulkPi,
                                             double* out15) {
  if (e && e->grp) return out15 ? is3d::group_evaluate_df_coefficients(e->grp, T, muB, E, P, bulkPi, out15) : IS3D_ERR_ARG;
  if (!e || !out15) return IS3D_ERR_ARG;
  int rc = finalize_tables(e);
  if (rc) return rc;
  HIPCHK(e, hipSetDevice(e->device));
  DevBuf<double> buf;
  if (!buf.reserve(16)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc failed");
  double* const d = buf.get();
  hipLaunchKernelGGL(k_df_eval, dim3(1), dim3(1), 0, 0, e->dtb, T, muB, E, P, bulkPi, d, (int*)(d + 15));
  HIPCHK(e, hipDeviceSynchronize());
  int derr = 0;
  HIPCHK(e, hipMemcpy(out15, d, 15 * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(&derr, d + 15, sizeof(int), hipMemcpyDeviceToHost));
  return df_error(e, derr, "df coefficient error");
}

extern "C" int is3d_total_yield(is3d_engine* e, const double* plasma, double y_cut, double* n_total,
                                double* densities) {
  if (e && e->grp) return is3d::group_total_yield(e->grp, plasma, y_cut, n_total, densities);
  if (!e || !plasma || !n_total) return IS3D_ERR_ARG;
  int rc = finalize_tables(e);
  if (rc) return rc;
  if (!e->have_gla || e->gla_alpha < 4) return e->fail(IS3D_ERR_STATE, "is3d_set_gauss_laguerre: alpha = 1..3 tables needed");
  if (e->gla_pts > 64) return e->fail(IS3D_ERR_ARG, "Gauss-Laguerre table longer than 64 points");
  HIPCHK(e, hipSetDevice(e->device));
  const int np = (int)e->mass.size();
  const long n = e->ncell;
  const long nb = (n + 255) / 256;
  DevBuf<double> buf;       // densities [3 np] | k_yield's partial sums [nb]
  if (!buf.reserve(3L * np + std::max(nb, 1L) + 1)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc failed");
  double* const d = buf.get();
  int derr = plasma_densities(e, plasma, d);
  if (derr < 0) return IS3D_ERR_DEVICE;
  std::vector<double> part((size_t)std::max(nb, 1L), 0.0);
  if (!derr && n > 0) {     // k_yield reports through the same error word
    YieldArgs ya{};
    ya.k = make_consts(e); ya.tb = e->dtb; ya.surf = e->d_surf; ya.n = n; ya.dens = d; ya.npart = np;
    ya.partial = d + 3 * (size_t)np; ya.err = e->d_err.get();
    hipLaunchKernelGGL(k_yield, dim3((unsigned)nb), dim3(256), 0, 0, ya);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipDeviceSynchronize());
    HIPCHK(e, hipMemcpy(&derr, e->d_err.get(), sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(e, hipMemcpy(part.data(), d + 3 * (size_t)np, nb * sizeof(double), hipMemcpyDeviceToHost));
  }
  if (densities) HIPCHK(e, hipMemcpy(densities, d, 3 * (size_t)np * sizeof(double), hipMemcpyDeviceToHost));
  if (derr) return df_error(e, derr, "df coefficient error");
  double Ntot = 0.0;
  for (long b = 0; b < nb; b++) Ntot += part[b];
  if (e->p.dimension == 2) Ntot *= 2.0 * y_cut;     // :628-631
  *n_total = Ntot;
  return IS3D_OK;
}

// ------------------------------------------------------------------------------------------
// operation = 2 particle sampler (ParticleSampler.cpp:638-1134; kernels in sampler.hip)
// ------------------------------------------------------------------------------------------
static_assert(sizeof(is3d_particle) == 96 && sizeof(is3d::sampler::Particle) == sizeof(is3d_particle),
              "is3d_particle is the sampler's 96-byte record");

// cell_base: global index of this engine's cell 0 (a shard of a device-list engine holds only its window)
static is3d::sampler::Bins sampler_bins(const is3d_sample_bins& b) {
  return is3d::sampler::make_bins(b.pT_min, b.pT_max, b.pT_bins, b.y_cut, b.y_bins, b.phip_bins, b.eta_cut, b.eta_bins,
                                  b.tau_min, b.tau_max, b.tau_bins, b.r_min, b.r_max, b.r_bins);
}

// famod: the df_mode 5 method (is3d_sample_famod; plasma unused, fast ignored): the Newton prepass under the sampler's
// chain rule first, then the same sampler with the k_cells / k_sample famod variants reading d_sol
static int sample_any(is3d_engine* e, const is3d_sample_params* sp, const double* plasma, long cell_base, int binned,
                      bool famod) {
  if (!e || e->grp) return IS3D_ERR_ARG;
  e->sampled = false;
  e->binned = false;
  e->decayed = false;
  if (!sp || (!famod && !plasma)) return e->fail(IS3D_ERR_ARG, "is3d_sample: null argument");
  if (!famod && e->have_params && e->p.df_mode == PTMA)
    return e->fail(IS3D_ERR_UNSUPPORTED, "is3d_sample: df_mode 5 has its own method (sample_dN_pTdpTdphidy_famod): call is3d_sample_famod");
  if (famod && (!e->have_params || e->p.df_mode != PTMA))
    return e->fail(IS3D_ERR_STATE, "is3d_sample_famod: needs params with df_mode 5 (df_mode 1-4: is3d_sample)");
  if (famod && e->pdg_mass.empty()) return e->fail(IS3D_ERR_STATE, "is3d_sample_famod: no PDG table set (is3d_set_pdg)");
  if (famod && e->chain_q1 >= 0) return e->fail(IS3D_ERR_STATE, "is3d_sample_famod: a chain range is set (is3d_set_chain_range); the sampler solves the whole chain");
  if (sp->n_events < 1) return e->fail(IS3D_ERR_ARG, "is3d_sample: n_events must be >= 1");
  if (!(sp->y_cut > 0.0)) return e->fail(IS3D_ERR_ARG, "is3d_sample: y_cut must be positive");
  if (sp->seed < 0) return e->fail(IS3D_ERR_ARG, "is3d_sample: the seed must be non-negative (a negative sampler_seed takes the clock on the host)");
  if (binned && !e->have_sbins) return e->fail(IS3D_ERR_STATE, "is3d_sample_binned: is3d_set_sample_bins not called");
  int rc = finalize_tables(e);
  if (rc) return rc;
  if (!e->have_surf) return e->fail(IS3D_ERR_STATE, "is3d_sample: no surface set");
  const int fast = (sp->fast && !famod) ? 1 : 0;
  if (!e->have_gla || e->gla_alpha < (fast ? 4 : 3)) return e->fail(IS3D_ERR_STATE, "is3d_set_gauss_laguerre: alpha = 1..3 tables needed");
  if (e->gla_pts > 64) return e->fail(IS3D_ERR_ARG, "Gauss-Laguerre table longer than 64 points");
  HIPCHK(e, hipSetDevice(e->device));
  if (e->smp_dirty) {
    const std::string m = is3d::sampler::tables_build(e->smp, e->mass, e->sign, e->degen, e->baryon);
    if (!m.empty()) return e->fail(IS3D_ERR_DEVICE, "is3d_sample: " + m);
    e->smp_dirty = false;
  }
  const int np = (int)e->mass.size();
  is3d::sampler::Config c;
  c.run.k = make_consts(e);
  c.run.fast = fast;
  c.run.y_max = e->p.dimension == 2 ? sp->y_cut : 0.5;
  c.run.Tavg = famod ? 0.0 : plasma[0]; c.run.F_avg = 0.0; c.run.betabulk_avg = 1.0;
  c.tb = e->dtb; c.surf = e->d_surf; c.n = e->ncell;
  cell_window(e, c.lo, c.hi);
  c.cell_base = cell_base; c.seed = (uint64_t)sp->seed; c.n_events = sp->n_events; c.sample_bytes = e->sample_bytes;
  DevBuf<double> dens;
  if (fast) {     // Plasma-average densities (DeltafData.cpp:555-690) and PTM's average df coefficients (:664-673)
    if (!dens.reserve(3L * np)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc failed");
    const int derr = plasma_densities(e, plasma, dens.get());
    if (derr) return derr < 0 ? IS3D_ERR_DEVICE : df_error(e, derr, "df coefficient error");
    if (e->p.df_mode == PTM) {
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
    e->sfst = is3d_sample_famod_stats{e->st.pl_negative, e->st.recon_fail, e->st.iterations};
    c.sol = e->d_sol.get();
  } else if (famod) {
    e->sfst = is3d_sample_famod_stats{};
  }
  is3d::sampler::Bins sb{};
  if (binned) {
    sb = sampler_bins(e->sbins);
    e->hist_nc = is3d::sampler::hist_counts(sb, np);
    e->hist_nv = is3d::sampler::hist_vn(sb, np);
    const long words = e->hist_nc + e->hist_nv;
    if (!e->d_hist.reserve(words)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(sampler histogram) failed");
    HIPCHK(e, hipMemset(e->d_hist.get(), 0, (size_t)words * sizeof(unsigned long long)));
    c.bins = &sb; c.hist = e->d_hist.get(); c.keep_list = binned == 2;
  }
  is3d::sampler::Stats st;
  int derr = 0;
  std::string msg;
  const int s = is3d::sampler::run(e->smp, c, e->particles, e->particle_offsets, st, derr, msg);
  if (s == is3d::sampler::S_DF) return df_error(e, derr, "df coefficient error");
  if (s == is3d::sampler::S_DEVICE) return e->fail(IS3D_ERR_DEVICE, "is3d_sample: " + msg);
  if (s == is3d::sampler::S_BUDGET) return e->fail(IS3D_ERR_ARG, "is3d_sample: " + msg);
  e->sst = is3d_sample_stats{st.cells, st.breakdown, st.candidates, st.kept, st.proposals, st.acceptances, st.capped,
                             st.clamped, st.batches};
  if (binned) {
    e->hist.assign((size_t)(e->hist_nc + e->hist_nv), 0);
    HIPCHK(e, hipMemcpy(e->hist.data(), e->d_hist.get(), e->hist.size() * sizeof(long long), hipMemcpyDeviceToHost));
    e->binned = true;
  }
  e->sampled = true;
  e->sampled_famod = famod;
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
  if (e && e->grp) return out ? is3d::group_get_sample_famod_stats(e->grp, out) : IS3D_ERR_ARG;
  if (!e || !out) return IS3D_ERR_ARG;
  if (!e->sampled || !e->sampled_famod) return IS3D_ERR_STATE;
  *out = e->sfst;
  return IS3D_OK;
}

const long long* is3d_internal_sample_hist(const is3d_engine* e) { return (e && e->binned) ? e->hist.data() : nullptr; }

extern "C" int is3d_sample(is3d_engine* e, const is3d_sample_params* sp, const double* plasma) {
  if (e && e->grp) return is3d::group_sample(e->grp, sp, plasma, 0);
  return is3d_internal_sample(e, sp, plasma, 0, 0);
}

extern "C" int is3d_set_sample_bins(is3d_engine* e, const is3d_sample_bins* b) {
  if (e && e->grp) return b ? is3d::group_set_sample_bins(e->grp, b) : IS3D_ERR_ARG;
  if (!e || !b) return IS3D_ERR_ARG;
  if (b->pT_bins < 1 || b->y_bins < 1 || b->phip_bins < 1 || b->eta_bins < 1 || b->tau_bins < 1 || b->r_bins < 1)
    return e->fail(IS3D_ERR_ARG, "is3d_set_sample_bins: every bin count must be >= 1");
  if (!(b->pT_max > b->pT_min) || !(b->tau_max > b->tau_min) || !(b->r_max > b->r_min))
    return e->fail(IS3D_ERR_ARG, "is3d_set_sample_bins: pT, tau and r ranges must be increasing");
  if (!(b->y_cut > 0.0) || !(b->eta_cut > 0.0)) return e->fail(IS3D_ERR_ARG, "is3d_set_sample_bins: y_cut and eta_cut must be positive");
  e->sbins = *b;
  e->have_sbins = true;
  e->binned = false;
  return IS3D_OK;
}

extern "C" int is3d_sample_binned(is3d_engine* e, const is3d_sample_params* sp, const double* plasma, int keep_list) {
  if (e && e->grp) return is3d::group_sample(e->grp, sp, plasma, keep_list ? 2 : 1);
  return is3d_internal_sample(e, sp, plasma, 0, keep_list ? 2 : 1);
}

extern "C" long is3d_sample_hist_size(const is3d_engine* e, long* n_counts, long* n_vn) {
  if (e && e->grp) return is3d::group_sample_hist_size(e->grp, n_counts, n_vn);
  if (!e || !e->have_sbins || e->mass.empty()) return -1;
  const is3d::sampler::Bins sb = sampler_bins(e->sbins);
  const long nc = is3d::sampler::hist_counts(sb, (int)e->mass.size()), nv = is3d::sampler::hist_vn(sb, (int)e->mass.size());
  if (n_counts) *n_counts = nc;
  if (n_vn) *n_vn = nv;
  return nc + nv;
}

extern "C" int is3d_get_sample_hist(const is3d_engine* e, long* counts, double* vn) {
  if (e && e->grp) return (counts && vn) ? is3d::group_get_sample_hist(e->grp, counts, vn) : IS3D_ERR_ARG;
  if (!e || !counts || !vn) return IS3D_ERR_ARG;
  if (!e->binned) return IS3D_ERR_STATE;
  for (long i = 0; i < e->hist_nc; i++) counts[i] = (long)e->hist[(size_t)i];
  for (long i = 0; i < e->hist_nv; i++) vn[i] = is3d::sampler::vn_value(e->hist[(size_t)(e->hist_nc + i)]);
  return IS3D_OK;
}

extern "C" long is3d_sample_count(const is3d_engine* e) {
  if (e && e->grp) return is3d::group_sample_count(e->grp);
  return (e && e->sampled) ? (long)e->particles.size() : -1;
}

extern "C" int is3d_sample_offsets(const is3d_engine* e, long* offsets) {
  if (e && e->grp) return is3d::group_sample_offsets(e->grp, offsets);
  if (!e || !offsets) return IS3D_ERR_ARG;
  if (!e->sampled) return IS3D_ERR_STATE;
  std::copy(e->particle_offsets.begin(), e->particle_offsets.end(), offsets);
  return IS3D_OK;
}

extern "C" int is3d_get_particles(const is3d_engine* e, long first, long count, is3d_particle* out) {
  if (e && e->grp) return is3d::group_get_particles(e->grp, first, count, out);
  if (!e || (!out && count > 0)) return IS3D_ERR_ARG;
  if (!e->sampled) return IS3D_ERR_STATE;
  if (first < 0 || count < 0 || first + count > (long)e->particles.size()) return IS3D_ERR_ARG;
  if (count > 0) std::memcpy(out, e->particles.data() + first, (size_t)count * sizeof(is3d_particle));
  return IS3D_OK;
}

extern "C" int is3d_get_sample_stats(const is3d_engine* e, is3d_sample_stats* out) {
  if (e && e->grp) return out ? is3d::group_get_sample_stats(e->grp, out) : IS3D_ERR_ARG;
  if (!e || !out) return IS3D_ERR_ARG;
  if (!e->sampled) return IS3D_ERR_STATE;
  *out = e->sst;
  return IS3D_OK;
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
  if (!e->have_decays) return e->fail(IS3D_ERR_STATE, w + "no decay channels set (is3d_set_decays)");
  if (bin && !e->have_sbins) return e->fail(IS3D_ERR_STATE, w + "is3d_set_sample_bins not called");
  if (seed < 0) return e->fail(IS3D_ERR_ARG, w + "the seed must be non-negative");
  if (n_events < 0 || !offsets) return e->fail(IS3D_ERR_ARG, w + "bad event offsets");
  const std::string plan_err = is3d::decay_mc::check_plan(e->dk_plan);
  if (!plan_err.empty()) return e->fail(IS3D_ERR_ARG, w + plan_err);
  const int np = (int)e->mass.size();
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
  if (e->dl_dirty) {
    const std::string m = is3d::decay_list::tables_build(e->dl, e->dk_plan, e->mass);
    if (!m.empty()) return e->fail(IS3D_ERR_DEVICE, w + m);
    e->dl_dirty = false;
  }
  is3d::decay_list::Config c;
  c.seed = (uint64_t)seed;
  c.sample_bytes = e->sample_bytes;
  is3d::sampler::Bins sb{};
  long nc = 0, nv = 0;
  if (bin) {
    sb = sampler_bins(e->sbins);
    nc = is3d::sampler::hist_counts(sb, np);
    nv = is3d::sampler::hist_vn(sb, np);
    if (!e->d_hist.reserve(nc + nv)) return e->fail(IS3D_ERR_DEVICE, w + "hipMalloc(histogram) failed");
    HIPCHK(e, hipMemset(e->d_hist.get(), 0, (size_t)(nc + nv) * sizeof(unsigned long long)));
    c.bins = &sb; c.hist = e->d_hist.get();
  }
  static_assert(sizeof(is3d_particle) == sizeof(is3d::sampler::Particle), "is3d_particle is the sampler's record");
  std::vector<is3d::sampler::Particle> out;
  std::vector<long> origin;
  is3d::decay_list::Stats st;
  std::string msg;
  const int s = is3d::decay_list::run(e->dl, c, n, reinterpret_cast<const is3d::sampler::Particle*>(in) + i0, prim.data(), out,
                                      origin, st, msg);
  if (s == is3d::decay_list::S_DEVICE) return e->fail(IS3D_ERR_DEVICE, w + msg);
  if (s == is3d::decay_list::S_BUDGET) return e->fail(IS3D_ERR_ARG, w + msg);
  std::vector<long long> hist;
  if (bin) {
    hist.assign((size_t)(nc + nv), 0);
    HIPCHK(e, hipMemcpy(hist.data(), e->d_hist.get(), hist.size() * sizeof(long long), hipMemcpyDeviceToHost));
  }
  // the offsets of the decayed list: origins are non-decreasing, so event k ends where the origins reach its end
  std::vector<long> off((size_t)n_events + 1, 0);
  size_t j = 0;
  for (int k = 0; k < n_events; k++) {
    while (j < origin.size() && origin[j] < offsets[k + 1] - i0) j++;
    off[(size_t)k + 1] = (long)j;
  }
  for (long& o : origin) o += i0;
  e->particles.swap(out);
  e->particle_offsets.swap(off);
  e->origins.swap(origin);
  e->dl_stats = is3d_decay_list_stats{st.primaries, st.decays, st.undecayed, st.dropped_daughters, st.capped,
                                      st.final_particles, st.passes, st.batches, st.ms_total};
  if (bin) {
    e->hist.swap(hist);
    e->hist_nc = nc; e->hist_nv = nv;
    e->binned = true;
  }
  e->sampled = true;
  e->decayed = true;
  return IS3D_OK;
}

extern "C" int is3d_decay_particles(is3d_engine* e, long seed, int n_events, const long* offsets, const is3d_particle* in, int bin) {
  if (e && e->grp) return is3d::group_decay_particles(e->grp, seed, n_events, offsets, in, bin);
  if (!e) return IS3D_ERR_ARG;
  const int rc = decay_list_any(e, seed, n_events, offsets, in, bin, "is3d_decay_particles");
  if (!rc) e->sampled_famod = false;
  return rc;
}

extern "C" int is3d_decay_sampled(is3d_engine* e, long seed, int bin) {
  if (e && e->grp) return is3d::group_decay_sampled(e->grp, seed, bin);
  if (!e) return IS3D_ERR_ARG;
  if (!e->have_decays) return e->fail(IS3D_ERR_STATE, "is3d_decay_sampled: no decay channels set (is3d_set_decays)");
  if (!e->sampled || e->particle_offsets.empty() ||
      (e->particles.empty() && e->sst.kept > 0))     // a binned-only call counted particles and kept none
    return e->fail(IS3D_ERR_STATE, "is3d_decay_sampled: no sampled list (is3d_sample, or a binned call that keeps the list)");
  return decay_list_any(e, seed, (int)e->particle_offsets.size() - 1, e->particle_offsets.data(),
                        reinterpret_cast<const is3d_particle*>(e->particles.data()), bin, "is3d_decay_sampled");
}

extern "C" int is3d_get_particle_origins(const is3d_engine* e, long first, long count, long* origin) {
  if (e && e->grp) return is3d::group_get_particle_origins(e->grp, first, count, origin);
  if (!e || (!origin && count > 0)) return IS3D_ERR_ARG;
  if (!e->sampled || !e->decayed) return IS3D_ERR_STATE;
  if (first < 0 || count < 0 || first + count > (long)e->origins.size()) return IS3D_ERR_ARG;
  std::copy(e->origins.begin() + first, e->origins.begin() + first + count, origin);
  return IS3D_OK;
}

extern "C" int is3d_get_decay_list_stats(const is3d_engine* e, is3d_decay_list_stats* out) {
  if (e && e->grp) return out ? is3d::group_get_decay_list_stats(e->grp, out) : IS3D_ERR_ARG;
  if (!e || !out) return IS3D_ERR_ARG;
  if (!e->sampled || !e->decayed) return IS3D_ERR_STATE;
  *out = e->dl_stats;
  return IS3D_OK;
}

extern "C" int is3d_get_jonah_table(const is3d_engine* e, double* l2, double* z, double* bp, double* bpmax) {
  if (e && e->grp) return is3d::group_get_jonah_table(e->grp, l2, z, bp, bpmax);
  if (!e || e->jx.size() != 301) return IS3D_ERR_STATE;
  std::copy(e->jl2.begin(), e->jl2.end(), l2);
  std::copy(e->jz.begin(), e->jz.end(), z);
  std::copy(e->jx.begin(), e->jx.end(), bp);
  *bpmax = e->bp_max;
  return IS3D_OK;
}

extern "C" int is3d_surface_averages(long n, const is3d_surface* s, int include_baryon, double* out) {
  if (!s || !out || n <= 0) return IS3D_ERR_ARG;
  double T_avg = 0, E_avg = 0, P_avg = 0, muB_avg = 0, nB_avg = 0, vol = 0;
  for (long i = 0; i < n; i++) {
    const double tau = s->tau[i], tau2 = tau * tau, ux = s->ux[i], uy = s->uy[i], un = s->un[i];
    const double ut = std::sqrt(1. + ux * ux + uy * uy + tau2 * un * un);
    const double dat = s->dat[i], dax = s->dax[i], day = s->day[i], dan = s->dan[i];
    const double uds = ut * dat + ux * dax + uy * day + un * dan;
    const double ds_ds = dat * dat - dax * dax - day * day - dan * dan / tau2;
    const double ds_max = std::fabs(uds) + std::sqrt(std::fabs(uds * uds - ds_ds));
    const double muB = (include_baryon && s->muB) ? s->muB[i] : 0.0;
    const double nB = (include_baryon && s->nB) ? s->nB[i] : 0.0;
    vol += ds_max;
    E_avg += (s->E[i] * ds_max); T_avg += (s->T[i] * ds_max); P_avg += (s->P[i] * ds_max);
    muB_avg += (muB * ds_max); nB_avg += (nB * ds_max);
  }
  const double v[5] = {T_avg / vol, E_avg / vol, P_avg / vol, muB_avg / vol, nB_avg / vol};
  for (int k = 0; k < 5; k++) {   // ofstream << setprecision(15) then fscanf %lf (readindata.cpp:364-366, :104-119)
    char buf[64];
    std::snprintf(buf, sizeof(buf), "%.15g", v[k]);
    out[k] = std::strtod(buf, nullptr);
  }
  return IS3D_OK;
}
