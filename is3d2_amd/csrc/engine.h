// engine.h -- struct is3d_engine and the host sequences its translation units share (private; the C ABI is
// include/is3d_amd.h).  The units, by operation:
//   engine.hip         create / destroy, the setters, finalize_tables, the surface, the prepass, the spectra plan, launch
//                      and reduction, is3d_finish, stats, the df-coefficient and Jonah-table kernels
//   engine_dndx.hip    operation 0 (dN/dX) and the cell yields
//   engine_sample.hip  operation 2: the total yield, the sampler, its bins / histogram / list getters, the list decays
//   engine_post.hip    spin polarization and resonance-decay feed-down of the spectra (kernels in polzn.hip, decay.hip)
// Each unit compiles its own kernels; this header holds no device code.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>
#include <vector>

#include "../../include/is3d_amd.h"
#include "cf_math.h"
#include "kernels.h"
#include "decay.h"
#include "decay_list.h"
#include "devbuf.h"
#include "polzn.h"
#include "sampled_list.h"
#include "sampler.h"

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

namespace is3d {
struct Group;

// ---- kernel arguments that live in the engine between the stages of a launch (kernels: engine_kernels.h) ----------
struct PrepArgs {
  PrepConsts k;
  DfTables tb;
  const double* surf;   // [NSURF][n]
  double* rec;          // [n][NREC]
  double* aux;          // PTM/PTB: [9][n]; PTMA: [9][n] Newton inputs
  long n;               // cells held (the field stride of surf / aux)
  long c0, c1;          // cells [c0, c1) prepared by this launch
  int* err;
  unsigned long long* cnt;  // [0] breakdown [1] pl<0 [2] recon fail [3] iterations
};

struct ChainArgs {
  const double* rec; const double* ain; double* sol;   // ain [9][n], sol [6][n]
  double* sta;           // [4][n] chain state after each cell (prev_ok, lambda, aT, aL)
  int* info;             // [n] Newton iterations | pl/pt < 0 << 16 | reconstruction failure << 17
  double* send;          // [2][4][nseg] segment end states, by pass parity
  double* sstart;        // [4][nseg] the start state of each segment's stored run
  int* changed;          // [kChainPasses] pass j changed some segment's end state
  long n, C, L, nspc;    // cells, chains, positions per segment, segments per chain
  // positions [q0, q1) of every chain (cells [q0 C, q1 C)): the whole chain on one engine; a device group's shard
  // solves its own range, starting each chain from the end state its predecessor shard pushes into bin
  long q0, q1;
  int has_pred;          // q0 > 0: chain position q0 - 1 lives on the previous shard
  int npass;             // passes enqueued (<= kChainPasses)
  double* bin;           // [3][4 C + 1] boundary in: end states of position q0 - 1 by pass parity, [2] = final + walk flag
  double* bout;          // [3][4 C + 1] boundary out: this range's end states (position q1 - 1), same slots
  Hadrons h;
  double fp2;
  int srule;             // the particle sampler's chain rule (aniso_math.h aniso_cell)
};

constexpr int kFbBlocks = 1024;   // k_fbcount / k_fbwrite: blocks of the fallback-cell scan (enqueue_fbscan)

// one launch's state between the stages of a staged launch (launch_begin .. launch_end)
struct LaunchCtx {
  hipStream_t st = nullptr;
  double* dev_out = nullptr;
  long wlo = 0, whi = 0, nw = 0, p0 = 0, p1 = 0;
  bool chained = false, empty = false;
  PrepArgs pa{};
  ChainArgs ca{};
};

// ---- what a changed input invalidates -------------------------------------------------------------------------------
enum Input : int { IN_PARAMS, IN_SPECIES, IN_CLASSES, IN_PDG, IN_GRID, IN_WEIGHTS, IN_GLA, IN_DF, IN_DECAYS, N_INPUTS };
// derived state, each rebuilt by its first user while its bit is set in is3d_engine::stale
enum Derived : unsigned {
  D_TABLES = 1,         // finalize_tables: d_tables / d_const and the classes
  D_POLZN = 2,          // polarization tables (is3d_launch_polarization)
  D_SAMPLER = 4,        // sampler species tables (is3d_sample*)
  D_DECAY_PACK = 8,     // feed-down's packed tables (is3d_launch_feeddown)
  D_DECAY_LIST = 16,    // list-decay tables (is3d_decay_particles / _sampled)
  D_DECAY_PLAN = 32,    // the channel plan of is3d_set_decays itself: while set, no decays are set
};
constexpr unsigned kInvalidates[N_INPUTS] = {
    /* IN_PARAMS  */ D_TABLES | D_POLZN | D_DECAY_PACK,                // the packed decay tables depend on ny
    /* IN_SPECIES */ D_TABLES | D_POLZN | D_SAMPLER | D_DECAY_PLAN,    // the channels index the species
    /* IN_CLASSES */ D_TABLES | D_POLZN,
    /* IN_PDG     */ D_TABLES,
    /* IN_GRID    */ D_TABLES | D_POLZN | D_DECAY_PLAN,                // is3d_set_decays checked the grid it saw
    /* IN_WEIGHTS */ D_TABLES,
    /* IN_GLA     */ D_TABLES,
    /* IN_DF      */ D_TABLES,
    /* IN_DECAYS  */ D_DECAY_PLAN | D_DECAY_PACK | D_DECAY_LIST,       // is3d_set_decays clears D_DECAY_PLAN on success
};
}  // namespace is3d

struct is3d_engine {
  int device = 0;
  std::string err;
  // is3d_create_devices: the shard engines and their reduction (group.hip); every entry point forwards
  is3d::Group* grp = nullptr;
  unsigned stale = ~0u;      // is3d::Derived bits to rebuild (input_changed)

  // what the setters store
  struct Inputs {
    bool have_params = false, have_species = false, have_pdg = false, have_grid = false, have_gla = false, have_df = false;
    is3d_params p{};
    // species (original order) and mass-sorted permutation
    std::vector<double> mass, sign, degen, baryon;
    std::vector<int> order;
    std::vector<double> pdg_mass, pdg_sign, pdg_degen, pdg_baryon;
    std::vector<double> pT, phi, y, eta, eta_w;
    std::vector<double> pT_w, phi_w;       // operation 0 quadrature weights
    bool have_weights = false;
    int gla_alpha = 0, gla_pts = 0;
    std::vector<double> gla_r, gla_w;
    int nT = 0, nmuB = 0;
    std::vector<double> Tarr, muBarr, tab;
    double T_avg = 0.0;
    // integrand classes (is3d_set_species_classes, default on): the momentum integrals see a species only through
    // its (mass, sign, baryon) -- plus, in PTM, whether its degeneracy is zero (ptm_gkey) -- and the engine applies the degeneracy once, to the cell sum, in k_reduce (the reference
    // multiplies every cell's term by prefactor x degeneracy, MomentumSpectra.cpp:365: the same product up to
    // rounding), so sorted species with identical keys have bit-identical cell sums: the integrand classes (SMASH 444 -> 193, UrQMD 305 -> 124), which
    // is3d_species_integrated counts.  k_spectra / k_dndx integrate one lane per *lane class* and the reduction writes
    // every member: the lane classes are the integrand classes, or fewer when the run is baryon-blind
    // (Tables::nlane: 135 / 75; is3d_lanes_integrated).
    bool classes = true;
  } in;

  // what finalize_tables derives from the inputs (D_TABLES)
  struct Tables {
    // derived host tables
    std::vector<double> jl2, jz, jx, jl2c, jzc;
    double bp_max = -1.0;
    // device: every allocation, stream and event is a DevBuf / DevStream / DevEvent member (devbuf.h); the raw pointers
    // below are views into d_tables / d_const
    is3d::DevBuf<double> d_tables;
    is3d::DfTables dtb{};
    is3d::DevBuf<double> d_const;    // species, grids, gla, pdg
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
    // d_rrep[k] = a representative sorted species of class k (SMASH 444 -> nrcls classes).  A baryon-blind run keys
    // them without the baryon number, as the lane classes.
    int* d_rcls = nullptr;
    int* d_rrep = nullptr;
    int nrcls = 0;
    // Two levels of classes (Inputs::classes).
    //  - ncls: the integrand classes under the documented key (mass, sign, baryon [, PTM: g == 0]); a count only, what
    //    is3d_species_integrated reports.
    //  - nlane: the lane classes, what the kernels integrate and every table below describes.  Their key is the class
    //    key without the baryon number when the run is baryon-blind (finalize_tables baryon_blind: include_baryon = 0
    //    and every delta-f table entry that multiplies the baryon number is zero), else the class key itself: SMASH 193
    //    classes -> 135 lanes, UrQMD 124 -> 75.  The lane's baryon operand is its first member's; a blind run only
    //    ever multiplies it by zeros.
    // d_cmass/d_csign/d_cbaryon: lane values, d_crcls: lane -> renorm class, d_cmem[d_cmem_off[c] ..]: member sorted
    // species of lane c (each written with its own degeneracy), d_scls: sorted species -> lane.
    // nlane counts the lane slots of the tables, nlive the lane classes among them (is3d_lanes_integrated): the same,
    // except where finalize_tables appends empty lanes to keep a table launch.
    int ncls = 0, nlane = 0, nlive = 0;
    bool blind = false;      // the run is baryon-blind and classes are on: lanes merge baryon / antibaryon pairs
    std::vector<int> scls;   // host copy of d_scls
    const double *d_cmass = nullptr, *d_csign = nullptr, *d_cbaryon = nullptr;
    int *d_crcls = nullptr, *d_cmem_off = nullptr, *d_cmem = nullptr, *d_scls = nullptr;
  } tbl;

  struct Surface {
    // the surface [NSURF][ncell]: a view of surf_own (an uploaded or copied surface) or of the caller's device memory
    // (is3d_set_surface_device; surf_own is then empty)
    double* d_surf = nullptr; long ncell = 0;
    is3d::DevBuf<double> surf_own;
    bool have_surf = false;    // a surface was set (an empty one set from device memory has no d_surf)
    // cell window [win_lo, win_hi) of the held surface that k_spectra integrates (-1: every cell); set by a
    // group whose shards hold the whole surface for the PTMA warm-start chains
    long win_lo = -1, win_hi = -1;
    // is3d_set_chain_range: PTMA warm-start chain positions [chain_q0, chain_q1) this engine solves (-1: all), for the
    // staged launch of one process per GPU
    long chain_q0 = -1, chain_q1 = -1;
  } sf;

  // the working set of a launch: the prepass records, the spectra slabs, the launch in flight and its stats
  struct Work {
    is3d::DevBuf<double> d_chain;     // PTMA warm-start chain segments (k_chain_pass)
    is3d::DevBuf<double> d_rec, d_aux, d_sol, d_renorm, d_slab, d_out;
    is3d::DevBuf<int> d_fb;           // modified modes: [0] fallback cell count, [1..] k_fbwrite's cell list
    // F_TS launches: k_phitab's per-(cell, pT, phi) rows of one chunk of cells and, behind them, k_ytab's y-term rows
    is3d::DevBuf<double> d_phtab;
    is3d::DevBuf<double> d_phtab2;    // ... and of the next chunk, integrated on the side stream meanwhile
    // the streams and events of the chunked F_TS launches are made by the first launch that needs them
    is3d::DevStream side;             // F_TS chunks alternate between the launch stream and this one
    is3d::DevEvent fork, join;
    // folded F_TS chunks: k_fold runs on its own stream, in chunk order, after each chunk's k_spectra
    // (ev_spec); a chunk reusing a slab buffer waits for the fold that emptied it (ev_fold)
    is3d::DevStream fold_st;
    is3d::DevEvent ev_spec[2], ev_fold[2], fold_join;
    // is3d_set_tuning: F_TS table chunking (defaults IS3D_PHITAB_ONE / IS3D_PHITAB_BYTES): tables of the whole window
    // up to phitab_one bytes are one chunk, larger ones chunks of whole cell splits of about phitab_chunk bytes
    long phitab_one = IS3D_PHITAB_ONE, phitab_chunk = IS3D_PHITAB_BYTES;
    long last_nchunk = 0;       // F_TS chunks of the last launch (0: not an F_TS launch)
    // is3d_set_tuning: k_spectra's cell splits (defaults IS3D_MAX_SPLITS / IS3D_SLAB_BYTES / IS3D_SPLIT_BYTES)
    long max_splits = IS3D_MAX_SPLITS, slab_bytes = IS3D_SLAB_BYTES, split_bytes = IS3D_SPLIT_BYTES;
    long last_nsplit = 0;       // cell splits of the last launch's main plan
    long last_nslab = 0;        // ... and the output-sized partial slabs it held (folded F_TS chunks: 1 + 2 spc)
    is3d::DevBuf<int> d_err;                  // the device error word (cf_math.h DF_*)
    is3d::DevBuf<unsigned long long> d_cnt;   // [8] counters (PrepArgs::cnt)
    is3d::DevEvent ev[4];             // timing events of a launch's stages
    is3d::LaunchCtx lc;               // the launch in flight (staged launches)
    is3d_stats st{};
    bool launched = false;
  } ws;

  // operation 0
  struct Dndx {
    bool have_bins = false;
    is3d_spacetime_bins bins{};
    is3d::DevBuf<double> d_ycell, d_part;
    is3d::DevBuf<int> d_keys, d_perm;
    is3d::DevBuf<long> d_offs;
    long ycell_n = -1;
  } op0;

  // spin polarization (mode 5, polzn.hip): thermal vorticity [6][ncell] of the surface set last (a new surface
  // clears it) and the kernels' constants (D_POLZN)
  struct Polzn {
    is3d::DevBuf<double> d_vort; bool have_vort = false;
    is3d::polzn::Tables tables;
  } pol;

  // resonance-decay feed-down (decay.hip): the channel table as given, its plan (built by is3d_set_decays, D_DECAY_PLAN),
  // the packed tables (D_DECAY_PACK) and the log slabs
  struct Feeddown {
    std::vector<is3d_decay_channel4> ch;
    bool launched = false;
    is3d::decay::Rule rule{};
    is3d::decay::Plan plan;
    is3d::decay::Packed pack;
    is3d::DevBuf<double> d_d, d_log, d_io;
    is3d::DevBuf<int> d_i;
    is3d::DevEvent ev[2];
    is3d_decay_stats stats{};
  } fd;

  // particle sampler (operation 2, sampler.hip): species tables in the original order (D_SAMPLER), the "sample_bytes"
  // bound on a batch's working buffers, and the list / histogram / stats of the last sample or list-decay call
  struct Sampler {
    is3d::sampler::Tables tables;
    long sample_bytes = IS3D_SAMPLE_BYTES;
    // test_sampler = 1: the bins and the device histogram of a binned call (zeroed at its start)
    is3d_sample_bins bins{};
    bool have_bins = false;
    is3d::DevBuf<unsigned long long> d_hist;
    is3d::SampledList list;
    // bytes of particle records, stream keys and origins the last sampling or list-decay call copied to / from the
    // device ("list_h2d_bytes" / "list_d2h_bytes"), summed where the copies are made
    long list_h2d = 0, list_d2h = 0;
  } smp;

  // Monte Carlo decays of a particle list (decay_list.hip): the plan's tables on the device (D_DECAY_LIST)
  struct ListDecay {
    is3d::decay_list::Tables tables;
  } dl;

  int fail(int code, const std::string& msg) { err = msg; return code; }
  bool is_stale(is3d::Derived d) const { return (stale & d) != 0; }
  void rebuilt(is3d::Derived d) { stale &= ~(unsigned)d; }
  bool have_decays() const { return !is_stale(is3d::D_DECAY_PLAN); }
  // the one place a setter says what it changed
  void input_changed(is3d::Input i) {
    stale |= is3d::kInvalidates[i];
    if (is3d::kInvalidates[i] & is3d::D_DECAY_PLAN) fd.ch.clear();
  }
};

// ---- host sequences the units share (defined in engine.hip) ---------------------------------------------------------
int hip_fail(is3d_engine* e, hipError_t h, const char* what);
#define HIPCHK(e, x)                                           \
  do {                                                         \
    hipError_t h_ = (x);                                       \
    if (h_ != hipSuccess) return hip_fail((e), h_, #x);        \
  } while (0)
// The device error word (cf_math.h DfErr) as the IS3D_ERR_* code and message of every entry point that reads one; the
// table errors carry the reference's printed messages.  other: the caller's message for any other nonzero word
int df_error(is3d_engine* e, int derr, const char* other);
// Build the derived tables (splines, Jonah) and upload everything read-only to HBM.
int finalize_tables(is3d_engine* e);
is3d::PrepConsts make_consts(const is3d_engine* e);
// cells [lo, hi) of the held surface that a launch covers: the cell window, or every cell
void cell_window(const is3d_engine* e, long& lo, long& hi);
// a launch's prologue on its stream: fresh stats, the error word and the counters cleared, ev[0] recorded
int begin_stats(is3d_engine* e, long cells, hipStream_t st);
// ... and the stage times between its four events, once ev[3] has completed
void read_timings(is3d_engine* e);
// the prepass of cells [c0, c1) of the held surface into rec / aux (operation 1; a caller for another sets k.operation)
is3d::PrepArgs prep_args(const is3d_engine* e, double* rec, double* aux, long c0, long c1, int* err, unsigned long long* cnt);
int enqueue_prep(is3d_engine* e, const is3d::PrepArgs& pa, hipStream_t st);
// PTM: the renormalisation factors of cells [c0, c0 + n) (records and aux of `stride` cells), one per renorm class
int enqueue_renorm(is3d_engine* e, const is3d::PrepConsts& k, long c0, long n, long stride, hipStream_t st);
// modified modes: the separable-fallback cells of records rec [nw] into list ([0] count, [1..] cells, then kFbBlocks
// block counts)
void enqueue_fbscan(const double* rec, long nw, int* list, hipStream_t st);
// PTMA: the C / B matrices of cells [p0, p1) of the launch in flight from their (lambda, aT, aL) in d_sol
int enqueue_famod_b(is3d_engine* e);
// the whole prepass of a launch on this engine alone (prepass_begin, every chain pass, chain_end).  srule: the chain
// rule (aniso_math.h aniso_cell), 0 for the spectra, 1 for the particle sampler; op: the prep constants' operation
int run_prepass(is3d_engine* e, void* stream, int srule, int op);
// the prepass counters of a launch whose stream has been waited for: d_cnt -> the stats
int read_counters(is3d_engine* e);

// f(std::integral_constant<int, MODE>{}) for df_mode `mode`: the one place a templated launcher's mode is chosen.
// FIRST: the lowest mode the site sees (an F_FB launch: PTM), so that it names no launcher for the modes below it
template <int FIRST = is3d::GRAD, class F>
static void with_mode(int mode, F f) {
  using namespace is3d;
  if constexpr (FIRST <= GRAD) { if (mode == GRAD) return f(std::integral_constant<int, GRAD>{}); }
  if constexpr (FIRST <= CE) { if (mode == CE) return f(std::integral_constant<int, CE>{}); }
  if (mode == PTM) return f(std::integral_constant<int, PTM>{});
  if (mode == PTB) return f(std::integral_constant<int, PTB>{});
  return f(std::integral_constant<int, PTMA>{});
}

// what is3d_calculate_spectra and is3d_calculate_polarization share: launch(d_out) into the engine's output buffer of
// outsize doubles on the null stream, finished and downloaded to `out`
template <class L>
static int calculate(is3d_engine* e, long outsize, double* out, L launch) {
  HIPCHK(e, hipSetDevice(e->device));
  if (!e->ws.d_out.reserve(outsize)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(output) failed");
  int rc = launch(e->ws.d_out.get());
  if (!rc) rc = is3d_finish(e);
  if (rc) return rc;
  HIPCHK(e, hipMemcpy(out, e->ws.d_out.get(), outsize * sizeof(double), hipMemcpyDeviceToHost));
  return IS3D_OK;
}
