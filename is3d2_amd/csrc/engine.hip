// engine.hip -- MI355X (gfx950) Cooper-Frye continuous-spectra engine behind the
// C ABI of include/is3d_amd.h: the core unit (engine.h lists the others).  This file is the host side of the setters,
// the tables, the prepass and the spectra; the kernels named below are in engine_kernels.h (the prepass, the
// reductions) and kernels.h (the momentum integrals).
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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <map>
#include <set>
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
#include "engine.h"

using namespace is3d;
using namespace is3d::kern;

#include "engine_kernels.h"   // this unit's device code (k_prep ... k_df_eval)

int hip_fail(is3d_engine* e, hipError_t h, const char* what) {
  return e->fail(IS3D_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(h));
}

int df_error(is3d_engine* e, int derr, const char* other) {
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
  if (!e->ws.d_err.reserve(1) || !e->ws.d_cnt.reserve(8)) {
    delete e;
    return nullptr;
  }
  for (auto& v : e->ws.ev) (void)v.create(hipEventDefault);
  for (auto& v : e->fd.ev) (void)v.create(hipEventDefault);
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
  e->sf.chain_q0 = e->sf.chain_q1 = -1;
  if (lo < 0 || hi < 0) { e->sf.win_lo = e->sf.win_hi = -1; return IS3D_OK; }
  if (lo > hi || hi > e->sf.ncell) return e->fail(IS3D_ERR_ARG, "cell window outside the surface");
  e->sf.win_lo = lo; e->sf.win_hi = hi;
  return IS3D_OK;
}

extern "C" int is3d_set_tuning(is3d_engine* e, const char* key, long value) {
  if (e && e->grp) return key ? is3d::group_set_tuning(e->grp, key, value) : IS3D_ERR_ARG;
  if (!e || !key) return IS3D_ERR_ARG;
  if (!std::strcmp(key, "phitab_one_bytes")) e->ws.phitab_one = value < 0 ? (long)IS3D_PHITAB_ONE : value;
  else if (!std::strcmp(key, "phitab_chunk_bytes")) e->ws.phitab_chunk = value <= 0 ? (long)IS3D_PHITAB_BYTES : value;
  else if (!std::strcmp(key, "max_splits")) e->ws.max_splits = value <= 0 ? (long)IS3D_MAX_SPLITS : value;
  else if (!std::strcmp(key, "slab_bytes")) e->ws.slab_bytes = value <= 0 ? (long)IS3D_SLAB_BYTES : value;
  else if (!std::strcmp(key, "split_bytes")) e->ws.split_bytes = value <= 0 ? (long)IS3D_SPLIT_BYTES : value;
  else if (!std::strcmp(key, "sample_bytes")) e->smp.sample_bytes = value <= 0 ? (long)IS3D_SAMPLE_BYTES : value;
  else return e->fail(IS3D_ERR_ARG, std::string("is3d_set_tuning: unknown key ") + key);
  return IS3D_OK;
}

extern "C" long is3d_get_tuning(const is3d_engine* e, const char* key) {
  if (!e || !key) return -1;
  if (e->grp) return is3d::group_get_tuning(e->grp, key);
  if (!std::strcmp(key, "phitab_one_bytes")) return e->ws.phitab_one;
  if (!std::strcmp(key, "phitab_chunk_bytes")) return e->ws.phitab_chunk;
  if (!std::strcmp(key, "phitab_chunks")) return e->ws.last_nchunk;
  if (!std::strcmp(key, "max_splits")) return e->ws.max_splits;
  if (!std::strcmp(key, "slab_bytes")) return e->ws.slab_bytes;
  if (!std::strcmp(key, "split_bytes")) return e->ws.split_bytes;
  if (!std::strcmp(key, "splits")) return e->ws.last_nsplit;
  if (!std::strcmp(key, "slabs")) return e->ws.last_nslab;
  if (!std::strcmp(key, "sample_bytes")) return e->smp.sample_bytes;
  if (!std::strcmp(key, "sample_batches")) return e->smp.list.stats.batches;
  if (!std::strcmp(key, "list_h2d_bytes")) return e->smp.list_h2d;
  if (!std::strcmp(key, "list_d2h_bytes")) return e->smp.list_d2h;
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
  e->in.p = *p;
  e->in.have_params = true;
  e->input_changed(IN_PARAMS);
  return IS3D_OK;
}

extern "C" int is3d_set_species(is3d_engine* e, int n, const double* mass, const double* sign, const double* degeneracy,
                                const double* baryon) {
  if (e && e->grp) return is3d::group_set_species(e->grp, n, mass, sign, degeneracy, baryon);
  if (!e || n <= 0 || !mass || !sign || !degeneracy || !baryon) return e ? e->fail(IS3D_ERR_ARG, "bad species arrays") : IS3D_ERR_ARG;
  e->in.mass.assign(mass, mass + n); e->in.sign.assign(sign, sign + n); e->in.degen.assign(degeneracy, degeneracy + n);
  e->in.baryon.assign(baryon, baryon + n);
  e->in.order.resize(n);
  for (int i = 0; i < n; i++) e->in.order[i] = i;
  // lanes of a wavefront take consecutive species: sort by mass so that whole wavefronts hit the
  // exp-underflow early-out together (output order is unchanged)
  std::stable_sort(e->in.order.begin(), e->in.order.end(), [&](int a, int b) { return e->in.mass[a] < e->in.mass[b]; });
  e->in.have_species = true;
  e->input_changed(IN_SPECIES);
  return IS3D_OK;
}

extern "C" int is3d_set_species_classes(is3d_engine* e, int on) {
  if (e && e->grp) return is3d::group_set_species_classes(e->grp, on);
  if (!e) return IS3D_ERR_ARG;
  e->in.classes = on != 0;
  e->input_changed(IN_CLASSES);
  return IS3D_OK;
}

extern "C" int is3d_species_integrated(is3d_engine* e) {
  if (e && e->grp) return is3d::group_species_integrated(e->grp);
  if (!e) return -IS3D_ERR_ARG;
  const int rc = finalize_tables(e);
  return rc ? -rc : e->tbl.ncls;       // an error as minus its IS3D_ERR_* code (a count is >= 1)
}

extern "C" int is3d_lanes_integrated(is3d_engine* e) {
  if (e && e->grp) return is3d::group_lanes_integrated(e->grp);
  if (!e) return -IS3D_ERR_ARG;
  const int rc = finalize_tables(e);
  return rc ? -rc : e->tbl.nlive;      // without the empty lanes that keep a table launch (finalize_tables)
}

extern "C" int is3d_set_pdg(is3d_engine* e, int n, const double* mass, const double* sign, const double* degeneracy,
                            const double* baryon) {
  if (e && e->grp) return is3d::group_set_pdg(e->grp, n, mass, sign, degeneracy, baryon);
  if (!e || n <= 0 || !mass || !sign || !degeneracy || !baryon) return e ? e->fail(IS3D_ERR_ARG, "bad pdg arrays") : IS3D_ERR_ARG;
  e->in.pdg_mass.assign(mass, mass + n); e->in.pdg_sign.assign(sign, sign + n); e->in.pdg_degen.assign(degeneracy, degeneracy + n);
  e->in.pdg_baryon.assign(baryon, baryon + n);
  e->in.have_pdg = true;
  e->input_changed(IN_PDG);
  return IS3D_OK;
}

extern "C" int is3d_set_momentum_grid(is3d_engine* e, int npT, const double* pT, int nphi, const double* phi, int ny,
                                      const double* y, int neta, const double* eta, const double* eta_weight) {
  if (e && e->grp) return is3d::group_set_momentum_grid(e->grp, npT, pT, nphi, phi, ny, y, neta, eta, eta_weight);
  if (!e) return IS3D_ERR_ARG;
  if (npT <= 0 || nphi <= 0 || !pT || !phi) return e->fail(IS3D_ERR_ARG, "empty pT/phi table");
  e->in.pT.assign(pT, pT + npT); e->in.phi.assign(phi, phi + nphi);
  e->in.y.assign(y ? y : pT, y ? y + std::max(ny, 0) : pT);
  e->in.eta.assign(eta ? eta : pT, eta ? eta + std::max(neta, 0) : pT);
  e->in.eta_w.assign(eta_weight ? eta_weight : pT, eta_weight ? eta_weight + std::max(neta, 0) : pT);
  e->in.have_grid = true;
  e->input_changed(IN_GRID);
  return IS3D_OK;
}

extern "C" int is3d_set_momentum_weights(is3d_engine* e, const double* pT_weight, const double* phi_weight) {
  if (e && e->grp) return is3d::group_set_momentum_weights(e->grp, pT_weight, phi_weight);
  if (!e) return IS3D_ERR_ARG;
  if (!e->in.have_grid) return e->fail(IS3D_ERR_STATE, "is3d_set_momentum_grid not called");
  if (!pT_weight || !phi_weight) return e->fail(IS3D_ERR_ARG, "null pT/phi weights");
  e->in.pT_w.assign(pT_weight, pT_weight + e->in.pT.size());
  e->in.phi_w.assign(phi_weight, phi_weight + e->in.phi.size());
  e->in.have_weights = true;
  e->input_changed(IN_WEIGHTS);
  return IS3D_OK;
}

extern "C" int is3d_set_spacetime_bins(is3d_engine* e, const is3d_spacetime_bins* b) {
  if (e && e->grp) return b ? is3d::group_set_spacetime_bins(e->grp, b) : IS3D_ERR_ARG;
  if (!e || !b) return IS3D_ERR_ARG;
  if (b->tau_bins <= 0 || b->r_bins <= 0 || b->phip_bins <= 0) return e->fail(IS3D_ERR_ARG, "spacetime bins must be positive");
  if (!(b->tau_max > b->tau_min) || !(b->r_max > b->r_min)) return e->fail(IS3D_ERR_ARG, "spacetime bin ranges must be increasing");
  if (b->threads < 0) return e->fail(IS3D_ERR_ARG, "spacetime threads must be >= 0");
  e->op0.bins = *b;
  e->op0.have_bins = true;
  return IS3D_OK;
}

extern "C" int is3d_set_gauss_laguerre(is3d_engine* e, int alpha, int points, const double* roots, const double* weights) {
  if (e && e->grp) return is3d::group_set_gauss_laguerre(e->grp, alpha, points, roots, weights);
  if (!e) return IS3D_ERR_ARG;
  if (alpha < 3 || points <= 0 || !roots || !weights) return e->fail(IS3D_ERR_ARG, "Gauss-Laguerre table needs alpha >= 3");
  e->in.gla_alpha = alpha; e->in.gla_pts = points;
  e->in.gla_r.assign(roots, roots + (size_t)alpha * points);
  e->in.gla_w.assign(weights, weights + (size_t)alpha * points);
  e->in.have_gla = true;
  e->input_changed(IN_GLA);
  return IS3D_OK;
}

extern "C" int is3d_set_df_tables(is3d_engine* e, int nT, int nmuB, const double* T, const double* muB,
                                  const double* tables, double T_avg) {
  if (e && e->grp) return is3d::group_set_df_tables(e->grp, nT, nmuB, T, muB, tables, T_avg);
  if (!e) return IS3D_ERR_ARG;
  if (nT < 3 || nmuB < 1 || !T || !muB || !tables) return e->fail(IS3D_ERR_ARG, "bad df coefficient tables");
  e->in.nT = nT; e->in.nmuB = nmuB;
  e->in.Tarr.assign(T, T + nT); e->in.muBarr.assign(muB, muB + nmuB);
  e->in.tab.assign(tables, tables + (size_t)10 * nmuB * nT);
  e->in.T_avg = T_avg;
  e->in.have_df = true;
  e->input_changed(IN_DF);
  return IS3D_OK;
}

// PTB Jonah table on the device (k_jonah_terms + k_jonah_sum) into e->tbl.jl2 / jz / jx / bp_max; the
// host keeps only the two 301-point spline solves
static int device_jonah_table(is3d_engine* e, const double* r2, const double* w2) {
  const int npdg = (int)e->in.pdg_mass.size(), pts = e->in.gla_pts;
  if (npdg == 0) return e->fail(IS3D_ERR_STATE, "PTB needs the PDG (is3d_set_pdg)");
  std::vector<double> in;
  in.insert(in.end(), e->in.pdg_mass.begin(), e->in.pdg_mass.end());
  in.insert(in.end(), e->in.pdg_degen.begin(), e->in.pdg_degen.end());
  in.insert(in.end(), e->in.pdg_sign.begin(), e->in.pdg_sign.end());
  in.insert(in.end(), r2, r2 + pts);
  in.insert(in.end(), w2, w2 + pts);
  const size_t nterms = (size_t)(kJonahN + 1) * 2 * npdg, nout = 3 * (size_t)kJonahN;
  DevBuf<double> buf;
  if (!buf.reserve((long)(in.size() + nterms + nout))) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(Jonah table) failed");
  double* const d = buf.get();
  JonahArgs ja{};
  ja.T = e->in.T_avg; ja.npdg = npdg; ja.pts = pts;
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
  e->tbl.jl2.assign(out.begin(), out.begin() + kJonahN);
  e->tbl.jz.assign(out.begin() + kJonahN, out.begin() + 2 * kJonahN);
  e->tbl.jx.assign(out.begin() + 2 * kJonahN, out.end());
  e->tbl.bp_max = -1.0;
  for (int i = 0; i < kJonahN; i++) e->tbl.bp_max = std::fmax(e->tbl.bp_max, e->tbl.jx[i]);
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
  const int mode = e->in.p.df_mode, dim = e->in.p.dimension;
  const int np = e->tbl.nlane, nphi = (int)e->in.phi.size();     // lane species: the lane classes
  const int npT = (int)e->in.pT.size();
  const int nk = (dim == 3) ? (int)e->in.y.size() : 1, nl = (dim == 3) ? 1 : (int)e->in.eta.size();
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
    P.tb = ((mode == GRAD || mode == CE) && (!e->in.p.include_baryon || ts_shape) &&
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
      // records x 3, trig + {pc, ps}, grid, y-term rows x 2 (k_ytab's, kYRowTS), exp table, T1 rows
      // [tile][qrows][KJ + 2] (+ 1: alignment)
      return sizeof(double) * (3 * tile * NREC + 4 * nphp + (size_t)(nk + 2 * nl) +
                               2 * tile * std::min(qrows, P.nq) * kYRowTS + kExpTabN + tile * qrows * (P.KJ + 2) + 1 +
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
  // the phi block's lane fill is judged by the integrand classes, not by the lanes a baryon-blind run merges them
  // into (the same count otherwise): a merge then never moves a grid of one or two q rows off its one-block table
  // launch (SMASH, 24 phi points, one rapidity: 193 tasks keep KJ = 24 and F_TS where 135 would take KJ = 8)
  shape(spectra_kj_fill(nphi, (long)e->tbl.ncls * P.nq));
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
  P.by = (P.ts && e->in.p.include_baryon) ? F_BY : 0;
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

// Baryon-blind runs: the lanes of a baryon and of its antibaryon of equal (mass, sign) integrate the same integrand, so
// the lane classes drop the baryon number from their key (finalize_tables).  A lane's baryon number b enters only as a
// factor of per-cell quantities:
//   the separable lanes   b R_CHEM, mT b Y_S1, b R_SCB, b R_SSB, b R_L0B      (sep_skips, sep_setup)
//   the modified lanes    b R_CHEMM                                            (mod_skips, mod_setup)
//   ptm_renorm            b alphaB, b alphaB_mod, b N10 G
// With include_baryon = 0 every prologue packs alphaB = 0, nB / (E + P) = 0 and V^mu = 0 whatever the surface holds
// (prep_grad_ce, prep_feqmod, prep_famod_a), which zeroes R_CHEM and every V^mu product (Grad's c3 and c4, the betaV
// terms).  What is left comes from the delta-f table, per mode:
//   Grad (1)        c1, column 1: R_BULK1 = c1 Pi -> Y_S1, R_SCB, R_SSB
//   RTA-CE (2)      G, column 6:  R_BULK1 = G Pi / betabulk -> R_L0B
//   PTM (3)         G, column 6:  the same in its linearised fallback; alphaB_mod = alphaB + Pi G / betabulk -> R_CHEMM;
//                   N10 G in ptm_renorm
//   PTB (4)         none: R_CHEM = 0, lambda and z come from the Jonah table (and include_baryon = 1 is refused)
//   PTMA (5)        none: R_CHEM = R_CHEMM = alphaB, no delta-f coefficient reaches the lanes
// df_eval sets c1 = G = 0 without reading them when include_baryon = 0 -- but that is the assumption this function
// exists to check: the column must be identically zero on the table row such a run uses (muB row 0, every T), or the
// lanes keep the full key.  Tables from is3d_generate_df_tables reach the engine through is3d_set_df_tables like any
// other, so the same check sees them.
constexpr double kEmptyLaneMass = 1.0e6;   // GeV: the lanes finalize_tables adds to keep a table launch (no members)
static bool baryon_blind(const is3d_engine* e) {
  if (e->in.p.include_baryon) return false;
  const int mode = e->in.p.df_mode;
  const int col = mode == GRAD ? 1 : (mode == CE || mode == PTM) ? 6 : -1;
  if (col < 0) return true;
  const double* row = e->in.tab.data() + (size_t)col * e->in.nmuB * e->in.nT;   // muB row 0
  for (int i = 0; i < e->in.nT; i++)
    if (row[i] != 0.0) return false;     // NaN too
  return true;
}

int finalize_tables(is3d_engine* e) {
  if (!e->in.have_params) return e->fail(IS3D_ERR_STATE, "is3d_set_params not called");
  if (!e->in.have_species) return e->fail(IS3D_ERR_STATE, "is3d_set_species not called");
  if (!e->in.have_grid) return e->fail(IS3D_ERR_STATE, "is3d_set_momentum_grid not called");
  if (!e->in.have_df) return e->fail(IS3D_ERR_STATE, "is3d_set_df_tables not called");
  const int mode = e->in.p.df_mode;
  if ((mode == PTM || mode == PTB) && !e->in.have_gla) return e->fail(IS3D_ERR_STATE, "is3d_set_gauss_laguerre not called");
  if ((mode == PTB || mode == PTMA) && !e->in.have_pdg) return e->fail(IS3D_ERR_STATE, "is3d_set_pdg not called");
  if (e->in.p.dimension == 3 && e->in.y.empty()) return e->fail(IS3D_ERR_ARG, "dimension = 3 needs a y table");
  if (e->in.p.dimension == 2 && e->in.eta.empty()) return e->fail(IS3D_ERR_ARG, "dimension = 2 needs an eta table");
  if (!e->is_stale(D_TABLES)) return IS3D_OK;
  HIPCHK(e, hipSetDevice(e->device));
  const int nT = e->in.nT, nmuB_used = e->in.p.include_baryon ? e->in.nmuB : 1;
  // --- delta-f blob: T | muB | tab | 7 x (y, c) | jonah x, l2, l2c, z, zc
  std::vector<double> blob;
  auto put = [&](const double* v, size_t n) { size_t off = blob.size(); blob.insert(blob.end(), v, v + n); return off; };
  const size_t oT = put(e->in.Tarr.data(), nT);
  const size_t omu = put(e->in.muBarr.data(), e->in.nmuB);
  const size_t otab = put(e->in.tab.data(), e->in.tab.size());
  size_t osy[NSPL] = {0}, osc[NSPL] = {0};
  const int spl_col[NSPL] = {0, 2, 3, 5, 7, 8, 9};   // c0 c2 c3 F betabulk betaV betapi
  if (!e->in.p.include_baryon) {
    for (int k = 0; k < NSPL; k++) {
      const double* yv = e->in.tab.data() + (size_t)spl_col[k] * e->in.nmuB * nT;   // muB row 0
      std::vector<double> c;
      if (!cspline_coeffs(e->in.Tarr.data(), yv, nT, c)) return e->fail(IS3D_ERR_ARG, "gsl: x values must be strictly increasing (T table)");
      osy[k] = put(yv, nT);
      osc[k] = put(c.data(), nT);
    }
  }
  size_t ojx = 0, ojl = 0, ojlc = 0, ojz = 0, ojzc = 0;
  int nj = 0;
  if (!e->in.p.include_baryon && mode == PTB) {
    const double* r2 = e->in.gla_r.data() + 2 * e->in.gla_pts;
    const double* w2 = e->in.gla_w.data() + 2 * e->in.gla_pts;
    const int rc = device_jonah_table(e, r2, w2);
    if (rc) return rc;
    if (!cspline_coeffs(e->tbl.jx.data(), e->tbl.jl2.data(), 301, e->tbl.jl2c) || !cspline_coeffs(e->tbl.jx.data(), e->tbl.jz.data(), 301, e->tbl.jzc))
      return e->fail(IS3D_ERR_DF_RANGE, "gsl: x values must be strictly increasing (Jonah bulkPi/P table)");
    nj = 301;
    ojx = put(e->tbl.jx.data(), 301); ojl = put(e->tbl.jl2.data(), 301); ojlc = put(e->tbl.jl2c.data(), 301);
    ojz = put(e->tbl.jz.data(), 301); ojzc = put(e->tbl.jzc.data(), 301);
  }
  e->tbl.d_tables.reset();      // a new blob every time, as large as it needs to be
  if (!e->tbl.d_tables.reserve((long)blob.size())) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(tables) failed");
  const double* const dt = e->tbl.d_tables.get();
  HIPCHK(e, hipMemcpy(e->tbl.d_tables.get(), blob.data(), blob.size() * sizeof(double), hipMemcpyHostToDevice));
  DfTables& tb = e->tbl.dtb;
  tb.df_mode = mode; tb.include_baryon = e->in.p.include_baryon;
  tb.nT = nT; tb.nmuB = nmuB_used;
  tb.T = dt + oT; tb.muB = dt + omu; tb.tab = dt + otab;
  tb.T_min = e->in.Tarr[0]; tb.muB_min = e->in.muBarr[0];
  tb.dT = std::fabs(e->in.Tarr[1] - e->in.Tarr[0]);
  tb.dmuB = e->in.nmuB > 1 ? std::fabs(e->in.muBarr[1] - e->in.muBarr[0]) : 0.0;
  for (int k = 0; k < NSPL; k++) { tb.sy[k] = dt + osy[k]; tb.sc[k] = dt + osc[k]; }
  tb.nj = nj; tb.jx = dt + ojx; tb.jl2 = dt + ojl; tb.jl2c = dt + ojlc;
  tb.jz = dt + ojz; tb.jzc = dt + ojzc;
  tb.bulk_over_P_max = e->tbl.bp_max;
  // tab is laid out [10][nmuB][nT]; with include_baryon = 0 only muB row 0 is used (nmuB_used = 1)
  // but the stride must stay the file's nmuB
  if (!e->in.p.include_baryon) tb.nmuB = 1;
  // --- constants blob: sorted species, original degeneracy, grids, gla, pdg
  const int np = (int)e->in.mass.size();
  std::vector<double> cb;
  auto cput = [&](const double* v, size_t n) { size_t off = cb.size(); cb.insert(cb.end(), v, v + n); return off; };
  std::vector<double> sm(np), ss(np), sb(np), sd(np);
  for (int i = 0; i < np; i++) { const int o = e->in.order[i]; sm[i] = e->in.mass[o]; ss[i] = e->in.sign[o]; sb[i] = e->in.baryon[o]; sd[i] = e->in.degen[o]; }
  const size_t osm = cput(sm.data(), np), oss = cput(ss.data(), np), osb = cput(sb.data(), np), osd = cput(sd.data(), np);
  const size_t odg = cput(e->in.degen.data(), np);
  const size_t opt = cput(e->in.pT.data(), e->in.pT.size());
  std::vector<double> cph(e->in.phi.size()), sph(e->in.phi.size());
  for (size_t j = 0; j < e->in.phi.size(); j++) { cph[j] = std::cos(e->in.phi[j]); sph[j] = std::sin(e->in.phi[j]); }
  const size_t oc = cput(cph.data(), cph.size()), os = cput(sph.data(), sph.size());
  const size_t oy = cput(e->in.y.data(), e->in.y.size()), oe = cput(e->in.eta.data(), e->in.eta.size()), ow = cput(e->in.eta_w.data(), e->in.eta_w.size());
  std::vector<double> pTw(e->in.pT.size(), 0.0), phiw(e->in.phi.size(), 0.0);
  if (e->in.have_weights) { pTw = e->in.pT_w; phiw = e->in.phi_w; }
  const size_t opw = cput(pTw.data(), pTw.size()), ophw = cput(phiw.data(), phiw.size());
  // The classes of the sorted species, on two levels (engine.h Tables).  The integrand classes keep the documented key
  // and are only counted; the lane classes, which every table below describes, drop the baryon number from it when
  // the run is baryon-blind.  First occurrence order, so the lane list stays mass-sorted.
  const bool blind = e->in.classes && baryon_blind(e);
  auto bkey = [&](int i) { return blind ? (uint64_t)0 : __builtin_bit_cast(uint64_t, sb[i]); };
  std::vector<int> scls(np), crep, cmem_off, cmem;
  {
    std::map<std::array<uint64_t, 4>, int> cls;
    std::set<std::array<uint64_t, 4>> full;
    for (int i = 0; i < np; i++) {
      const uint64_t gk = mode == PTM ? ptm_gkey(sd[i]) : (uint64_t)0;
      const std::array<uint64_t, 4> key{__builtin_bit_cast(uint64_t, sm[i]), __builtin_bit_cast(uint64_t, ss[i]), bkey(i), gk};
      full.insert({key[0], key[1], __builtin_bit_cast(uint64_t, sb[i]), gk});
      int c = (int)crep.size();
      if (e->in.classes) {
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
    e->tbl.nlive = e->tbl.nlane = nc;
    e->tbl.ncls = e->in.classes ? (int)full.size() : np;
    e->tbl.blind = blind;
    e->tbl.scls = scls;
    // A merge must not cost the Grad / RTA-CE table launches (F_TB, F_TS): a workgroup's 256 tasks span at most
    // kTbQ q rows only from kTbLanes lanes on (spectra_plan nqmax).  A list whose classes reach that count but whose
    // merged lanes do not (UrQMD: 124 classes, 75 lanes) gets empty lanes up to it: no member, so nothing is written
    // for them, and a mass no cell can reach, so every one is skipped at the lane's first test (sep_skips) like the
    // heavy resonances of a cold cell.  86 lane slots still beat 124.
    constexpr int kTbLanes = (kBlock - 1) / (kTbQ - 1) + 1;
    static_assert((kBlock - 1) / kTbLanes + 2 <= kTbQ && (kBlock - 1) / (kTbLanes - 1) + 2 > kTbQ, "the smallest lane count of the table launches");
    if (blind && mode <= CE && nc < kTbLanes && e->tbl.ncls >= kTbLanes) {
      e->tbl.nlane = kTbLanes;
      cmem_off.resize(kTbLanes + 1, cmem_off.back());
    }
  }
  const int nlane = e->tbl.nlane, nlive = e->tbl.nlive;
  std::vector<double> cm(nlane, kEmptyLaneMass), csn(nlane, 1.0), cby(nlane, 0.0);
  for (int c = 0; c < nlive; c++) { cm[c] = sm[crep[c]]; csn[c] = ss[crep[c]]; cby[c] = sb[crep[c]]; }
  const size_t ocm = cput(cm.data(), nlane), ocs_ = cput(csn.data(), nlane), ocb = cput(cby.data(), nlane);
  // {pT cos phi, pT sin phi} per (pT, padded phi slot) for k_spectra's scalar loads (same products as
  // its LDS copy s_cs); 16-byte aligned
  if (cb.size() & 1) cb.push_back(0.0);
  const int kj_cs = spectra_plan(e).KJ;
  const int nphp_cs = (int)((e->in.phi.size() + kj_cs - 1) / kj_cs) * kj_cs;
  std::vector<double> csv((size_t)e->in.pT.size() * nphp_cs * 2, 0.0);
  for (size_t i = 0; i < e->in.pT.size(); i++)
    for (size_t j = 0; j < e->in.phi.size(); j++) {
      csv[(i * nphp_cs + j) * 2] = e->in.pT[i] * cph[j];
      csv[(i * nphp_cs + j) * 2 + 1] = e->in.pT[i] * sph[j];
    }
  const size_t ocs = cput(csv.data(), csv.size());
  const size_t og = cput(e->in.gla_r.data(), e->in.gla_r.size());
  cput(e->in.gla_w.data(), e->in.gla_w.size());
  const size_t opd = cput(e->in.pdg_mass.data(), e->in.pdg_mass.size());
  cput(e->in.pdg_sign.data(), e->in.pdg_sign.size());
  cput(e->in.pdg_degen.data(), e->in.pdg_degen.size());
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
    const int nh = std::min(320, (int)e->in.pdg_mass.size());
    for (int i = 0; i < nh; i++) {
      int k = -1;
      for (size_t u = 0; u < am.size(); u++)
        if (am[u] == e->in.pdg_mass[i] && as[u] == e->in.pdg_sign[i]) { k = (int)u; break; }
      if (k < 0) { am.push_back(e->in.pdg_mass[i]); as.push_back(e->in.pdg_sign[i]); ag.push_back(e->in.pdg_degen[i]); }
      else ag[k] += e->in.pdg_degen[i];
    }
    if (am.empty()) { am.push_back(0.0); as.push_back(0.0); ag.push_back(0.0); }
  }
  e->tbl.n_aniso_h = e->in.pdg_mass.empty() ? 0 : (int)am.size();
  const size_t oah = cput(am.data(), am.size());
  cput(as.data(), as.size());
  cput(ag.data(), ag.size());
  std::vector<int> rcls(np), rrep;
  {
    std::map<std::array<uint64_t, 4>, int> cls;
    for (int i = 0; i < np; i++) {
      const std::array<uint64_t, 4> key{__builtin_bit_cast(uint64_t, sm[i]), __builtin_bit_cast(uint64_t, ss[i]),
                                        ptm_gkey(sd[i]), bkey(i)};     // baryon-blind: as the lanes (baryon_blind)
      auto it = cls.find(key);
      if (it == cls.end()) { it = cls.emplace(key, (int)rrep.size()).first; rrep.push_back(i); }
      rcls[i] = it->second;
    }
  }
  e->tbl.nrcls = (int)rrep.size();
  const int nc = nlane;
  std::vector<int> crcls(nc, 0);
  for (int c = 0; c < nlive; c++) crcls[c] = rcls[crep[c]];
  // ints after the doubles: sorig[np] | rcls[np] | rrep[np] | crcls[nc] | cmem_off[nc + 1] | cmem[np] | scls[np]
  std::vector<int> ib;
  for (int i = 0; i < np; i++) ib.push_back(e->in.order[i]);
  ib.insert(ib.end(), rcls.begin(), rcls.end());
  rrep.resize(np, 0);
  ib.insert(ib.end(), rrep.begin(), rrep.end());
  ib.insert(ib.end(), crcls.begin(), crcls.end());
  ib.insert(ib.end(), cmem_off.begin(), cmem_off.end());
  ib.insert(ib.end(), cmem.begin(), cmem.end());
  ib.insert(ib.end(), scls.begin(), scls.end());
  e->tbl.d_const.reset();
  if (!e->tbl.d_const.reserve((long)(cb.size() + (ib.size() + 1) / 2))) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(constants) failed");
  double* const dc = e->tbl.d_const.get();
  HIPCHK(e, hipMemcpy(dc, cb.data(), cb.size() * sizeof(double), hipMemcpyHostToDevice));
  int* const di = (int*)(dc + cb.size());
  HIPCHK(e, hipMemcpy(di, ib.data(), ib.size() * sizeof(int), hipMemcpyHostToDevice));
  e->tbl.d_sorig = di;
  e->tbl.d_rcls = di + np;
  e->tbl.d_rrep = di + 2 * (size_t)np;
  e->tbl.d_crcls = di + 3 * (size_t)np;
  e->tbl.d_cmem_off = e->tbl.d_crcls + nc;
  e->tbl.d_cmem = e->tbl.d_cmem_off + nc + 1;
  e->tbl.d_scls = e->tbl.d_cmem + np;
  e->tbl.d_cmass = dc + ocm; e->tbl.d_csign = dc + ocs_; e->tbl.d_cbaryon = dc + ocb;
  e->tbl.d_smass = dc + osm; e->tbl.d_ssign = dc + oss; e->tbl.d_sbaryon = dc + osb; e->tbl.d_sdegen = dc + osd;
  e->tbl.d_degen_orig = dc + odg; e->tbl.d_pT = dc + opt; e->tbl.d_cphi = dc + oc; e->tbl.d_sphi = dc + os;
  e->tbl.d_y = dc + oy; e->tbl.d_eta = dc + oe; e->tbl.d_etaw = dc + ow;
  e->tbl.d_gla = dc + og; e->tbl.d_pdg = dc + opd; e->tbl.d_aniso_h = dc + oah;
  e->tbl.d_pTw = dc + opw; e->tbl.d_phiw = dc + ophw;
  e->tbl.d_csg = dc + ocs;
  e->rebuilt(D_TABLES);
  return IS3D_OK;
}

// What every surface setter does on taking a surface of n cells.  owned: d_surf becomes the engine's own buffer --
// reallocated when too small, or more than twice the size (a device group's cost prepass uploads the whole surface
// to shard 0 before its own window); otherwise that buffer is dropped and the caller points d_surf at its memory.
// The vorticity, the cell window and the chain range belonged to the previous surface.
static int adopt_surface(is3d_engine* e, long n, bool owned) {
  if (!owned || e->sf.surf_own.capacity() > (long)NSURF * (2 * n + 4096)) e->sf.surf_own.reset();
  const bool ok = !owned || e->sf.surf_own.reserve((long)NSURF * std::max(n, 1L));
  e->sf.d_surf = e->sf.surf_own.get();
  if (!ok) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(surface) failed");
  e->sf.ncell = n;
  e->sf.have_surf = true;
  e->pol.have_vort = false;
  e->sf.win_lo = e->sf.win_hi = -1;
  e->sf.chain_q0 = e->sf.chain_q1 = -1;
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
    double* dst = e->sf.d_surf + (size_t)f * n;
    if (fields[f]) HIPCHK(e, hipMemcpy(dst, fields[f], n * sizeof(double), hipMemcpyHostToDevice));
    else HIPCHK(e, hipMemset(dst, 0, n * sizeof(double)));
  }
  return IS3D_OK;
}

extern "C" int is3d_set_surface_device(is3d_engine* e, long n, const double* dev_fields) {
  if (e && e->grp) return is3d::group_set_surface_device(e->grp, n, dev_fields);
  if (!e || n < 0 || (!dev_fields && n > 0)) return e ? e->fail(IS3D_ERR_ARG, "bad device surface") : IS3D_ERR_ARG;
  (void)adopt_surface(e, n, false);
  e->sf.d_surf = const_cast<double*>(dev_fields);
  return IS3D_OK;
}

extern "C" int is3d_internal_copy_surface(is3d_engine* e, long n, const double* src, long src_n, int src_device, long lo) {
  if (!e || e->grp || n < 0 || lo < 0 || lo + n > src_n || (!src && n > 0)) return e ? e->fail(IS3D_ERR_ARG, "bad surface copy") : IS3D_ERR_ARG;
  HIPCHK(e, hipSetDevice(e->device));
  const int rc = adopt_surface(e, n, true);
  if (rc) return rc;
  for (int f = 0; f < NSURF && n > 0; f++)
    HIPCHK(e, hipMemcpyPeer(e->sf.d_surf + (size_t)f * n, e->device, src + (size_t)f * src_n + lo, src_device, n * sizeof(double)));
  return IS3D_OK;
}

extern "C" long is3d_output_size(const is3d_engine* e) {
  if (e && e->grp) return is3d::group_output_size(e->grp);
  if (!e || !e->in.have_species || !e->in.have_grid || !e->in.have_params) return -1;
  const long ny = (e->in.p.dimension == 3) ? (long)e->in.y.size() : 1;
  return (long)e->in.mass.size() * (long)e->in.pT.size() * (long)e->in.phi.size() * ny;
}

PrepConsts make_consts(const is3d_engine* e) {
  PrepConsts k{};
  k.operation = 1;
  k.df_mode = e->in.p.df_mode; k.dim = e->in.p.dimension; k.include_baryon = e->in.p.include_baryon;
  k.include_bulk = e->in.p.include_bulk_deltaf; k.include_shear = e->in.p.include_shear_deltaf;
  k.include_diff = e->in.p.include_baryondiff_deltaf;
  k.deta_min = e->in.p.deta_min; k.mass_pion0 = e->in.p.mass_pion0;
  k.gla_pts = e->in.gla_pts;
  if (e->in.have_gla) {
    k.gla_r1 = e->tbl.d_gla + 1 * e->in.gla_pts; k.gla_r2 = e->tbl.d_gla + 2 * e->in.gla_pts;
    const double* w = e->tbl.d_gla + (size_t)e->in.gla_alpha * e->in.gla_pts;
    k.gla_w1 = w + 1 * e->in.gla_pts; k.gla_w2 = w + 2 * e->in.gla_pts;
  }
  k.two_pi2_hbarC3 = 2.0 * std::pow(M_PI, 2) * std::pow(kHbarC, 3);
  k.pT_max = 0.0; k.b_max = 0.0;
  for (double v : e->in.pT) k.pT_max = std::max(k.pT_max, std::fabs(v));
  for (double v : e->in.baryon) k.b_max = std::max(k.b_max, std::fabs(v));
  return k;
}

// ---- host sequences the entry points share (declared in engine.h) ------------------------------------------------
void cell_window(const is3d_engine* e, long& lo, long& hi) {
  lo = e->sf.win_hi >= 0 ? e->sf.win_lo : 0;
  hi = e->sf.win_hi >= 0 ? e->sf.win_hi : e->sf.ncell;
}

int begin_stats(is3d_engine* e, long cells, hipStream_t st) {
  e->ws.st = is3d_stats{};
  e->ws.st.cells = cells;
  HIPCHK(e, hipMemsetAsync(e->ws.d_err.get(), 0, sizeof(int), st));
  HIPCHK(e, hipMemsetAsync(e->ws.d_cnt.get(), 0, 8 * sizeof(unsigned long long), st));
  HIPCHK(e, hipEventRecord(e->ws.ev[0].get(), st));
  return IS3D_OK;
}

void read_timings(is3d_engine* e) {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, e->ws.ev[0].get(), e->ws.ev[1].get()) == hipSuccess) e->ws.st.ms_prepass = ms;
  if (hipEventElapsedTime(&ms, e->ws.ev[1].get(), e->ws.ev[2].get()) == hipSuccess) e->ws.st.ms_spectra = ms;
  if (hipEventElapsedTime(&ms, e->ws.ev[0].get(), e->ws.ev[3].get()) == hipSuccess) e->ws.st.ms_total = ms;
}

PrepArgs prep_args(const is3d_engine* e, double* rec, double* aux, long c0, long c1, int* err,
                          unsigned long long* cnt) {
  PrepArgs pa{};
  pa.k = make_consts(e); pa.tb = e->tbl.dtb; pa.surf = e->sf.d_surf; pa.rec = rec; pa.aux = aux; pa.n = e->sf.ncell;
  pa.c0 = c0; pa.c1 = c1;
  pa.err = err; pa.cnt = cnt;
  return pa;
}
// the ascending fallback-cell list of nw records into list[1 ..], its length into list[0]; list holds nw + 1 +
// kFbBlocks ints (the per-range counts after the list)
void enqueue_fbscan(const double* rec, long nw, int* list, hipStream_t st) {
  int* bcnt = list + 1 + nw;
  hipLaunchKernelGGL(k_fbcount, dim3(kFbBlocks), dim3(256), 0, st, rec, nw, bcnt);
  hipLaunchKernelGGL(k_fbwrite, dim3(kFbBlocks), dim3(256), 0, st, rec, nw, (const int*)bcnt, list + 1, list);
}

int enqueue_prep(is3d_engine* e, const PrepArgs& pa, hipStream_t st) {
  const dim3 g1((unsigned)std::max(1L, (pa.c1 - pa.c0 + 255) / 256)), b1(256);
  with_mode(e->in.p.df_mode, [&](auto M) { hipLaunchKernelGGL(k_prep<decltype(M)::value>, g1, b1, 0, st, pa); });
  HIPCHK(e, hipGetLastError());
  return IS3D_OK;
}

int enqueue_renorm(is3d_engine* e, const PrepConsts& k, long c0, long n, long stride, hipStream_t st) {
  const long tot = n * (long)e->tbl.nrcls;
  if (!e->ws.d_renorm.reserve(tot)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(renorm) failed");
  RenormArgs ra{};
  ra.k = k; ra.rec = e->ws.d_rec.get(); ra.aux = e->ws.d_aux.get(); ra.renorm = e->ws.d_renorm.get();
  ra.mass = e->tbl.d_smass; ra.sign = e->tbl.d_ssign; ra.degen = e->tbl.d_sdegen; ra.baryon = e->tbl.d_sbaryon;
  ra.c0 = c0; ra.n = n; ra.stride = stride;
  ra.npart = e->tbl.nrcls; ra.rrep = e->tbl.d_rrep;
  hipLaunchKernelGGL(k_renorm, dim3((unsigned)std::max(1L, (tot + 255) / 256)), dim3(256), 0, st, ra);
  HIPCHK(e, hipGetLastError());
  return IS3D_OK;
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
  LaunchCtx& L = e->ws.lc;
  L = LaunchCtx{};
  hipStream_t st = (hipStream_t)stream;
  L.st = st;
  const long n = e->sf.ncell;
  const int mode = e->in.p.df_mode;
  // cell window (group shards holding the whole surface): k_spectra integrates [wlo, whi); the prepass covers
  // the window too, except for PTMA's warm-start chains, which walk every cell (MomentumSpectra.cpp:1308-1364) --
  // or, when a device group splits the chains (q1 >= 0), the cells of this shard's positions, which are its window
  long wlo, whi;
  cell_window(e, wlo, whi);
  const long nw = whi - wlo;
  const bool chained = mode == PTMA && e->in.p.famod_chains > 0;
  const bool split_chain = chained && q1 >= 0;
  const long p0 = chained && !split_chain ? 0 : wlo, p1 = chained && !split_chain ? n : whi;
  L.wlo = wlo; L.whi = whi; L.nw = nw; L.p0 = p0; L.p1 = p1; L.chained = chained;
  int rc = begin_stats(e, nw, st);
  if (rc) return rc;
  if (nw == 0) {
    L.empty = true;
    return IS3D_OK;
  }
  if (!e->ws.d_rec.reserve((long)NREC * n)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(records) failed");
  if (!e->ws.d_aux.reserve(9L * n)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(aux) failed");
  if (mode == PTMA && !e->ws.d_sol.reserve(6L * n)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(sol) failed");
  L.pa = prep_args(e, e->ws.d_rec.get(), e->ws.d_aux.get(), p0, p1, e->ws.d_err.get(), e->ws.d_cnt.get());
  L.pa.k.operation = op;
  rc = enqueue_prep(e, L.pa, st);
  if (rc) return rc;
  if (mode == PTMA) {
    AnisoArgs aa{};
    aa.rec = e->ws.d_rec.get(); aa.ain = e->ws.d_aux.get(); aa.sol = e->ws.d_sol.get(); aa.stride = n;
    aa.c0 = p0; aa.n = p1 - p0;
    aa.chains = chained ? std::min<long>(e->in.p.famod_chains, n) : std::max(1L, p1 - p0);
    const int nh = e->tbl.n_aniso_h;
    aa.h = Hadrons{nh, e->tbl.d_aniso_h, e->tbl.d_aniso_h + nh, e->tbl.d_aniso_h + 2 * nh};
    aa.fp2 = 4.0 * std::pow(M_PI, 2) * std::pow(kHbarC, 3);
    aa.cnt = e->ws.d_cnt.get();
    aa.srule = srule;
    if (!chained) {
      hipLaunchKernelGGL(k_aniso, dim3((unsigned)aa.chains), dim3(64), 0, st, aa);
      HIPCHK(e, hipGetLastError());
    } else {
      // warm-start chains in parallel segments (k_chain_pass): ~16k segments of this engine's positions keep the
      // GPU full
      ChainArgs& ca = L.ca;
      ca.rec = e->ws.d_rec.get(); ca.ain = e->ws.d_aux.get(); ca.sol = e->ws.d_sol.get(); ca.n = n; ca.C = aa.chains; ca.h = aa.h; ca.fp2 = aa.fp2;
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
      if (!e->ws.d_chain.reserve(need)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(chain state) failed");
      ca.sta = e->ws.d_chain.get(); ca.info = (int*)(e->ws.d_chain.get() + 4 * n);
      ca.send = e->ws.d_chain.get() + 4 * n + (n + 1) / 2; ca.sstart = ca.send + 8 * nseg;
      ca.changed = (int*)(ca.sstart + 4 * nseg);
      ca.bin = ca.sstart + 4 * nseg + kChainPasses;
      ca.bout = ca.bin + kBndSlots * bw;
      HIPCHK(e, hipMemsetAsync(ca.changed, 0, kChainPasses * sizeof(int), st));
    }
  }
  return IS3D_OK;
}

static int chain_pass(is3d_engine* e, int pass) {
  LaunchCtx& L = e->ws.lc;
  if (L.empty || !L.chained) return IS3D_OK;
  HIPCHK(e, hipSetDevice(e->device));
  hipLaunchKernelGGL(k_chain_pass, dim3((unsigned)(L.ca.C * L.ca.nspc)), dim3(64 * IS3D_CHAIN_W), 0, L.st, L.ca, pass);
  HIPCHK(e, hipGetLastError());
  return IS3D_OK;
}

static int chain_end(is3d_engine* e) {
  LaunchCtx& L = e->ws.lc;
  if (L.empty || !L.chained) return IS3D_OK;
  HIPCHK(e, hipSetDevice(e->device));
  const long c_lo = L.ca.q0 * L.ca.C, c_hi = std::min(e->sf.ncell, L.ca.q1 * L.ca.C);
  hipLaunchKernelGGL(k_chain_finish, dim3(1), dim3(64 * IS3D_CHAIN_W), 0, L.st, L.ca);
  hipLaunchKernelGGL(k_chain_count, dim3((unsigned)std::min(1024L, std::max(1L, (c_hi - c_lo + 255) / 256))), dim3(256), 0,
                     L.st, (const double*)e->ws.d_rec.get(), (const int*)L.ca.info, c_lo, c_hi, e->ws.d_cnt.get());
  HIPCHK(e, hipGetLastError());
  return IS3D_OK;
}

int run_prepass(is3d_engine* e, void* stream, int srule, int op) {
  int rc = prepass_begin(e, stream, 0, -1, 0, srule, op);
  for (int pass = 0; !rc && e->ws.lc.chained && pass < e->ws.lc.ca.npass; pass++) rc = chain_pass(e, pass);
  return rc ? rc : chain_end(e);
}

// whole: the chains too (run_prepass: is3d_launch); otherwise the caller stages them (a chain range q0, q1, has_pred)
static int launch_begin(is3d_engine* e, double* dev_out, void* stream, long q0, long q1, int has_pred, bool whole = false) {
  int rc = finalize_tables(e);
  if (rc) return rc;
  if (!dev_out) return e->fail(IS3D_ERR_ARG, "null output buffer");
  rc = whole ? run_prepass(e, stream, 0, 1) : prepass_begin(e, stream, q0, q1, has_pred, 0, 1);
  if (rc) return rc;
  e->ws.lc.dev_out = dev_out;
  if (e->ws.lc.empty) HIPCHK(e, hipMemsetAsync(dev_out, 0, is3d_output_size(e) * sizeof(double), e->ws.lc.st));
  return IS3D_OK;
}

int enqueue_famod_b(is3d_engine* e) {
  const LaunchCtx& L = e->ws.lc;
  hipLaunchKernelGGL(k_famod_b, dim3((unsigned)std::max(1L, (L.p1 - L.p0 + 255) / 256)), dim3(256), 0, L.st, L.pa,
                     (const double*)e->ws.d_sol.get());
  HIPCHK(e, hipGetLastError());
  return IS3D_OK;
}

int read_counters(is3d_engine* e) {
  unsigned long long cnt[4] = {0, 0, 0, 0};
  HIPCHK(e, hipMemcpy(cnt, e->ws.d_cnt.get(), sizeof(cnt), hipMemcpyDeviceToHost));
  e->ws.st.breakdown = (long)cnt[0]; e->ws.st.pl_negative = (long)cnt[1]; e->ws.st.recon_fail = (long)cnt[2]; e->ws.st.iterations = (long)cnt[3];
  return IS3D_OK;
}

// Cell splits and slab geometry of one k_spectra plan over a launch window of nw cells.
struct IntegralPlan {
  SpectraPlan P;
  long ntask = 0, bx = 0, wgs = 0, nsplit = 0, cps = 0, sstride = 0, nsplit_fb = 0;
  // F_TS table chunks: spc splits per chunk, nchunk chunks; fold: each chunk's slabs are folded into one accumulator
  // slab as soon as the chunk is integrated (3+1D, several chunks), so the slabs take 1 + 2 spc output sizes of HBM
  // instead of nsplit (config 4: 947 -> 67 slabs, 47 -> 3.4 GB)
  long spc = 0, nchunk = 0, rw = 0, tabw = 0;
  bool fold = false;
  long slabs() const { return fold ? 1 + 2 * spc : nsplit + nsplit_fb; }
};

// F_TS chunking of plan I over nw cells: tables of the whole window up to phitab_one bytes in one chunk, larger ones in
// chunks of whole cell splits of about phitab_chunk bytes; both within half the device's free memory (plus the table
// buffers this engine already holds)
static void ts_chunking(is3d_engine* e, IntegralPlan& I) {
  const int npT = (int)e->in.pT.size();
  I.rw = phitab_row(e->in.p.df_mode, I.P.KJ, I.P.by != 0);
  // doubles per cell of a chunk's table buffer: k_phitab's rows of every pT and, behind them, k_ytab's y-term rows
  I.tabw = (long)npT * I.rw + (long)I.P.nq * kYRowTS;
  const long per_split = I.cps * I.tabw;
  const long whole = per_split * I.nsplit * 8;          // bytes of the whole surface's rows
  long one = e->ws.phitab_one, chunk = e->ws.phitab_chunk;
  {
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess && tot > 0) {
      const long avail = (long)(fr / 2) + (e->ws.d_phtab.capacity() + e->ws.d_phtab2.capacity()) * (long)sizeof(double);
      one = std::min(one, avail);
      chunk = std::max(8L * per_split, std::min(chunk, avail / 2));
    }
  }
  const long budget = whole <= one ? whole : chunk;
  I.spc = std::max(1L, std::min(I.nsplit, budget / 8 / per_split));
  I.nchunk = (I.nsplit + I.spc - 1) / I.spc;
  I.fold = I.nchunk > 1 && e->in.p.dimension == 3 && I.nsplit_fb == 0;
}

static int integral_plan(is3d_engine* e, const SpectraPlan& P, long nw, IntegralPlan& I, long cap_slabs = 0) {
  const int dim = e->in.p.dimension, mode = e->in.p.df_mode;
  const int npT = (int)e->in.pT.size();
  const int nk = (dim == 3) ? (int)e->in.y.size() : 1, nl = (dim == 3) ? 1 : (int)e->in.eta.size();
  const int KJ = P.KJ, njb = P.njb;
  if (!spectra_kj_supported(KJ)) return e->fail(IS3D_ERR_ARG, "internal: no k_spectra instantiation for this phi block");
  if (P.shmem > 160 * 1024) return e->fail(IS3D_ERR_ARG, "momentum grid too large for the LDS tile (phi table)");
  const int nc = e->tbl.nlane;     // lane species: one per lane class (the reduction writes the members)
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
  const long by_l2 = ((long)NREC * 8 * nw + e->ws.split_bytes - 1) / e->ws.split_bytes;
  const long sstride = (long)npT * bx * KJ * kBlock;
  // slab memory: the tuning cap, and at most half of the device's total memory -- deterministic inputs only, since
  // the split count sets the summation order (free memory changes from launch to launch with other engines, ranks
  // and torch's cache; it decides only the F_TS chunking and folding below, which leave the bits unchanged)
  long slab_budget = e->ws.slab_bytes;
  {
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess && tot > 0) slab_budget = std::min(slab_budget, (long)(tot / 2));
  }
  long max_slabs = std::max(8L, std::min(e->ws.max_splits, (slab_budget / 8) / std::max(1L, sstride)));
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
  const int mode = e->in.p.df_mode, dim = e->in.p.dimension;
  const int npT = (int)e->in.pT.size(), nphi = (int)e->in.phi.size();
  const int ny_out = (dim == 3) ? (int)e->in.y.size() : 1;
  const int nk = ny_out, nl = (dim == 3) ? 1 : (int)e->in.eta.size();
  const int KJ = P.KJ, njb = P.njb, nc = e->tbl.nlane;
  const long nsplit = I.nsplit, cps = I.cps, wgs = I.wgs;
  if (mode >= PTM) {
    if (!e->ws.d_fb.reserve(nw + 1 + kFbBlocks)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(fallback list) failed");
    enqueue_fbscan(rec_w, nw, e->ws.d_fb.get(), st);
    HIPCHK(e, hipGetLastError());
  }
  SpecArgs sa{};
  sa.err = e->ws.d_err.get();
  sa.rec = rec_w; sa.n = nw; sa.renorm = e->ws.d_renorm.get(); sa.rcls = e->tbl.d_crcls; sa.nrcls = e->tbl.nrcls; sa.slab = e->ws.d_slab.get();
  sa.outsize = is3d_output_size(e);
  sa.smass = e->tbl.d_cmass; sa.ssign = e->tbl.d_csign; sa.sbaryon = e->tbl.d_cbaryon; sa.sorig = e->tbl.d_sorig;
  sa.csg = e->tbl.d_csg;
  sa.pT = e->tbl.d_pT; sa.cphi = e->tbl.d_cphi; sa.sphi = e->tbl.d_sphi; sa.yv = e->tbl.d_y; sa.etav = e->tbl.d_eta; sa.etaw = e->tbl.d_etaw;
  sa.npart = nc; sa.npT = npT; sa.nphi = nphi; sa.ny_out = ny_out; sa.nk = nk; sa.nl = nl; sa.nq = nk * nl; sa.njb = njb;
  sa.nqmax = P.nqmax;
  sa.ntask = I.ntask; sa.cells_per_split = cps; sa.nbx = (int)I.bx; sa.nsplit = (int)nsplit; sa.sstride = I.sstride;
  sa.npw = P.npw;
  sa.regulate = e->in.p.regulate_deltaf; sa.outflow = e->in.p.outflow; sa.dim = dim; sa.op = 1;
  sa.gate = gate; sa.gate_want = want;
  const size_t shmem = P.shmem;
  const int tb = P.tb | P.ly | P.t8 | P.mp | P.ts | P.by;
  const int kflags = (e->in.p.regulate_deltaf ? F_REG : 0) | (e->in.p.outflow ? F_OUT : 0) | tb;
  if (P.ts) {
    // F_TS: k_phitab writes the per-(cell, pT, phi) rows of a chunk of whole cell splits (at most
    // phitab_chunk bytes, is3d_set_tuning), then k_spectra integrates that chunk's splits; one chunk at config 2
    // (3.7 GB).  Several chunks (config 4: 61 GB of rows) alternate between the launch stream and a side stream
    // with a table buffer each, so the next chunk's k_phitab and the first workgroups of its k_spectra fill the
    // CUs the previous launch's last workgroups leave idle (config 4: 11 chunks ran 2811 ms back to back, one
    // 61 GB chunk 2739 ms)
    const long rw = I.rw, spc = I.spc, nchunk = I.nchunk;
    const long phn = spc * cps;
    e->ws.last_nchunk = nchunk;
    if (!e->ws.d_phtab.reserve(phn * I.tabw)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(phi tables) failed");
    if (nchunk > 1) {
      if (!e->ws.d_phtab2.reserve(phn * I.tabw)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(phi tables) failed");
      if (!e->ws.side) HIPCHK(e, e->ws.side.create(hipStreamNonBlocking));
      if (!e->ws.fork) HIPCHK(e, e->ws.fork.create(hipEventDisableTiming));
      if (!e->ws.join) HIPCHK(e, e->ws.join.create(hipEventDisableTiming));
      HIPCHK(e, hipEventRecord(e->ws.fork.get(), st));
      HIPCHK(e, hipStreamWaitEvent(e->ws.side.get(), e->ws.fork.get(), 0));
    }
    if (I.fold) {
      if (!e->ws.fold_st) HIPCHK(e, e->ws.fold_st.create(hipStreamNonBlocking));
      for (auto* v : {&e->ws.ev_spec[0], &e->ws.ev_spec[1], &e->ws.ev_fold[0], &e->ws.ev_fold[1], &e->ws.fold_join})
        if (!*v) HIPCHK(e, v->create(hipEventDisableTiming));
      HIPCHK(e, hipStreamWaitEvent(e->ws.fold_st.get(), e->ws.fork.get(), 0));
    }
    // folded: slab 0 is the accumulator, chunk ic's splits go to buffer ic & 1 (slabs 1 + (ic & 1) spc ...)
    const int fgrid = (int)std::min(4096L, std::max(1L, (I.sstride + 255) / 256));
    for (long ic = 0; ic < nchunk; ic++) {
      const long s0 = ic * spc, ns = std::min(spc, nsplit - s0);
      const long c0 = s0 * cps, ncc = std::min(nw, (s0 + ns) * cps) - c0;
      hipStream_t cs = (ic & 1) ? e->ws.side.get() : st;
      double* tab = (ic & 1) ? e->ws.d_phtab2.get() : e->ws.d_phtab.get();
      PhiTabArgs ta{};
      ta.rec = rec_w; ta.c0 = c0; ta.nc = ncc; ta.pT = e->tbl.d_pT; ta.cphi = e->tbl.d_cphi; ta.sphi = e->tbl.d_sphi;
      ta.npT = npT; ta.nphi = nphi; ta.nphp = KJ; ta.tab = tab; ta.phn = phn; ta.by = P.by != 0;
      ta.gate = gate; ta.gate_want = want;
      // the chunk's y-term rows (k_ytab), behind its phi rows in the same buffer: k_spectra finds them at
      // phtab + npT phn rw
      YTabArgs ya{};
      ya.rec = rec_w; ya.c0 = c0; ya.nc = ncc; ya.yv = e->tbl.d_y; ya.etav = e->tbl.d_eta; ya.etaw = e->tbl.d_etaw;
      ya.nk = nk; ya.nl = nl; ya.dim = dim; ya.op = sa.op; ya.tab = tab + phn * npT * rw;
      ya.gate = gate; ya.gate_want = want;
      SpecArgs sc = sa;
      sc.split0 = (int)s0; sc.nsplit = (int)ns; sc.phtab = tab; sc.phn = phn; sc.phc0 = c0; sc.phrow = (int)rw;
      double* buf = e->ws.d_slab.get() + (1 + (ic & 1) * spc) * I.sstride;
      if (I.fold) { sc.slab = buf; sc.slab0 = (int)s0; }
      const dim3 grid((unsigned)(wgs * ns));
      if (mode == GRAD) { launch_phitab<GRAD>(cs, ta); launch_ytab<GRAD>(cs, ya); }
      else { launch_phitab<CE>(cs, ta); launch_ytab<CE>(cs, ya); }
      // a folded chunk reusing slab buffer ic & 1 waits for the fold of chunk ic - 2, which emptied it
      if (I.fold && ic >= 2) HIPCHK(e, hipStreamWaitEvent(cs, e->ws.ev_fold[ic & 1].get(), 0));
      if (mode == GRAD) launch_spectra<GRAD>(grid, shmem, cs, sc, kflags, KJ);
      else launch_spectra<CE>(grid, shmem, cs, sc, kflags, KJ);
      HIPCHK(e, hipGetLastError());
      if (I.fold) {
        HIPCHK(e, hipEventRecord(e->ws.ev_spec[ic & 1].get(), cs));
        HIPCHK(e, hipStreamWaitEvent(e->ws.fold_st.get(), e->ws.ev_spec[ic & 1].get(), 0));
        hipLaunchKernelGGL(k_fold, dim3((unsigned)fgrid), dim3(256), 0, e->ws.fold_st.get(), e->ws.d_slab.get(), (const double*)buf,
                           I.sstride, (int)ns, ic == 0 ? 1 : 0, gate, want);
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, hipEventRecord(e->ws.ev_fold[ic & 1].get(), e->ws.fold_st.get()));
      }
    }
    if (nchunk > 1) {
      HIPCHK(e, hipEventRecord(e->ws.join.get(), e->ws.side.get()));
      HIPCHK(e, hipStreamWaitEvent(st, e->ws.join.get(), 0));
    }
    if (I.fold) {
      HIPCHK(e, hipEventRecord(e->ws.fold_join.get(), e->ws.fold_st.get()));
      HIPCHK(e, hipStreamWaitEvent(st, e->ws.fold_join.get(), 0));
    }
  } else {
    const dim3 grid((unsigned)(wgs * nsplit));
    with_mode(mode, [&](auto M) { launch_spectra<decltype(M)::value>(grid, shmem, st, sa, kflags, KJ); });
  }
  HIPCHK(e, hipGetLastError());
  if (mode >= PTM) {
    SpecArgs fa = sa;
    fa.slab = e->ws.d_slab.get() + nsplit * I.sstride; fa.nsplit = (int)I.nsplit_fb; fa.cells_per_split = 0;
    fa.fbcells = e->ws.d_fb.get() + 1; fa.fbcount = e->ws.d_fb.get();
    const int fflags = (e->in.p.regulate_deltaf ? F_REG : 0) | (e->in.p.outflow ? F_OUT : 0) | F_FB;
    const dim3 gfb((unsigned)(I.bx * npT * I.nsplit_fb));
    with_mode<PTM>(mode, [&](auto M) { launch_spectra<decltype(M)::value>(gfb, P.shmem_fb, st, fa, fflags, KJ); });
    HIPCHK(e, hipGetLastError());
  }
  return IS3D_OK;
}

// sum of one plan's slabs into the reference-layout output (k_reduce / k_reduce_wave), gated as enqueue_spectra
static int enqueue_reduce(is3d_engine* e, const IntegralPlan& I, double* dev_out, hipStream_t st,
                          const unsigned long long* gate, int want) {
  const int dim = e->in.p.dimension;
  const int npT = (int)e->in.pT.size(), nphi = (int)e->in.phi.size();
  const int ny_out = (dim == 3) ? (int)e->in.y.size() : 1;
  const int nk = ny_out, nl = (dim == 3) ? 1 : (int)e->in.eta.size();
  const int nc = e->tbl.nlane;
  ReduceArgs ra{};
  ra.slab = e->ws.d_slab.get(); ra.sstride = I.sstride; ra.nsplit = I.fold ? 1 : (int)(I.nsplit + I.nsplit_fb);
  ra.nbx = (int)I.bx; ra.npart = nc; ra.npT = npT; ra.nphi = nphi; ra.nk = nk; ra.nl = nl; ra.ny_out = ny_out; ra.kj = I.P.KJ;
  ra.ntask = I.ntask;
  ra.sorig = e->tbl.d_sorig; ra.degen_orig = e->tbl.d_degen_orig; ra.prefactor = std::pow(2.0 * M_PI * kHbarC, -3);
  ra.cmem_off = e->tbl.d_cmem_off; ra.cmem = e->tbl.d_cmem;
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
  LaunchCtx& L = e->ws.lc;
  hipStream_t st = L.st;
  double* dev_out = L.dev_out;
  HIPCHK(e, hipSetDevice(e->device));
  if (L.empty) {
    HIPCHK(e, hipEventRecord(e->ws.ev[1].get(), st));
    HIPCHK(e, hipEventRecord(e->ws.ev[2].get(), st));
    HIPCHK(e, hipEventRecord(e->ws.ev[3].get(), st));
    e->ws.launched = true;
    return IS3D_OK;
  }
  const long n = e->sf.ncell;
  const int mode = e->in.p.df_mode;
  const long wlo = L.wlo, nw = L.nw;
  int rc = mode == PTMA ? enqueue_famod_b(e) : mode == PTM ? enqueue_renorm(e, L.pa.k, wlo, nw, n, st) : IS3D_OK;
  if (rc) return rc;
  HIPCHK(e, hipEventRecord(e->ws.ev[1].get(), st));
  // the integral and the reduction see the window only: records from wlo on, nw cells
  const double* rec_w = e->ws.d_rec.get() + wlo * (long)NREC;
  // --- main integral
  // Grad / RTA-CE F_TS: a surface with cells whose lanes may leave the fast path (k_prep counts them in cnt[4]; none
  // in any tabulated delta-f range) needs the kernels that carry the slow loop, which the F_TS ones do not.  The
  // choice is made on the device: both plans are enqueued, each gated on cnt[4] (gate_closed: the other plan's
  // workgroups return at once, ~10 us), so is3d_launch never waits for the prepass (no host round trip)
  const SpectraPlan P = spectra_plan(e, true);
  e->ws.last_nchunk = 0;
  IntegralPlan I{}, J{};
  rc = integral_plan(e, P, nw, I);
  if (rc) return rc;
  e->ws.last_nsplit = I.nsplit;
  e->ws.last_nslab = I.slabs();
  const bool gated = mode <= CE && P.ts;
  if (gated) {
    // the fallback plan shares the slab memory: a folded main plan caps its splits at the same footprint
    rc = integral_plan(e, spectra_plan(e, false), nw, J, I.fold ? I.slabs() : 0);
    if (rc) return rc;
  }
  const long slab_need = std::max(I.slabs() * I.sstride, gated ? J.slabs() * J.sstride : 0L);
  if (!e->ws.d_slab.reserve(slab_need)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(slabs) failed");
  const unsigned long long* gate = gated ? e->ws.d_cnt.get() + 4 : nullptr;
  rc = enqueue_spectra(e, I, rec_w, nw, st, gate, 0);
  if (!rc && gated) rc = enqueue_spectra(e, J, rec_w, nw, st, gate, 1);
  if (rc) return rc;
  HIPCHK(e, hipEventRecord(e->ws.ev[2].get(), st));
  rc = enqueue_reduce(e, I, dev_out, st, gate, 0);
  if (!rc && gated) rc = enqueue_reduce(e, J, dev_out, st, gate, 1);
  if (rc) return rc;
  HIPCHK(e, hipEventRecord(e->ws.ev[3].get(), st));
  e->ws.launched = true;
  return IS3D_OK;
}

extern "C" int is3d_launch(is3d_engine* e, double* dev_out, void* stream) {
  if (e && e->grp) return is3d::group_launch(e->grp, dev_out, stream);
  if (!e) return IS3D_ERR_ARG;
  if (e->sf.chain_q1 >= 0)
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
int is3d_internal_chain_npass(const is3d_engine* e) { return e->ws.lc.chained && !e->ws.lc.empty ? e->ws.lc.ca.npass : 0; }
// boundary slot k (0, 1: pass parity, 2: final) of this engine's chain range: in (from the previous shard) or out
double* is3d_internal_chain_bnd(is3d_engine* e, int out, int slot) {
  if (!e->ws.lc.chained || e->ws.lc.empty) return nullptr;
  const long bw = 4 * e->ws.lc.ca.C + 1;
  return (out ? e->ws.lc.ca.bout : e->ws.lc.ca.bin) + slot * bw;
}
long is3d_internal_chain_bnd_bytes(const is3d_engine* e) { return (4 * e->ws.lc.ca.C + 1) * (long)sizeof(double); }

// ---- staged launch for PTMA warm-start chains split over processes (include/is3d_amd.h) ----------------------------
extern "C" int is3d_set_chain_range(is3d_engine* e, long q0, long q1) {
  if (!e) return IS3D_ERR_ARG;
  if (e->grp) return is3d::group_fail(e->grp, IS3D_ERR_UNSUPPORTED, "a device-list engine splits its chains itself");
  if (q0 < 0 || q1 < 0) { e->sf.chain_q0 = e->sf.chain_q1 = -1; e->sf.win_lo = e->sf.win_hi = -1; return IS3D_OK; }
  if (!e->in.have_params || e->in.p.df_mode != PTMA || e->in.p.famod_chains <= 0)
    return e->fail(IS3D_ERR_STATE, "a chain range needs PTMA (df_mode 5) with famod_chains > 0 set first");
  const long n = e->sf.ncell, C = std::max(1L, std::min<long>(e->in.p.famod_chains, std::max(n, 1L))), P = (n + C - 1) / C;
  if (q0 > q1 || q1 > P) return e->fail(IS3D_ERR_ARG, "chain range outside the surface's chain positions");
  e->sf.win_lo = std::min(n, q0 * C);
  e->sf.win_hi = std::min(n, q1 * C);
  e->sf.chain_q0 = q0; e->sf.chain_q1 = q1;
  return IS3D_OK;
}

extern "C" int is3d_launch_begin(is3d_engine* e, double* dev_out, void* stream) {
  if (!e) return IS3D_ERR_ARG;
  if (e->grp) return is3d::group_fail(e->grp, IS3D_ERR_UNSUPPORTED, "the staged launch runs on one-device engines");
  if (e->sf.chain_q1 >= 0 && (e->in.p.df_mode != PTMA || e->in.p.famod_chains <= 0))
    return e->fail(IS3D_ERR_STATE, "a chain range needs PTMA with famod_chains > 0 (params changed since)");
  const bool range = e->sf.chain_q1 >= 0;
  if (range) {
    // the integration window follows the chain positions under the current famod_chains C (set_params may have
    // changed C since is3d_set_chain_range): cells [q0 C, q1 C), so the ranks' windows still tile the surface
    const long n = e->sf.ncell, C = std::max(1L, std::min<long>(e->in.p.famod_chains, std::max(n, 1L))), P = (n + C - 1) / C;
    if (e->sf.chain_q1 > P) return e->fail(IS3D_ERR_ARG, "chain range outside the surface's chain positions (famod_chains changed)");
    e->sf.win_lo = std::min(n, e->sf.chain_q0 * C);
    e->sf.win_hi = std::min(n, e->sf.chain_q1 * C);
  }
  return launch_begin(e, dev_out, stream, range ? e->sf.chain_q0 : 0, range ? e->sf.chain_q1 : -1, range && e->sf.chain_q0 > 0);
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
  return (e && !e->grp && e->ws.lc.chained && !e->ws.lc.empty) ? 4 * e->ws.lc.ca.C + 1 : 0;
}
// boundary slot `slot` (0, 1: pass parity, 2: the finisher's) out of this range into dev_buf / from dev_buf into this
// range's incoming slot, on the launch stream (hipMemcpyDefault: a host buffer works too, read after a stream sync)
extern "C" int is3d_chain_boundary_get(is3d_engine* e, int slot, double* dev_buf) {
  if (!e || e->grp || !dev_buf || slot < 0 || slot >= kBndSlots) return e ? e->fail(IS3D_ERR_ARG, "bad chain boundary slot") : IS3D_ERR_ARG;
  const long nb = is3d_chain_boundary_size(e);
  if (nb == 0) return e->fail(IS3D_ERR_STATE, "no chains in the launch in flight");
  HIPCHK(e, hipSetDevice(e->device));
  HIPCHK(e, hipMemcpyAsync(dev_buf, is3d_internal_chain_bnd(e, 1, slot), nb * sizeof(double), hipMemcpyDefault, e->ws.lc.st));
  return IS3D_OK;
}
extern "C" int is3d_chain_boundary_put(is3d_engine* e, int slot, const double* dev_buf) {
  if (!e || e->grp || !dev_buf || slot < 0 || slot >= kBndSlots) return e ? e->fail(IS3D_ERR_ARG, "bad chain boundary slot") : IS3D_ERR_ARG;
  const long nb = is3d_chain_boundary_size(e);
  if (nb == 0) return e->fail(IS3D_ERR_STATE, "no chains in the launch in flight");
  HIPCHK(e, hipSetDevice(e->device));
  HIPCHK(e, hipMemcpyAsync(is3d_internal_chain_bnd(e, 0, slot), dev_buf, nb * sizeof(double), hipMemcpyDefault, e->ws.lc.st));
  return IS3D_OK;
}

extern "C" int is3d_cell_costs(is3d_engine* e, double* cost) {
  if (e && e->grp) return is3d::group_fail(e->grp, IS3D_ERR_UNSUPPORTED, "is3d_cell_costs: call it on a one-device engine");
  if (!e || !cost) return IS3D_ERR_ARG;
  int rc = finalize_tables(e);
  if (rc) return rc;
  const long n = e->sf.ncell;
  if (n <= 0) return IS3D_OK;
  HIPCHK(e, hipSetDevice(e->device));
  const int mode = e->in.p.df_mode;
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
  if (!e->ws.launched && !e->fd.launched) return e->fail(IS3D_ERR_STATE, "nothing launched");
  HIPCHK(e, hipSetDevice(e->device));
  if (e->fd.launched) {       // is3d_launch_feeddown: no device error word, its own two events
    e->fd.launched = false;
    HIPCHK(e, hipEventSynchronize(e->fd.ev[1].get()));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e->fd.ev[0].get(), e->fd.ev[1].get()) == hipSuccess) e->fd.stats.ms_total = ms;
    if (!e->ws.launched) return IS3D_OK;
  }
  HIPCHK(e, hipEventSynchronize(e->ws.ev[3].get()));
  e->ws.launched = false;
  int derr = 0;
  HIPCHK(e, hipMemcpy(&derr, e->ws.d_err.get(), sizeof(int), hipMemcpyDeviceToHost));
  const int rc = read_counters(e);
  if (rc) return rc;
  read_timings(e);
  return df_error(e, derr, "Error: choose df_mode = (1,2,3,4,5)");
}

extern "C" int is3d_calculate_spectra(is3d_engine* e, double* dN_out) {
  if (e && e->grp) return is3d::group_calculate_spectra(e->grp, dN_out);
  if (!e || !dN_out) return e ? e->fail(IS3D_ERR_ARG, "null output") : IS3D_ERR_ARG;
  const int rc = finalize_tables(e);
  if (rc) return rc;
  return calculate(e, is3d_output_size(e), dN_out, [&](double* d) { return is3d_launch(e, d, nullptr); });
}

extern "C" int is3d_get_stats(const is3d_engine* e, is3d_stats* out) {
  if (e && e->grp) return out ? is3d::group_get_stats(e->grp, out) : IS3D_ERR_ARG;
  if (!e || !out) return IS3D_ERR_ARG;
  *out = e->ws.st;
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
  hipLaunchKernelGGL(k_df_eval, dim3(1), dim3(1), 0, 0, e->tbl.dtb, T, muB, E, P, bulkPi, d, (int*)(d + 15));
  HIPCHK(e, hipDeviceSynchronize());
  int derr = 0;
  HIPCHK(e, hipMemcpy(out15, d, 15 * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(&derr, d + 15, sizeof(int), hipMemcpyDeviceToHost));
  return df_error(e, derr, "df coefficient error");
}

extern "C" int is3d_get_jonah_table(const is3d_engine* e, double* l2, double* z, double* bp, double* bpmax) {
  if (e && e->grp) return is3d::group_get_jonah_table(e->grp, l2, z, bp, bpmax);
  if (!e || e->tbl.jx.size() != 301) return IS3D_ERR_STATE;
  std::copy(e->tbl.jl2.begin(), e->tbl.jl2.end(), l2);
  std::copy(e->tbl.jz.begin(), e->tbl.jz.end(), z);
  std::copy(e->tbl.jx.begin(), e->tbl.jx.end(), bp);
  *bpmax = e->tbl.bp_max;
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
