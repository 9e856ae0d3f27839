// engine_dndx.hip -- operation = 0 of the engine (engine.h): the spacetime distributions dN/dX of every species and the
// per-cell yields behind them.  The yields are k_dndx (kernels.h, compiled per delta-f mode in spectra_tu.hip); this
// unit's own kernels are the bin keys and the bin sums (engine_dndx_kernels.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/is3d_amd.h"
#include "cf_math.h"
#include "kernels.h"
#include "group.h"
#include "engine.h"

using namespace is3d;
using namespace is3d::kern;

#include "engine_dndx_kernels.h"   // this unit's device code (k_stkeys, k_stbin)

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
  const long nsurf = e->sf.ncell;
  const int mode = e->in.p.df_mode, dim = e->in.p.dimension;
  const int np = (int)e->in.mass.size(), npT = (int)e->in.pT.size(), nphi = (int)e->in.phi.size();
  const int nk = (dim == 3) ? (int)e->in.y.size() : 1, nl = (dim == 3) ? 1 : (int)e->in.eta.size();
  const is3d_spacetime_bins& B = e->op0.bins;
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
    const int nc = e->tbl.nlane;   // lane species: the lane classes (k_stbin scales and writes the members)
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
    if (!e->op0.d_ycell.reserve((long)nc * n)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(cell yields) failed");
    da.rec = e->ws.d_rec.get() + wlo * (long)NREC; da.n = n; da.renorm = e->ws.d_renorm.get(); da.rcls = e->tbl.d_crcls; da.nrcls = e->tbl.nrcls; da.ycell = e->op0.d_ycell.get();
    da.smass = e->tbl.d_cmass; da.ssign = e->tbl.d_csign; da.sbaryon = e->tbl.d_cbaryon;
    da.pT = e->tbl.d_pT; da.pTw = e->tbl.d_pTw; da.cphi = e->tbl.d_cphi; da.sphi = e->tbl.d_sphi; da.phiw = e->tbl.d_phiw;
    da.yv = e->tbl.d_y; da.etav = e->tbl.d_eta; da.etaw = e->tbl.d_etaw;
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
    const int kflags = (e->in.p.regulate_deltaf ? F_REG : 0) | (e->in.p.outflow ? F_OUT : 0);
    with_mode(mode, [&](auto M) { launch_dndx<decltype(M)::value>(dim3((unsigned)nwg), shmem, st, da, kflags, KJ); });
    HIPCHK(e, hipGetLastError());
    if (mode >= PTM) {
      // the separable-fallback lanes of the cells k_fbwrite lists (breakdown, narrow rapidity windows) in their own
      // launch (kernels.h k_dndx F_FB), added to ycell; the list's length stays on the device, so the grid is sized
      // for the whole surface and the workgroups split whatever the list holds
      if (!e->ws.d_fb.reserve(n + 1 + kFbBlocks)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(fallback list) failed");
      enqueue_fbscan(da.rec, n, e->ws.d_fb.get(), st);
      DndxArgs fa = da;
      fa.fbcells = e->ws.d_fb.get() + 1; fa.fbcount = e->ws.d_fb.get();
      fa.nchunk = std::max(1L, std::min(da.nchunk, (4096L + da.nbx - 1) / da.nbx));
      const long nfw = (long)da.nbx * fa.nchunk;
      with_mode<PTM>(mode, [&](auto M) { launch_dndx<decltype(M)::value>(dim3((unsigned)nfw), shmem_fb, st, fa, kflags | F_FB, KJ); });
      HIPCHK(e, hipGetLastError());
    }
    e->op0.ycell_n = n;
  } else {
    e->op0.ycell_n = 0;
  }
  HIPCHK(e, hipEventRecord(e->ws.ev[2].get(), st));
  if (n > 0) {
    // --- bin keys on the device, CSR (thread slice, bin) -> cells on the host, sums on the device
    if (!e->op0.d_keys.reserve(3 * n)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(keys) failed");
    KeyArgs ka{};
    ka.tau = e->sf.d_surf + wlo; ka.x = e->sf.d_surf + nsurf + wlo; ka.y = e->sf.d_surf + 2 * nsurf + wlo; ka.n = n;
    ka.tau_min = B.tau_min; ka.tau_width = (B.tau_max - B.tau_min) / (double)B.tau_bins;
    ka.r_min = B.r_min; ka.r_width = (B.r_max - B.r_min) / (double)B.r_bins;
    ka.phip_width = 2.0 * M_PI / (double)B.phip_bins;
    ka.tau_bins = B.tau_bins; ka.r_bins = B.r_bins; ka.phip_bins = B.phip_bins; ka.keys = e->op0.d_keys.get();
    hipLaunchKernelGGL(k_stkeys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ka);
    HIPCHK(e, hipGetLastError());
    std::vector<int> keys((size_t)3 * n);
    HIPCHK(e, hipMemcpy(keys.data(), e->op0.d_keys.get(), keys.size() * sizeof(int), hipMemcpyDeviceToHost));
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
    if (!e->op0.d_perm.reserve((long)perm.size())) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(perm) failed");
    if (!e->op0.d_offs.reserve(nent + 1)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(offsets) failed");
    if (!e->op0.d_part.reserve((long)np * nent)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(bins) failed");
    HIPCHK(e, hipMemcpy(e->op0.d_perm.get(), perm.data(), perm.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(e->op0.d_offs.get(), offs.data(), offs.size() * sizeof(long), hipMemcpyHostToDevice));
    BinArgs ba{};
    ba.ycell = e->op0.d_ycell.get(); ba.n = n; ba.npart = np;
    ba.perm = e->op0.d_perm.get(); ba.offs = e->op0.d_offs.get(); ba.nent = nent;
    ba.sorig = e->tbl.d_sorig; ba.sdegen = e->tbl.d_sdegen; ba.prefactor = std::pow(2.0 * M_PI * kHbarC, -3);
    ba.scls = e->tbl.d_scls;
    ba.part = e->op0.d_part.get();
    const long nthr = nent * np;
    hipLaunchKernelGGL(k_stbin, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st, ba);
    HIPCHK(e, hipGetLastError());
  }
  HIPCHK(e, hipEventRecord(e->ws.ev[3].get(), st));
  HIPCHK(e, hipEventSynchronize(e->ws.ev[3].get()));
  int derr = 0;
  HIPCHK(e, hipMemcpy(&derr, e->ws.d_err.get(), sizeof(int), hipMemcpyDeviceToHost));
  if (n > 0) HIPCHK(e, hipMemcpy(part.data(), e->op0.d_part.get(), part.size() * sizeof(double), hipMemcpyDeviceToHost));
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
  if (!e->in.have_params) return e->fail(IS3D_ERR_STATE, "is3d_set_params not called");
  return IS3D_OK;
}

extern "C" int is3d_calculate_dN_dX(is3d_engine* e, double* dN_taudtaudy, double* dN_2pirdrdy, double* dN_dphidy) {
  if (e && e->grp) return is3d::group_calculate_dN_dX(e->grp, dN_taudtaudy, dN_2pirdrdy, dN_dphidy);
  if (!e) return IS3D_ERR_ARG;
  int rc = dndx_begin(e, dN_taudtaudy, dN_2pirdrdy, dN_dphidy);
  if (rc) return rc;
  if (e->in.p.df_mode == PTMA)
    return e->fail(IS3D_ERR_UNSUPPORTED, "calculate_spectra error: no spacetime distribution routine for famod yet "
                                         "(the per-cell decomposition of the PTMA spectra: call is3d_calculate_dN_dX_famod)");
  if (!e->in.have_weights) return e->fail(IS3D_ERR_STATE, "is3d_set_momentum_weights not called");
  if (!e->op0.have_bins) return e->fail(IS3D_ERR_STATE, "is3d_set_spacetime_bins not called");
  rc = finalize_tables(e);
  if (rc) return rc;
  HIPCHK(e, hipSetDevice(e->device));
  hipStream_t st = nullptr;
  const long n = e->sf.ncell;
  rc = begin_stats(e, n, st);
  if (rc) return rc;
  if (n > 0) {
    if (!e->ws.d_rec.reserve((long)NREC * n)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(records) failed");
    if (!e->ws.d_aux.reserve(9L * n)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(aux) failed");
    PrepArgs pa = prep_args(e, e->ws.d_rec.get(), e->ws.d_aux.get(), 0, n, e->ws.d_err.get(), e->ws.d_cnt.get());
    pa.k.operation = 0;
    rc = enqueue_prep(e, pa, st);
    if (!rc && e->in.p.df_mode == PTM) rc = enqueue_renorm(e, pa.k, 0, n, n, st);
    if (rc) return rc;
  }
  HIPCHK(e, hipEventRecord(e->ws.ev[1].get(), st));
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
  if (e->in.p.df_mode != PTMA)
    return e->fail(IS3D_ERR_UNSUPPORTED, "is3d_calculate_dN_dX_famod: needs df_mode 5 (df_mode 1-4: is3d_calculate_dN_dX)");
  if (e->sf.chain_q1 >= 0)
    return e->fail(IS3D_ERR_STATE, "is3d_calculate_dN_dX_famod: a chain range is set (is3d_set_chain_range); this entry solves the whole chain");
  if (!e->in.have_weights) return e->fail(IS3D_ERR_STATE, "is3d_set_momentum_weights not called");
  if (!e->op0.have_bins) return e->fail(IS3D_ERR_STATE, "is3d_set_spacetime_bins not called");
  rc = finalize_tables(e);
  if (rc) return rc;
  rc = run_prepass(e, nullptr, 0, 0);
  const LaunchCtx& L = e->ws.lc;
  if (!rc && !L.empty) rc = enqueue_famod_b(e);
  if (rc) return rc;
  HIPCHK(e, hipEventRecord(e->ws.ev[1].get(), L.st));
  rc = dndx_finish(e, L.wlo, L.nw, "Error: choose df_mode = (1,2,3,4,5)", dN_taudtaudy, dN_2pirdrdy, dN_dphidy);
  return rc ? rc : read_counters(e);     // dndx_finish has waited for the stream
}

extern "C" int is3d_get_cell_yields(const is3d_engine* e, double* dN_dy_cell) {
  if (e && e->grp) return is3d::group_get_cell_yields(e->grp, dN_dy_cell);
  if (!e || !dN_dy_cell) return IS3D_ERR_ARG;
  if (e->op0.ycell_n < 0) return IS3D_ERR_STATE;
  const long n = e->op0.ycell_n;
  const int np = (int)e->in.mass.size();
  if (n == 0) return IS3D_OK;
  std::vector<double> y((size_t)e->tbl.nlane * n);
  if (hipSetDevice(e->device) != hipSuccess) return IS3D_ERR_DEVICE;
  if (hipMemcpy(y.data(), e->op0.d_ycell.get(), y.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return IS3D_ERR_DEVICE;
  const double pref = std::pow(2.0 * M_PI * kHbarC, -3);
  for (int s = 0; s < np; s++) {
    const int so = e->in.order[s];
    for (long c = 0; c < n; c++) dN_dy_cell[(size_t)so * n + c] = pref * e->in.degen[so] * y[(size_t)e->tbl.scls[s] * n + c];
  }
  return IS3D_OK;
}
