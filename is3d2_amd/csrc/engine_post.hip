// engine_post.hip -- what the engine (engine.h) does to or beside the continuous spectra: spin polarization from thermal
// vorticity, the resonance-decay feed-down and the delta-f coefficient generator.  Host side only: the kernels are in
// polzn.hip, decay.hip and dfgen.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/is3d_amd.h"
#include "group.h"
#include "engine.h"
#include "dfgen.h"
#include "dfgen_math.h"

using namespace is3d;

// ------------------------------------------------------------------------------------------
// spin polarization from thermal vorticity (mode 5; Polarization.cpp:25-263, kernels in polzn.hip)
// ------------------------------------------------------------------------------------------
extern "C" int is3d_set_vorticity(is3d_engine* e, long n, const is3d_vorticity* w) {
  if (e && e->grp) return is3d::group_set_vorticity(e->grp, n, w);
  if (!e) return IS3D_ERR_ARG;
  if (!e->sf.have_surf) return e->fail(IS3D_ERR_STATE, "is3d_set_vorticity: set the surface first");
  if (!w || n != e->sf.ncell) return e->fail(IS3D_ERR_ARG, "is3d_set_vorticity: the vorticity must have one entry per surface cell");
  const double* f[6] = {w->wtx, w->wty, w->wtn, w->wxy, w->wxn, w->wyn};
  for (int k = 0; k < 6; k++)
    if (!f[k] && n > 0) return e->fail(IS3D_ERR_ARG, "is3d_set_vorticity: vorticity component missing");
  HIPCHK(e, hipSetDevice(e->device));
  if (!e->pol.d_vort.reserve(6L * n)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(vorticity) failed");
  for (int k = 0; k < 6 && n > 0; k++)
    HIPCHK(e, hipMemcpy(e->pol.d_vort.get() + (size_t)k * n, f[k], n * sizeof(double), hipMemcpyHostToDevice));
  e->pol.have_vort = true;
  return IS3D_OK;
}

extern "C" long is3d_polarization_size(const is3d_engine* e) {
  const long n = is3d_output_size(e);
  return n < 0 ? n : 5 * n;
}

extern "C" int is3d_launch_polarization(is3d_engine* e, double T_avg, double* dev_out, void* stream) {
  if (e && e->grp) return is3d::group_launch_polarization(e->grp, T_avg, dev_out, stream);
  if (!e) return IS3D_ERR_ARG;
  if (!e->in.have_params || !e->in.have_species || !e->in.have_grid)
    return e->fail(IS3D_ERR_STATE, "polarization: params, species and momentum grid must be set");
  if (!e->sf.have_surf) return e->fail(IS3D_ERR_STATE, "polarization: no surface set");
  if (!e->pol.have_vort) return e->fail(IS3D_ERR_STATE, "polarization: no thermal vorticity set for this surface (is3d_set_vorticity)");
  if (!(T_avg > 0.0)) return e->fail(IS3D_ERR_ARG, "polarization: T_avg must be positive");
  if (!dev_out) return e->fail(IS3D_ERR_ARG, "null output buffer");
  HIPCHK(e, hipSetDevice(e->device));
  if (e->is_stale(D_POLZN)) {
    const std::string msg = is3d::polzn::tables_build(e->pol.tables, e->in.p.dimension, e->in.classes, e->in.mass, e->in.sign, e->in.pT, e->in.phi,
                                                      e->in.y, e->in.eta, e->in.eta_w);
    if (!msg.empty()) return e->fail(IS3D_ERR_ARG, "polarization: " + msg);
    e->rebuilt(D_POLZN);
  }
  hipStream_t st = (hipStream_t)stream;
  const long n = e->sf.ncell;
  long wlo, whi;
  cell_window(e, wlo, whi);
  const long nw = whi - wlo;
  const int rc = begin_stats(e, nw, st);
  if (rc) return rc;
  HIPCHK(e, hipEventRecord(e->ws.ev[1].get(), st));     // no prepass: k_polzn reads the surface itself
  if (nw == 0) {
    HIPCHK(e, hipMemsetAsync(dev_out, 0, e->pol.tables.out_size() * sizeof(double), st));
    HIPCHK(e, hipEventRecord(e->ws.ev[2].get(), st));
  } else {
    const is3d::polzn::Plan P = is3d::polzn::make_plan(e->pol.tables, nw, e->ws.max_splits, e->ws.split_bytes, e->ws.slab_bytes);
    if (!P.ok) return e->fail(IS3D_ERR_ARG, "polarization: the phi / y / eta tables do not fit a workgroup's LDS tile");
    if (!e->ws.d_slab.reserve(P.nsplit * P.sstride)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(slabs) failed");
    e->ws.last_nchunk = 0;
    e->ws.last_nsplit = P.nsplit;
    e->ws.last_nslab = P.nsplit;
    HIPCHK(e, is3d::polzn::enqueue(e->pol.tables, P, e->sf.d_surf, e->pol.d_vort.get(), n, wlo, whi, T_avg, e->ws.d_slab.get(), dev_out, st, e->ws.ev[2].get()));
  }
  HIPCHK(e, hipEventRecord(e->ws.ev[3].get(), st));
  e->ws.launched = true;
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
// both entry points: the table in the four-slot form; keep_four: is3d_set_decays4's rule (open 4-body rows are kept)
static int set_decays(is3d_engine* e, const std::string& who, int n, const is3d_decay_channel4* ch, bool keep_four) {
  if (!e->in.have_species || !e->in.have_grid) return e->fail(IS3D_ERR_STATE, who + ": set the species and the momentum grid first");
  if (n < 0 || (n > 0 && !ch)) return e->fail(IS3D_ERR_ARG, who + ": bad channel table");
  e->input_changed(IN_DECAYS);     // no decays are set until this call has succeeded
  std::string msg = is3d::decay::check_grid((int)e->in.pT.size(), e->in.pT.data(), (int)e->in.phi.size(), e->in.phi.data(), 0, nullptr);
  if (!msg.empty()) return e->fail(IS3D_ERR_ARG, who + ": " + msg);
  e->fd.rule = is3d::decay::make_rule();
  msg = is3d::decay::build_plan(e->fd.plan, e->fd.rule, (int)e->in.mass.size(), e->in.mass.data(), n, ch, keep_four);
  if (!msg.empty()) return e->fail(IS3D_ERR_ARG, who + ": " + msg);
  e->fd.ch.assign(ch, ch + n);
  e->fd.stats = e->fd.plan.stats;
  e->rebuilt(D_DECAY_PLAN);
  return IS3D_OK;
}

extern "C" int is3d_set_decays(is3d_engine* e, int n, const is3d_decay_channel* ch) {
  if (e && e->grp) return is3d::group_set_decays(e->grp, n, ch);
  if (!e) return IS3D_ERR_ARG;
  std::vector<is3d_decay_channel4> wide;
  if (n > 0 && ch) {
    wide.resize((size_t)n);
    for (int i = 0; i < n; i++) wide[(size_t)i] = is3d::decay::widen(ch[i]);
  }
  return set_decays(e, "is3d_set_decays", n, ch ? wide.data() : nullptr, false);
}

extern "C" int is3d_set_decays4(is3d_engine* e, int n, const is3d_decay_channel4* ch) {
  if (e && e->grp) return is3d::group_set_decays4(e->grp, n, ch);
  if (!e) return IS3D_ERR_ARG;
  return set_decays(e, "is3d_set_decays4", n, ch, true);
}

extern "C" int is3d_get_decay_stats(const is3d_engine* e, is3d_decay_stats* out) {
  if (e && e->grp) return out ? is3d::group_get_decay_stats(e->grp, out) : IS3D_ERR_ARG;
  if (!e || !out) return IS3D_ERR_ARG;
  if (!e->have_decays()) return IS3D_ERR_STATE;
  *out = e->fd.stats;
  return IS3D_OK;
}

extern "C" int is3d_launch_feeddown(is3d_engine* e, double* dev_inout, void* stream) {
  if (e && e->grp) return is3d::group_launch_feeddown(e->grp, dev_inout, stream);
  if (!e) return IS3D_ERR_ARG;
  if (!e->in.have_params || !e->in.have_species || !e->in.have_grid)
    return e->fail(IS3D_ERR_STATE, "feed-down: params, species and momentum grid must be set");
  if (!e->have_decays()) return e->fail(IS3D_ERR_STATE, "feed-down: no decay channels set (is3d_set_decays)");
  if (!dev_inout) return e->fail(IS3D_ERR_ARG, "null spectra buffer");
  HIPCHK(e, hipSetDevice(e->device));
  const int ny = e->in.p.dimension == 3 ? (int)e->in.y.size() : 1;
  if (e->is_stale(D_DECAY_PACK)) {
    if (ny < 1) return e->fail(IS3D_ERR_ARG, "feed-down: empty y table");
    const std::string msg = is3d::decay::check_grid((int)e->in.pT.size(), e->in.pT.data(), (int)e->in.phi.size(), e->in.phi.data(), ny, e->in.y.data());
    if (!msg.empty()) return e->fail(IS3D_ERR_ARG, "feed-down: " + msg);
    e->fd.pack = is3d::decay::pack(e->fd.plan, e->fd.rule, e->in.pT, e->in.phi, ny, e->in.y);
    const is3d::decay::Packed& K = e->fd.pack;
    if (K.nb < 1 || K.lds > 64 * 1024) return e->fail(IS3D_ERR_ARG, "feed-down: the phi table does not fit a workgroup's LDS");
    if (!e->fd.d_d.reserve((long)K.d.size()) || !e->fd.d_i.reserve((long)K.i.size()))
      return e->fail(IS3D_ERR_DEVICE, "hipMalloc(decay tables) failed");
    HIPCHK(e, hipMemcpy(e->fd.d_d.get(), K.d.data(), K.d.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(e->fd.d_i.get(), K.i.data(), K.i.size() * sizeof(int), hipMemcpyHostToDevice));
    e->rebuilt(D_DECAY_PACK);
  }
  const long per = (long)e->in.pT.size() * ny;
  for (int l = 0; l < e->fd.plan.levels(); l++)
    if ((long)(e->fd.plan.lvl_r0[l + 1] - e->fd.plan.lvl_r0[l]) * per > 0x7fffffffL)
      return e->fail(IS3D_ERR_ARG, "feed-down: a level has more than 2^31 workgroups");
  if (!e->fd.d_log.reserve(is3d_output_size(e))) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(decay logs) failed");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(e, hipEventRecord(e->fd.ev[0].get(), st));
  HIPCHK(e, is3d::decay::enqueue(e->fd.plan, e->fd.pack, e->fd.d_d.get(), e->fd.d_i.get(), dev_inout, e->fd.d_log.get(), st));
  HIPCHK(e, hipEventRecord(e->fd.ev[1].get(), st));
  e->fd.launched = true;
  return IS3D_OK;
}

extern "C" int is3d_decay_feeddown(is3d_engine* e, double* dN) {
  if (e && e->grp) return is3d::group_decay_feeddown(e->grp, dN);
  if (!e || !dN) return e ? e->fail(IS3D_ERR_ARG, "null spectra array") : IS3D_ERR_ARG;
  const long n = is3d_output_size(e);
  if (n < 0) return e->fail(IS3D_ERR_STATE, "feed-down: params, species and momentum grid must be set");
  if (!e->have_decays()) return e->fail(IS3D_ERR_STATE, "feed-down: no decay channels set (is3d_set_decays)");
  HIPCHK(e, hipSetDevice(e->device));
  if (!e->fd.d_io.reserve(n)) return e->fail(IS3D_ERR_DEVICE, "hipMalloc(spectra) failed");
  HIPCHK(e, hipMemcpy(e->fd.d_io.get(), dN, n * sizeof(double), hipMemcpyHostToDevice));
  int rc = is3d_launch_feeddown(e, e->fd.d_io.get(), nullptr);
  if (rc) return rc;
  rc = is3d_finish(e);
  if (rc) return rc;
  HIPCHK(e, hipMemcpy(dN, e->fd.d_io.get(), n * sizeof(double), hipMemcpyDeviceToHost));
  return IS3D_OK;
}

// ------------------------------------------------------------------------------------------
// the delta-f coefficient tables of the PDG list (generate_delta_f_coefficients/*/df_vh_dimensionless; dfgen.hip)
// ------------------------------------------------------------------------------------------
extern "C" int is3d_generate_df_tables(is3d_engine* e, int nT, int nmuB, const double* T, const double* muB, double* tables) {
  if (e && e->grp) return is3d::group_generate_df_tables(e->grp, nT, nmuB, T, muB, tables);
  if (!e) return IS3D_ERR_ARG;
  if (!T || !muB || !tables) return e->fail(IS3D_ERR_ARG, "df generator: null argument");
  if (nT < 1 || nmuB < 1) return e->fail(IS3D_ERR_ARG, "df generator: the (T, muB) grid needs at least one point each way");
  if ((long)nT * nmuB > (1L << 24)) return e->fail(IS3D_ERR_ARG, "df generator: more than 2^24 grid points");
  for (int i = 0; i < nT; i++)
    if (!(T[i] > 0.0) || !std::isfinite(T[i])) return e->fail(IS3D_ERR_ARG, "df generator: T must be positive");
  for (int i = 0; i < nmuB; i++)
    if (!std::isfinite(muB[i])) return e->fail(IS3D_ERR_ARG, "df generator: muB must be finite");
  for (int i = 1; i < nT; i++)
    if (!(T[i] > T[i - 1])) return e->fail(IS3D_ERR_ARG, "df generator: the T grid must be strictly ascending");
  for (int i = 1; i < nmuB; i++)
    if (!(muB[i] > muB[i - 1])) return e->fail(IS3D_ERR_ARG, "df generator: the muB grid must be strictly ascending");
  if (!e->in.have_pdg) return e->fail(IS3D_ERR_STATE, "df generator: is3d_set_pdg not called");
  if (!e->in.have_gla || e->in.gla_alpha < 1 + dfgen::kFamilies)
    return e->fail(IS3D_ERR_STATE, "df generator: needs a Gauss-Laguerre table with the rows alpha = 1 .. 4 (is3d_set_gauss_laguerre, alpha >= 5)");
  const int nh = (int)e->in.pdg_mass.size(), npts = e->in.gla_pts;
  std::vector<double> had((size_t)dfgen::kHadronStride * nh);
  for (int h = 0; h < nh; h++) {
    double* r = &had[(size_t)dfgen::kHadronStride * h];
    r[0] = e->in.pdg_mass[h]; r[1] = e->in.pdg_degen[h]; r[2] = e->in.pdg_baryon[h]; r[3] = e->in.pdg_sign[h];
  }
  // rows 1 .. 4 of the table; the node weights w e^root once, on the host
  const size_t ngl = (size_t)dfgen::kFamilies * npts;
  std::vector<double> roots(e->in.gla_r.begin() + npts, e->in.gla_r.begin() + npts + ngl), wts(ngl);
  for (size_t k = 0; k < ngl; k++) wts[k] = dfgen::node_weight(roots[k], e->in.gla_w[npts + k]);
  std::vector<int> codes((size_t)nT * nmuB);
  HIPCHK(e, hipSetDevice(e->device));
  const std::string msg = dfgen::generate(nh, had.data(), npts, roots.data(), wts.data(), nT, nmuB, T, muB, tables, codes.data());
  if (!msg.empty()) return e->fail(IS3D_ERR_DEVICE, msg);
  int code = dfgen::OK;
  const long at = dfgen::first_error(codes.data(), (long)codes.size(), &code);
  if (at >= 0) {
    char where[96];
    std::snprintf(where, sizeof where, " at T = %.17g GeV, muB = %.17g GeV", T[at % nT], muB[at / nT]);
    return e->fail(IS3D_ERR_DF_RANGE, std::string(dfgen::message(code)) + where);
  }
  return IS3D_OK;
}
