// CPU emulator of the resonance-decay feed-down: is3d2_amd/csrc/decay_math.h compiled for the host and run in the
// kernel's order (decay.hip k_decay_feed: per output row the terms of a level, each term's (v, zeta) nodes, added
// sequentially), so the GPU and this file differ by libm and contraction rounding only.  Built by tests/decay_ref.py.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../is3d2_amd/csrc/decay_math.h"

using namespace is3d::decay;

// S[npart][npT][nphi][ny] in place.  sum_abs (optional, same shape, caller-zeroed): the sum of |term| of every output,
// the denominator of the parity metric.  Returns 0, or 1 with msg (what is3d_set_decays / the feed-down would refuse).
extern "C" int decay_emulate(int npart, const double* mass, int npT, const double* pT, int nphi, const double* phi, int ny,
                             const double* y, int n, const is3d_decay_channel* ch, double* S, double* sum_abs,
                             is3d_decay_stats* stats, long* slots, char* msg, int msg_len) {
  auto fail = [&](const std::string& m) {
    if (msg && msg_len > 0) {
      std::strncpy(msg, m.c_str(), msg_len - 1);
      msg[msg_len - 1] = 0;
    }
    return 1;
  };
  std::string err = check_grid(npT, pT, nphi, phi, ny > 1 ? ny : 0, y);
  if (!err.empty()) return fail(err);
  const Rule rule = make_rule();
  Plan P;
  err = build_plan(P, rule, npart, mass, n, ch);
  if (!err.empty()) return fail(err);
  if (stats) *stats = P.stats;
  if (slots) *slots = P.slots;
  const long slab = (long)npT * nphi * ny;
  std::vector<double> L((size_t)npart * slab, 0.0);
  for (int l = 0; l < P.levels(); l++) {
    for (int q = P.lvl_p0[l]; q < P.lvl_p0[l + 1]; q++) {
      const long o = (long)P.par[q] * slab;
      for (long i = 0; i < slab; i++) L[o + i] = log_or_nan(S[o + i]);
    }
    const long rows = (long)(P.lvl_r0[l + 1] - P.lvl_r0[l]) * npT * ny;
#pragma omp parallel for schedule(dynamic, 4)
    for (long row = 0; row < rows; row++) {
      const int r = P.lvl_r0[l] + (int)(row / ((long)npT * ny));
      const int rem = (int)(row % ((long)npT * ny));
      const int ipT = rem / ny, iy = rem % ny;
      const int d = P.recv_d[r];
      std::vector<double> acc(nphi, 0.0), absacc(nphi, 0.0), g(nphi);
      for (int s = P.recv_s0[r]; s < P.recv_s1[r]; s++) {
        const Sub& sub = P.subs[s];
        const double* Sp = S + (long)sub.parent * slab;
        const double* Lp = L.data() + (long)sub.parent * slab;
        for (int node = 0; node < kNodes; node++) {
          const Node nd = node_eval(sub, rule, node / kGL, node % kGL, pT[ipT], ny > 1 ? y[iy] : 0.0, npT, pT, ny, y);
          for (int j = 0; j < nphi; j++) g[j] = parent_value(Sp, Lp, nphi, ny, nd, j);
          for (int i = 0; i < nphi; i++) {
            const double t = nd.weight * (phi_interp(g.data(), phi, nphi, phi[i] + nd.delta) +
                                          phi_interp(g.data(), phi, nphi, phi[i] - nd.delta));
            acc[i] += t;
            absacc[i] += std::fabs(t);
          }
        }
      }
      for (int i = 0; i < nphi; i++) {
        const long o = (long)d * slab + ((long)ipT * nphi + i) * ny + iy;
        S[o] += acc[i];
        if (sum_abs) sum_abs[o] += absacc[i];
      }
    }
  }
  return 0;
}

extern "C" void decay_gauss_legendre(int n, double* x, double* w) { gauss_legendre(n, x, w); }
extern "C" int decay_channel_size(void) { return (int)sizeof(is3d_decay_channel); }
