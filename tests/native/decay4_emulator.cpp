// CPU emulator of the decays with four-body channels: is3d2_amd/csrc/decay_math.h and decay_mc_math.h compiled for the
// host behind the four-slot channel table (is3d_decay_channel4), the counterpart of decay_emulator.cpp and
// decay_list_emulator.cpp for is3d_set_decays4.  keep_four = 0 takes is3d_set_decays' rule (every row with >= 4 bodies
// skipped), so the two rules can be compared on one table.  Built by tests/decay4_ref.py.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../is3d2_amd/csrc/decay_mc_math.h"

using namespace is3d;
using decay_mc::Particle;

namespace {
std::vector<Particle> g_out;
std::vector<long> g_origin;

int fail(char* msg, int msg_len, const std::string& m) {
  if (msg && msg_len > 0) { std::strncpy(msg, m.c_str(), msg_len - 1); msg[msg_len - 1] = 0; }
  return 1;
}
}  // namespace

// decay_list_emulator.cpp's dl_emulate over a four-slot table
extern "C" long dl4_emulate(int npart, const double* mass, int nch, const is3d_decay_channel4* ch, int keep_four, long seed, long n,
                            const Particle* in, const unsigned* prim, long* stats, is3d_decay_stats* plan_stats, char* msg,
                            int msg_len) {
  const decay::Rule rule = decay::make_rule();
  decay::Plan P;
  std::string err = decay::build_plan(P, rule, npart, mass, nch, ch, keep_four != 0);
  if (err.empty()) err = decay_mc::check_plan(P);
  if (!err.empty()) { fail(msg, msg_len, err); return -1; }
  if (plan_stats) *plan_stats = P.stats;
  const decay_mc::HostTable H = decay_mc::make_table(P, npart, mass);
  const decay_mc::Table T = H.view();
  const int levels = P.levels();
  struct Node { Particle p; long path; };
  std::vector<std::vector<Particle>> leaves((size_t)n);
  long tl[4] = {0, 0, 0, 0};
#pragma omp parallel
  {
    decay_mc::Tally t{0, 0, 0, 0};
    std::vector<Node> a, b;
#pragma omp for schedule(dynamic, 1024)
    for (long i = 0; i < n; i++) {
      a.assign(1, Node{in[i], 0});
      for (int pass = 0; pass < levels; pass++) {
        b.clear();
        for (const Node& nd : a) {
          decay_mc::decay_node(T, pass, (uint64_t)seed, nd.p, (long)prim[i], nd.path, t, [&](int slot, const decay_mc::Mom& m) {
            b.push_back(Node{nd.p, slot < 0 ? nd.path : 4 * nd.path + slot + 1});
            if (slot >= 0) decay_mc::apply(b.back().p, m);
          });
        }
        a.swap(b);
      }
      leaves[(size_t)i].reserve(a.size());
      for (const Node& nd : a) leaves[(size_t)i].push_back(nd.p);
    }
#pragma omp critical
    { tl[0] += t.decays; tl[1] += t.undecayed; tl[2] += t.dropped; tl[3] += t.capped; }
  }
  g_out.clear();
  g_origin.clear();
  for (long i = 0; i < n; i++)
    for (const Particle& p : leaves[(size_t)i]) { g_out.push_back(p); g_origin.push_back(i); }
  if (stats) {
    stats[0] = n; stats[1] = tl[0]; stats[2] = tl[1]; stats[3] = tl[2]; stats[4] = tl[3];
    stats[5] = (long)g_out.size(); stats[6] = levels; stats[7] = 0;
  }
  return (long)g_out.size();
}

extern "C" void dl4_fetch(Particle* out, long* origin) {
  if (!g_out.empty()) std::memcpy(out, g_out.data(), g_out.size() * sizeof(Particle));
  if (!g_origin.empty()) std::memcpy(origin, g_origin.data(), g_origin.size() * sizeof(long));
}

// the kept channels as the Monte Carlo sees them: per channel (parent, nbody, d0 .. d3) and
// (cum, M, m0 .. m3, k0, k1, k2); returns their number (or -1), at most cap are written; levels (optional): the plan's
extern "C" int dl4_channels(int npart, const double* mass, int nch, const is3d_decay_channel4* ch, int keep_four, int cap, int* ints,
                            double* dbls, int* level, int* levels) {
  const decay::Rule rule = decay::make_rule();
  decay::Plan P;
  if (!decay::build_plan(P, rule, npart, mass, nch, ch, keep_four != 0).empty()) return -1;
  const decay_mc::HostTable H = decay_mc::make_table(P, npart, mass);
  if (levels) *levels = P.levels();
  for (int p = 0; p < npart; p++) {
    if (level) level[p] = H.level[p];
    for (int q = H.first[p]; q < H.first[p + 1] && q < cap; q++) {
      const decay_mc::Chan& c = H.ch[q];
      const int iv[6] = {p, c.nbody, c.d[0], c.d[1], c.d[2], c.d[3]};
      const double dv[9] = {c.cum, c.M, c.m[0], c.m[1], c.m[2], c.m[3], c.k0, c.k1, c.k2};
      std::memcpy(ints + 6 * q, iv, sizeof(iv));
      std::memcpy(dbls + 9 * q, dv, sizeof(dv));
    }
  }
  return (int)H.ch.size();
}

// The envelope of one four-body channel over `draws` tries of the header's own draw (the (u, u, accept) triples of
// the node stream (seed, 0, 0, 0)): out[0] = the largest p1 p2 p3 / w_max, out[1] = the accepted share, out[2] = w_max
extern "C" void dl4_envelope(double M, const double* m, long seed, long draws, double* out) {
  decay_mc::Chan c{};
  c.M = M; c.nbody = 4;
  for (int k = 0; k < 4; k++) c.m[k] = m[k];
  decay_mc::chan_constants(c);
  decay_mc::Stream s = decay_mc::node_stream((uint64_t)seed, 0, 0, 0);
  double worst = 0.0;
  long acc = 0;
  for (long i = 0; i < draws; i++) {
    const double ua = sampler::stream_next(s), ub = sampler::stream_next(s);
    const double lo = ua < ub ? ua : ub, hi = ua < ub ? ub : ua;
    const double w34 = c.m[2] + c.m[3] + lo * c.k0, w234 = c.m[1] + c.m[2] + c.m[3] + hi * c.k0;
    const double f = decay_mc::pstar(c.M, c.m[0], w234) * decay_mc::pstar(w234, c.m[1], w34) * decay_mc::pstar(w34, c.m[2], c.m[3]);
    const double u = sampler::stream_next(s);
    if (f / c.k1 > worst) worst = f / c.k1;
    acc += u * c.k1 < f;
  }
  out[0] = worst; out[1] = (double)acc / (double)draws; out[2] = c.k1;
}

// the s nodes and the normalised weights of one slot of a four-body channel: daughter mass m1 against mo[3], the inner
// rule with phi3_points nodes.  s[12], w[12]; returns 0 when the slot is not open
extern "C" int decay4_slot_weights(double M, double m1, const double* mo, int phi3_points, double* s, double* w) {
  const decay::Rule rule = decay::make_rule();
  const decay::Inner in = decay::make_inner(phi3_points);
  std::vector<decay::Sub> subs;
  const bool ok = decay::push_terms(subs, rule, 0, 1.0, M, m1, 3, mo, &in);
  if ((int)subs.size() != decay::kGL) return 0;
  for (int k = 0; k < decay::kGL; k++) {
    s[k] = M * M + m1 * m1 - 2.0 * M * subs[k].Estar;
    w[k] = subs[k].coef * 4.0 * decay::kPi * subs[k].dY0;
  }
  return ok ? 1 : 0;
}

extern "C" double decay4_phi3(double s, double a, double b, double c, int points) {
  return decay::phi3(decay::make_inner(points), s, a, b, c);
}

// decay_emulator.cpp's decay_emulate over a four-slot table; terms (optional): the number of two-body terms
extern "C" int decay4_emulate(int npart, const double* mass, int npT, const double* pT, int nphi, const double* phi, int ny,
                              const double* y, int n, const is3d_decay_channel4* ch, int keep_four, int phi3_points, double* S,
                              double* sum_abs, is3d_decay_stats* stats, long* slots, long* terms, char* msg, int msg_len) {
  using namespace is3d::decay;
  std::string err = check_grid(npT, pT, nphi, phi, ny > 1 ? ny : 0, y);
  if (!err.empty()) return fail(msg, msg_len, err);
  const Rule rule = make_rule();
  Plan P;
  err = build_plan(P, rule, npart, mass, n, ch, keep_four != 0, phi3_points);
  if (!err.empty()) return fail(msg, msg_len, err);
  if (stats) *stats = P.stats;
  if (slots) *slots = P.slots;
  if (terms) *terms = (long)P.subs.size();
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

extern "C" int decay4_channel_size(void) { return (int)sizeof(is3d_decay_channel4); }
extern "C" int dl4_particle_size(void) { return (int)sizeof(Particle); }
