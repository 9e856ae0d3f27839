// CPU emulator of the Monte Carlo decays of a particle list: is3d2_amd/csrc/decay_mc_math.h compiled for the host and
// run over a list, one primary's tree at a time, pass by pass as decay_list.hip does, so the GPU and this file differ
// by libm and contraction rounding only.  Built by tests/decay_list_ref.py.
#include <cstring>
#include <string>
#include <vector>

#include "../../is3d2_amd/csrc/decay_mc_math.h"

using namespace is3d;
using decay_mc::Particle;

namespace {
std::vector<Particle> g_out;
std::vector<long> g_origin;
}  // namespace

// Decays in[0 .. n); prim[i]: the index of primary i inside its event.  Returns the number of final records (fetch
// them with dl_fetch), or -1 with msg.  stats[8]: primaries, decays, undecayed, dropped daughters, capped, final
// particles, passes, 0.  plan_stats (optional): the feed-down plan's statistics of the same table.
extern "C" long dl_emulate(int npart, const double* mass, int nch, const is3d_decay_channel* ch, long seed, long n,
                           const Particle* in, const unsigned* prim, long* stats, is3d_decay_stats* plan_stats, char* msg,
                           int msg_len) {
  const decay::Rule rule = decay::make_rule();
  decay::Plan P;
  std::string err = decay::build_plan(P, rule, npart, mass, nch, ch);
  if (err.empty()) err = decay_mc::check_plan(P);
  if (!err.empty()) {
    if (msg && msg_len > 0) { std::strncpy(msg, err.c_str(), msg_len - 1); msg[msg_len - 1] = 0; }
    return -1;
  }
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

extern "C" void dl_fetch(Particle* out, long* origin) {
  if (!g_out.empty()) std::memcpy(out, g_out.data(), g_out.size() * sizeof(Particle));
  if (!g_origin.empty()) std::memcpy(origin, g_origin.data(), g_origin.size() * sizeof(long));
}

// the first n uniforms of the node stream (seed, P_DECAY, prim, event, path): uniform 0 is the channel draw
extern "C" void dl_uniforms(long seed, long prim, long event, long path, int n, double* out) {
  decay_mc::Stream s = decay_mc::node_stream((uint64_t)seed, prim, event, path);
  for (int i = 0; i < n; i++) out[i] = sampler::stream_next(s);
}

// the kept channels of a table as the Monte Carlo sees them: per channel (parent, nbody, d0, d1, d2) and
// (cum, M, m0, m1, m2, k0, k1, k2); returns their number (or -1), at most cap are written
extern "C" int dl_channels(int npart, const double* mass, int nch, const is3d_decay_channel* ch, int cap, int* ints, double* dbls,
                           int* level) {
  const decay::Rule rule = decay::make_rule();
  decay::Plan P;
  if (!decay::build_plan(P, rule, npart, mass, nch, ch).empty()) return -1;
  const decay_mc::HostTable H = decay_mc::make_table(P, npart, mass);
  for (int p = 0; p < npart; p++) {
    if (level) level[p] = H.level[p];
    for (int q = H.first[p]; q < H.first[p + 1] && q < cap; q++) {
      const decay_mc::Chan& c = H.ch[q];
      const int iv[5] = {p, c.nbody, c.d[0], c.d[1], c.d[2]};
      const double dv[8] = {c.cum, c.M, c.m[0], c.m[1], c.m[2], c.k0, c.k1, c.k2};
      std::memcpy(ints + 5 * q, iv, sizeof(iv));
      std::memcpy(dbls + 8 * q, dv, sizeof(dv));
    }
  }
  return (int)H.ch.size();
}

extern "C" int dl_particle_size(void) { return (int)sizeof(Particle); }
