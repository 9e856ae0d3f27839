// decay_mc_math.h -- host/device math of the Monte Carlo resonance decays of a sampled particle list, shared by the
// kernels (decay_list.hip) and the CPU emulator (tests/native/decay_list_emulator.cpp).  DESIGN.md 7.7 has the method;
// it is the Monte Carlo counterpart of the feed-down of the continuous spectra (decay_math.h, 7.6) and uses its channel
// plan unchanged (decay::Plan::kept: the open 2- and 3-body channels -- and, after is3d_set_decays4, 4-body channels --
// in canonical order, adjusted masses included).
//
// State of a particle: (species, pT, phi, y) and its position -- what the feed-down's grid remembers.  A record is on
// its species' pole mass shell; y = asinh(pz / mT).  One decay of a particle of species p (decay_node below):
//   u = the first uniform of the node's stream; the cumulative branching of p's kept channels is walked in canonical
//   order; u >= sum b: the particle stays (undecayed).  Otherwise the parent enters the channel at (pT, phi, y) on the
//   channel's parent mass M (the pole mass unless the closed-channel rule adjusted it).
//   2-body: isotropic in the rest frame with the channel's masses (E1* = (M^2 + m1^2 - m2^2) / 2M, E2* = M - E1*), boosted.
//   3-body: flat Dalitz plot.  s23 is drawn with density f(s) = sqrt(lambda(M^2, m1^2, s) lambda(s, m2^2, m3^2)) / s
//   (the flat-Dalitz marginal, 7.6's f) by rejection under the constant envelope
//   sqrt(lambda(M^2, m1^2, s_lo)) sqrt(lambda(s_hi, m2^2, m3^2)) / s_hi (lambda_1 falls and sqrt(lambda_2) / s rises
//   over [s_lo, s_hi]), at most kDalitzCap tries (a capped decay leaves the parent as it is and is counted); then
//   R -> 1 + (23) and (23) -> 2 + 3, both isotropic.
//   4-body: flat four-body phase space as a chain of two-body decays (Raubold-Lynch): R -> 1 + (234), (234) -> 2 + (34),
//   (34) -> 3 + 4, each isotropic; the density of (M234, M34) is proportional to p1 p2 p3 with p1 = p*(M; m1, M234),
//   p2 = p*(M234; m2, M34), p3 = p*(M34; m3, m4).  K = M - sum m; two uniforms, ordered u_lo <= u_hi, give
//   M34 = m3 + m4 + u_lo K and M234 = m2 + m3 + m4 + u_hi K (uniform over the allowed triangle), and a third accepts
//   when u w_max < p1 p2 p3, w_max = p*(M; m1, m2 + m3 + m4) p*(M - m1; m2, m3 + m4) p*(M - m1 - m2; m3, m4).  w_max bounds
//   the product because p*(W; a, b) rises in W and falls in a and in b: p1 falls in M234 (largest at its lower end),
//   p2 rises in M234 and falls in M34 (largest at M234 = M - m1, M34 = m3 + m4), p3 rises in M34 (largest at
//   M34 = M - m1 - m2).  Acceptance with pion masses: 0.068 at M = 1.72 GeV, 0.12 at threshold, so the cap is its own
//   constant kFourCap = 1024 tries ((1 - 0.068)^1024 < 1e-30).
//   A daughter is written on its species' pole mass shell at the (pT, phi, y) it was produced with: px, py and the
//   rapidity are kept (nothing changes when the channel's daughter mass is the pole mass).
//
// Random numbers: the sampler's Philox streams (sampler_math.h) with the purpose P_DECAY = 4, keyed as
// (seed, P_DECAY, index of the primary inside its event, the record's event, path code); path code: root 0, child
// slot s of node c is 4 c + s + 1 (slot 3 of a 4-body channel: 4 c + 4).  P_DECAY << 22 is bit 24 of the counter word,
// which the sampler's purposes use only for a cell index >= 2^32; the index of a primary inside its event is below 2^32 (checked by the caller).  The
// counter has 32 bits for the path code: a plan has at most kMaxLevels = 16 levels (4^16 - 1 is the largest code
// through slots 0 .. 2).  Through slot 3 the largest code at depth d is 4 (4^d - 1) / 3: below 2^32 for d <= 15, above it
// for d = 16, so a plan that holds a 4-body channel has at most kMaxLevelsFour = 15 levels.
#pragma once
#include <cmath>
#include <cstdint>

#include "decay_math.h"
#include "sampler_math.h"

namespace is3d {
namespace decay_mc {

using sampler::Particle;
using sampler::Stream;

constexpr int P_DECAY = 4;
constexpr int kDalitzCap = 256;
constexpr int kFourCap = 1024;
constexpr int kMaxLevels = 16;
constexpr int kMaxLevelsFour = 15;

// one kept channel.  cum: the cumulative branching of the parent's channels up to and including this one
// 2-body: k0 = p*, k1 = E1*, k2 = E2*;  3-body: k0 = s_lo, k1 = s_hi, k2 = the envelope;
// 4-body: k0 = K = M - sum m, k1 = w_max, k2 = 0
struct Chan {
  double cum, M, m[4], k0, k1, k2;
  int nbody, d[4];
  int pad;
};

// read-only tables of a plan: species p's channels are ch[first[p] .. first[p + 1]); level[p]: the pass in which p
// decays (-1: never); mass[p]: the pole mass
struct Table {
  const int* first;
  const int* level;
  const double* mass;
  const Chan* ch;
  int npart;
};

struct Tally { long decays, undecayed, dropped, capped; };

enum Outcome : int { D_LATER = 0, D_UNDECAYED = 1, D_CAPPED = 2, D_DECAY = 3 };

IS3D_HD double lambda1(const Chan& c, double s) { return ((c.M + c.m[0]) * (c.M + c.m[0]) - s) * ((c.M - c.m[0]) * (c.M - c.m[0]) - s); }
IS3D_HD double lambda2(const Chan& c, double s) { return (s - (c.m[1] + c.m[2]) * (c.m[1] + c.m[2])) * (s - (c.m[1] - c.m[2]) * (c.m[1] - c.m[2])); }
IS3D_HD double pos_sqrt(double v) { return sqrt(v > 0.0 ? v : 0.0); }
// p*(W; a, b): the rest-frame momentum of W -> a + b (0 below the threshold)
IS3D_HD double pstar(double W, double a, double b) { return pos_sqrt((W * W - (a + b) * (a + b)) * (W * W - (a - b) * (a - b))) / (2.0 * W); }

// the constants of a channel from its masses (host: the table builder; the emulator uses the same)
inline void chan_constants(Chan& c) {
  if (c.nbody == 2) {
    c.k1 = (c.M * c.M + c.m[0] * c.m[0] - c.m[1] * c.m[1]) / (2.0 * c.M);
    c.k2 = c.M - c.k1;
    c.k0 = pos_sqrt(c.k1 * c.k1 - c.m[0] * c.m[0]);
  } else if (c.nbody == 3) {
    c.k0 = (c.m[1] + c.m[2]) * (c.m[1] + c.m[2]);
    c.k1 = (c.M - c.m[0]) * (c.M - c.m[0]);
    c.k2 = pos_sqrt(lambda1(c, c.k0)) * pos_sqrt(lambda2(c, c.k1)) / c.k1;
  } else {
    c.k0 = c.M - (c.m[0] + c.m[1] + c.m[2] + c.m[3]);
    c.k1 = pstar(c.M, c.m[0], c.m[1] + c.m[2] + c.m[3]) * pstar(c.M - c.m[0], c.m[1], c.m[2] + c.m[3]) *
           pstar(c.M - c.m[0] - c.m[1], c.m[2], c.m[3]);
    c.k2 = 0.0;
  }
}

IS3D_HD Stream node_stream(uint64_t seed, long prim, long event, long path) {
  return sampler::stream_open(seed, P_DECAY, prim, event, path);
}

// the channel draw: index of the first channel of species sp whose cumulative branching is above u, -1: none
IS3D_HD int channel_draw(const Table& T, int sp, double u) {
  for (int q = T.first[sp]; q < T.first[sp + 1]; q++)
    if (u < T.ch[q].cum) return q;
  return -1;
}

// s23 of a 3-body channel; false: the cap was reached
IS3D_HD bool dalitz_draw(Stream& s, const Chan& c, double* s23) {
  for (int it = 0; it < kDalitzCap; it++) {
    const double v = c.k0 + sampler::stream_next(s) * (c.k1 - c.k0);
    const double f = pos_sqrt(lambda1(c, v)) * pos_sqrt(lambda2(c, v)) / v;
    const double u = sampler::stream_next(s);
    if (u * c.k2 < f) { *s23 = v; return true; }
  }
  return false;
}

// (M234, M34) of a 4-body channel; false: the cap was reached.  Three uniforms a try: the two masses, the acceptance
IS3D_HD bool four_draw(Stream& s, const Chan& c, double* m234, double* m34) {
  for (int it = 0; it < kFourCap; it++) {
    const double ua = sampler::stream_next(s), ub = sampler::stream_next(s);
    const double lo = ua < ub ? ua : ub, hi = ua < ub ? ub : ua;
    const double w34 = c.m[2] + c.m[3] + lo * c.k0, w234 = c.m[1] + c.m[2] + c.m[3] + hi * c.k0;
    const double f = pstar(c.M, c.m[0], w234) * pstar(w234, c.m[1], w34) * pstar(w34, c.m[2], c.m[3]);
    const double u = sampler::stream_next(s);
    if (u * c.k1 < f) { *m234 = w234; *m34 = w34; return true; }
  }
  return false;
}

// What becomes of a record of species sp in pass `pass`: the stream s is left after the channel draw (and, for a
// 3-body channel, after the s23 draws; for a 4-body channel, after the (M234, M34) draws), so a count kernel and an
// emit kernel that each reopen the stream agree.  3-body: *wa = s23.  4-body: *wa = M234, *wb = M34.
IS3D_HD int node_choice(const Table& T, int sp, int pass, uint64_t seed, long prim, long event, long path, Stream& s, int* q,
                        double* wa, double* wb) {
  if (T.level[sp] != pass) return D_LATER;
  s = node_stream(seed, prim, event, path);
  *q = channel_draw(T, sp, sampler::stream_next(s));
  if (*q < 0) return D_UNDECAYED;
  const int nbody = T.ch[*q].nbody;
  if (nbody == 3 && !dalitz_draw(s, T.ch[*q], wa)) return D_CAPPED;
  if (nbody == 4 && !four_draw(s, T.ch[*q], wa, wb)) return D_CAPPED;
  return D_DECAY;
}

// records the node becomes: itself, or its chosen daughters
IS3D_HD int node_count(const Table& T, int outcome, int q) {
  if (outcome != D_DECAY) return 1;
  const Chan& c = T.ch[q];
  int n = 0;
  for (int k = 0; k < c.nbody; k++) n += c.d[k] >= 0;
  return n;
}

struct P4 { double E, x, y, z; };
struct V3 { double x, y, z; };

// isotropic direction times p from two uniforms
IS3D_HD V3 isotropic(Stream& s, double p) {
  const double ct = 2.0 * sampler::stream_next(s) - 1.0, phi = sampler::kTwoPi * sampler::stream_next(s);
  const double st = pos_sqrt(1.0 - ct * ct);
  return V3{p * st * cos(phi), p * st * sin(phi), p * ct};
}

// (e, q) in the rest frame of the system (P, mass M) -> its frame
IS3D_HD P4 boost(const P4 P, double M, double e, const V3 q) {
  const double Pq = P.x * q.x + P.y * q.y + P.z * q.z;
  const double g = Pq / (M * (P.E + M)) + e / M;
  return P4{(P.E * e + Pq) / M, q.x + g * P.x, q.y + g * P.y, q.z + g * P.z};
}

// the parent's four-momentum on the channel mass M at the record's (pT, phi, y)
IS3D_HD P4 parent_p4(const Particle& r, double pole, double M) {
  const double pT2 = r.px * r.px + r.py * r.py;
  const double sh = r.pz / sqrt(pole * pole + pT2), MT = sqrt(M * M + pT2);
  return P4{MT * sqrt(1.0 + sh * sh), r.px, r.py, MT * sh};
}

// the momenta of the channel's daughters in the lab from the stream left by node_choice
struct Daughters { P4 a, b, c; };     // returned by value: a kernel then keeps the three momenta in registers

// the two halves of W -> 1 + 2 (masses given by e1 and W - e1, momentum p) for a system W moving with P in some frame
struct Pair { P4 a, b; };
IS3D_HD Pair split(Stream& s, const P4& P, double W, double e1, double p) {
  const V3 q = isotropic(s, p);
  return Pair{boost(P, W, e1, q), boost(P, W, W - e1, V3{-q.x, -q.y, -q.z})};
}

// 4-body chain R -> 1 + (234), (234) -> 2 + (34), (34) -> 3 + 4 in R's rest frame; every daughter goes into the lab
// and to out(slot, momentum) as soon as it is known, in slot order.  A branch of its own that hands the daughters over
// one at a time: only the system still to split stays live, so k_dl_emit needs no more registers than its 3-body path
// (four momenta returned together cost it 136 VGPRs and two of its five waves)
template <class Out>
IS3D_HD void four_kinematics(Stream& s, const Chan& c, const P4& R, double w234, double w34, Out out) {
  const double e1 = (c.M * c.M + c.m[0] * c.m[0] - w234 * w234) / (2.0 * c.M);
  const Pair A = split(s, P4{c.M, 0.0, 0.0, 0.0}, c.M, e1, pstar(c.M, c.m[0], w234));          // 1, (234)
  out(0, boost(R, c.M, A.a.E, V3{A.a.x, A.a.y, A.a.z}));
  const double e2 = (w234 * w234 + c.m[1] * c.m[1] - w34 * w34) / (2.0 * w234);
  const Pair B = split(s, A.b, w234, e2, pstar(w234, c.m[1], w34));                            // 2, (34)
  out(1, boost(R, c.M, B.a.E, V3{B.a.x, B.a.y, B.a.z}));
  const double e3 = (w34 * w34 + c.m[2] * c.m[2] - c.m[3] * c.m[3]) / (2.0 * w34);
  const Pair C = split(s, B.b, w34, e3, pstar(w34, c.m[2], c.m[3]));                           // 3, 4
  out(2, boost(R, c.M, C.a.E, V3{C.a.x, C.a.y, C.a.z}));
  out(3, boost(R, c.M, C.b.E, V3{C.b.x, C.b.y, C.b.z}));
}

// 2- and 3-body channels
IS3D_HD Daughters decay_kinematics(Stream& s, const Chan& c, const P4& R, double s23) {
  if (c.nbody == 2) {
    const V3 q = isotropic(s, c.k0);
    return Daughters{boost(R, c.M, c.k1, q), boost(R, c.M, c.k2, V3{-q.x, -q.y, -q.z}), P4{0.0, 0.0, 0.0, 0.0}};
  }
  const double m23 = sqrt(s23);
  const double p1 = pos_sqrt(lambda1(c, s23)) / (2.0 * c.M), e1 = (c.M * c.M + c.m[0] * c.m[0] - s23) / (2.0 * c.M);
  const V3 q1 = isotropic(s, p1);
  const P4 o0 = boost(R, c.M, e1, q1);
  const P4 S{c.M - e1, -q1.x, -q1.y, -q1.z};     // the (23) system in R's rest frame
  const double p2 = pos_sqrt(lambda2(c, s23)) / (2.0 * m23), e2 = (s23 + c.m[1] * c.m[1] - c.m[2] * c.m[2]) / (2.0 * m23);
  const V3 q2 = isotropic(s, p2);
  const P4 a = boost(S, m23, e2, q2);
  const P4 b = boost(S, m23, m23 - e2, V3{-q2.x, -q2.y, -q2.z});
  return Daughters{o0, boost(R, c.M, a.E, V3{a.x, a.y, a.z}), boost(R, c.M, b.E, V3{b.x, b.y, b.z})};
}

// what a decay changes of a record: the species and the momentum (the position, cell and event stay the parent's)
struct Mom {
  int species;
  double E, px, py, pz;
};

// a daughter of species d produced with momentum p on the channel's mass mc: (px, py, y) on d's pole mass
IS3D_HD Mom daughter_mom(int d, double pole, double mc, const P4& p) {
  double pz = p.z;
  const double pT2 = p.x * p.x + p.y * p.y;
  if (mc != pole) pz = sqrt(pole * pole + pT2) * (p.z / sqrt(mc * mc + pT2));
  return Mom{d, sqrt(pole * pole + pT2 + pz * pz), p.x, p.y, pz};
}

IS3D_HD void apply(Particle& r, const Mom& m) {
  r.species = m.species; r.E = m.E; r.px = m.px; r.py = m.py; r.pz = m.pz;
}

// One node in pass `pass`: emit(slot, mom) is called for every record the node becomes, in daughter-slot order -- the
// parent's record with mom applied (slot -1: the record itself, mom unused); returns their number.  The whole of k_dl_emit's per-record work and of the emulator's.
// The daughters are named variables handed over one at a time, so a kernel keeps them in registers.
template <class Emit>
IS3D_HD int decay_node(const Table& T, int pass, uint64_t seed, const Particle& r, long prim, long path, Tally& t, Emit emit) {
  Stream s;
  int q = -1;
  double s23 = 0.0, w34 = 0.0;     // 4-body: s23 holds M234
  const int oc = node_choice(T, r.species, pass, seed, prim, (long)r.event, path, s, &q, &s23, &w34);
  if (oc != D_DECAY) {
    t.undecayed += oc == D_UNDECAYED;
    t.capped += oc == D_CAPPED;
    emit(-1, Mom{r.species, r.E, r.px, r.py, r.pz});
    return 1;
  }
  t.decays++;
  int n = 0;
  auto daughter = [&](int k, int d, double mc, const P4 p) __attribute__((always_inline)) {
    if (d < 0) { t.dropped++; return; }
    emit(k, daughter_mom(d, T.mass[d], mc, p));
    n++;
  };
  if (T.ch[q].nbody == 4) {
    // the channel is read where it lies (each field when it is needed) and the slot is a constant at each of the
    // four calls, so d[k] and m[k] are named values after inlining
    const Chan& f = T.ch[q];
    four_kinematics(s, f, parent_p4(r, T.mass[r.species], f.M), s23, w34, [&](int k, const P4 p) __attribute__((always_inline)) {
      daughter(k, f.d[k], f.m[k], p);
    });
    return n;
  }
  const Chan c = T.ch[q];
  const Daughters D = decay_kinematics(s, c, parent_p4(r, T.mass[r.species], c.M), s23);
  daughter(0, c.d[0], c.m[0], D.a);
  daughter(1, c.d[1], c.m[1], D.b);
  if (c.nbody == 3) daughter(2, c.d[2], c.m[2], D.c);
  return n;
}

// ---------------------------------------------------------------------------------------------------------
// host: plan -> tables
// ---------------------------------------------------------------------------------------------------------
struct HostTable {
  std::vector<int> first, level;
  std::vector<double> mass;
  std::vector<Chan> ch;
  Table view() const { return Table{first.data(), level.data(), mass.data(), ch.data(), (int)mass.size()}; }
};

// the Monte Carlo tables of a feed-down plan; species_mass[npart]: the pole masses
inline HostTable make_table(const decay::Plan& P, int npart, const double* species_mass) {
  HostTable H;
  H.first = P.first;
  H.level = P.level_of;
  H.first.resize((size_t)npart + 1, P.first.empty() ? 0 : P.first.back());
  H.level.resize((size_t)npart, -1);
  H.mass.assign(species_mass, species_mass + npart);
  for (int p = 0; p < npart; p++) {
    double cum = 0.0;
    for (int q = H.first[p]; q < H.first[p + 1]; q++) {
      const decay::Kept& k = P.kept[q];
      Chan c{};
      cum += k.c.branching;
      c.cum = cum;
      c.M = k.M;
      c.nbody = k.c.n_body;
      for (int i = 0; i < 4; i++) { c.m[i] = k.m[i]; c.d[i] = i < c.nbody ? k.c.daughter[i] : -1; }
      chan_constants(c);
      H.ch.push_back(c);
    }
  }
  return H;
}

// what the Monte Carlo refuses of a plan the feed-down accepts (an IS3D_ERR_ARG for the caller), or an empty string
inline std::string check_plan(const decay::Plan& P) {
  bool four = false;
  for (const decay::Kept& k : P.kept) four = four || k.c.n_body == 4;
  if (four && P.levels() > kMaxLevelsFour)
    return "the decay plan holds a 4-body channel and has " + std::to_string(P.levels()) + " levels, more than " +
           std::to_string(kMaxLevelsFour) + " (the path code of the random streams has 32 bits)";
  if (P.levels() > kMaxLevels)
    return "the decay plan has " + std::to_string(P.levels()) + " levels, more than " + std::to_string(kMaxLevels) +
           " (the path code of the random streams has 32 bits)";
  return "";
}

}  // namespace decay_mc
}  // namespace is3d
