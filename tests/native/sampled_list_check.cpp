// sampled_list_check.cpp -- CPU check of is3d2_amd/csrc/sampled_list.h: one SampledList walked through every
// transition the engine and the device group make, with the code of every getter asserted in each state (the codes the
// ABI getters return: is3d_sample_count / _offsets, is3d_get_particles, is3d_get_particle_origins,
// is3d_get_sample_hist, is3d_get_sample_stats, is3d_get_sample_famod_stats, is3d_get_decay_list_stats).
// Built with -fsanitize=address,undefined by tests/test_sampled_list_cpu.py; exit 0 and "ok" = every check held.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../is3d2_amd/csrc/sampled_list.h"

using is3d::SampledList;

static int g_checks = 0;
#define CHECK(x)                                                              \
  do {                                                                        \
    g_checks++;                                                               \
    if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); std::exit(1); } \
  } while (0)

constexpr int OK = IS3D_OK, ST = IS3D_ERR_STATE, ARG = IS3D_ERR_ARG;

// the codes of the eight getters with valid, in-range arguments
struct Codes { long count; int offsets, particles, origins, hist, stats, famod, decay; };

static void expect(const SampledList& l, const Codes& want, int line) {
  std::vector<long> off(l.offsets.size() + 1), org(l.origins.size() + 1), counts((size_t)l.hist_nc + 1);
  std::vector<double> vn((size_t)l.hist_nv + 1);
  std::vector<is3d_particle> p(l.particles.size() + 1);
  is3d_sample_stats s{};
  is3d_sample_famod_stats f{};
  is3d_decay_list_stats d{};
  const Codes got{l.count(),
                  l.get_offsets(off.data()),
                  l.get_particles(0, (long)l.particles.size(), p.data()),
                  l.get_origins(0, (long)l.origins.size(), org.data()),
                  l.get_hist(counts.data(), vn.data()),
                  l.get_stats(&s),
                  l.get_famod_stats(&f),
                  l.get_decay_stats(&d)};
  g_checks++;
  if (got.count != want.count || got.offsets != want.offsets || got.particles != want.particles ||
      got.origins != want.origins || got.hist != want.hist || got.stats != want.stats || got.famod != want.famod ||
      got.decay != want.decay) {
    std::printf("FAILED state at line %d: got %ld %d %d %d %d %d %d %d\n", line, got.count, got.offsets, got.particles,
                got.origins, got.hist, got.stats, got.famod, got.decay);
    std::exit(1);
  }
  // a null output is IS3D_ERR_ARG in every state, before the state is looked at
  CHECK(l.get_offsets(nullptr) == ARG);
  CHECK(l.get_particles(0, 1, nullptr) == ARG);
  CHECK(l.get_origins(0, 1, nullptr) == ARG);
  CHECK(l.get_hist(nullptr, vn.data()) == ARG && l.get_hist(counts.data(), nullptr) == ARG);
  CHECK(l.get_stats(nullptr) == ARG && l.get_famod_stats(nullptr) == ARG && l.get_decay_stats(nullptr) == ARG);
}
#define EXPECT(l, ...) expect(l, Codes{__VA_ARGS__}, __LINE__)

// 2 events of 3 and 0 particles
static void fill_list(SampledList& l) {
  l.particles.assign(3, is3d::sampler::Particle{});
  for (int i = 0; i < 3; i++) { l.particles[i].species = i; l.particles[i].px = 0.25 * (i + 1); }
  l.offsets = {0, 3, 3};
  l.stats = is3d_sample_stats{};
  l.stats.kept = 3;
}
// a histogram of 3 counts and 2 fixed-point vn sums, one negative
static void fill_hist(SampledList& l) {
  l.hist = {5, 0, 7, -(3LL << 31), (1LL << 32) + 1};
  l.hist_nc = 3; l.hist_nv = 2;
}
// the decayed form of fill_list's: 4 records of the 3 primaries
static SampledList decayed_form(bool with_hist) {
  SampledList d;
  d.particles.assign(4, is3d::sampler::Particle{});
  d.offsets = {0, 4, 4};
  d.origins = {0, 1, 1, 2};
  d.decay_stats.primaries = 3; d.decay_stats.final_particles = 4;
  if (with_hist) { d.hist = {1, 2, 3, 4, 5}; d.hist_nc = 3; d.hist_nv = 2; }
  return d;
}

int main() {
  SampledList l;
  // a fresh list
  EXPECT(l, -1, ST, ST, ST, ST, ST, ST, ST);
  CHECK(!l.has_list());

  // after a list-only sample
  l.begin_sample();
  EXPECT(l, -1, ST, ST, ST, ST, ST, ST, ST);
  fill_list(l);
  l.commit_sample(false, false);
  EXPECT(l, 3, OK, OK, ST, ST, OK, ST, ST);
  CHECK(l.has_list());
  {
    long off[3] = {-1, -1, -1};
    CHECK(l.get_offsets(off) == OK && off[0] == 0 && off[1] == 3 && off[2] == 3);
    is3d_particle p[3];
    CHECK(l.get_particles(1, 2, p) == OK && p[0].species == 1 && p[1].species == 2 && p[1].px == 0.75);
    is3d_sample_stats s{};
    CHECK(l.get_stats(&s) == OK && s.kept == 3);
    // the range checks
    CHECK(l.get_particles(-1, 1, p) == ARG);
    CHECK(l.get_particles(0, -1, p) == ARG);
    CHECK(l.get_particles(2, 2, p) == ARG);          // first + count > size
    CHECK(l.get_particles(3, 1, p) == ARG);
    CHECK(l.get_particles(0, 1, nullptr) == ARG);    // null out with count > 0
    CHECK(l.get_particles(0, 0, nullptr) == OK);     // count == 0 with null out
    CHECK(l.get_particles(3, 0, nullptr) == OK);
    CHECK(l.get_particles(4, 0, nullptr) == ARG);
  }

  // after a binned-only sample: the list is empty though particles were kept
  l.begin_sample();
  l.particles.clear();
  l.offsets = {0, 0, 0};
  l.stats = is3d_sample_stats{};
  l.stats.kept = 3;
  fill_hist(l);
  l.commit_sample(false, true);
  EXPECT(l, 0, OK, OK, ST, OK, OK, ST, ST);
  CHECK(!l.has_list());                              // nothing for is3d_decay_sampled
  {
    long counts[3];
    double vn[2];
    CHECK(l.get_hist(counts, vn) == OK && counts[0] == 5 && counts[1] == 0 && counts[2] == 7);
    CHECK(vn[0] == is3d::sampler::vn_value(-(3LL << 31)) && vn[0] == -1.5);
    CHECK(vn[1] == is3d::sampler::vn_value((1LL << 32) + 1) && vn[1] == 1.0 + is3d::sampler::kVnQuantum);
  }
  // ... and one that kept nothing at all has an (empty) list
  l.stats.kept = 0;
  CHECK(l.has_list());

  // after a binned sample that keeps the list
  l.begin_sample();
  fill_list(l);
  fill_hist(l);
  l.commit_sample(false, true);
  EXPECT(l, 3, OK, OK, ST, OK, OK, ST, ST);
  CHECK(l.has_list());

  // after is3d_set_sample_bins: the histogram is invalid, the list still valid
  l.bins_changed();
  EXPECT(l, 3, OK, OK, ST, ST, OK, ST, ST);
  CHECK(l.has_list());

  // after a PTMA sample
  l.begin_sample();
  fill_list(l);
  l.famod_stats = is3d_sample_famod_stats{1, 2, 30};
  l.commit_sample(true, false);
  EXPECT(l, 3, OK, OK, ST, ST, OK, OK, ST);
  {
    is3d_sample_famod_stats f{};
    CHECK(l.get_famod_stats(&f) == OK && f.plpt_negative == 1 && f.reconstruction_fail == 2 && f.iterations == 30);
  }

  // after "decayed" (is3d_decay_sampled, no histogram): the list is the decayed one, the sample's stats stay
  {
    SampledList d = decayed_form(false);
    l.replace_decayed(d, false);
  }
  EXPECT(l, 4, OK, OK, OK, ST, OK, OK, OK);
  {
    long org[4];
    CHECK(l.get_origins(0, 4, org) == OK && org[0] == 0 && org[1] == 1 && org[2] == 1 && org[3] == 2);
    CHECK(l.get_origins(2, 2, org) == OK && org[0] == 1 && org[1] == 2);
    CHECK(l.get_origins(-1, 1, org) == ARG);
    CHECK(l.get_origins(0, -1, org) == ARG);
    CHECK(l.get_origins(3, 2, org) == ARG);
    CHECK(l.get_origins(0, 1, nullptr) == ARG);
    CHECK(l.get_origins(0, 0, nullptr) == OK);
    long off[3];
    CHECK(l.get_offsets(off) == OK && off[1] == 4 && off[2] == 4);
    is3d_decay_list_stats ds{};
    CHECK(l.get_decay_stats(&ds) == OK && ds.primaries == 3 && ds.final_particles == 4);
    is3d_sample_stats s{};
    CHECK(l.get_stats(&s) == OK && s.kept == 3);
  }
  // ... decayed again with bin = 1: its histogram
  {
    SampledList d = decayed_form(true);
    l.replace_decayed(d, true);
  }
  EXPECT(l, 4, OK, OK, OK, OK, OK, OK, OK);
  {
    long counts[3];
    double vn[2];
    CHECK(l.get_hist(counts, vn) == OK && counts[2] == 3 && vn[1] == 5 * is3d::sampler::kVnQuantum);
  }
  // ... a caller's list (is3d_decay_particles) is no PTMA sample; without bin an earlier histogram stays readable
  {
    SampledList d = decayed_form(false);
    l.replace_decayed(d, false);
    l.famod = false;
  }
  EXPECT(l, 4, OK, OK, OK, OK, OK, ST, OK);
  // ... until the bins change
  l.bins_changed();
  EXPECT(l, 4, OK, OK, OK, ST, OK, ST, OK);
  // ... and is3d_decay_particles on a fresh list leaves a list (of a call that sampled nothing)
  {
    SampledList fresh, d = decayed_form(false);
    fresh.replace_decayed(d, false);
    EXPECT(fresh, 4, OK, OK, OK, ST, OK, ST, OK);
  }

  // after a failed call: nothing is valid, whatever was there
  l.begin_sample();
  EXPECT(l, -1, ST, ST, ST, ST, ST, ST, ST);
  CHECK(!l.has_list());

  std::printf("ok %d checks\n", g_checks);
  return 0;
}
