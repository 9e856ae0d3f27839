// sample_decay_plan_check.cpp -- CPU check of is3d2_amd/csrc/sample_decay_plan.h (the index and sub-range arithmetic
// of is3d_sample_decayed) and of the SampledList transition the call makes (sampled_list.h):
//   * the in-event index of every kept record of random sampler batches, computed as the device does -- from the
//     counts' exclusive sum (slots), the kept flags' exclusive sum (pos), the event bounds and the carry -- against a
//     brute-force loop that walks the candidates and counts; empty events, empty cells, events split over 2-5 windows;
//   * the 2^32 refusal with a carry just below the limit;
//   * the sub-range planner: every primary covered once, in order, no range above the bound's guess, whatever halves;
//   * the getter codes after commit_sample_decayed in the list and binned-only forms, and after a failed call.
// Built with -fsanitize=address,undefined by tests/test_sample_decay_plan_cpu.py; exit 0 and "ok" = every check held.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../is3d2_amd/csrc/sample_decay_plan.h"
#include "../../is3d2_amd/csrc/sampled_list.h"

using namespace is3d;

static long g_checks = 0;
#define CHECK(x)                                                              \
  do {                                                                        \
    g_checks++;                                                               \
    if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); std::exit(1); } \
  } while (0)

// one sampler batch as the device holds it after compaction
struct Batch {
  long nev = 0, ncb = 0;
  std::vector<int> counts, flags;    // [nev * ncb + 1] (trailing zero), [total + 1] (trailing zero)
  std::vector<long> slots, pos;      // their exclusive sums
  long total = 0, kept = 0;
};

static Batch make_batch(std::mt19937_64& rng, long nev, long ncb, double p_empty_event, double p_empty_cell, int max_count) {
  Batch b;
  b.nev = nev; b.ncb = ncb;
  std::uniform_real_distribution<double> u(0.0, 1.0);
  b.counts.assign((size_t)(nev * ncb) + 1, 0);
  for (long k = 0; k < nev; k++) {
    const bool empty = u(rng) < p_empty_event;
    for (long c = 0; c < ncb; c++)
      b.counts[(size_t)(k * ncb + c)] = (empty || u(rng) < p_empty_cell) ? 0 : (int)(rng() % (unsigned)(max_count + 1));
  }
  b.slots.assign(b.counts.size(), 0);
  for (size_t i = 1; i < b.counts.size(); i++) b.slots[i] = b.slots[i - 1] + b.counts[i - 1];
  b.total = b.slots.back();
  b.flags.assign((size_t)b.total + 1, 0);
  for (long i = 0; i < b.total; i++) b.flags[(size_t)i] = u(rng) < 0.6 ? 1 : 0;
  b.pos.assign(b.flags.size(), 0);
  for (size_t i = 1; i < b.flags.size(); i++) b.pos[i] = b.pos[i - 1] + b.flags[i - 1];
  b.kept = b.pos.back();
  return b;
}

// the bounds as k_dl_bounds computes them, and every record's index against the brute-force walk.  seen[e]: kept records
// of event e so far (over the windows before this batch): the brute-force carry
static void check_batch(const Batch& b, long e0, sdp::Carry& carry, std::vector<uint64_t>& seen) {
  std::vector<long> bounds((size_t)b.nev + 1);
  for (long k = 0; k <= b.nev; k++) bounds[(size_t)k] = sdp::event_first(b.slots.data(), b.pos.data(), k, b.ncb);
  CHECK(bounds[0] == 0 && bounds[(size_t)b.nev] == b.kept);
  const uint64_t cy = carry.before(e0, b.nev);
  // brute force: walk events, cells and candidates in the batch's order; a kept candidate is the next compacted record
  long rec = 0;
  for (long k = 0; k < b.nev; k++) {
    uint64_t in_event = seen[(size_t)(e0 + k)];
    long in_batch = 0;
    for (long c = 0; c < b.ncb; c++)
      for (int j = 0; j < b.counts[(size_t)(k * b.ncb + c)]; j++) {
        const long slot = b.slots[(size_t)(k * b.ncb + c)] + j;
        if (!b.flags[(size_t)slot]) continue;
        CHECK(b.pos[(size_t)slot] == rec);
        CHECK(sdp::event_of(bounds.data(), b.nev, rec) == k);
        CHECK(sdp::in_event_index(bounds.data(), b.nev, rec, cy) == in_event);
        rec++; in_event++; in_batch++;
      }
    CHECK(bounds[(size_t)k + 1] - bounds[(size_t)k] == in_batch);
    CHECK(sdp::event_fits(k == 0 ? cy : 0, in_batch));
    seen[(size_t)(e0 + k)] = in_event;
  }
  CHECK(rec == b.kept);
  carry.after(e0, b.nev, b.kept);
}

static void check_indices() {
  std::mt19937_64 rng(20240607);
  for (int round = 0; round < 60; round++) {
    // a call: whole-event batches and, here and there, one event split over 2-5 cell windows
    const long n_events = 1 + (long)(rng() % 40);
    std::vector<uint64_t> seen((size_t)n_events, 0);
    sdp::Carry carry;
    long e0 = 0;
    while (e0 < n_events) {
      const bool split = rng() % 3 == 0;
      if (split) {
        const int windows = 2 + (int)(rng() % 4);
        for (int w = 0; w < windows; w++) {
          const Batch b = make_batch(rng, 1, 1 + (long)(rng() % 9), w == 1 ? 1.0 : 0.1, 0.3, 6);   // window 1 keeps nothing
          check_batch(b, e0, carry, seen);
        }
        e0 += 1;
      } else {
        const long nev = 1 + (long)(rng() % (unsigned long)(n_events - e0));
        const Batch b = make_batch(rng, nev, 1 + (long)(rng() % 12), 0.3, 0.4, 5);
        check_batch(b, e0, carry, seen);
        e0 += nev;
      }
    }
  }
  // a batch with nothing kept, and a one-event batch after a split event of the same index never carries over
  sdp::Carry c;
  c.after(3, 1, 10);
  CHECK(c.before(3, 1) == 10 && c.before(4, 1) == 0 && c.before(3, 2) == 0);
  c.after(3, 1, 0);
  CHECK(c.before(3, 1) == 10);
  c.after(4, 1, 7);
  CHECK(c.before(4, 1) == 7 && c.before(3, 1) == 0);
  c.after(5, 4, 100);
  CHECK(c.before(5, 1) == 0 && c.before(8, 1) == 0);
}

static void check_limit() {
  // the key's high word holds an index below 2^32: an event may have 2^32 - 1 primaries... and one more is refused
  const uint64_t just_below = sdp::kEventLimit - 5;
  CHECK(sdp::event_fits(just_below, 5));
  CHECK(!sdp::event_fits(just_below, 6));
  CHECK(sdp::event_fits(0, 0xffffffffL) && !sdp::event_fits(0, 0x100000000L));
  CHECK(!sdp::event_fits(sdp::kEventLimit, 1) && sdp::event_fits(sdp::kEventLimit, 0));
  // the index of the last record that fits, with the carry, is the largest 32-bit value minus one... and it is exact
  const long bounds[2] = {0, 5};
  CHECK(sdp::in_event_index(bounds, 1, 4, just_below) == sdp::kEventLimit - 1);
  CHECK((sdp::in_event_index(bounds, 1, 4, just_below) << 32 >> 32) == sdp::kEventLimit - 1);
}

static void check_sub_ranges() {
  std::mt19937_64 rng(99);
  for (int round = 0; round < 2000; round++) {
    const long n = (long)(rng() % 5000);
    const long guess = sdp::first_guess((long)(rng() % 400000), (long)(rng() % 2 ? 100 : 0), 340);
    CHECK(guess >= 1);
    sdp::SubRanges R(n, guess);
    long next = 0, last_len = guess, steps = 0;
    bool refused = false;
    while (!R.done()) {
      CHECK(R.at == next && R.len >= 1 && R.len <= guess && R.at + R.len <= n);
      CHECK(R.len <= last_len);                       // a halved size is kept
      CHECK(++steps < 100000);
      if (rng() % 4 == 0) {                           // the range's records exceed the bound
        const long before = R.len;
        if (!R.halve()) { CHECK(before == 1); refused = true; break; }
        CHECK(R.len == before / 2 && R.at == next);   // the same primaries again, fewer of them
        last_len = R.len;
        continue;
      }
      next += R.len;
      last_len = R.len;
      R.accept();
    }
    CHECK(refused || next == n);
  }
  sdp::SubRanges none(0, 10);
  CHECK(none.done());
  CHECK(sdp::first_guess(1L << 30, 100, 340) == (1L << 30) / 1120 && sdp::first_guess(-5, 0, 340) == 1);
}

static void check_transition() {
  constexpr int OK = IS3D_OK, ST = IS3D_ERR_STATE, ARG = IS3D_ERR_ARG;
  auto decayed = [](SampledList& d, bool hist) {
    d.particles.assign(5, sampler::Particle{});
    d.origins = {0, 0, 1, 2, 2};
    d.offsets = {0, 3, 5};
    d.decay_stats.primaries = 3; d.decay_stats.final_particles = 5;
    if (hist) { d.hist.assign(4, 7); d.hist_nc = 3; d.hist_nv = 1; }
  };
  long off[3], org[5], counts[3];
  double vn[1];
  is3d_particle p[5];
  is3d_sample_stats s{};
  is3d_sample_famod_stats f{};
  is3d_decay_list_stats ds{};
  // list = 1, bin = 1 after an earlier binned-only sample
  SampledList l;
  l.begin_sample();
  l.stats.kept = 9;
  l.commit_sample(false, true);
  l.begin_sample();
  CHECK(l.count() == -1 && l.get_stats(&s) == ST && l.get_hist(counts, vn) == ST);
  l.stats.kept = 3;
  SampledList d;
  decayed(d, true);
  l.commit_sample_decayed(d, false, true, true);
  CHECK(l.count() == 5 && l.get_offsets(off) == OK && off[1] == 3 && off[2] == 5);
  CHECK(l.get_particles(0, 5, p) == OK && l.get_particles(0, 6, p) == ARG);
  CHECK(l.get_origins(0, 5, org) == OK && org[4] == 2 && l.get_origins(1, 5, org) == ARG);
  CHECK(l.get_hist(counts, vn) == OK && counts[2] == 7);
  CHECK(l.get_stats(&s) == OK && s.kept == 3 && l.get_decay_stats(&ds) == OK && ds.final_particles == 5);
  CHECK(l.get_famod_stats(&f) == ST && l.has_list());
  // list = 1, bin = 0 from the famod method: no histogram, the famod stats
  l.begin_sample();
  SampledList d2;
  decayed(d2, false);
  l.commit_sample_decayed(d2, true, true, false);
  CHECK(l.count() == 5 && l.get_hist(counts, vn) == ST && l.get_famod_stats(&f) == OK && l.get_decay_stats(&ds) == OK);
  // list = 0, bin = 1: the count and the offsets of a binned-only sample, the true stats, origins only for count = 0
  l.begin_sample();
  SampledList d3;
  decayed(d3, true);
  l.commit_sample_decayed(d3, false, false, true);
  off[1] = off[2] = -1;
  CHECK(l.count() == 0 && l.get_offsets(off) == OK && off[0] == 0 && off[1] == 0 && off[2] == 0);
  CHECK(l.get_particles(0, 0, p) == OK && l.get_particles(0, 1, p) == ARG);
  CHECK(l.get_origins(0, 0, org) == OK && l.get_origins(0, 1, org) == ARG);
  CHECK(l.get_hist(counts, vn) == OK && l.get_stats(&s) == OK && s.kept == 3);
  CHECK(l.get_decay_stats(&ds) == OK && ds.primaries == 3 && ds.final_particles == 5);
  CHECK(!l.has_list());                              // nothing for is3d_decay_sampled
  // a failed call: begin_sample and no commit
  l.begin_sample();
  CHECK(l.count() == -1 && l.get_offsets(off) == ST && l.get_particles(0, 0, p) == ST && l.get_origins(0, 0, org) == ST);
  CHECK(l.get_hist(counts, vn) == ST && l.get_stats(&s) == ST && l.get_decay_stats(&ds) == ST && l.get_famod_stats(&f) == ST);
  CHECK(!l.has_list());
}

int main() {
  check_indices();
  check_limit();
  check_sub_ranges();
  check_transition();
  std::printf("ok %ld checks\n", g_checks);
  return 0;
}
