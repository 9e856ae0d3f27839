// decay_list.h -- private interface between engine_sample.hip and the Monte Carlo decays of a particle list (decay_list.hip).
//
// The method is in decay_mc_math.h.  The engine passes the list on the host and the plan's tables;
// decay_list.hip owns the working buffers of a call and returns the decayed list on the host.  The passes themselves
// are one shared stage over device-resident primaries (Stage): run() feeds it from an upload, is3d_sample_decayed
// from the sampler's compacted batches.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "decay_mc_math.h"
#include "devbuf.h"
#include "sampler_bins.h"

namespace is3d {
namespace decay_list {

using sampler::Particle;

// the plan's Monte Carlo tables on the device (one blob, move-only)
struct Tables {
  DevBuf<char> d;
  decay_mc::Table view{};
  int levels = 0;
};
std::string tables_build(Tables& t, const decay::Plan& P, const std::vector<double>& mass);

struct Config {
  uint64_t seed = 0;
  long sample_bytes = 0;             // bound on the working buffers of one batch
  const sampler::Bins* bins = nullptr;   // bin the final records into hist (device words the caller zeroed)
  unsigned long long* hist = nullptr;
};

struct Stats {
  long primaries = 0, decays = 0, undecayed = 0, dropped_daughters = 0, capped = 0, final_particles = 0, passes = 0,
       batches = 0;
  double ms_total = 0.0;
  long list_h2d = 0, list_d2h = 0;   // bytes of records, stream keys and origins copied to / from the device
};

enum Status : int { S_OK = 0, S_DEVICE = 1, S_BUDGET = 2 };

// what the bound counts: the upload of one primary (its record and stream key), and one working record in both
// ping-pong buffers with its count, position, final record and origin
constexpr long kPrimBytes = 96 + 4;
constexpr long kRecBytes = 2 * 112 + 12 + 96 + 8;

// n primaries on the device and where their stream keys (the index inside the event) come from: `prim` (uploaded), or
// the event bounds of a sampler batch (sample_decay_plan.h: bounds[nev + 1] on the device, `first` = the position of
// d[0] in the batch, `carry` of the batch's first event).  origin0: the origin of d[0]
struct Source {
  const Particle* d = nullptr;
  long n = 0, origin0 = 0;
  const uint32_t* prim = nullptr;
  const long* bounds = nullptr;
  long nev = 0, first = 0;
  uint64_t carry = 0;
};

// The shared decay stage: k_dl_count, scan and k_dl_emit per level of the plan, then k_dl_final, over one range of
// device-resident primaries.  It owns the working records of a call; they are grown on demand and kept from range to
// range.  Everything runs on the null stream.
class Stage {
 public:
  Stage();
  ~Stage();
  Stage(const Stage&) = delete;
  Stage& operator=(const Stage&) = delete;
  // One range.  fixed_bytes: what the caller holds on the device next to the stage's records; the range fits while
  // fixed_bytes + its records stay within c.sample_bytes.  S_BUDGET: it does not (need = the bound it would take;
  // nothing was binned, counted or written: decay a smaller range).  S_OK: `finals` records -- with keep_list in
  // out() / origin() on the device until the next call, without it only binned -- and st has the range's tallies,
  // device time and one more batch.
  int decay(const Tables& t, const Config& c, const Source& src, long fixed_bytes, bool keep_list, Stats& st, long& finals,
            long& need, std::string& msg);
  const Particle* out() const;
  const long* origin() const;

 private:
  struct Buffers;
  Buffers* b_;
};

// Decays in[0 .. n) down their chains.  prim[i]: the index of primary i inside its event (the stream key).  out: the
// final records, primaries in input order, each replaced by its leaves in depth-first daughter-slot order; origin[j]:
// the input index of the primary final record j descends from.
int run(const Tables& t, const Config& c, long n, const Particle* in, const uint32_t* prim, std::vector<Particle>& out,
        std::vector<long>& origin, Stats& st, std::string& msg);

// the event bounds of a sampler batch (sample_decay_plan.h) into d_bounds[nev + 1], on the null stream
hipError_t batch_bounds(const long* slots, const long* pos, long nev, long ncb, long* d_bounds);
// a range's finals from the stage to the end of out / origin, synchronously
int download(const Stage& S, long finals, std::vector<Particle>& out, std::vector<long>& origin, Stats& st, std::string& msg);
// the message of a primary whose products alone exceed the bound
std::string too_big_message(long primary, long need, long budget);

}  // namespace decay_list
}  // namespace is3d
