// decay_list.h -- private interface between engine_sample.hip and the Monte Carlo decays of a particle list (decay_list.hip).
//
// The method is in decay_mc_math.h.  The engine passes the list on the host and the plan's tables;
// decay_list.hip owns the working buffers of a call and returns the decayed list on the host.
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
};

enum Status : int { S_OK = 0, S_DEVICE = 1, S_BUDGET = 2 };

// Decays in[0 .. n) down their chains.  prim[i]: the index of primary i inside its event (the stream key).  out: the
// final records, primaries in input order, each replaced by its leaves in depth-first daughter-slot order; origin[j]:
// the input index of the primary final record j descends from.
int run(const Tables& t, const Config& c, long n, const Particle* in, const uint32_t* prim, std::vector<Particle>& out,
        std::vector<long>& origin, Stats& st, std::string& msg);

}  // namespace decay_list
}  // namespace is3d
