// sampler.h -- private interface between engine_sample.hip and the operation = 2 particle sampler (sampler.hip).
//
// The GPU form of EmissionFunctionArray::sample_dN_pTdpTdphidy (ParticleSampler.cpp:638-1134; df_mode 1-4) and of
// sample_dN_pTdpTdphidy_famod (:1138-1627; df_mode 5, Config::sol).  The
// math, the random-number streams and the iteration caps are in sampler_math.h; the engine passes its surface and
// tables as plain pointers, sampler.hip owns the working buffers of a call and returns the list on the host.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "devbuf.h"
#include "sampler_bins.h"
#include "sampler_math.h"

namespace is3d {
namespace sampler {

// chosen species in their original order (the species draw follows the reference's discrete_distribution order)
struct Tables {
  DevBuf<double> d;                // the blob the views below point into (move-only)
  int npart = 0;
  const double *mass = nullptr, *sign = nullptr, *degen = nullptr, *baryon = nullptr;
};
std::string tables_build(Tables& t, const std::vector<double>& mass, const std::vector<double>& sign,
                         const std::vector<double>& degen, const std::vector<double>& baryon);

struct Config {
  Run run;
  DfTables tb;
  const double* surf = nullptr;    // [25][n] field-major
  // df_mode 5 (sample_dN_pTdpTdphidy_famod): [6][n] rows (lambda, aT, aL, broken, beta_pi_perp, beta_W_perp) of the
  // Newton prepass under the sampler's chain rule (device); null for df_mode 1-4
  const double* sol = nullptr;
  long n = 0, lo = 0, hi = 0;      // cells held and the window [lo, hi) sampled
  long cell_base = 0;              // global index of held cell 0 (a shard of a device-list engine)
  uint64_t seed = 0;
  long n_events = 1;
  const double* dens = nullptr;    // fast = 1: [3][npart] Plasma-average densities (device)
  long sample_bytes = 0;           // bound on the working buffers of one batch
  const char* bound_note = "";     // appended to the message of a batch that cannot fit (a caller that passes a share)
  // test_sampler = 1: kept particles are also binned into hist (device, hist_counts + hist_vn 8-byte words that the
  // caller zeroed; the vn words in their integer form).  keep_list = false: binned only -- no candidate slots, no
  // compaction and no list; a batch then costs only its (event, cell) counts.
  const Bins* bins = nullptr;
  unsigned long long* hist = nullptr;
  bool keep_list = true;
};

struct Stats {
  long cells = 0, breakdown = 0, candidates = 0, kept = 0, proposals = 0, acceptances = 0, capped = 0, clamped = 0,
       batches = 0;
  long list_d2h = 0;     // bytes of particle records copied to the host
};

enum Status : int { S_OK = 0, S_DEVICE = 1, S_DF = 2, S_BUDGET = 3 };

// One compacted batch on the device, as its consumer sees it on the null stream right after k_compact: the kept
// particles of events [e0, e0 + nev) over cells [c0, c1) (held-surface indices; nev = 1 when the window is a part of
// the call's), events contiguous.  slots / pos: the two exclusive sums of sample_decay_plan.h (device), and
// batch_bytes: what the sampler's pair and candidate buffers of this batch hold.  All of it is valid until the
// consumer returns.
struct Batch {
  const Particle* d = nullptr;
  long kept = 0, e0 = 0, nev = 0, c0 = 0, c1 = 0;
  const long *slots = nullptr, *pos = nullptr;
  long batch_bytes = 0;
};
// returns a Status (S_OK to go on); msg says what went wrong otherwise
using Consumer = std::function<int(const Batch&, std::string& msg)>;

// Samples n_events events of the window.  parts: kept particles, events contiguous, ordered by (cell, candidate)
// within an event (the reference's loop order); offsets: n_events + 1 (a binned-only call leaves parts empty and the
// offsets zero; st.kept and st.candidates then come from device tallies).  Returns a Status; S_DF: df_err holds the
// DfErr; msg says what went wrong otherwise.
int run(const Tables& t, const Config& c, std::vector<Particle>& parts, std::vector<long>& offsets, Stats& st,
        int& df_err, std::string& msg);

// The same with every compacted batch that kept something handed to `consume` instead of the host list (the list
// form above is the consumer that downloads it).  st.kept is the sum of the batches'; binned-only calls have no batches.
int run(const Tables& t, const Config& c, const Consumer& consume, Stats& st, int& df_err, std::string& msg);

// test hook: the first n uniforms of stream (seed, purpose, cell, event, candidate), generated on the device
hipError_t uniforms(uint64_t seed, int purpose, long cell, long event, long candidate, int n, double* host_out);

}  // namespace sampler
}  // namespace is3d
