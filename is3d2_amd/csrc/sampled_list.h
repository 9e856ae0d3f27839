// sampled_list.h -- the result of a sampler or list-decay call and the rules for reading it back: the one owner of
// what is3d_sample_count / _offsets, is3d_get_particles, is3d_get_particle_origins, is3d_get_sample_hist and the three
// stats getters return.  A one-device engine holds one (the list of its last call), a device-list engine's group holds
// one (the shards' lists merged).  Host only: no HIP headers, so the CPU tier compiles it with g++
// (tests/native/sampled_list_check.cpp).
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/is3d_amd.h"
#include "sampler_bins.h"

namespace is3d {

static_assert(sizeof(is3d_particle) == 96 && sizeof(sampler::Particle) == sizeof(is3d_particle),
              "is3d_particle is the sampler's 96-byte record");

struct SampledList {
  std::vector<sampler::Particle> particles;
  std::vector<long> offsets;            // [n_events + 1]: event k is particles [offsets[k], offsets[k + 1])
  std::vector<long> origins;            // a decayed list: the index, in the input list, of each record's primary
  // test_sampler = 1: the histogram in integer form, hist_nc counts, then hist_nv fixed-point vn sums
  std::vector<long long> hist;
  long hist_nc = 0, hist_nv = 0;
  is3d_sample_stats stats{};
  is3d_sample_famod_stats famod_stats{};   // is3d_sample_famod: the reconstruction counters of the last call
  is3d_decay_list_stats decay_stats{};
  // what is valid: a list (of a successful sample or decay call), made by is3d_sample_famod, with a histogram of the
  // current bins, replaced by its decayed form
  bool sampled = false, famod = false, binned = false, decayed = false;

  // ---- transitions ----
  // a sample call starts: nothing is valid until commit_sample (a failed call leaves nothing)
  void begin_sample() { sampled = famod = binned = decayed = false; }
  // ... and has succeeded with particles / offsets / stats (and hist, famod_stats) filled in
  void commit_sample(bool from_famod, bool with_hist) {
    sampled = true;
    famod = from_famod;
    binned = with_hist;
  }
  // is3d_set_sample_bins: a histogram of other bins is no longer readable; the list stays
  void bins_changed() { binned = false; }
  // the list replaced by a decayed one: d's particles, offsets, origins and decay stats and, with_hist, its histogram
  // (otherwise an earlier histogram stays); the sample stats and `famod` are the caller's
  void replace_decayed(SampledList& d, bool with_hist) {
    particles.swap(d.particles);
    offsets.swap(d.offsets);
    origins.swap(d.origins);
    decay_stats = d.decay_stats;
    if (with_hist) {
      hist.swap(d.hist);
      hist_nc = d.hist_nc; hist_nv = d.hist_nv;
      binned = true;
    }
    sampled = true;
    decayed = true;
  }
  // is3d_sample_decayed has succeeded (after begin_sample; stats and famod_stats are filled in): d holds the decay stats
  // and, with_list, the decayed list with its offsets and origins -- the state after a sample call and is3d_decay_sampled.
  // Without a list (binned only) the count and the offsets are zero and there is no origin to read, as after a
  // binned-only sample, while both stats are the true ones.  with_hist: d's histogram of the final hadrons
  void commit_sample_decayed(SampledList& d, bool from_famod, bool with_list, bool with_hist) {
    const size_t nev1 = d.offsets.size();
    if (!with_list) {
      d.particles.clear();
      d.origins.clear();
      d.offsets.assign(nev1, 0);
    }
    commit_sample(from_famod, false);
    replace_decayed(d, with_hist);
  }
  // is3d_decay_sampled's input: a binned-only call counted particles and kept none
  bool has_list() const { return sampled && !offsets.empty() && !(particles.empty() && stats.kept > 0); }

  // ---- getters: the bodies of the ABI's, after its null-engine check ----
  long count() const { return sampled ? (long)particles.size() : -1; }
  int get_offsets(long* out) const {
    if (!out) return IS3D_ERR_ARG;
    if (!sampled) return IS3D_ERR_STATE;
    std::copy(offsets.begin(), offsets.end(), out);
    return IS3D_OK;
  }
  int get_particles(long first, long n, is3d_particle* out) const {
    if (!out && n > 0) return IS3D_ERR_ARG;
    if (!sampled) return IS3D_ERR_STATE;
    if (first < 0 || n < 0 || first + n > (long)particles.size()) return IS3D_ERR_ARG;
    if (n > 0) std::memcpy(out, particles.data() + first, (size_t)n * sizeof(is3d_particle));
    return IS3D_OK;
  }
  int get_origins(long first, long n, long* out) const {
    if (!out && n > 0) return IS3D_ERR_ARG;
    if (!sampled || !decayed) return IS3D_ERR_STATE;
    if (first < 0 || n < 0 || first + n > (long)origins.size()) return IS3D_ERR_ARG;
    std::copy(origins.begin() + first, origins.begin() + first + n, out);
    return IS3D_OK;
  }
  int get_hist(long* counts, double* vn) const {
    if (!counts || !vn) return IS3D_ERR_ARG;
    if (!binned) return IS3D_ERR_STATE;
    for (long i = 0; i < hist_nc; i++) counts[i] = (long)hist[(size_t)i];
    for (long i = 0; i < hist_nv; i++) vn[i] = sampler::vn_value(hist[(size_t)(hist_nc + i)]);
    return IS3D_OK;
  }
  int get_stats(is3d_sample_stats* out) const {
    if (!out) return IS3D_ERR_ARG;
    if (!sampled) return IS3D_ERR_STATE;
    *out = stats;
    return IS3D_OK;
  }
  int get_famod_stats(is3d_sample_famod_stats* out) const {
    if (!out) return IS3D_ERR_ARG;
    if (!sampled || !famod) return IS3D_ERR_STATE;
    *out = famod_stats;
    return IS3D_OK;
  }
  int get_decay_stats(is3d_decay_list_stats* out) const {
    if (!out) return IS3D_ERR_ARG;
    if (!sampled || !decayed) return IS3D_ERR_STATE;
    *out = decay_stats;
    return IS3D_OK;
  }
};

}  // namespace is3d
