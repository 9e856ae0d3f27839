// sample_decay_plan.h -- the index and sub-range arithmetic that joins the sampler's compacted batches to the list
// decays (is3d_sample_decayed).  Host + device, no HIP header: sampler.hip and decay_list.hip use it in
// kernels and on the host, and the CPU tier compiles it with g++ (tests/native/sample_decay_plan_check.cpp).
//
// A sampler batch holds events [e0, e0 + nev) over the cells [c0, c1) of the window, ncb = c1 - c0.  Its (event, cell)
// pairs are event-major (k_count: pair = k * ncb + cell), slots is the exclusive sum of the pairs' candidate counts and
// pos the exclusive sum of the candidates' kept flags, so the kept records of batch event k are the compacted records
// [pos[slots[k * ncb]], pos[slots[(k + 1) * ncb]]): `bounds`, nev + 1 longs.  A decay's stream key is the primary's
// index inside its event: the position in that range, plus -- while one event is sampled in several cell windows (the
// planner's nev = 1 batches) -- the kept count of the event's earlier windows, the carry.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IS3D_SDP_HD __host__ __device__ inline
#else
#define IS3D_SDP_HD inline
#endif

namespace is3d {
namespace sdp {

constexpr uint64_t kEventLimit = 0xffffffffull;   // an event holds at most 2^32 - 1 primaries (the key's high word)

// bounds[k], k = 0 .. nev: the first compacted record of batch event k (k = nev: the batch's kept count).  slots has
// nev * ncb + 1 entries (the last is the candidate total) and pos one more than that total
IS3D_SDP_HD long event_first(const long* slots, const long* pos, long k, long ncb) { return pos[slots[k * ncb]]; }

// the batch event that holds compacted record i: the last k with bounds[k] <= i (empty events share a bound and are
// skipped, as are empty cells inside an event); 0 <= i < bounds[nev]
IS3D_SDP_HD long event_of(const long* bounds, long nev, long i) {
  long lo = 0, hi = nev - 1;
  while (lo < hi) {
    const long mid = (lo + hi + 1) >> 1;
    if (bounds[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// the stream key's high word of compacted record i: its index inside its event.  carry belongs to the batch's first
// event (it is non-zero only when nev = 1)
IS3D_SDP_HD uint64_t in_event_index(const long* bounds, long nev, long i, uint64_t carry) {
  const long k = event_of(bounds, nev, i);
  return (uint64_t)(i - bounds[k]) + (k == 0 ? carry : 0ull);
}

// the carry from batch to batch.  before(): the carry of the batch about to be decayed; after(): the batch kept `kept`
struct Carry {
  long event = -1;        // the event whose windows are being summed
  uint64_t kept = 0;
  uint64_t before(long e0, long nev) const { return (nev == 1 && e0 == event) ? kept : 0ull; }
  void after(long e0, long nev, long n) {
    if (nev != 1) { event = -1; kept = 0; return; }
    if (e0 != event) { event = e0; kept = 0; }
    kept += (uint64_t)n;
  }
};

// an event of `count` more primaries after `carry` earlier ones still fits the key: the 2^32 refusal of the list decays
inline bool event_fits(uint64_t carry, long count) { return carry + (uint64_t)count <= kEventLimit; }

// The sub-ranges in which a list of n device- or host-resident primaries is decayed: [at, at + len) with len <= the
// first guess, halved when a range's passes show that its records exceed the bound (the primaries are decayed again,
// never sampled again), and kept at that size for the ranges that follow.  done(): every primary covered once, in order
struct SubRanges {
  long n = 0, at = 0, len = 0;
  SubRanges(long n_, long first_guess) : n(n_), at(0), len(first_guess < 1 ? 1 : first_guess) { clip(); }
  bool done() const { return at >= n; }
  bool halve() {            // false: one primary alone does not fit
    if (len <= 1) return false;
    len /= 2;
    return true;
  }
  void accept() { at += len; clip(); }
 private:
  void clip() { if (len > n - at && n - at > 0) len = n - at; }
};

// first guess of a range: three final records per primary, of `rec_bytes` each, next to `prim_bytes` per primary
inline long first_guess(long budget, long prim_bytes, long rec_bytes) {
  const long g = budget / (prim_bytes + 3 * rec_bytes);
  return g < 1 ? 1 : (g > 0x3ffffff0L ? 0x3ffffff0L : g);
}

}  // namespace sdp
}  // namespace is3d
