// decay_list.hip -- Monte Carlo resonance decays of a sampled particle list on gfx950 (decay_mc_math.h).
//
// Every decay is a pure function of (seed, primary's index in its event, event, path code), so the decayed list does
// not depend on the batches below.  A batch of primaries is uploaded and expanded in place, one pass per level of the
// plan (after pass l no species of a level <= l can appear again):
//   k_dl_init    one thread per primary: the working record (the 96-byte particle, origin, stream key) from the upload
//   k_dl_init_batch  the same from a sampler's compacted batch on the device: the key from the batch's event bounds
//                (k_dl_bounds, sample_decay_plan.h), nothing uploaded (is3d_sample_decayed)
//   per pass:
//   k_dl_count   one thread per working record: the channel draw (and a 3-body channel's s23 or a 4-body channel's
//                (M234, M34) rejection loop, which decides whether the decay is capped) -> the number of records the
//                particle becomes
//   scan         exclusive sum: every record's position after the pass
//   k_dl_emit    redraws the channel from the reopened stream, does the kinematics and writes the daughters at the
//                scanned position; a record that does not decay in this pass is copied
//   k_dl_final   the records as is3d_particle + origin; BIN: also binned (sampler_bins.h) into the call's histogram;
//                the form that only bins writes no record
// Expansion in place keeps the order for free: primaries in input order, each replaced by its leaves in depth-first
// daughter-slot order.  The records ping-pong between two buffers.  Nothing appends with atomics; the only atomics
// are the 64-bit integer tallies and the histogram adds, so the histogram is the same bits for every batching.
#include "decay_list.h"
#include "sample_decay_plan.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>

namespace is3d {
namespace decay_list {

namespace {

using decay_mc::Chan;
using decay_mc::Table;

constexpr int kBlock = 256;

// the working record: 112 bytes.  key = index of the primary inside its event << 32 | path code
struct Rec {
  Particle p;
  long origin;
  unsigned long long key;
};
static_assert(sizeof(Rec) == 112, "working record");

static_assert(kPrimBytes == sizeof(Particle) + sizeof(uint32_t), "the upload of one primary");
static_assert(kRecBytes == 2 * sizeof(Rec) + 12 + sizeof(Particle) + sizeof(long), "both buffers, count + position, the output");

struct Args {
  Table T;
  unsigned long long seed;
  int pass;
  long n, total;                 // records before the pass, records after it
  const Rec* in;
  Rec* out;
  int* counts;                   // [n] (+ 1 trailing zero)
  const long* pos;               // exclusive sum of counts
  unsigned long long* tally;     // decays, undecayed, dropped daughters, capped
};

__global__ __launch_bounds__(kBlock) void k_dl_init(const Particle* in, const uint32_t* prim, long n, long origin0, Rec* out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Rec r;
  r.p = in[i];
  r.origin = origin0 + i;
  r.key = (unsigned long long)prim[i] << 32;
  out[i] = r;
}

__global__ __launch_bounds__(kBlock) void k_dl_count(Args A) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const int sp = A.in[i].p.species, ev = A.in[i].p.event;
  const unsigned long long key = A.in[i].key;
  decay_mc::Stream s;
  int q = -1;
  double wa = 0.0, wb = 0.0;
  const int oc = decay_mc::node_choice(A.T, sp, A.pass, A.seed, (long)(key >> 32), (long)ev, (long)(key & 0xffffffffull), s, &q, &wa, &wb);
  A.counts[i] = decay_mc::node_count(A.T, oc, q);
}

__global__ __launch_bounds__(kBlock) void k_dl_emit(Args A) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const Rec& r = A.in[i];                  // read in place: the pass writes the other buffer
  const unsigned long long path = r.key & 0xffffffffull;
  long at = A.pos[i];
  decay_mc::Tally t{0, 0, 0, 0};
  decay_mc::decay_node(A.T, A.pass, A.seed, r.p, (long)(r.key >> 32), (long)path, t, [&](int slot, const decay_mc::Mom& m) __attribute__((always_inline)) {
    if (at >= A.total) return;             // the count kernel drew the same numbers: never taken, and never a write outside
    Rec* o = A.out + at++;
    o->p = r.p;
    if (slot >= 0) decay_mc::apply(o->p, m);
    o->origin = r.origin;
    o->key = slot < 0 ? r.key : ((r.key & ~0xffffffffull) | (4ull * path + (unsigned long long)slot + 1ull));
  });
  if (t.decays) atomicAdd(&A.tally[0], (unsigned long long)t.decays);
  if (t.undecayed) atomicAdd(&A.tally[1], (unsigned long long)t.undecayed);
  if (t.dropped) atomicAdd(&A.tally[2], (unsigned long long)t.dropped);
  if (t.capped) atomicAdd(&A.tally[3], (unsigned long long)t.capped);
}

// the working records straight from a sampler's compacted batch: the key's high word from the batch's event bounds
__global__ __launch_bounds__(kBlock) void k_dl_init_batch(const Particle* in, long n, long origin0, const long* bounds, long nev,
                                                          long first, unsigned long long carry, Rec* out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Rec r;
  r.p = in[i];
  r.origin = origin0 + i;
  r.key = (unsigned long long)sdp::in_event_index(bounds, nev, first + i, carry) << 32;
  out[i] = r;
}

__global__ __launch_bounds__(kBlock) void k_dl_bounds(const long* slots, const long* pos, long nev, long ncb, long* bounds) {
  const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k <= nev) bounds[k] = sdp::event_first(slots, pos, k, ncb);
}

// LIST: the records as is3d_particle + origin; BIN: binned into the call's histogram (alone: nothing is written)
template <bool LIST, bool BIN>
__global__ __launch_bounds__(kBlock) void k_dl_final(const Rec* in, long n, Particle* out, long* origin, sampler::Bins bins,
                                                     int npart, unsigned long long* hist) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Particle p = in[i].p;
  if (LIST) {
    out[i] = p;
    origin[i] = in[i].origin;
  }
  if (BIN) {
    const sampler::Landing l = sampler::bin_particle(bins, sampler::particle_rapidity(3, 0.0, p.E, p.pz), p.eta, p.px, p.py, p.tau, p.x, p.y);
    sampler::hist_accumulate(bins, npart, p.species, l, [hist](long word, long long v) { atomicAdd(hist + word, (unsigned long long)v); });
  }
}

struct ToLong {
  __host__ __device__ long operator()(int v) const { return (long)v; }
};

// exclusive sum of in[0 .. n) (ints) into out (longs); in[n - 1] is the caller's trailing zero, so out[n - 1] = total
hipError_t scan(const int* in, long* out, long n, DevBuf<char>& tmp) {
  hipcub::TransformInputIterator<long, ToLong, const int*> it(in, ToLong());
  size_t need = 0;
  hipError_t h = hipcub::DeviceScan::ExclusiveSum(nullptr, need, it, out, (int)n, (hipStream_t) nullptr);
  if (h != hipSuccess) return h;
  if (!tmp.reserve((long)need)) return hipErrorOutOfMemory;
  return hipcub::DeviceScan::ExclusiveSum(tmp.get(), need, it, out, (int)n, (hipStream_t) nullptr);
}

hipError_t alloc(bool ok) { return ok ? hipSuccess : hipErrorOutOfMemory; }

unsigned blocks(long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

std::string tables_build(Tables& t, const decay::Plan& P, const std::vector<double>& mass) {
  t = Tables{};
  const int np = (int)mass.size();
  const decay_mc::HostTable H = decay_mc::make_table(P, np, mass.data());
  // doubles first, then the channels (8-byte aligned), then the ints
  const size_t o_mass = 0, o_ch = o_mass + (size_t)np * sizeof(double), o_first = o_ch + H.ch.size() * sizeof(Chan),
               o_level = o_first + (size_t)(np + 1) * sizeof(int), bytes = o_level + (size_t)np * sizeof(int);
  static_assert(sizeof(Chan) % 8 == 0, "blob layout");
  std::vector<char> h(bytes + 8, 0);
  std::memcpy(h.data() + o_mass, H.mass.data(), (size_t)np * sizeof(double));
  if (!H.ch.empty()) std::memcpy(h.data() + o_ch, H.ch.data(), H.ch.size() * sizeof(Chan));
  std::memcpy(h.data() + o_first, H.first.data(), (size_t)(np + 1) * sizeof(int));
  std::memcpy(h.data() + o_level, H.level.data(), (size_t)np * sizeof(int));
  if (!t.d.reserve((long)h.size()) || hipMemcpy(t.d.get(), h.data(), h.size(), hipMemcpyHostToDevice) != hipSuccess) {
    t = Tables{};
    return "hipMalloc / upload of the decay tables failed";
  }
  const char* d = t.d.get();
  t.view = Table{(const int*)(d + o_first), (const int*)(d + o_level), (const double*)(d + o_mass), (const Chan*)(d + o_ch), np};
  t.levels = P.levels();
  return "";
}

hipError_t batch_bounds(const long* slots, const long* pos, long nev, long ncb, long* d_bounds) {
  hipLaunchKernelGGL(k_dl_bounds, dim3(blocks(nev + 1)), dim3(kBlock), 0, 0, slots, pos, nev, ncb, d_bounds);
  return hipGetLastError();
}

struct Stage::Buffers {
  DevBuf<Rec> rec[2];
  DevBuf<int> counts;
  DevBuf<long> pos, origin;
  DevBuf<Particle> out;
  DevBuf<unsigned long long> tally;
  DevBuf<char> tmp;
  DevEvent ev0, ev1;
};

Stage::Stage() : b_(new Buffers()) {}
Stage::~Stage() { delete b_; }
const Particle* Stage::out() const { return b_->out.get(); }
const long* Stage::origin() const { return b_->origin.get(); }

int Stage::decay(const Tables& t, const Config& c, const Source& src, long fixed_bytes, bool keep_list, Stats& st,
                 long& finals, long& need, std::string& msg) {
  finals = 0;
  need = 0;
  Buffers& B = *b_;
  const long nb = src.n;
  if (nb <= 0) return S_OK;
#define DCHK(x)                                                                       \
  do {                                                                                \
    const hipError_t h_ = (x);                                                        \
    if (h_ != hipSuccess) { msg = std::string(#x) + ": " + hipGetErrorString(h_); return S_DEVICE; } \
  } while (0)
  if (!B.ev0) DCHK(B.ev0.create(hipEventDefault));
  if (!B.ev1) DCHK(B.ev1.create(hipEventDefault));
  DCHK(alloc(B.tally.reserve(4) && B.rec[0].reserve(nb)));
  const long budget = std::max(c.sample_bytes, 1L);
  Args A{};
  A.T = t.view; A.seed = c.seed; A.tally = B.tally.get();
  DCHK(hipEventRecord(B.ev0.get(), nullptr));
  DCHK(hipMemsetAsync(B.tally.get(), 0, 4 * sizeof(unsigned long long), nullptr));
  if (src.prim) hipLaunchKernelGGL(k_dl_init, dim3(blocks(nb)), dim3(kBlock), 0, 0, src.d, src.prim, nb, src.origin0, B.rec[0].get());
  else hipLaunchKernelGGL(k_dl_init_batch, dim3(blocks(nb)), dim3(kBlock), 0, 0, src.d, nb, src.origin0, src.bounds, src.nev, src.first, (unsigned long long)src.carry, B.rec[0].get());
  DCHK(hipGetLastError());
  long cur = nb;
  int from = 0;
  bool too_big = false;
  for (int pass = 0; pass < t.levels && cur > 0; pass++) {     // cur = 0: every daughter was dropped
    DCHK(alloc(B.counts.reserve(cur + 1) && B.pos.reserve(cur + 1)));
    DCHK(hipMemsetAsync(B.counts.get() + cur, 0, sizeof(int), nullptr));
    A.pass = pass; A.n = cur; A.in = B.rec[from].get(); A.counts = B.counts.get(); A.pos = B.pos.get();
    hipLaunchKernelGGL(k_dl_count, dim3(blocks(cur)), dim3(kBlock), 0, 0, A);
    DCHK(hipGetLastError());
    DCHK(scan(B.counts.get(), B.pos.get(), cur + 1, B.tmp));
    long total = 0;
    DCHK(hipMemcpy(&total, B.pos.get() + cur, sizeof(long), hipMemcpyDeviceToHost));
    need = fixed_bytes + std::max(cur, total) * kRecBytes;
    if (need > budget || total + 1 >= 0x7fffffffL) { too_big = true; break; }
    DCHK(alloc(B.rec[1 - from].reserve(total)));
    A.total = total; A.out = B.rec[1 - from].get();
    hipLaunchKernelGGL(k_dl_emit, dim3(blocks(cur)), dim3(kBlock), 0, 0, A);
    DCHK(hipGetLastError());
    from = 1 - from;
    cur = total;
  }
  if (t.levels == 0) { need = fixed_bytes + cur * kRecBytes; too_big = need > budget; }
  if (!too_big && cur > 0) {
    const Rec* r = B.rec[from].get();
    const sampler::Bins bins = c.bins ? *c.bins : sampler::Bins{};
    if (keep_list) {
      DCHK(alloc(B.out.reserve(cur) && B.origin.reserve(cur)));
      if (c.bins) hipLaunchKernelGGL((k_dl_final<true, true>), dim3(blocks(cur)), dim3(kBlock), 0, 0, r, cur, B.out.get(), B.origin.get(), bins, t.view.npart, c.hist);
      else hipLaunchKernelGGL((k_dl_final<true, false>), dim3(blocks(cur)), dim3(kBlock), 0, 0, r, cur, B.out.get(), B.origin.get(), bins, t.view.npart, c.hist);
    } else if (c.bins) {
      hipLaunchKernelGGL((k_dl_final<false, true>), dim3(blocks(cur)), dim3(kBlock), 0, 0, r, cur, (Particle*)nullptr, (long*)nullptr, bins, t.view.npart, c.hist);
    }
    DCHK(hipGetLastError());
  }
  // the device time of an attempt that was too big counts too: the work was done
  DCHK(hipEventRecord(B.ev1.get(), nullptr));
  DCHK(hipEventSynchronize(B.ev1.get()));
  float ms = 0.0f;
  DCHK(hipEventElapsedTime(&ms, B.ev0.get(), B.ev1.get()));
  st.ms_total += ms;
  if (too_big) return S_BUDGET;
  unsigned long long tl[4] = {0};
  DCHK(hipMemcpy(tl, B.tally.get(), sizeof(tl), hipMemcpyDeviceToHost));
#undef DCHK
  st.decays += (long)tl[0]; st.undecayed += (long)tl[1]; st.dropped_daughters += (long)tl[2]; st.capped += (long)tl[3];
  st.final_particles += cur;
  st.batches++;
  finals = cur;
  return S_OK;
}

std::string too_big_message(long primary, long need, long budget) {
  return "primary " + std::to_string(primary) + " alone needs " + std::to_string(need) +
         " bytes for its decay products: more than the \"sample_bytes\" bound of " + std::to_string(budget) +
         "; raise it with is3d_set_tuning";
}

int download(const Stage& S, long finals, std::vector<Particle>& out, std::vector<long>& origin, Stats& st, std::string& msg) {
  if (finals <= 0) return S_OK;
  const size_t at = out.size();
  out.resize(at + (size_t)finals);
  origin.resize(at + (size_t)finals);
  hipError_t h = hipMemcpy(out.data() + at, S.out(), (size_t)finals * sizeof(Particle), hipMemcpyDeviceToHost);
  if (h == hipSuccess) h = hipMemcpy(origin.data() + at, S.origin(), (size_t)finals * sizeof(long), hipMemcpyDeviceToHost);
  if (h != hipSuccess) { msg = std::string("download of the decayed records: ") + hipGetErrorString(h); return S_DEVICE; }
  st.list_d2h += finals * (long)(sizeof(Particle) + sizeof(long));
  return S_OK;
}

// the input stage of a host list: each sub-range is uploaded (again after a halving) and handed to the shared stage
int run(const Tables& t, const Config& c, long n, const Particle* in, const uint32_t* prim, std::vector<Particle>& out,
        std::vector<long>& origin, Stats& st, std::string& msg) {
  out.clear();
  origin.clear();
  st = Stats{};
  st.primaries = n;
  st.passes = t.levels;
  if (n <= 0) return S_OK;
  DevBuf<Particle> d_in;
  DevBuf<uint32_t> d_prim;
  Stage S;
  const long budget = std::max(c.sample_bytes, 1L);
  sdp::SubRanges R(n, sdp::first_guess(budget, kPrimBytes, kRecBytes));
  while (!R.done()) {
    const long i0 = R.at, nb = R.len;
    hipError_t h = alloc(d_in.reserve(nb) && d_prim.reserve(nb));
    if (h == hipSuccess) h = hipMemcpy(d_in.get(), in + i0, (size_t)nb * sizeof(Particle), hipMemcpyHostToDevice);
    if (h == hipSuccess) h = hipMemcpy(d_prim.get(), prim + i0, (size_t)nb * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (h != hipSuccess) { msg = std::string("upload of the primaries: ") + hipGetErrorString(h); return S_DEVICE; }
    st.list_h2d += nb * kPrimBytes;
    Source src;
    src.d = d_in.get(); src.n = nb; src.origin0 = i0; src.prim = d_prim.get();
    long finals = 0, need = 0;
    int s = S.decay(t, c, src, nb * kPrimBytes, true, st, finals, need, msg);
    if (s == S_BUDGET) {
      if (R.halve()) continue;
      msg = too_big_message(i0, need, budget);
      return S_BUDGET;
    }
    if (s == S_OK) s = download(S, finals, out, origin, st, msg);
    if (s != S_OK) return s;
    R.accept();
  }
  return S_OK;
}

}  // namespace decay_list
}  // namespace is3d
