// sampler.hip -- operation = 2 particle sampler on gfx950.
//
// GPU form of EmissionFunctionArray::sample_dN_pTdpTdphidy (ParticleSampler.cpp:638-1134, df_mode 1-4) and, as
// compile-time variants of k_cells and k_sample, of sample_dN_pTdpTdphidy_famod (:1138-1627, df_mode 5: the cells'
// (lambda, aT, aL) come from the engine's Newton prepass, Config::sol); the math and the
// counter-based random streams are in sampler_math.h.  Every draw is a pure function of (seed, purpose, global cell,
// event, candidate, draw counter), so the list below is the same for every launch geometry, event batch, cell window
// and shard count, and its order -- events contiguous, (cell, candidate) inside an event -- is the reference's loop
// order without a sort:
//
//   k_cells     one wavefront per cell, once per call: the cell prologue (lane 0), the species weights dn_list (lanes
//               over species, fast = 0: 32-point thermal sums each), their sum in species order -> Cell record, dn_tot
//   per batch of events (and, when one event alone exceeds the memory bound, of cells):
//   k_count     one thread per (event, cell): N ~ Poisson(dn_tot) from the poisson stream
//   scan        exclusive sum of N over (event, cell): every candidate's slot
//   k_sample    one wavefront per cell with candidates in the batch: rebuilds dn_list and its running sum in LDS, then
//               the lanes take the cell's (event, candidate) pairs 64 at a time -- species draw, sample_momentum,
//               delta-f / flux weights, keep draw, lab boost -- and write kept particles and a flag into their slots
//   scan + k_compact   stable compaction of the kept slots; the batch is copied to the host list
//
// test_sampler = 1 (Config::bins): k_sample also bins every kept particle (sampler_bins.h) straight from its registers
// into the call's histogram with no-return 64-bit integer atomics from the lanes -- counts, and the vn sums in
// fixed point, so the histogram is the same bits for every batch, window, geometry and shard.  A binned-only call
// (keep_list = false) runs k_count and the k_sample variant that writes no slot, and nothing else: no slot scan, no
// flags, no compaction, no copy; its batches are sized by their (event, cell) counts alone, and the candidate and kept
// totals are device tallies.
//
// Nothing here appends with atomics; the only atomics are the integer tallies of the stats and the histogram adds.
#include "sampler.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>

namespace is3d {
namespace sampler {

namespace {

constexpr int kWave = 64;
constexpr size_t kCellLds = (sizeof(Cell) + 15) / 16 * 16;
constexpr size_t kPreLds = ((kWave + 1) * sizeof(long) + 15) / 16 * 16;
constexpr long kPairBytes = 12;         // count + slot offset of one (event, cell)
constexpr long kCandBytes = 2 * sizeof(Particle) + 12;   // slot + compacted copy + flag + position

struct Args {
  Run run;
  DfTables tb;
  const double* surf;
  long n, lo, hi, cell_base;
  unsigned long long seed;
  const double *mass, *sign, *degen, *baryon, *dens;
  int npart;
  Cell* cells;          // [hi - lo]
  double* dn;           // [hi - lo]
  int* err;
  unsigned long long* tally;   // breakdown, proposals, acceptances, capped, clamped, poisson capped
  // batch
  long e0, nev, c0, c1;        // events [e0, e0 + nev), cells [c0, c1)
  int* counts;                 // [nev][c1 - c0] (+ 1 trailing zero)
  const long* slots;           // exclusive sum of counts
  Particle* cand;
  int* flags;
  // binned distributions
  Bins bins;
  unsigned long long* hist;
  const double* sol;    // famod: [6][n] rows of the Newton prepass (Config::sol)
};

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
  return v;
}

// species weights of cell c into w[npart] (lanes over species), then lane 0: the plain sum (returned to every lane
// through w's owner) and, when cumulative, the running sum of max(w, 0) in place
template <bool FAMOD>
__device__ double species_list(const Args& A, const Cell& c, double* w, bool cumulative) {
  const int lane = threadIdx.x;
  for (int s = lane; s < A.npart; s += kWave) {
    if (FAMOD) w[s] = species_weight_famod(A.run, c, A.mass[s], A.degen[s], A.sign[s], A.baryon[s]);
    else w[s] = A.run.fast ? species_weight_fast(A.run, c, A.dens[s], A.dens[A.npart + s])
                      : species_weight(A.run, c, A.mass[s], A.degen[s], A.sign[s], A.baryon[s]);
  }
  __syncthreads();
  double sum = 0.0;
  if (lane == 0) {
    double run = 0.0;
    for (int s = 0; s < A.npart; s++) {
      const double v = w[s];
      sum += v;
      if (cumulative) { run += v > 0.0 ? v : 0.0; w[s] = run; }
    }
  }
  __syncthreads();
  return sum;     // lane 0 only
}

// FAMOD: the df_mode 5 prologue from the surface and the cell's row of the Newton prepass; it has no df tables to fail
template <bool FAMOD>
__global__ __launch_bounds__(kWave) void k_cells(Args A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Cell& sc = *reinterpret_cast<Cell*>(smem);
  int* serr = reinterpret_cast<int*>(smem + kCellLds);
  double* w = reinterpret_cast<double*>(smem + kCellLds + kPreLds);
  const long ci = blockIdx.x, cell = A.lo + ci;
  const int lane = threadIdx.x;
  if (lane == 0) {
    double s[NSURF];
    for (int f = 0; f < NSURF; f++) s[f] = A.surf[(long)f * A.n + cell];
    if (FAMOD) {
      double sol[6];
      for (int f = 0; f < 6; f++) sol[f] = A.sol[(long)f * A.n + cell];
      cell_setup_famod(A.run, s, sol, sc);
      *serr = 0;
    } else {
      *serr = cell_setup(A.run, A.tb, s, sc);
    }
    if (*serr) { atomicMax(A.err, *serr); sc.live = 0.0; }
  }
  __syncthreads();
  if (sc.live == 0.0) {           // uniform: every lane reads the same LDS word
    if (lane == 0) { A.cells[ci] = sc; A.dn[ci] = 0.0; }
    return;
  }
  const double sum = species_list<FAMOD>(A, sc, w, false);
  if (lane == 0) {
    cell_finish(A.run, sc, sum);
    if (sc.live != 0.0 && sc.breaks != 0.0) atomicAdd(&A.tally[0], 1ull);
    A.cells[ci] = sc;
    A.dn[ci] = sc.dn_tot;
  }
}

__global__ __launch_bounds__(256) void k_count(Args A) {
  const long ncb = A.c1 - A.c0;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.nev * ncb) return;
  const long ev = A.e0 + i / ncb, cell = A.c0 + i % ncb;
  const double mean = A.dn[cell - A.lo];
  int n = 0;
  if (mean > 0.0) {
    Stream s = stream_open(A.seed, P_POISSON, A.cell_base + cell, ev, 0);
    int capped = 0;
    const long v = poisson_draw(s, mean, &capped);
    n = (int)(v < 0x7fffffffL ? v : 0x7fffffffL);
    if (capped || v >= 0x7fffffffL) atomicAdd(&A.tally[5], 1ull);
  }
  A.counts[i] = n;
}

// LIST: kept particles and flags go to their slots; BIN: kept particles are binned into A.hist; FAMOD: the df_mode 5
// species weights and candidate
template <bool LIST, bool BIN, bool FAMOD = false>
__global__ __launch_bounds__(kWave) void k_sample(Args A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Cell& sc = *reinterpret_cast<Cell*>(smem);
  long* pre = reinterpret_cast<long*>(smem + kCellLds);
  double* cum = reinterpret_cast<double*>(smem + kCellLds + kPreLds);
  const long ncb = A.c1 - A.c0, ci = blockIdx.x, cell = A.c0 + ci;
  const int lane = threadIdx.x;
  if (A.dn[cell - A.lo] <= 0.0) return;
  int any = 0;
  for (long ev = lane; ev < A.nev; ev += kWave) any |= A.counts[ev * ncb + ci] > 0;
  if (!__syncthreads_or(any)) return;
  if (lane == 0) sc = A.cells[cell - A.lo];
  __syncthreads();
  species_list<FAMOD>(A, sc, cum, true);
  Tally t{0, 0, 0, 0};
  unsigned long long ncand = 0, nkept = 0;     // binned-only: there is no scan to count them
  for (long evb = 0; evb < A.nev; evb += kWave) {
    const long ev = evb + lane;
    pre[lane + 1] = ev < A.nev ? (long)A.counts[ev * ncb + ci] : 0L;
    __syncthreads();
    if (lane == 0) {
      pre[0] = 0;
      for (int k = 1; k <= kWave; k++) pre[k] += pre[k - 1];
    }
    __syncthreads();
    const long total = pre[kWave];
    for (long j = lane; j < total; j += kWave) {
      int lo = 0, hi = kWave - 1;             // the event whose candidates hold j: pre[lo] <= j < pre[lo + 1]
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pre[mid] <= j) lo = mid; else hi = mid - 1;
      }
      const long evl = evb + lo, nc = j - pre[lo];
      Particle p;
      double drawn = 0.0;
      const bool kept = FAMOD ? candidate_famod(A.run, sc, A.seed, A.cell_base + cell, A.e0 + evl, nc, cum, A.npart, A.mass,
                                                A.sign, A.baryon, &p, t, drawn)
                              : candidate(A.run, sc, A.seed, A.cell_base + cell, A.e0 + evl, nc, cum, A.npart, A.mass, A.sign,
                                          A.baryon, &p, t, nullptr, drawn);
      if (LIST) {
        const long slot = A.slots[evl * ncb + ci] + nc;
        A.flags[slot] = kept ? 1 : 0;
        if (kept) A.cand[slot] = p;
      } else {
        ncand++;
        nkept += kept ? 1 : 0;
      }
      if (BIN && kept) {
        const Landing l = bin_particle(A.bins, particle_rapidity(A.run.k.dim, drawn, p.E, p.pz), p.eta, p.px, p.py, p.tau, p.x, p.y);
        unsigned long long* hist = A.hist;
        hist_accumulate(A.bins, A.npart, p.species, l, [hist](long word, long long v) { atomicAdd(hist + word, (unsigned long long)v); });
      }
    }
    __syncthreads();
  }
  const unsigned long long v[4] = {wave_sum((unsigned long long)t.proposals), wave_sum((unsigned long long)t.acceptances),
                                   wave_sum((unsigned long long)t.capped), wave_sum((unsigned long long)t.clamped)};
  if (lane == 0)
    for (int k = 0; k < 4; k++)
      if (v[k]) atomicAdd(&A.tally[1 + k], v[k]);
  if (!LIST) {
    const unsigned long long nk = wave_sum(nkept), nc = wave_sum(ncand);
    if (lane == 0) {
      if (nk) atomicAdd(&A.tally[6], nk);
      if (nc) atomicAdd(&A.tally[7], nc);
    }
  }
}

__global__ __launch_bounds__(256) void k_compact(const Particle* cand, const int* flags, const long* pos, long n, Particle* out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && flags[i]) out[pos[i]] = cand[i];
}

__global__ void k_uniforms(unsigned long long seed, int purpose, long cell, long event, long candidate, int n, double* out) {
  Stream s = stream_open(seed, purpose, cell, event, candidate);
  for (int i = 0; i < n; i++) out[i] = stream_next(s);
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

// working buffers of a call, grown on demand and freed when it ends
struct Buffers {
  DevBuf<Cell> cells;
  DevBuf<double> dn;
  DevBuf<int> err, counts, flags;
  DevBuf<unsigned long long> tally;
  DevBuf<long> slots, pos;
  DevBuf<Particle> cand, out;
  DevBuf<char> tmp;     // the scans' scratch
  hipError_t pairs(long n) { return alloc(counts.reserve(n) && slots.reserve(n)); }
  hipError_t cands(long n) { return alloc(cand.reserve(n) && out.reserve(n) && flags.reserve(n) && pos.reserve(n)); }
};

}  // namespace

std::string tables_build(Tables& t, const std::vector<double>& mass, const std::vector<double>& sign,
                         const std::vector<double>& degen, const std::vector<double>& baryon) {
  t = Tables{};
  const size_t np = mass.size();
  if (np == 0 || sign.size() != np || degen.size() != np || baryon.size() != np) return "species tables are empty";
  std::vector<double> h;
  for (const auto* v : {&mass, &sign, &degen, &baryon}) h.insert(h.end(), v->begin(), v->end());
  if (!t.d.reserve((long)h.size()) ||
      hipMemcpy(t.d.get(), h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
    t = Tables{};
    return "hipMalloc / upload of the sampler's species tables failed";
  }
  t.npart = (int)np;
  const double* d = t.d.get();
  t.mass = d; t.sign = d + np; t.degen = d + 2 * np; t.baryon = d + 3 * np;
  return "";
}

hipError_t uniforms(uint64_t seed, int purpose, long cell, long event, long candidate, int n, double* host_out) {
  DevBuf<double> d;
  if (!d.reserve(n)) return hipErrorOutOfMemory;
  hipLaunchKernelGGL(k_uniforms, dim3(1), dim3(1), 0, 0, (unsigned long long)seed, purpose, cell, event, candidate, n, d.get());
  hipError_t h = hipGetLastError();
  if (h == hipSuccess) h = hipDeviceSynchronize();
  if (h == hipSuccess && n > 0) h = hipMemcpy(host_out, d.get(), (size_t)n * sizeof(double), hipMemcpyDeviceToHost);
  return h;
}

int run(const Tables& t, const Config& c, std::vector<Particle>& parts, std::vector<long>& offsets, Stats& st,
        int& df_err, std::string& msg) {
  parts.clear();
  offsets.assign((size_t)c.n_events + 1, 0);
  long copied = 0;
  const int s = run(t, c, [&](const Batch& b, std::string& m) -> int {
    const size_t at = parts.size();
    parts.resize(at + (size_t)b.kept);
    const hipError_t h = hipMemcpy(parts.data() + at, b.d, (size_t)b.kept * sizeof(Particle), hipMemcpyDeviceToHost);
    if (h != hipSuccess) { m = std::string("download of a batch: ") + hipGetErrorString(h); return S_DEVICE; }
    copied += b.kept * (long)sizeof(Particle);
    return S_OK;
  }, st, df_err, msg);
  st.list_d2h = copied;
  if (s != S_OK) return s;
  for (const Particle& p : parts) offsets[(size_t)p.event + 1]++;
  for (long e = 0; e < c.n_events; e++) offsets[e + 1] += offsets[e];
  return S_OK;
}

int run(const Tables& t, const Config& c, const Consumer& consume, Stats& st, int& df_err, std::string& msg) {
  st = Stats{};
  df_err = 0;
  const long nw = c.hi - c.lo;
  st.cells = nw;
  if (nw <= 0) return S_OK;
  const size_t lds = kCellLds + kPreLds + (size_t)t.npart * sizeof(double);
  if (lds > 64 * 1024) { msg = "too many chosen species for the sampler's LDS species list"; return S_BUDGET; }
#define SCHK(x)                                                                       \
  do {                                                                                \
    const hipError_t h_ = (x);                                                        \
    if (h_ != hipSuccess) { msg = std::string(#x) + ": " + hipGetErrorString(h_); return S_DEVICE; } \
  } while (0)
  Buffers B;
  SCHK(alloc(B.cells.reserve(nw) && B.dn.reserve(nw) && B.err.reserve(1) && B.tally.reserve(8)));
  SCHK(hipMemset(B.err.get(), 0, sizeof(int)));
  SCHK(hipMemset(B.tally.get(), 0, 8 * sizeof(unsigned long long)));
  Args A{};
  A.run = c.run; A.tb = c.tb; A.surf = c.surf; A.sol = c.sol; A.n = c.n; A.lo = c.lo; A.hi = c.hi; A.cell_base = c.cell_base;
  A.seed = c.seed; A.mass = t.mass; A.sign = t.sign; A.degen = t.degen; A.baryon = t.baryon; A.dens = c.dens;
  A.npart = t.npart; A.cells = B.cells.get(); A.dn = B.dn.get(); A.err = B.err.get(); A.tally = B.tally.get();
  const bool famod = c.sol != nullptr;
  if (famod) hipLaunchKernelGGL(k_cells<true>, dim3((unsigned)nw), dim3(kWave), lds, 0, A);
  else hipLaunchKernelGGL(k_cells<false>, dim3((unsigned)nw), dim3(kWave), lds, 0, A);
  SCHK(hipGetLastError());
  std::vector<double> dn((size_t)nw);
  SCHK(hipMemcpy(dn.data(), B.dn.get(), nw * sizeof(double), hipMemcpyDeviceToHost));
  SCHK(hipMemcpy(&df_err, B.err.get(), sizeof(int), hipMemcpyDeviceToHost));
  if (df_err) return S_DF;
  // expected candidates of one event over cells [0, i): the batch planner's estimate
  std::vector<double> acc((size_t)nw + 1, 0.0);
  for (long i = 0; i < nw; i++) acc[i + 1] = acc[i] + dn[i];
  const long budget = std::max(c.sample_bytes, 1L);
  const bool binned_only = c.bins && !c.keep_list;
  if (c.bins) { A.bins = *c.bins; A.hist = c.hist; }
  if (binned_only) {
    // a batch costs kPairBytes per (event, cell) and nothing per candidate, so its size is known before it runs:
    // whole events while they fit, else windows of cells of one event (one (event, cell) always fits)
    const long max_pairs = std::max(1L, std::min(budget / kPairBytes, 0x7ffffff0L));
    long e0 = 0, a = 0;
    while (e0 < c.n_events) {
      long nev = 1, b = std::min(nw, a + max_pairs);
      if (a == 0 && nw <= max_pairs) { nev = std::min(c.n_events - e0, max_pairs / nw); b = nw; }
      const long ncb = b - a, np = nev * ncb;
      SCHK(B.pairs(np));
      A.e0 = e0; A.nev = nev; A.c0 = c.lo + a; A.c1 = c.lo + b; A.counts = B.counts.get(); A.slots = B.slots.get();
      hipLaunchKernelGGL(k_count, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, 0, A);
      SCHK(hipGetLastError());
      if (famod) hipLaunchKernelGGL((k_sample<false, true, true>), dim3((unsigned)ncb), dim3(kWave), lds, 0, A);
      else hipLaunchKernelGGL((k_sample<false, true>), dim3((unsigned)ncb), dim3(kWave), lds, 0, A);
      SCHK(hipGetLastError());
      st.batches++;
      if (b == nw) { e0 += nev; a = 0; } else { a = b; }
    }
    SCHK(hipDeviceSynchronize());
  }
  auto estimate = [&](long nev, long a, long b) {     // bytes of a batch of nev events over window cells [a, b)
    const double mean = (double)nev * (acc[b] - acc[a]);
    return (double)nev * (double)(b - a) * kPairBytes + (mean + 6.0 * std::sqrt(mean) + 16.0) * kCandBytes;
  };
  long e0 = binned_only ? c.n_events : 0, a = 0;      // a: first window cell of the next batch (> 0: event e0 is split)
  while (e0 < c.n_events) {
    long nev = 1, b = nw;
    if (a == 0) {
      const double per = estimate(1, 0, nw);
      nev = std::max(1L, std::min(c.n_events - e0, (long)((double)budget / per)));
    }
    if (nev == 1 && estimate(1, a, nw) > (double)budget) {
      b = a + 1;
      while (b < nw && estimate(1, a, b + 1) <= (double)budget) b++;
    }
    for (;;) {      // count, and shrink the batch while what it really holds exceeds the bound
      const long ncb = b - a, np = nev * ncb + 1;
      bool too_big = np >= 0x7fffffffL;
      long total = 0;
      if (!too_big) {
        SCHK(B.pairs(np));
        A.e0 = e0; A.nev = nev; A.c0 = c.lo + a; A.c1 = c.lo + b; A.counts = B.counts.get(); A.slots = B.slots.get();
        SCHK(hipMemsetAsync(B.counts.get() + (np - 1), 0, sizeof(int), 0));
        hipLaunchKernelGGL(k_count, dim3((unsigned)((np - 1 + 255) / 256)), dim3(256), 0, 0, A);
        SCHK(hipGetLastError());
        SCHK(scan(B.counts.get(), B.slots.get(), np, B.tmp));
        SCHK(hipMemcpy(&total, B.slots.get() + (np - 1), sizeof(long), hipMemcpyDeviceToHost));
        too_big = total + 1 >= 0x7fffffffL || (double)(np - 1) * kPairBytes + (double)total * kCandBytes > (double)budget;
      }
      if (too_big) {
        if (nev > 1) { nev /= 2; continue; }
        if (ncb > 1) { b = a + ncb / 2; continue; }
        msg = "cell " + std::to_string(c.cell_base + c.lo + a) + " of event " + std::to_string(e0) + " alone draws " +
              std::to_string(total) + " candidates (" + std::to_string(total * kCandBytes) +
              " bytes): more than the \"sample_bytes\" bound of " + std::to_string(budget) + c.bound_note +
              "; raise it with is3d_set_tuning";
        return S_BUDGET;
      }
      st.batches++;
      st.candidates += total;
      if (total > 0) {
        SCHK(B.cands(total + 1));
        A.cand = B.cand.get(); A.flags = B.flags.get();
        SCHK(hipMemsetAsync(B.flags.get() + total, 0, sizeof(int), 0));
        if (famod && c.bins) hipLaunchKernelGGL((k_sample<true, true, true>), dim3((unsigned)ncb), dim3(kWave), lds, 0, A);
        else if (famod) hipLaunchKernelGGL((k_sample<true, false, true>), dim3((unsigned)ncb), dim3(kWave), lds, 0, A);
        else if (c.bins) hipLaunchKernelGGL((k_sample<true, true>), dim3((unsigned)ncb), dim3(kWave), lds, 0, A);
        else hipLaunchKernelGGL((k_sample<true, false>), dim3((unsigned)ncb), dim3(kWave), lds, 0, A);
        SCHK(hipGetLastError());
        SCHK(scan(B.flags.get(), B.pos.get(), total + 1, B.tmp));
        long kept = 0;
        SCHK(hipMemcpy(&kept, B.pos.get() + total, sizeof(long), hipMemcpyDeviceToHost));
        if (kept > 0) {
          hipLaunchKernelGGL(k_compact, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, 0, B.cand.get(), B.flags.get(), B.pos.get(), total, B.out.get());
          SCHK(hipGetLastError());
          Batch bt;
          bt.d = B.out.get(); bt.kept = kept; bt.e0 = e0; bt.nev = nev; bt.c0 = A.c0; bt.c1 = A.c1;
          bt.slots = B.slots.get(); bt.pos = B.pos.get();
          bt.batch_bytes = (np - 1) * kPairBytes + total * kCandBytes;
          const int cs = consume(bt, msg);
          if (cs != S_OK) return cs;
          st.kept += kept;
        }
      }
      break;
    }
    if (b == nw) { e0 += nev; a = 0; } else { a = b; }
  }
#undef SCHK
  unsigned long long tally[8] = {0};
  if (hipMemcpy(tally, B.tally.get(), sizeof(tally), hipMemcpyDeviceToHost) != hipSuccess) { msg = "reading the sampler tallies failed"; return S_DEVICE; }
  st.breakdown = (long)tally[0]; st.proposals = (long)tally[1]; st.acceptances = (long)tally[2];
  st.capped = (long)(tally[3] + tally[5]); st.clamped = (long)tally[4];
  if (binned_only) { st.kept = (long)tally[6]; st.candidates = (long)tally[7]; }
  return S_OK;
}

}  // namespace sampler
}  // namespace is3d
