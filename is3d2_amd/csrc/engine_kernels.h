// engine_kernels.h -- the device code of the engine.hip translation unit: the prepass (k_prep, k_aniso, the PTMA
// warm-start chain kernels, k_famod_b, k_renorm), the fallback-cell scan, the slab fold and reduction, the cell costs,
// the df-coefficient probe and the Jonah table, each with its argument struct (PrepArgs and ChainArgs, which the
// engine keeps between the stages of a launch, are in engine.h).  The momentum integrals are in kernels.h.  engine.hip includes
// this header once, after kernels.h and its using-directives; it is not a unit of its own.
#pragma once
#include <hip/hip_runtime.h>

#include "aniso_math.h"
#include "cf_math.h"
#include "engine.h"     // PrepArgs, ChainArgs, kFbBlocks
#include "kernels.h"

namespace {

struct DevTables {            // device copy of the delta-f tables (pointers into one blob)
  DfTables tb;
};

// ------------------------------------------------------------------------------------------
// prepass kernels
// ------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void k_prep(PrepArgs A) {
  const long c = A.c0 + (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= A.c1) return;
  double s[NSURF];
#pragma unroll
  for (int f = 0; f < NSURF; f++) s[f] = A.surf[(long)f * A.n + c];
  double R[NREC];
  int err = DF_OK;
  if (MODE == GRAD || MODE == CE) {
    err = prep_grad_ce(A.k, A.tb, s, R);
  } else if (MODE == PTM || MODE == PTB) {
    double aux[9];
    int flags[2];
    err = prep_feqmod(A.k, A.tb, s, R, aux, flags);
    if (!err) {
#pragma unroll
      for (int f = 0; f < 9; f++) A.aux[(long)f * A.n + c] = aux[f];
      if (flags[0] && R[R_KIND] != 0.0) atomicAdd(&A.cnt[0], 1ull);
      if (flags[1]) atomicAdd(&A.cnt[1], 1ull);
    }
  } else {
    double ain[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    prep_famod_a(A.k, s, R, ain);
#pragma unroll
    for (int f = 0; f < 9; f++) A.aux[(long)f * A.n + c] = ain[f];
  }
  if (err) { atomicMax(A.err, err); R[R_KIND] = 0.0; }
  if (R[R_KIND] != 0.0) sep_cell_consts(MODE, R);
  // Grad / RTA-CE: cells whose lanes may leave the fast path (|mu_B| / T beyond ~300) counted in cnt[4]: any such
  // cell sends the launch to the F_TB kernels, the F_TS ones carry no slow loop (launch_end)
  if (MODE <= CE && A.k.operation == 1 && R[R_KIND] != 0.0 && sep_slow_cell(R, A.k.pT_max, A.k.b_max))
    atomicAdd(&A.cnt[4], 1ULL);
#pragma unroll
  for (int f = 0; f < NREC; f++) A.rec[c * NREC + f] = R[f];
}

// k_ytab: the y-term rows of one chunk of cells for the F_TS k_spectra launches, rows [cell - c0][q][kYRowTS], one
// thread per (cell, q).  yterms() depends on (cell, q) only; built inside k_spectra, every workgroup's wave 0 rebuilt
// its 2-3 q rows for each of the pT values and lane groups (~110 evaluations per (cell, q) at 48 pT x 193 classes x 21 y).
// The same call as k_spectra's other launches make (tables_ab): 3+1D q = y index and eta from the record, 2+1D
// q = y x eta node.  Rows of skipped cells (R_KIND == 0) are copied but never used: zeros.
struct YTabArgs {
  const double* rec; long c0, nc;           // records of the launch window, first cell and cells of the chunk
  const double *yv, *etav, *etaw;
  int nk, nl, dim, op;
  double* tab;                              // [nc][nk nl][kYRowTS]
  const unsigned long long* gate; int gate_want;   // as SpecArgs
};

template <int MODE>
__global__ __launch_bounds__(256) void k_ytab(YTabArgs A) {
  if (gate_closed(A.gate, A.gate_want)) return;
  const int nq = A.nk * A.nl;
  const long total = A.nc * nq;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long c = idx / nq;
    const int q = (int)(idx % nq), kk = q / A.nl, l = q % A.nl;
    const double* R = A.rec + (A.c0 + c) * NREC;
    double Y[NYT];
#pragma unroll
    for (int f = 0; f < NYT; f++) Y[f] = 0.0;
    if (R[R_KIND] != 0.0) {
      const double y = (A.dim == 3) ? A.yv[kk] : 0.0;
      const double eta = (A.dim == 3) ? R[R_ETA] : A.etav[l];
      const double w = (A.dim == 3) ? 1.0 : A.etaw[l];
      yterms(MODE, A.op, R, y, eta, w, Y, true, false);
    }
    double* row = A.tab + idx * kYRowTS;
#pragma unroll
    for (int f = 0; f < kYW_TS; f++) row[f] = Y[f];
    row[kYW_TS] = Y[Y_W];
  }
}

template <int MODE>
void launch_ytab(hipStream_t st, const YTabArgs& a) {
  const long total = a.nc * a.nk * a.nl;
  const long blocks = std::max(1L, std::min((total + 255) / 256, 256L * 32));
  hipLaunchKernelGGL((k_ytab<MODE>), dim3((unsigned)blocks), dim3(256), 0, st, a);
}

// sum over the W wavefronts of a workgroup (W x 64 lanes share one cell's Newton terms): each wave's sums, then the
// W partials from LDS in wave order (every lane gets the same bits), two barriers per red_all call of up to kRedN
// values
constexpr int kRedN = 8;
template <int W>
struct BlockSum {
  double* s;   // LDS, kRedN x W doubles
  __device__ double operator()(double v) const;
};
template <int W, class... T>
__device__ __forceinline__ void red_all(const BlockSum<W>& r, T&... v) {
  static_assert(sizeof...(T) <= kRedN, "BlockSum: at most kRedN values per call");
  ((v = WaveSum()(v)), ...);
  if constexpr (W > 1) {
    const int wave = threadIdx.x >> 6;
    int k = 0;
    if ((threadIdx.x & 63) == 0) ((r.s[(k++) * W + wave] = v), ...);
    __syncthreads();
    k = 0;
    auto sum = [&](int kk) {
      double a = r.s[kk * W];
#pragma unroll
      for (int w = 1; w < W; w++) a += r.s[kk * W + w];
      return a;
    };
    ((v = sum(k++)), ...);
    __syncthreads();
  }
}
template <int W>
__device__ double BlockSum<W>::operator()(double v) const {
  red_all(*this, v);
  return v;
}

struct AnisoArgs {
  const double* rec; const double* ain; double* sol;   // rec [n][NREC], ain [9][stride], sol [6][stride]
  long c0, n, chains;   // cells [c0, c0 + n) in `chains` warm-start chains
  long stride;          // cells held
  Hadrons h;
  double fp2;
  unsigned long long* cnt;
  int srule;            // the particle sampler's chain rule (aniso_math.h aniso_cell)
};

// one wavefront per warm-start chain: cells chain, chain + C, chain + 2C, ... (MomentumSpectra.cpp:98-107)
__global__ __launch_bounds__(64, 1) void k_aniso(AnisoArgs A) {
  const long chain = blockIdx.x;
  const int lane = threadIdx.x;
  __shared__ double s_etab[kExpTabN];                       // aniso_math.h aexp
  for (int i = lane; i < kExpTabN; i += 64) s_etab[i] = kExp2Tab[i];
  __syncthreads();
  Hadrons h = A.h;
  h.etab = s_etab;
  double state[4] = {0.0, 0.0, 0.0, 0.0};
  long cnt[3] = {0, 0, 0};
  for (long c = A.c0 + chain; c < A.c0 + A.n; c += A.chains) {
    if (A.rec[c * NREC + R_KIND] == 0.0) continue;
    double ain[4];
#pragma unroll
    for (int f = 0; f < 4; f++) ain[f] = A.ain[(long)f * A.stride + c];
    double out[6];
    aniso_cell(ain, h, lane, 64, WaveSum(), A.fp2, state, out, cnt, A.srule);
    if (lane == 0) {
#pragma unroll
      for (int f = 0; f < 6; f++) A.sol[(long)f * A.stride + c] = out[f];
    }
  }
  if (lane == 0) {
    if (cnt[0]) atomicAdd(&A.cnt[1], (unsigned long long)cnt[0]);
    if (cnt[1]) atomicAdd(&A.cnt[2], (unsigned long long)cnt[1]);
    if (cnt[2]) atomicAdd(&A.cnt[3], (unsigned long long)cnt[2]);
  }
}

// ---- PTMA warm-start chains (MomentumSpectra.cpp:1308-1364) in parallel segments -----------------------
// The reference warm-starts each cell's Newton solve from the chain state the previous cell of its OpenMP
// thread left (chain c = cells c, c + C, c + 2C, ...; the shipped serial build is one chain).  That state
// recurrence is serial, and a lone wavefront walking it is latency-bound (354 us per cell on MI355X:
// 1e5 cells took 35 s).  The chain is instead cut into segments of L positions, one wavefront each:
//   pass 0      every segment runs its cells from a cold start (exact for each chain's first segment);
//   pass j >= 1 a segment whose incoming state (the end state the previous segment left in pass j - 1)
//               differs bitwise from the start its stored run used re-runs from the new start, and stops
//               at the first cell whose new chain state equals the stored one: from there on the stored
//               cells were computed from that same state, so they stand.  A segment that reaches its end
//               without re-synchronising publishes a new end state and flags pass j as changed.
// The passes stop once a pass changes nothing; then every segment's stored run starts from its
// predecessor's true end state, i.e. the stored states and solutions are the serial chain's, bit for bit.
// A chain state differs from a cold-start guess for ~10 cells on average before the Newton solves forget it
// (CPU sweep study, tests/native/cf_emulator.cpp emu_chain_sweeps), so a pass re-runs little.  After
// kChainPasses passes a single-wavefront finisher completes any remaining ripple serially (exact).
constexpr int kChainPasses = 24;

constexpr int kBndSlots = 3;   // bin / bout slots: pass parity 0, 1 and the finisher's

__device__ __forceinline__ bool state_eq(const double* a, const double* b) {
  bool eq = true;
#pragma unroll
  for (int f = 0; f < 4; f++) eq = eq && (__double_as_longlong(a[f]) == __double_as_longlong(b[f]));
  return eq;
}

// Run segment `seg` from `state` (its start): re-run mode (sync) stops at the first cell whose new state equals
// the stored one and returns true (end state unchanged); otherwise the state after the last cell is in `state`.
__device__ bool chain_segment_run(const ChainArgs& A, Hadrons h, long seg, double* state, bool sync) {
  const int lane = threadIdx.x;
  __shared__ double s_red[kRedN * IS3D_CHAIN_W];
  const long c = seg / A.nspc, s = seg % A.nspc;
  const long P = min((A.n - c + A.C - 1) / A.C, A.q1);      // positions of chain c in this range's end
  const long p0 = A.q0 + s * A.L, p1 = min(P, p0 + A.L);
  for (long pos = p0; pos < p1; pos++) {
    const long cell = c + pos * A.C;
    if (A.rec[cell * NREC + R_KIND] == 0.0) continue;       // u.dsigma <= 0: not in the chain (:1146)
    double ain[4];
#pragma unroll
    for (int f = 0; f < 4; f++) ain[f] = A.ain[(long)f * A.n + cell];
    // the stored state is read before the solve: its barriers keep lane 0's store below from racing a lagging
    // wavefront's read
    double old[4];
#pragma unroll
    for (int f = 0; f < 4; f++) old[f] = A.sta[(long)f * A.n + cell];
    double out[6];
    long cnt[3] = {0, 0, 0};
    aniso_cell(ain, h, lane, 64 * IS3D_CHAIN_W, BlockSum<IS3D_CHAIN_W>{s_red}, A.fp2, state, out, cnt, A.srule);
    const bool same = sync && state_eq(state, old);
    if (lane == 0) {
#pragma unroll
      for (int f = 0; f < 6; f++) A.sol[(long)f * A.n + cell] = out[f];
#pragma unroll
      for (int f = 0; f < 4; f++) A.sta[(long)f * A.n + cell] = state[f];
      A.info[cell] = (int)cnt[2] | ((int)cnt[0] << 16) | ((int)cnt[1] << 17);
    }
    if (same) return true;
  }
  return false;
}

// the chain kernels' Hadrons with the LDS exp table of aniso_math.h's aexp (filled by the whole workgroup)
__device__ __forceinline__ Hadrons chain_hadrons(const ChainArgs& A, double* s_etab) {
  for (int i = threadIdx.x; i < kExpTabN; i += blockDim.x) s_etab[i] = kExp2Tab[i];
  __syncthreads();
  Hadrons h = A.h;
  h.etab = s_etab;
  return h;
}

// one workgroup of IS3D_CHAIN_W wavefronts per segment (the lanes share each Newton evaluation's terms); every
// branch below is uniform over the workgroup (the reductions hand all lanes the same bits)
__global__ __launch_bounds__(64 * IS3D_CHAIN_W, 1) void k_chain_pass(ChainArgs A, int pass) {
  const long seg = blockIdx.x, nseg = A.C * A.nspc;
  const long c = seg / A.nspc, s = seg % A.nspc;
  const int lane = threadIdx.x;
  const long bw = 4 * A.C + 1;
  // converged: the remaining passes are no-ops (a shard with a predecessor always checks its starts: the boundary
  // pushed in may still move)
  if (pass > 0 && A.changed[pass - 1] == 0 && !A.has_pred) return;
  __shared__ double s_etab[kExpTabN];
  const Hadrons h = chain_hadrons(A, s_etab);
  const double* prev = A.send + (long)((pass + 1) & 1) * 4 * nseg;
  double* cur = A.send + (long)(pass & 1) * 4 * nseg;
  double state[4] = {0.0, 0.0, 0.0, 0.0};                   // cold: no previous success in this chain
  bool done = false;
  if (pass > 0) {
    double st0[4], used[4];
#pragma unroll
    for (int f = 0; f < 4; f++) used[f] = A.sstart[f * nseg + seg];
    if (s == 0) {
      const double* b = A.bin + (long)((pass - 1) & 1) * bw;
#pragma unroll
      for (int f = 0; f < 4; f++) st0[f] = A.has_pred ? b[f * A.C + c] : 0.0;
    } else {
#pragma unroll
      for (int f = 0; f < 4; f++) st0[f] = prev[f * nseg + seg - 1];
    }
    if (state_eq(st0, used)) {                              // same start: the stored run stands
      done = true;
    } else {
#pragma unroll
      for (int f = 0; f < 4; f++) state[f] = st0[f];
    }
    if (IS3D_CHAIN_W > 1) __syncthreads();   // every wavefront has read sstart before lane 0 rewrites it
    if (done && lane == 0) for (int f = 0; f < 4; f++) cur[f * nseg + seg] = prev[f * nseg + seg];
  }
  if (!done) {
    if (lane == 0) for (int f = 0; f < 4; f++) A.sstart[f * nseg + seg] = state[f];
    const bool synced = chain_segment_run(A, h, seg, state, pass > 0);
    if (lane == 0) {
      if (synced) {
        for (int f = 0; f < 4; f++) cur[f * nseg + seg] = prev[f * nseg + seg];
      } else {
        bool moved = pass == 0;
        for (int f = 0; f < 4; f++) {
          moved = moved || __double_as_longlong(state[f]) != __double_as_longlong(prev[f * nseg + seg]);
          cur[f * nseg + seg] = state[f];
        }
        if (moved && pass > 0) atomicOr(&A.changed[pass], 1);
      }
    }
    // pass 0 ran cold starts: exact only for the first segment of a range without a predecessor, so it flags a
    // change whenever some segment may be wrong (a finisher after a single pass must then walk)
    if (pass == 0 && lane == 0 && (A.nspc > 1 || A.has_pred)) atomicOr(&A.changed[0], 1);
  }
  // pass 0 fills both parity slots: a range without a predecessor and with one segment per chain is exact after
  // pass 0 and flags nothing, so passes 1.. return early above and never write slot 1 -- which the finisher's
  // no-walk copy and the successor shard's odd-pass boundary read
  if (pass == 0 && lane == 0) {
    double* other = A.send + 4 * nseg;
    for (int f = 0; f < 4; f++) other[f * nseg + seg] = cur[f * nseg + seg];
  }
  // the range's last segment of chain c: its end state is the next shard's boundary in
  if (s == A.nspc - 1 && lane == 0) {
    for (int slot = pass & 1; slot <= (pass == 0 ? 1 : (pass & 1)); slot++) {
      double* b = A.bout + (long)slot * bw;
      for (int f = 0; f < 4; f++) b[f * A.C + c] = cur[f * nseg + seg];
    }
  }
}

// Serial completion after the passes (one wavefront; normally returns at once): segments in chain order, each
// from its predecessor's current end state -- exact by induction.  It walks when this range's last pass changed
// something or the predecessor shard walked (bin[2] flag); either way it leaves the range's final end states and
// its walk flag in bout[2] for the next shard.
__global__ __launch_bounds__(64 * IS3D_CHAIN_W) void k_chain_finish(ChainArgs A) {
  const long nseg = A.C * A.nspc, bw = 4 * A.C + 1;
  double* cur = A.send + (long)((A.npass - 1) & 1) * 4 * nseg;
  const double* bfin = A.bin + 2 * bw;
  double* bo = A.bout + 2 * bw;
  const int lane = threadIdx.x;
  const bool walk = A.changed[A.npass - 1] != 0 || (A.has_pred && bfin[4 * A.C] != 0.0);
  if (!walk) {
    if (lane == 0) {
      for (long c = 0; c < A.C; c++)
        for (int f = 0; f < 4; f++) bo[f * A.C + c] = cur[f * nseg + c * A.nspc + A.nspc - 1];
      bo[4 * A.C] = 0.0;
    }
    return;
  }
  __shared__ double s_etab[kExpTabN];
  const Hadrons h = chain_hadrons(A, s_etab);
  // the running end state stays in registers (uniform over the wavefront): no memory round trip between
  // segments, and every array element this kernel reads was written by an earlier launch or not at all
  double carry[4] = {0.0, 0.0, 0.0, 0.0};
  for (long seg = 0; seg < nseg; seg++) {
    const long c = seg / A.nspc, s = seg % A.nspc;
    if (s == 0) {
#pragma unroll
      for (int f = 0; f < 4; f++) carry[f] = A.has_pred ? bfin[f * A.C + c] : 0.0;
    }
    double used[4];
#pragma unroll
    for (int f = 0; f < 4; f++) used[f] = A.sstart[f * nseg + seg];
    const bool same = state_eq(carry, used);
    if (IS3D_CHAIN_W > 1) __syncthreads();   // every wavefront has read sstart before lane 0 rewrites it
    if (same) {
#pragma unroll
      for (int f = 0; f < 4; f++) carry[f] = cur[f * nseg + seg];
    } else {
      if (lane == 0) for (int f = 0; f < 4; f++) A.sstart[f * nseg + seg] = carry[f];
      double state[4] = {carry[0], carry[1], carry[2], carry[3]};
      if (chain_segment_run(A, h, seg, state, true)) {
#pragma unroll
        for (int f = 0; f < 4; f++) carry[f] = cur[f * nseg + seg];
      } else {
#pragma unroll
        for (int f = 0; f < 4; f++) carry[f] = state[f];
        if (lane == 0) for (int f = 0; f < 4; f++) cur[f * nseg + seg] = state[f];
      }
    }
    if (s == A.nspc - 1 && lane == 0) for (int f = 0; f < 4; f++) bo[f * A.C + c] = carry[f];
  }
  if (lane == 0) bo[4 * A.C] = 1.0;
}

// the serial chain's counters from the per-cell records: [1] pl/pt < 0, [2] reconstruction failures,
// [3] Newton iterations
__global__ __launch_bounds__(256) void k_chain_count(const double* rec, const int* info, long c_lo, long c_hi,
                                                     unsigned long long* cnt) {
  __shared__ unsigned long long s[3][256];
  unsigned long long a = 0, b = 0, it = 0;
  for (long c = c_lo + (long)blockIdx.x * 256 + threadIdx.x; c < c_hi; c += (long)gridDim.x * 256) {
    if (rec[c * NREC + R_KIND] == 0.0) continue;
    const int v = info[c];
    it += (unsigned)(v & 0xffff); a += (v >> 16) & 1; b += (v >> 17) & 1;
  }
  s[0][threadIdx.x] = a; s[1][threadIdx.x] = b; s[2][threadIdx.x] = it;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o)
      for (int k = 0; k < 3; k++) s[k][threadIdx.x] += s[k][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (s[0][0]) atomicAdd(&cnt[1], s[0][0]);
    if (s[1][0]) atomicAdd(&cnt[2], s[1][0]);
    if (s[2][0]) atomicAdd(&cnt[3], s[2][0]);
  }
}

__global__ __launch_bounds__(256) void k_famod_b(PrepArgs A, const double* sol) {
  const long c = A.c0 + (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= A.c1) return;
  if (A.rec[c * NREC + R_KIND] == 0.0) return;
  double R[NREC], ain[9], so[6];
#pragma unroll
  for (int f = 0; f < NREC; f++) R[f] = A.rec[c * NREC + f];
#pragma unroll
  for (int f = 0; f < 9; f++) ain[f] = A.aux[(long)f * A.n + c];
#pragma unroll
  for (int f = 0; f < 6; f++) so[f] = sol[(long)f * A.n + c];
  int broken = 0;
  prep_famod_b(A.k, R, ain, so, &broken);
  if (broken) atomicAdd(&A.cnt[0], 1ull);
#pragma unroll
  for (int f = 0; f < NREC; f++) A.rec[c * NREC + f] = R[f];
}

struct RenormArgs {
  PrepConsts k;
  const double* rec; const double* aux; double* renorm;   // renorm[c - c0][class]
  const double *mass, *sign, *degen, *baryon;              // sorted species
  const int* rrep;                                         // representative sorted species of each class
  long c0, n, stride; int npart;                           // cells [c0, c0 + n) of stride held; npart = classes
};

__global__ __launch_bounds__(256) void k_renorm(RenormArgs A) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= A.n * A.npart) return;
  const long c = A.c0 + idx / A.npart;
  const int s = A.rrep[(int)(idx % A.npart)];
  if (A.rec[c * NREC + R_KIND] == 0.0) { A.renorm[idx] = 0.0; return; }
  double aux[9];
#pragma unroll
  for (int f = 0; f < 9; f++) aux[f] = A.aux[(long)f * A.stride + c];
  A.renorm[idx] = ptm_renorm(A.k, aux, A.mass[s], A.sign[s], A.degen[s], A.baryon[s]);
}

// per-cell cost estimate (is3d_cell_costs) from the prepared records
__global__ __launch_bounds__(256) void k_cell_cost(const double* rec, long n, double fb_cost, double* cost) {
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const double* R = rec + c * NREC;
  const bool fb = R[R_KIND] == 1.0 || (R[R_KIND] == 2.0 && R[R_NARROW] != 0.0);
  cost[c] = R[R_KIND] == 0.0 ? kSkipCost : (fb_cost > 0.0 && fb) ? fb_cost : 1.0;
}

// Modified modes: the cells whose lanes may take the separable fallback (breakdown: R_KIND == 1; narrow
// rapidity windows: R_NARROW != 0, MomentumSpectra.cpp:863-871), listed in ascending order for the F_FB
// launch.  kFbBlocks workgroups each own a contiguous cell range: k_fbcount counts each range's cells, k_fbwrite
// writes them in order after the counts of the ranges before it (wave ballots + an LDS prefix per 256 cells) --
// deterministic, and no host round trip (the count stays on the device).  (One workgroup walking per-thread chunks
// took 44 ms per config-5 pass, 5e6 cells.)
__device__ __forceinline__ bool fb_cell(const double* rec, long c) {
  const double* R = rec + c * NREC;
  return R[R_KIND] == 1.0 || (R[R_KIND] == 2.0 && R[R_NARROW] != 0.0);
}

__global__ __launch_bounds__(256) void k_fbcount(const double* rec, long n, int* bcnt) {
  const long ch = (n + kFbBlocks - 1) / kFbBlocks, lo = min(n, (long)blockIdx.x * ch), hi = min(n, lo + ch);
  int cnt = 0;
  for (long c = lo + threadIdx.x; c < hi; c += 256) cnt += fb_cell(rec, c) ? 1 : 0;
  __shared__ int s[256];
  s[threadIdx.x] = cnt;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (threadIdx.x < d) s[threadIdx.x] += s[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) bcnt[blockIdx.x] = s[0];
}

__global__ __launch_bounds__(256) void k_fbwrite(const double* rec, long n, const int* bcnt, int* cells, int* count) {
  const long ch = (n + kFbBlocks - 1) / kFbBlocks, lo = min(n, (long)blockIdx.x * ch), hi = min(n, lo + ch);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  __shared__ int s_base, s_w[4];
  if (t == 0) {
    int o = 0;
    for (int b = 0; b < (int)blockIdx.x; b++) o += bcnt[b];
    s_base = o;
    if (blockIdx.x == kFbBlocks - 1) *count = o + bcnt[blockIdx.x];
  }
  __syncthreads();
  for (long c0 = lo; c0 < hi; c0 += 256) {
    const long c = c0 + t;
    const bool f = c < hi && fb_cell(rec, c);
    const unsigned long long m = __ballot(f);
    if (lane == 0) s_w[wave] = __popcll(m);
    __syncthreads();
    int o = s_base;
    for (int w = 0; w < wave; w++) o += s_w[w];
    if (f) cells[o + __popcll(m & ((1ull << lane) - 1ull))] = (int)c;
    __syncthreads();
    if (t == 0) s_base += s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
  }
}

struct ReduceArgs {
  const double* slab; long sstride; int nsplit;
  int nbx, npart, npT, nphi, nk, nl, ny_out, kj; long ntask;   // npart: lane species (integrand classes)
  const int* sorig; const double* degen_orig; double prefactor;
  const int *cmem_off, *cmem;   // member sorted species of each class
  double* out;
  const unsigned long long* gate; int gate_want;   // launch_end's device-side plan choice (kernels.h SpecArgs)
};

// every member species of class c gets (2 pi hbarc)^-3 g_s x the class's sum
__device__ __forceinline__ void write_members(const ReduceArgs& A, int c, long off, double acc, int m0, int dm) {
  for (int m = A.cmem_off[c] + m0; m < A.cmem_off[c + 1]; m += dm) {
    const int so = A.sorig[A.cmem[m]];
    A.out[(long)so * A.npT * A.nphi * A.ny_out + off] = A.prefactor * A.degen_orig[so] * acc;
  }
}

// dN[s][pT][phi][y] = (2 pi hbarc)^-3 g_s * sum over eta nodes (2+1D) and cell splits, in fixed order.
// One thread per slab entry of an l = 0 lane; the lanes of the other eta nodes of the same (class, y,
// phi block) are task + l * npart.
__global__ __launch_bounds__(256) void k_reduce(ReduceArgs A) {
  if (gate_closed(A.gate, A.gate_want)) return;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= A.sstride) return;
  const int KJ = A.kj;
  const int lane = (int)(e % kBlock);
  const int jj = (int)((e / kBlock) % KJ);
  const long rest = e / ((long)kBlock * KJ);
  const int lane_group = (int)(rest % A.nbx), ipt = (int)(rest / A.nbx);
  const long task = (long)lane_group * kBlock + lane;
  if (task >= A.ntask) return;
  const int s = (int)(task % A.npart);
  const long r = task / A.npart;
  const long nq = (long)A.nk * A.nl;
  const int q = (int)(r % nq);
  if (q % A.nl != 0) return;
  const int k = q / A.nl, j = (int)(r / nq) * KJ + jj;
  if (j >= A.nphi) return;
  double acc = 0.0;
  for (int l = 0; l < A.nl; l++) {
    const long tl = task + (long)l * A.npart;
    const long el = ((long)ipt * A.nbx + tl / kBlock) * ((long)KJ * kBlock) + (long)jj * kBlock + tl % kBlock;
    for (int z = 0; z < A.nsplit; z++) acc += A.slab[(long)z * A.sstride + el];
  }
  write_members(A, s, ((long)ipt * A.nphi + j) * A.ny_out + k, acc, 0, 1);
}

// The same sum with one wavefront per output entry, for slabs with many (eta node, cell split) terms per
// output (2+1D: 24 eta nodes x hundreds of splits -- the per-thread loop above ran 8k dependent loads per
// output and took 2.4 ms for pikp 1e5 cells): lane i adds terms i, i + 64, ... of the (l, split) list,
// then a fixed xor-shuffle tree combines the lanes, so the order stays fixed (bit-reproducible).
__global__ __launch_bounds__(256) void k_reduce_wave(ReduceArgs A) {
  if (gate_closed(A.gate, A.gate_want)) return;
  const long o = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  const long nout = (long)A.npart * A.npT * A.nphi * A.ny_out;
  if (o >= nout) return;                                   // whole wavefronts exit together
  const int k = (int)(o % A.ny_out);
  const long r1 = o / A.ny_out;
  const int j = (int)(r1 % A.nphi);
  const long r2 = r1 / A.nphi;
  const int ipt = (int)(r2 % A.npT), s = (int)(r2 / A.npT);
  const int KJ = A.kj, jb = j / KJ, jj = j % KJ;
  const long nq = (long)A.nk * A.nl;
  const long task0 = s + (long)A.npart * (k * A.nl + nq * jb);
  const long nterm = (long)A.nl * A.nsplit;
  double acc = 0.0;
  for (long m = lane; m < nterm; m += 64) {
    const int l = (int)(m / A.nsplit), z = (int)(m % A.nsplit);
    const long tl = task0 + (long)l * A.npart;
    const long el = ((long)ipt * A.nbx + tl / kBlock) * ((long)KJ * kBlock) + (long)jj * kBlock + tl % kBlock;
    acc += A.slab[(long)z * A.sstride + el];
  }
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) acc += __shfl_xor(acc, w, 64);
  write_members(A, s, ((long)ipt * A.nphi + j) * A.ny_out + k, acc, lane, 64);
}

// Chunk-wise slab fold (folded F_TS launches, enqueue_spectra): acc[i] = (init ? 0 : acc[i]) + src[0][i] + ... +
// src[ns - 1][i], added in split order, so the folded accumulator equals k_reduce's sequential sum over all splits
// bit for bit (3+1D: one term per split and output).  Memory-bound: ns + 2 doubles per entry.
__global__ __launch_bounds__(256) void k_fold(double* acc, const double* src, long sstride, int ns, int init,
                                              const unsigned long long* gate, int gate_want) {
  if (gate_closed(gate, gate_want)) return;      // the other plan of a gated pair runs (launch_end)
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < sstride; i += (long)gridDim.x * blockDim.x) {
    double a = init ? 0.0 : acc[i];
    for (int z = 0; z < ns; z++) a += src[(long)z * sstride + i];
    acc[i] = a;
  }
}

// ------------------------------------------------------------------------------------------
// PTB "Jonah" table (DeltafData.cpp:220-295): thread (row, hadron) evaluates the two Gauss sums, one
// thread per row then adds the hadrons in PDG order (the reference's order), so the table is
// bit-reproducible; row kJonahN holds the lambda = 0 terms.
// ------------------------------------------------------------------------------------------
struct JonahArgs {
  double T; int npdg, pts;
  const double *mass, *degen, *sign, *r2, *w2;
  double* terms;                  // [kJonahN + 1][2][npdg]
  double *l2, *z, *bp;            // [kJonahN] each
};

__global__ __launch_bounds__(256) void k_jonah_terms(JonahArgs A) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)(kJonahN + 1) * A.npdg) return;
  const int i = (int)(idx / A.npdg), n = (int)(idx % A.npdg);
  const double lambda = (i < kJonahN) ? jonah_lambda(i) : 0.0;
  double* t = A.terms + (long)i * 2 * A.npdg;
  jonah_terms(A.T, A.mass[n], A.degen[n], A.sign[n], A.r2, A.w2, A.pts, lambda, t + n, t + A.npdg + n);
}

__global__ __launch_bounds__(64) void k_jonah_sum(JonahArgs A) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= kJonahN) return;
  const double* e0 = A.terms + (long)kJonahN * 2 * A.npdg;
  const double* p0 = e0 + A.npdg;
  const double* em = A.terms + (long)i * 2 * A.npdg;
  const double* pm = em + A.npdg;
  double E = 0.0, P = 0.0, Em = 0.0, Pm = 0.0;
  for (int n = 0; n < A.npdg; n++) {
    if (A.mass[n] == 0.0) continue;
    E += e0[n]; P += p0[n]; Em += em[n]; Pm += pm[n];
  }
  jonah_row(i, E, P, Em, Pm, A.l2, A.z, A.bp);
}

__global__ void k_df_eval(DfTables tb, double T, double muB, double E, double P, double bulkPi, double* out, int* err) {
  DfCoef df;
  *err = df_eval(tb, T, muB, E, P, bulkPi, df);
  const double o[15] = {df.c0, df.c1, df.c2, df.c3, df.c4, df.shear14, df.F, df.G, df.betabulk, df.betaV, df.betapi,
                        df.lambda, df.z, df.dlambda, df.dz};
  for (int i = 0; i < 15; i++) out[i] = o[i];
}

}  // namespace
