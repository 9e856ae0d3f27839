// decay.hip -- resonance-decay feed-down of the continuous spectra (decay_math.h) for gfx950.
//
// Gather form, no floating-point atomics.  One workgroup owns the nphi outputs of one (daughter, pT, y) and loops over
// the two-body terms that feed the daughter in this level, in the plan's order.  For a fixed (term, pT, y, v, zeta)
// the parent's MT, Y and angle delta do not depend on phi, so a batch of nb (v, zeta) nodes goes through four phases:
//   0  one lane per node: the node's weight, delta and MT / Y brackets (Node) into LDS
//   1  one lane per (node, phi_j): the parent row g_j = S_R(MT, phi_j, Y) into LDS
//   2  one lane per (node, phi_i): the term weight x (g(phi_i + delta) + g(phi_i - delta)) into LDS
//   3  one lane per phi_i: the nodes' terms added in node order
// Phase 3 is the only summation, sequential in the node index: the result does not depend on nb or the block size.
// The parent's log slab is read from global memory (3+1D: 258 KB at 48 x 32 x 21, it lives in L2).
#include "decay.h"

#include <cstring>

namespace is3d {
namespace decay {

namespace {

constexpr int kBlock = 256;
constexpr long kLdsElems = 3072;   // nb x nphi bound: G and T take 16 bytes per element, 48 KiB

// ln S of the parents par[0 .. np) (slab doubles each); NaN where S <= 0
__global__ __launch_bounds__(kBlock) void k_decay_logs(const double* __restrict__ S, double* __restrict__ L,
                                                       const int* __restrict__ par, int np, long slab) {
  const long n = (long)np * slab;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long o = (long)par[i / slab] * slab + i % slab;
    L[o] = log_or_nan(S[o]);
  }
}

struct FeedArgs {
  double* S;
  const double* L;
  const Rule* rule;
  const double *pT, *phi, *y;
  const Sub* subs;
  const int *recv_d, *recv_s0, *recv_s1;   // of this level
  int npT, nphi, ny, nb;
};

__global__ __launch_bounds__(kBlock) void k_decay_feed(FeedArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nphi = a.nphi, ny = a.ny, nb = a.nb;
  // carve (every offset a multiple of 16 bytes)
  const long nphi2 = (nphi + 1) & ~1L;
  double* s_phi = (double*)smem;
  double* s_acc = s_phi + nphi2;
  double* s_G = s_acc + nphi2;
  double* s_T = s_G + (((long)nb * nphi + 1) & ~1L);
  Node* s_node = (Node*)(s_T + (((long)nb * nphi + 1) & ~1L));

  const int tid = threadIdx.x;
  const long per = (long)a.npT * ny;
  const int r = (int)(blockIdx.x / per);
  const int rem = (int)(blockIdx.x % per);
  const int ipT = rem / ny, iy = rem % ny;
  const int d = a.recv_d[r], s0 = a.recv_s0[r], s1 = a.recv_s1[r];
  const double pT = a.pT[ipT], y = ny > 1 ? a.y[iy] : 0.0;
  const long slab = (long)a.npT * nphi * ny;
  const Rule& rule = *a.rule;

  for (int i = tid; i < nphi; i += kBlock) {
    s_phi[i] = a.phi[i];
    s_acc[i] = 0.0;
  }
  __syncthreads();

  for (int s = s0; s < s1; s++) {
    const Sub sub = a.subs[s];
    const double* Sp = a.S + (long)sub.parent * slab;
    const double* Lp = a.L + (long)sub.parent * slab;
    for (int n0 = 0; n0 < kNodes; n0 += nb) {
      for (int n = tid; n < nb; n += kBlock) {
        const int node = n0 + n;
        s_node[n] = node_eval(sub, rule, node / kGL, node % kGL, pT, y, a.npT, a.pT, ny, a.y);
      }
      __syncthreads();
      const int ntask = nb * nphi;
      for (int k = tid; k < ntask; k += kBlock) {
        const int n = k / nphi, j = k - n * nphi;
        s_G[k] = parent_value(Sp, Lp, nphi, ny, s_node[n], j);
      }
      __syncthreads();
      for (int k = tid; k < ntask; k += kBlock) {
        const int n = k / nphi, i = k - n * nphi;
        const double* g = s_G + (long)n * nphi;
        const double dl = s_node[n].delta, ph = s_phi[i];
        s_T[k] = s_node[n].weight * (phi_interp(g, s_phi, nphi, ph + dl) + phi_interp(g, s_phi, nphi, ph - dl));
      }
      __syncthreads();
      for (int i = tid; i < nphi; i += kBlock) {
        double acc = s_acc[i];
        for (int n = 0; n < nb; n++) acc += s_T[(long)n * nphi + i];
        s_acc[i] = acc;
      }
      // the next batch's phase 0 writes s_node, which phase 2 read: every lane is past phase 2 (the barrier above);
      // its phase 2 writes s_T after two more barriers
    }
  }
  __syncthreads();
  for (int i = tid; i < nphi; i += kBlock) {
    const long o = (long)d * slab + ((long)ipT * nphi + i) * ny + iy;
    a.S[o] += s_acc[i];
  }
}

}  // namespace

Packed pack(const Plan& P, const Rule& r, const std::vector<double>& pT, const std::vector<double>& phi, int ny,
            const std::vector<double>& y) {
  static_assert(sizeof(Rule) % sizeof(double) == 0 && sizeof(Sub) % sizeof(double) == 0, "blob layout");
  Packed K;
  K.npT = (int)pT.size();
  K.nphi = (int)phi.size();
  K.ny = ny;
  auto put = [&](const void* p, size_t bytes) {
    const long o = (long)K.d.size();
    K.d.resize(o + (bytes + 7) / 8 + 1, 0.0);     // + 1: never empty, so every offset is a valid pointer
    if (bytes) std::memcpy(K.d.data() + o, p, bytes);
    return o;
  };
  K.o_rule = put(&r, sizeof(Rule));
  K.o_pT = put(pT.data(), pT.size() * sizeof(double));
  K.o_phi = put(phi.data(), phi.size() * sizeof(double));
  K.o_y = put(y.data(), (size_t)(ny > 1 ? ny : 0) * sizeof(double));
  K.o_sub = put(P.subs.data(), P.subs.size() * sizeof(Sub));
  auto puti = [&](const std::vector<int>& v) {
    const long o = (long)K.i.size();
    K.i.insert(K.i.end(), v.begin(), v.end());
    K.i.push_back(0);
    return o;
  };
  K.o_rd = puti(P.recv_d);
  K.o_rs0 = puti(P.recv_s0);
  K.o_rs1 = puti(P.recv_s1);
  K.o_par = puti(P.par);
  // the largest divisor of kNodes whose batch fits the LDS bound
  K.nb = 0;
  for (int nb = kNodes; nb >= 1; nb--)
    if (kNodes % nb == 0 && (long)nb * K.nphi <= kLdsElems) { K.nb = nb; break; }
  const long nphi2 = (K.nphi + 1) & ~1L, gt = ((long)K.nb * K.nphi + 1) & ~1L;
  K.lds = (size_t)(2 * nphi2 + 2 * gt) * sizeof(double) + (size_t)K.nb * sizeof(Node);
  return K;
}

hipError_t enqueue(const Plan& P, const Packed& K, const double* dev_d, const int* dev_i, double* S, double* logs,
                   hipStream_t st) {
  const long slab = (long)K.npT * K.nphi * K.ny;
  FeedArgs a{};
  a.S = S;
  a.L = logs;
  a.rule = (const Rule*)(dev_d + K.o_rule);
  a.pT = dev_d + K.o_pT;
  a.phi = dev_d + K.o_phi;
  a.y = dev_d + K.o_y;
  a.subs = (const Sub*)(dev_d + K.o_sub);
  a.npT = K.npT; a.nphi = K.nphi; a.ny = K.ny; a.nb = K.nb;
  for (int l = 0; l < P.levels(); l++) {
    const int np = P.lvl_p0[l + 1] - P.lvl_p0[l], nr = P.lvl_r0[l + 1] - P.lvl_r0[l];
    if (np <= 0 || nr <= 0) continue;
    const long n = (long)np * slab;
    const unsigned gl = (unsigned)std::min<long>((n + kBlock - 1) / kBlock, 65536);
    hipLaunchKernelGGL(k_decay_logs, dim3(gl), dim3(kBlock), 0, st, (const double*)S, logs, dev_i + K.o_par + P.lvl_p0[l], np, slab);
    hipError_t h = hipGetLastError();
    if (h != hipSuccess) return h;
    a.recv_d = dev_i + K.o_rd + P.lvl_r0[l];
    a.recv_s0 = dev_i + K.o_rs0 + P.lvl_r0[l];
    a.recv_s1 = dev_i + K.o_rs1 + P.lvl_r0[l];
    const long blocks = (long)nr * K.npT * K.ny;
    hipLaunchKernelGGL(k_decay_feed, dim3((unsigned)blocks), dim3(kBlock), K.lds, st, a);
    h = hipGetLastError();
    if (h != hipSuccess) return h;
  }
  return hipSuccess;
}

}  // namespace decay
}  // namespace is3d
