// engine_sample_kernels.h -- the device code of the engine_sample.hip translation unit: the plasma-average densities and
// the yield estimate of operation 2 (k_densities, k_yield), each with its argument struct.  The sampler is sampler.hip.
// engine_sample.hip includes this header once, after kernels.h and its using-directives; it is not a unit of its own.
#pragma once
#include <hip/hip_runtime.h>

#include "cf_math.h"
#include "kernels.h"

namespace {

// ------------------------------------------------------------------------------------------
// operation = 2 oversampling estimate (ParticleSampler.cpp:447-636, DeltafData.cpp:555-690)
// ------------------------------------------------------------------------------------------
struct DensArgs {
  DfTables tb;
  const double *gla;              // [alpha][pts] roots then [alpha][pts] weights
  int gla_alpha, gla_pts;
  double T, E, P, muB, nB;        // Plasma averages
  const double *smass, *ssign, *sdegen, *sbaryon; const int* sorig;
  int npart, df_mode;
  double two_pi2_hbarC3;
  double* dens;                   // [3][npart] original species order
  int* err;
};

// one wavefront per (mass-sorted) species: lane k holds Gauss-Laguerre node k of each alpha
__global__ __launch_bounds__(64) void k_densities(DensArgs A) {
  const int s = blockIdx.x, lane = threadIdx.x;
  DfCoef df;
  const int err = df_eval(A.tb, A.T, A.muB, A.E, A.P, 0.0, df);     // DeltafData.cpp:574
  if (err) { if (lane == 0) atomicMax(A.err, err); return; }
  const double mass = A.smass[s], sign = A.ssign[s], baryon = A.sbaryon[s];
  const double mbar = mass / A.T, chem = baryon * (A.muB / A.T);
  const double* W = A.gla + (long)A.gla_alpha * A.gla_pts;
  static constexpr int kAlpha[6] = {1, 1, 1, 2, 3, 3};
  double J[6];
  WaveSum ws;
#pragma unroll
  for (int q = 0; q < 6; q++) {
    double v = 0.0;
    for (int k = lane; k < A.gla_pts; k += 64) {
      const long o = (long)kAlpha[q] * A.gla_pts + k;
      v += W[o] * gt_term(q, A.gla[o], mbar, chem, sign);
    }
    J[q] = ws(v);
  }
  if (lane == 0) {
    double d3[3];
    species_densities(A.df_mode, df, A.T, A.nB / (A.E + A.P), mass, A.sdegen[s], baryon, J, A.two_pi2_hbarC3, d3);
    const int so = A.sorig[s];
    for (int i = 0; i < 3; i++) A.dens[(long)i * A.npart + so] = d3[i];
  }
}

struct YieldArgs {
  PrepConsts k;
  DfTables tb;
  const double* surf; long n;
  const double* dens; int npart;
  double* partial;                // [gridDim.x] per-block sums
  int* err;
};

// one thread per cell, fixed-order tree sum per block (bit-reproducible); the host adds the blocks in order
__global__ __launch_bounds__(256) void k_yield(YieldArgs A) {
  __shared__ double red[256];
  __shared__ double dsum[3];
  const int tid = threadIdx.x;
  if (tid < 3) {                  // species sums in species order
    double a = 0.0;
    for (int i = 0; i < A.npart; i++) a += A.dens[(long)tid * A.npart + i];
    dsum[tid] = a;
  }
  __syncthreads();
  const long c = (long)blockIdx.x * 256 + tid;
  double v = 0.0;
  if (c < A.n) {
    double sv[NSURF];
#pragma unroll
    for (int f = 0; f < NSURF; f++) sv[f] = A.surf[(long)f * A.n + c];
    const int err = yield_cell(A.k, A.tb, sv, dsum, &v);
    if (err) { atomicMax(A.err, err); v = 0.0; }
  }
  red[tid] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) A.partial[blockIdx.x] = red[0];
}

}  // namespace
