// engine_dndx_kernels.h -- the device code of the engine_dndx.hip translation unit: operation 0's bin keys and bin sums
// (k_stkeys, k_stbin), each with its argument struct.  The per-cell yields are k_dndx (kernels.h).
// engine_dndx.hip includes this header once, after kernels.h and its using-directives; it is not a unit of its own.
#pragma once
#include <hip/hip_runtime.h>

#include "cf_math.h"
#include "kernels.h"

namespace {

// per-cell spacetime bin indices (SpacetimeDistribution.cpp:380-392): keys[0..2][c] = itau, ir, iphi (-1 outside)
struct KeyArgs {
  const double *tau, *x, *y; long n;
  double tau_min, tau_width, r_min, r_width, phip_width;
  int tau_bins, r_bins, phip_bins;
  int* keys;
};

__global__ __launch_bounds__(256) void k_stkeys(KeyArgs A) {
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= A.n) return;
  const double two_pi = 2.0 * M_PI;
  const double x = A.x[c], y = A.y[c], tau = A.tau[c];
  const double r = sqrt(x * x + y * y);
  double phi = atan2(y, x);
  if (phi < 0.0) phi += two_pi;
  const long itau = (int)floor((tau - A.tau_min) / A.tau_width);
  const long ir = (int)floor((r - A.r_min) / A.r_width);
  const long iphi = (int)floor(phi / A.phip_width);
  A.keys[c] = (itau >= 0 && itau < A.tau_bins) ? (int)itau : -1;
  A.keys[A.n + c] = (ir >= 0 && ir < A.r_bins) ? (int)ir : -1;
  A.keys[2 * A.n + c] = (iphi >= 0 && iphi < A.phip_bins) ? (int)iphi : -1;
}

// part[s_orig][e] = prefactor g_s x sum over the cells of entry e = (distribution, thread slice n, bin),
// cells in ascending order (the reference's per-thread order); perm/offs: CSR built on the host
struct BinArgs {
  const double* ycell; long n; int npart;          // ycell: [class][n]; npart sorted species
  const int *perm; const long* offs; long nent;
  const int* sorig; const double* sdegen; double prefactor;
  const int* scls;                                  // sorted species -> integrand class
  double* part;
};

__global__ __launch_bounds__(256) void k_stbin(BinArgs A) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= A.nent * A.npart) return;
  const int s = (int)(idx / A.nent);
  const long e = idx % A.nent;
  const double f = A.prefactor * A.sdegen[s];
  double acc = 0.0;
  for (long i = A.offs[e]; i < A.offs[e + 1]; i++) {
    acc += f * A.ycell[(long)A.scls[s] * A.n + A.perm[i]];
  }
  A.part[(long)A.sorig[s] * A.nent + e] = acc;
}

}  // namespace
