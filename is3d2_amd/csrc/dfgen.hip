// dfgen.hip -- the delta-f coefficient tables of a hadron list on a (T, muB) grid (is3d_generate_df_tables).
//
// k_dfgen: one 256-thread workgroup per grid point.  Wavefront a integrates Gauss-Laguerre family alpha = a + 1, a lane
// one node (tables of more than 64 points stride); the wavefront walks the hadron list in order, its operands
// (mass, degeneracy, baryon, sign) wave-uniform loads, the baryon test a uniform branch.  The lanes are summed by a
// fixed xor-shuffle tree, the four wavefronts meet in LDS and thread 0 closes the point (dfgen_math.h close_point).
// No atomics, no dependence on the grid a point sits in: a value is a pure function of (list, table, T, muB).
#include <hip/hip_runtime.h>

#include <string>

#include "devbuf.h"
#include "dfgen.h"
#include "dfgen_math.h"

namespace is3d {
namespace dfgen {

template <int FAM>
__device__ void family_sums(double* sh, int lane, int npts, const double* __restrict__ roots, const double* __restrict__ wts,
                            int nh, const double* __restrict__ had, double T, double muB) {
  constexpr int n = Family<FAM>::n;
  double tot[n];
  lane_sums<FAM>(tot, lane, npts, roots + (FAM - 1) * npts, wts + (FAM - 1) * npts, nh, had, T, muB);
#pragma unroll
  for (int i = 0; i < n; i++) {
    double v = tot[i];
#pragma unroll
    for (int off = kLanes / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, kLanes);
    if (lane == 0) sh[Family<FAM>::slot(i)] = v;
  }
}

__global__ __launch_bounds__(256) void k_dfgen(int nh, const double* __restrict__ had, int npts,
                                               const double* __restrict__ roots, const double* __restrict__ wts, int nT,
                                               long npoint, const double* __restrict__ Tarr,
                                               const double* __restrict__ muBarr, double* __restrict__ out,
                                               int* __restrict__ codes) {
  __shared__ double sh[kSlots];
  const long pt = blockIdx.x;
  if (pt >= npoint) return;
  const double T = Tarr[pt % nT], muB = muBarr[pt / nT];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  if (wave == 0) family_sums<1>(sh, lane, npts, roots, wts, nh, had, T, muB);
  else if (wave == 1) family_sums<2>(sh, lane, npts, roots, wts, nh, had, T, muB);
  else if (wave == 2) family_sums<3>(sh, lane, npts, roots, wts, nh, had, T, muB);
  else family_sums<4>(sh, lane, npts, roots, wts, nh, had, T, muB);
  __syncthreads();
  if (threadIdx.x == 0) {
    double I[kSlots], o[10];
#pragma unroll
    for (int k = 0; k < kSlots; k++) I[k] = sh[k];
    codes[pt] = close_point(I, T, o);
#pragma unroll
    for (int k = 0; k < 10; k++) out[k * npoint + pt] = o[k];
  }
}

std::string generate(int nh, const double* had, int npts, const double* roots, const double* wts, int nT, int nmuB,
                     const double* T, const double* muB, double* tables, int* codes) {
  const long npoint = (long)nT * nmuB;
  const long nhad = (long)kHadronStride * nh, ngl = (long)kFamilies * npts;
  // one blob: had | roots | wts | T | muB | out[10][npoint]
  DevBuf<double> d;
  DevBuf<int> dc;
  if (!d.reserve(nhad + 2 * ngl + nT + nmuB + 10 * npoint) || !dc.reserve(npoint)) return "hipMalloc(df tables) failed";
  double* const d_had = d.get();
  double* const d_roots = d_had + nhad;
  double* const d_wts = d_roots + ngl;
  double* const d_T = d_wts + ngl;
  double* const d_muB = d_T + nT;
  double* const d_out = d_muB + nmuB;
  auto up = [](double* dst, const double* src, long n) {
    return hipMemcpy(dst, src, (size_t)n * sizeof(double), hipMemcpyHostToDevice);
  };
  hipError_t h = up(d_had, had, nhad);
  if (h == hipSuccess) h = up(d_roots, roots, ngl);
  if (h == hipSuccess) h = up(d_wts, wts, ngl);
  if (h == hipSuccess) h = up(d_T, T, nT);
  if (h == hipSuccess) h = up(d_muB, muB, nmuB);
  if (h != hipSuccess) return std::string("hipMemcpy(df generator inputs): ") + hipGetErrorString(h);
  hipLaunchKernelGGL(k_dfgen, dim3((unsigned)npoint), dim3(256), 0, 0, nh, d_had, npts, d_roots, d_wts, nT, npoint, d_T,
                     d_muB, d_out, dc.get());
  h = hipGetLastError();
  if (h == hipSuccess) h = hipDeviceSynchronize();
  if (h == hipSuccess) h = hipMemcpy(tables, d_out, (size_t)(10 * npoint) * sizeof(double), hipMemcpyDeviceToHost);
  if (h == hipSuccess) h = hipMemcpy(codes, dc.get(), (size_t)npoint * sizeof(int), hipMemcpyDeviceToHost);
  if (h != hipSuccess) return std::string("k_dfgen: ") + hipGetErrorString(h);
  return "";
}

}  // namespace dfgen
}  // namespace is3d
