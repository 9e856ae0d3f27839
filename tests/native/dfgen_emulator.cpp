// Host build of is3d2_amd/csrc/dfgen_math.h (test-only): the delta-f coefficient generator on a (T, muB) grid, the
// points shared among OpenMP threads.  Built on demand by tests/df_gen_ref.py.
#include "../../is3d2_amd/csrc/dfgen_math.h"

#include <vector>

using namespace is3d::dfgen;

// had[nh][4] = (mass, degeneracy, baryon, sign); roots / weights[4][npts]: rows alpha = 1 .. 4 of a Gauss-Laguerre
// table; tables[10][nmuB][nT], codes[nmuB][nT] (close_point)
extern "C" int dfgen_emulate(int nh, const double* had, int npts, const double* roots, const double* weights, int nT, int nmuB,
                             const double* T, const double* muB, double* tables, int* codes) {
  const long npoint = (long)nT * nmuB;
  std::vector<double> wts((size_t)kFamilies * npts);
  for (size_t k = 0; k < wts.size(); k++) wts[k] = node_weight(roots[k], weights[k]);
#pragma omp parallel for schedule(dynamic, 1)
  for (long pt = 0; pt < npoint; pt++) {
    double o[10];
    codes[pt] = point_host(npts, roots, wts.data(), nh, had, T[pt % nT], muB[pt / nT], o);
    for (int k = 0; k < 10; k++) tables[k * npoint + pt] = o[k];
  }
  return 0;
}

// the first failing point in the reference's order: its index (-1: none), *code = its dfgen_math.h Code
extern "C" long dfgen_first_error(const int* codes, long n, int* code) { return first_error(codes, n, code); }
extern "C" const char* dfgen_message(int code) { return message(code); }
