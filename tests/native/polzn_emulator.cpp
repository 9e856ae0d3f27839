// polzn_emulator.cpp -- host build of the spin-polarization kernel's math (test-only).
//
// Runs is3d2_amd/csrc/polzn_math.h -- the functions k_polzn (polzn.hip) calls on the device -- serially, in the
// kernel's structure: per pT, per cell the (cell, q) and (cell, phi) tables, then per lane (species, q, phi block
// of KJ points) lane_setup + points<KJ>; one cell split; the eta nodes (2+1D) are added in k_polzn_reduce's order
// and the four spin components multiplied by -1/(4m).  Built with g++ by tests/test_polzn_cpu.py.
#include <cmath>
#include <vector>

#include "../../is3d2_amd/csrc/polzn_math.h"

using namespace is3d::polzn;

template <int KJ>
static void run(int dim3d, int npart, const double* mass, const double* sign, int npT, const double* pT, int nphi,
                const double* phi, int nq, const double* qv, const double* qw, long n, const double* surf,
                const double* w6, long lo, long hi, double T, double* out) {
  const int njb = (nphi + KJ - 1) / KJ, nphp = njb * KJ;
  const int ny_out = dim3d ? nq : 1;
  const long per = (long)npT * nphi * ny_out;
  std::vector<double> cphi(nphi), sphi(nphi);
  for (int j = 0; j < nphi; j++) { cphi[j] = std::cos(phi[j]); sphi[j] = std::sin(phi[j]); }
  // slab[c][species][pT][phi][q]
  std::vector<double> slab((size_t)5 * npart * npT * nphi * nq, 0.0);
  std::vector<QTerm> sq(nq);
  std::vector<PhiTerm> sf(nphp);
  const int field[9] = {0, 3, 4, 5, 6, 7, 8, 9, 10};
  for (int ipT = 0; ipT < npT; ipT++) {
    for (long c = lo; c < hi; c++) {
      Cell cell;
      double* dst = reinterpret_cast<double*>(&cell);
      for (int f = 0; f < 9; f++) dst[f] = surf[(long)field[f] * n + c];
      for (int f = 9; f < 15; f++) dst[f + 1] = w6[(long)(f - 9) * n + c];
      cell_finish(cell, T);
      for (int qi = 0; qi < nq; qi++) {
        const double d = dim3d ? qv[qi] - cell.eta : 0.0 - qv[qi];
        sq[qi] = q_terms(cell, d, qw[qi], T);
      }
      for (int j = 0; j < nphp; j++) {
        PhiTerm f{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (j < nphi) f = phi_terms(cell, pT[ipT] * cphi[j], pT[ipT] * sphi[j], pT[ipT], T);
        sf[j] = f;
      }
      for (int s = 0; s < npart; s++) {
        const double mT = std::sqrt(mass[s] * mass[s] + pT[ipT] * pT[ipT]);
        for (int q = 0; q < nq; q++) {
          const Lane L = lane_setup(sq[q], mT, pT[ipT] * cell.hT);
          for (int jb = 0; jb < njb; jb++) {
            double acc[KJ][5] = {};
            points<KJ>(L, sf.data() + jb * KJ, sign[s], qw[q], acc);
            for (int jj = 0; jj < KJ; jj++) {
              const int j = jb * KJ + jj;
              if (j >= nphi) continue;
              for (int k = 0; k < 5; k++)
                slab[(((((size_t)k * npart + s) * npT + ipT) * nphi + j) * nq) + q] += acc[jj][k];
            }
          }
        }
      }
    }
  }
  for (int k = 0; k < 5; k++)
    for (int s = 0; s < npart; s++)
      for (long r = 0; r < per; r++) {
        const int y = (int)(r % ny_out);
        const long pj = r / ny_out;
        const size_t base = (((size_t)k * npart + s) * npT * nphi + pj) * nq;
        double acc = 0.0;
        for (int q = (ny_out == 1 ? 0 : y); q < (ny_out == 1 ? nq : y + 1); q++) acc += slab[base + q];
        out[((size_t)k * npart + s) * per + r] = k < 4 ? acc * (-0.25 / mass[s]) : acc;
      }
}

// out[5][species][pT][phi][y]; qv / qw: the y table and ones (3+1D) or the eta table and eta weight x delta eta (2+1D)
extern "C" int polzn_emulate(int dimension, int npart, const double* mass, const double* sign, int npT, const double* pT,
                             int nphi, const double* phi, int nq, const double* qv, const double* qw, long n,
                             const double* surf25, const double* w6, long lo, long hi, double T, int kj, double* out) {
  const int d3 = dimension == 3;
  switch (kj) {
    case 1: run<1>(d3, npart, mass, sign, npT, pT, nphi, phi, nq, qv, qw, n, surf25, w6, lo, hi, T, out); return 0;
    case 4: run<4>(d3, npart, mass, sign, npT, pT, nphi, phi, nq, qv, qw, n, surf25, w6, lo, hi, T, out); return 0;
    case 8: run<8>(d3, npart, mass, sign, npT, pT, nphi, phi, nq, qv, qw, n, surf25, w6, lo, hi, T, out); return 0;
    default: return 1;
  }
}
