// polzn.h -- private interface between engine_post.hip and the spin-polarization kernels (polzn.hip).
//
// The mode-5 output of the reference (EmissionFunctionArray::calculate_spin_polzn, Polarization.cpp:25-263):
// S_t, S_x, S_y, S_n, Snorm [species][pT][phi][y] summed over freeze-out cells.  The math and the two deliberate
// departures from the reference are in polzn_math.h; the engine owns every buffer and passes plain pointers.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "devbuf.h"

namespace is3d {
namespace polzn {

// device constants of one (species, classes, grid, dimension) setup: one blob of doubles, one of ints
struct Tables {
  DevBuf<double> d;                // the blobs the views below point into (move-only)
  DevBuf<int> i;
  int npart = 0, ncls = 0, npT = 0, nphi = 0, nq = 0, ny_out = 0, dim3d = 0;
  const double *cmass = nullptr, *csign = nullptr, *pT = nullptr, *cphi = nullptr, *sphi = nullptr, *qv = nullptr, *qw = nullptr;
  const int *cmem_off = nullptr, *cmem = nullptr;   // members (original species indices) of each class
  long out_size() const { return 5L * npart * npT * nphi * ny_out; }
};

// Integrand classes: species with identical (mass, sign) share one class when `classes` is on (the degeneracy is
// not used, Polarization.cpp:145).  2+1D: y = 0 only, q runs over the eta table with
// w = eta weight x (eta[1] - eta[0]) (Polarization.cpp:58,68); 3+1D: q runs over the y table, w = 1.
// Returns an empty string, or what is wrong with the inputs / the device.
std::string tables_build(Tables& t, int dimension, bool classes, const std::vector<double>& mass,
                         const std::vector<double>& sign, const std::vector<double>& pT, const std::vector<double>& phi,
                         const std::vector<double>& y, const std::vector<double>& eta, const std::vector<double>& eta_w);

// launch plan of nw cells: a workgroup owns one pT and one cell range (split); each split writes its own partial
// slab, summed by k_polzn_reduce in split order (no atomics: bit-reproducible)
struct Plan {
  int kj = 8;            // phi points per lane
  int njb = 1;           // phi blocks
  int tile = 8;          // cells per LDS tile
  long ntask = 0;        // lanes: class x q x phi block
  int nbx = 1;           // workgroups per (pT, split)
  long nsplit = 1, cells_per_split = 0;
  long sstride = 0;      // doubles per slab
  size_t lds = 0;
  bool ok = false;       // false: the phi / y tables do not fit the LDS tile
};
Plan make_plan(const Tables& t, long nw, long max_splits, long split_bytes, long slab_bytes);

// k_polzn over cells [lo, hi) of the SoA surface surf[25][n] and vorticity vort[6][n] into slab, then
// k_polzn_reduce into dev_out[5][species][pT][phi][y]; `mid` (optional) is recorded between the two
hipError_t enqueue(const Tables& t, const Plan& p, const double* surf, const double* vort, long n, long lo, long hi,
                   double T_avg, double* slab, double* dev_out, hipStream_t st, hipEvent_t mid);

}  // namespace polzn
}  // namespace is3d
