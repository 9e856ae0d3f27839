// decay.h -- private interface between engine_post.hip and the resonance-decay feed-down kernels (decay.hip).
//
// The method is in decay_math.h (the reference has no working routine).  The engine owns every buffer (DevBuf
// members) and passes plain pointers; decay.hip packs the plan's tables and launches two kernels per level.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "decay_math.h"

namespace is3d {
namespace decay {

// the plan and the grids as two blobs for the device: doubles (rule, pT, phi, y, the terms) and ints (receivers)
struct Packed {
  std::vector<double> d;
  std::vector<int> i;
  long o_rule = 0, o_pT = 0, o_phi = 0, o_y = 0, o_sub = 0;   // offsets into d
  long o_rd = 0, o_rs0 = 0, o_rs1 = 0, o_par = 0;             // offsets into i
  int npT = 0, nphi = 0, ny = 0;
  int nb = 0;          // (v, zeta) nodes per LDS batch: a divisor of kNodes; 0: the phi table does not fit
  size_t lds = 0;
};
Packed pack(const Plan& P, const Rule& r, const std::vector<double>& pT, const std::vector<double>& phi, int ny,
            const std::vector<double>& y);

// every level of the plan on `st`: k_decay_logs over its parents (into logs, spectra-sized), then k_decay_feed over
// its receivers; S is updated in place
hipError_t enqueue(const Plan& P, const Packed& K, const double* dev_d, const int* dev_i, double* S, double* logs,
                   hipStream_t st);

}  // namespace decay
}  // namespace is3d
