// dfgen.h -- private interface between engine_post.hip and the delta-f coefficient generator (dfgen.hip).
//
// The reference's offline generator (generate_delta_f_coefficients/*/df_vh_dimensionless) as one launch: the ten
// coefficient tables of a hadron list on a (T, muB) grid.  The math is in dfgen_math.h; this unit owns its buffers for
// the length of the call and takes and returns host arrays.
#pragma once
#include <string>

namespace is3d {
namespace dfgen {

// had[nh][4] = (mass, degeneracy, baryon, sign) in list order; roots / wts[4][npts]: the Gauss-Laguerre roots of alpha =
// 1 .. 4 and their node weights w e^root (dfgen_math.h node_weight); T[nT], muB[nmuB].  Fills tables[10][nmuB][nT] and
// codes[nmuB][nT] (dfgen_math.h close_point) on the current device.  Returns an empty string or what the device said.
std::string generate(int nh, const double* had, int npts, const double* roots, const double* wts, int nT, int nmuB,
                     const double* T, const double* muB, double* tables, int* codes);

}  // namespace dfgen
}  // namespace is3d
