// polzn.hip -- spin polarization from thermal vorticity (mode 5) on gfx950: k_polzn + k_polzn_reduce.
//
// The same shape as k_spectra (kernels.h): a (cell x class x pT x phi x q) FP64 sum, here with five accumulators
// per momentum point (S_t, S_x, S_y, S_n, Snorm), no delta-f and one temperature for the whole surface
// (Polarization.cpp:25-263; the math, its exactness rules and the two departures from the reference are in
// polzn_math.h).
//
// Work decomposition: a lane owns one (class, q, phi block) -- q = y (3+1D) or the eta node (2+1D, summed by the
// reduction) -- and keeps KJ x 5 accumulators in VGPRs (KJ = 8 phi points: 80 VGPRs; a whole 32-point phi row
// would need 320); a workgroup of 256 lanes owns one pT and one cell range.  Per tile of cells the workgroup
// builds, in LDS, the cells, the (cell, q) terms (one cosh / sinh pair each) and the (cell, phi) terms (one exp
// each); a lane then pays one exp per (cell, KJ points) and ~20 FP64 operations plus a quarter division per point.
// Every cell range writes its own slab; k_polzn_reduce adds the slabs (and the eta nodes) in a fixed order and
// writes -1/(4m) x the sum to every member species of the class.
#include "polzn.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "polzn_math.h"

namespace is3d {
namespace polzn {

namespace {

constexpr int kWg = 256;
constexpr int kFillWgs = 2048;            // workgroups the cell splits aim for
constexpr size_t kLdsBudget = 48 * 1024;  // per workgroup: three fit a CU's 160 KB
constexpr int kCellBytes = 15 * 8;        // surface + vorticity bytes k_polzn reads per cell

struct Args {
  const double *surf, *vort;
  long n, lo, hi, cells_per_split;
  double T;
  const double *cmass, *csign, *pT, *cphi, *sphi, *qv, *qw;
  int ncls, npT, nphi, nq, njb, tile, dim3d;
  long ntask;
  double* slab;
  long sstride;
};

// slab[split][c][class][pT][phi][q]
__device__ __forceinline__ long slab_index(const Args& A, int c, int cls, int ipT, int j, int q) {
  return ((((long)c * A.ncls + cls) * A.npT + ipT) * A.nphi + j) * A.nq + q;
}

template <int KJ>
__global__ __launch_bounds__(kWg) void k_polzn(Args A) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x;
  const int nphp = A.njb * KJ;
  Cell* sc = reinterpret_cast<Cell*>(lds);
  QTerm* sq = reinterpret_cast<QTerm*>(lds + (size_t)kCellDoubles * A.tile);
  PhiTerm* sf = reinterpret_cast<PhiTerm*>(lds + (size_t)(kCellDoubles + 6 * A.nq) * A.tile);

  const int ipT = blockIdx.y;
  const double pT = A.pT[ipT];
  const long t = (long)blockIdx.x * kWg + tid;
  const bool valid = t < A.ntask;
  const long tt = valid ? t : 0;
  const int cls = (int)(tt % A.ncls);
  const int q = (int)((tt / A.ncls) % A.nq);
  const int jb = (int)(tt / ((long)A.ncls * A.nq));
  const double m = A.cmass[cls], s = A.csign[cls], w = A.qw[q];
  const double mT = sqrt(m * m + pT * pT);

  const long c_lo = A.lo + (long)blockIdx.z * A.cells_per_split;
  const long c_hi = c_lo + A.cells_per_split < A.hi ? c_lo + A.cells_per_split : A.hi;

  double acc[KJ][5];
#pragma unroll
  for (int j = 0; j < KJ; j++)
#pragma unroll
    for (int c = 0; c < 5; c++) acc[j][c] = 0.0;

  // surface fields of Cell slots 0..8: tau eta dat dax day dan ux uy un (is3d_surface order)
  constexpr int kField[9] = {0, 3, 4, 5, 6, 7, 8, 9, 10};
  for (long base = c_lo; base < c_hi; base += A.tile) {
    const int nt = (int)(c_hi - base < A.tile ? c_hi - base : A.tile);
    __syncthreads();                       // the previous tile's tables are no longer read
    for (int i = tid; i < nt * 15; i += kWg) {
      const int ci = i / 15, f = i % 15;
      double* dst = reinterpret_cast<double*>(&sc[ci]);
      if (f < 9) dst[f] = A.surf[(long)kField[f] * A.n + base + ci];
      else dst[f + 1] = A.vort[(long)(f - 9) * A.n + base + ci];
    }
    __syncthreads();
    if (tid < nt) cell_finish(sc[tid], A.T);
    __syncthreads();
    for (int i = tid; i < nt * A.nq; i += kWg) {
      const int ci = i / A.nq, qi = i % A.nq;
      const double d = A.dim3d ? A.qv[qi] - sc[ci].eta : 0.0 - A.qv[qi];
      sq[ci * A.nq + qi] = q_terms(sc[ci], d, A.qw[qi], A.T);
    }
    for (int i = tid; i < nt * nphp; i += kWg) {
      const int ci = i / nphp, j = i % nphp;
      PhiTerm f{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};          // padding of the last phi block: x = 0
      if (j < A.nphi) f = phi_terms(sc[ci], pT * A.cphi[j], pT * A.sphi[j], pT, A.T);
      sf[ci * nphp + j] = f;
    }
    __syncthreads();
    if (valid) {
      for (int ci = 0; ci < nt; ci++) {
        const Lane L = lane_setup(sq[ci * A.nq + q], mT, pT * sc[ci].hT);
        points<KJ>(L, sf + ci * nphp + jb * KJ, s, w, acc);
      }
    }
  }
  if (!valid) return;
  double* slab = A.slab + (long)blockIdx.z * A.sstride;
#pragma unroll
  for (int jj = 0; jj < KJ; jj++) {
    const int j = jb * KJ + jj;
    if (j < A.nphi) {
#pragma unroll
      for (int c = 0; c < 5; c++) slab[slab_index(A, c, cls, ipT, j, q)] = acc[jj][c];
    }
  }
}

struct RedArgs {
  const double* slab;
  long sstride, nsplit;
  int npart, ncls, npT, nphi, nq, ny_out;
  const double* cmass;
  const int *cmem_off, *cmem;
  double* out;     // [5][species][pT][phi][y]
};

// one thread per (component, class, pT, phi, y): the sum over eta nodes (2+1D) and cell splits in a fixed order,
// x -1/(4m) for the four spin components (Polarization.cpp:190-194), written to every member species
__global__ __launch_bounds__(kWg) void k_polzn_reduce(RedArgs A) {
  const long per = (long)A.npT * A.nphi * A.ny_out;
  const long total = 5L * A.ncls * per;
  const long o = (long)blockIdx.x * kWg + threadIdx.x;
  if (o >= total) return;
  const long r = o % per;
  const int cls = (int)((o / per) % A.ncls), c = (int)(o / (per * A.ncls));
  const int k = (int)(r % A.ny_out);
  const long pj = r / A.ny_out;              // ipT * nphi + j
  const long base = (((long)c * A.ncls + cls) * A.npT * A.nphi + pj) * A.nq;
  const int q0 = A.ny_out == 1 ? 0 : k, q1 = A.ny_out == 1 ? A.nq : k + 1;
  double acc = 0.0;
  for (int q = q0; q < q1; q++)
    for (long z = 0; z < A.nsplit; z++) acc += A.slab[z * A.sstride + base + q];
  const double v = c < 4 ? acc * (-0.25 / A.cmass[cls]) : acc;
  for (int mm = A.cmem_off[cls]; mm < A.cmem_off[cls + 1]; mm++)
    A.out[((long)c * A.npart + A.cmem[mm]) * per + r] = v;
}

}  // namespace

std::string tables_build(Tables& t, int dimension, bool classes, const std::vector<double>& mass,
                         const std::vector<double>& sign, const std::vector<double>& pT, const std::vector<double>& phi,
                         const std::vector<double>& y, const std::vector<double>& eta, const std::vector<double>& eta_w) {
  t = Tables{};
  const int np = (int)mass.size();
  if (np <= 0 || pT.empty() || phi.empty()) return "species / pT / phi tables are empty";
  std::vector<double> qv, qw;
  if (dimension == 3) {
    if (y.empty()) return "3+1D polarization needs the y table";
    qv = y;
    qw.assign(y.size(), 1.0);
  } else {
    // delta_eta = eta_tab(2) - eta_tab(1), read unconditionally by the reference (Polarization.cpp:58)
    if (eta.size() < 2 || eta_w.size() != eta.size()) return "2+1D polarization needs an eta table of at least two nodes";
    const double delta_eta = eta[1] - eta[0];
    qv = eta;
    for (size_t k = 0; k < eta.size(); k++) qw.push_back(eta_w[k] * delta_eta);
  }
  // classes in order of first appearance; bitwise-equal (mass, sign) only
  std::vector<double> cmass, csign;
  std::vector<std::vector<int>> mem;
  for (int s = 0; s < np; s++) {
    int hit = -1;
    for (int c = 0; classes && c < (int)cmass.size(); c++)
      if (!std::memcmp(&cmass[c], &mass[s], sizeof(double)) && !std::memcmp(&csign[c], &sign[s], sizeof(double))) { hit = c; break; }
    if (hit < 0) { hit = (int)cmass.size(); cmass.push_back(mass[s]); csign.push_back(sign[s]); mem.emplace_back(); }
    mem[hit].push_back(s);
  }
  const int nc = (int)cmass.size(), npT = (int)pT.size(), nphi = (int)phi.size(), nq = (int)qv.size();
  std::vector<double> hd;
  std::vector<int> hi;
  auto put = [&](const std::vector<double>& v) { const size_t o = hd.size(); hd.insert(hd.end(), v.begin(), v.end()); return o; };
  std::vector<double> cphi(nphi), sphi(nphi);
  for (int j = 0; j < nphi; j++) { cphi[j] = std::cos(phi[j]); sphi[j] = std::sin(phi[j]); }   // Polarization.cpp:33-38
  const size_t o_m = put(cmass), o_s = put(csign), o_pT = put(pT), o_c = put(cphi), o_sn = put(sphi), o_qv = put(qv), o_qw = put(qw);
  hi.push_back(0);
  for (int c = 0; c < nc; c++) hi.push_back(hi.back() + (int)mem[c].size());
  for (int c = 0; c < nc; c++) hi.insert(hi.end(), mem[c].begin(), mem[c].end());
  if (!t.d.reserve((long)hd.size()) || !t.i.reserve((long)hi.size()) ||
      hipMemcpy(t.d.get(), hd.data(), hd.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(t.i.get(), hi.data(), hi.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
    t = Tables{};
    return "hipMalloc / upload of the polarization tables failed";
  }
  t.npart = np; t.ncls = nc; t.npT = npT; t.nphi = nphi; t.nq = nq; t.dim3d = dimension == 3;
  t.ny_out = dimension == 3 ? nq : 1;
  const double* d = t.d.get();
  t.cmass = d + o_m; t.csign = d + o_s; t.pT = d + o_pT; t.cphi = d + o_c; t.sphi = d + o_sn;
  t.qv = d + o_qv; t.qw = d + o_qw;
  t.cmem_off = t.i.get(); t.cmem = t.i.get() + nc + 1;
  return "";
}

Plan make_plan(const Tables& t, long nw, long max_splits, long split_bytes, long slab_bytes) {
  Plan p;
  p.kj = t.nphi == 1 ? 1 : t.nphi <= 4 ? 4 : 8;
  p.njb = (t.nphi + p.kj - 1) / p.kj;
  const size_t per_cell = (size_t)(kCellDoubles + 6 * t.nq + 6 * p.njb * p.kj) * sizeof(double);
  p.tile = 8;
  while (p.tile > 1 && per_cell * p.tile > kLdsBudget) p.tile /= 2;
  p.lds = per_cell * p.tile;
  if (p.lds > 64 * 1024 || t.npT > 65535) return p;
  p.ntask = (long)t.ncls * t.nq * p.njb;
  p.nbx = (int)((p.ntask + kWg - 1) / kWg);
  p.sstride = 5L * t.ncls * t.npT * t.nphi * t.nq;
  const long tiles = std::max(1L, (nw + p.tile - 1) / p.tile);
  const long by_bytes = (nw * kCellBytes + std::max(1L, split_bytes) - 1) / std::max(1L, split_bytes);
  const long by_fill = (kFillWgs + (long)p.nbx * t.npT - 1) / ((long)p.nbx * t.npT);
  long ns = std::max(by_bytes, by_fill);
  ns = std::min(ns, std::max(1L, slab_bytes / (p.sstride * (long)sizeof(double))));
  ns = std::max(1L, std::min({ns, std::max(1L, max_splits), tiles, 65535L}));
  const long tiles_per = (tiles + ns - 1) / ns;
  p.cells_per_split = tiles_per * p.tile;
  p.nsplit = std::max(1L, (nw + p.cells_per_split - 1) / p.cells_per_split);
  p.ok = true;
  return p;
}

hipError_t enqueue(const Tables& t, const Plan& p, const double* surf, const double* vort, long n, long lo, long hi,
                   double T_avg, double* slab, double* dev_out, hipStream_t st, hipEvent_t mid) {
  Args a{};
  a.surf = surf; a.vort = vort; a.n = n; a.lo = lo; a.hi = hi; a.cells_per_split = p.cells_per_split; a.T = T_avg;
  a.cmass = t.cmass; a.csign = t.csign; a.pT = t.pT; a.cphi = t.cphi; a.sphi = t.sphi; a.qv = t.qv; a.qw = t.qw;
  a.ncls = t.ncls; a.npT = t.npT; a.nphi = t.nphi; a.nq = t.nq; a.njb = p.njb; a.tile = p.tile; a.dim3d = t.dim3d;
  a.ntask = p.ntask; a.slab = slab; a.sstride = p.sstride;
  const dim3 grid((unsigned)p.nbx, (unsigned)t.npT, (unsigned)p.nsplit), block(kWg);
  switch (p.kj) {
    case 1: hipLaunchKernelGGL(k_polzn<1>, grid, block, p.lds, st, a); break;
    case 4: hipLaunchKernelGGL(k_polzn<4>, grid, block, p.lds, st, a); break;
    default: hipLaunchKernelGGL(k_polzn<8>, grid, block, p.lds, st, a); break;
  }
  hipError_t h = hipGetLastError();
  if (h != hipSuccess) return h;
  if (mid && (h = hipEventRecord(mid, st)) != hipSuccess) return h;
  RedArgs r{};
  r.slab = slab; r.sstride = p.sstride; r.nsplit = p.nsplit;
  r.npart = t.npart; r.ncls = t.ncls; r.npT = t.npT; r.nphi = t.nphi; r.nq = t.nq; r.ny_out = t.ny_out;
  r.cmass = t.cmass; r.cmem_off = t.cmem_off; r.cmem = t.cmem; r.out = dev_out;
  const long total = 5L * t.ncls * t.npT * t.nphi * t.ny_out;
  hipLaunchKernelGGL(k_polzn_reduce, dim3((unsigned)((total + kWg - 1) / kWg)), block, 0, st, r);
  return hipGetLastError();
}

}  // namespace polzn
}  // namespace is3d
