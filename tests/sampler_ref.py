"""Helpers of the particle-sampler tests: the host build of is3d2_amd/csrc/sampler_math.h
(tests/native/sampler_emulator.cpp), the derived statistical bars, the numerically integrated thermal CDF and the
physics cases (sampled moments against the oracle's continuous spectra) that the CPU and the GPU tier share.

The bars are fixed by the issue, not tuned: a count with expectation mu passes within 5 sqrt(mu), a mean within 5
standard errors, a Kolmogorov-Smirnov distance below sqrt(ln(2 / alpha) / (2 n)) with alpha = 1e-9."""
import ctypes as C
import os
import subprocess

import numpy as np

from is3d2_amd import make_spec, synth
from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_SRC = os.path.join(HERE, "native", "sampler_emulator.cpp")
EMU_LIB = os.path.join(HERE, "native", "libsampler_emulator.so")
ALPHA = 1e-9
PARTICLE_DTYPE = [("species", "<i4"), ("event", "<i4"), ("cell", "<i8")] + \
                 [(k, "<f8") for k in ("tau", "x", "y", "eta", "t", "z", "E", "px", "py", "pz")]


def emulator():
    srcs = [EMU_SRC] + [os.path.join(ROOT, "is3d2_amd", "csrc", h) for h in ("sampler_math.h", "cf_math.h", "spline_host.h")]
    if not os.path.exists(EMU_LIB) or any(os.path.getmtime(s) > os.path.getmtime(EMU_LIB) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", EMU_LIB, EMU_SRC])
    lib = C.CDLL(EMU_LIB)
    pd, pl, pu = C.POINTER(C.c_double), C.POINTER(C.c_long), C.POINTER(C.c_uint)
    lib.smp_philox.argtypes = [pu, pu, pu]
    lib.smp_philox.restype = None
    lib.smp_uniforms.argtypes = [C.c_long, C.c_int, C.c_long, C.c_long, C.c_long, C.c_int, pd]
    lib.smp_uniforms.restype = None
    lib.smp_poisson.argtypes = [C.c_long, C.c_double, C.c_long, pl]
    lib.smp_poisson.restype = C.c_long
    lib.smp_momentum.argtypes = [C.c_long, C.c_double, C.c_double, C.c_double, C.c_long, pd]
    lib.smp_momentum.restype = C.c_long
    lib.smp_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, pd, C.c_long, C.c_long, C.c_double, C.c_int, C.c_long,
                               C.c_long, pl, pl, C.c_void_p, C.c_long]
    lib.smp_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, pd, C.c_long, C.c_double, C.c_int, C.c_long, C.c_long, pd,
                              C.c_long]
    lib.smp_trace.restype = C.c_long
    return lib


def philox(ctr, key):
    c = (C.c_uint * 4)(*ctr); k = (C.c_uint * 2)(*key); o = (C.c_uint * 4)()
    emulator().smp_philox(c, k, o)
    return list(o)


def uniforms(seed, purpose, cell, event, candidate, n):
    out = np.zeros(n)
    emulator().smp_uniforms(seed, purpose, cell, event, candidate, n, out.ctypes.data_as(C.POINTER(C.c_double)))
    return out


def poisson(seed, mean, n):
    out = np.zeros(n, dtype=np.int64)
    capped = emulator().smp_poisson(seed, mean, n, out.ctypes.data_as(C.POINTER(C.c_long)))
    return out, capped


def momentum(seed, mbar, sign, chem, n):
    """(pbar, costheta, phi, branch, proposals)[n] and the number of capped draws."""
    out = np.zeros((n, 5))
    capped = emulator().smp_momentum(seed, mbar, sign, chem, n, out.ctypes.data_as(C.POINTER(C.c_double)))
    return out, capped


STATS = ("live_cells", "breakdown", "candidates", "kept", "proposals", "acceptances", "capped", "clamped")


def sample(spec, surf, plasma, seed, n_events, y_cut=0.5, fast=0, lo=0, hi=None, keep=0):
    """The serial sampler over cells [lo, hi): (kept counts per species, stats dict, first `keep` particles)."""
    lib = emulator()
    inp = O._Inputs(spec, surf, plasma[0], 1)
    n = len(surf["tau"])
    pl = np.ascontiguousarray(plasma, dtype=np.float64)
    counts = np.zeros(len(spec["species"]["mass"]), dtype=np.int64)
    stats = np.zeros(8, dtype=np.int64)
    parts = np.zeros(max(keep, 1), dtype=PARTICLE_DTYPE)
    lp = C.POINTER(C.c_long)
    rc = lib.smp_sample(C.byref(inp.params), C.byref(inp.setup), C.byref(inp.surf), pl.ctypes.data_as(C.POINTER(C.c_double)),
                        seed, n_events, y_cut, fast, lo, n if hi is None else hi, counts.ctypes.data_as(lp),
                        stats.ctypes.data_as(lp), C.c_void_p(parts.ctypes.data if keep else 0), keep)
    assert rc == 0, "sampler emulator rc=%d" % rc
    st = dict(zip(STATS, [int(v) for v in stats]))
    return counts, st, parts[:min(keep, st["kept"])]


def trace(spec, surf, plasma, seed, cell, event, y_cut=0.5, fast=0, cap=4096):
    """The candidates of one (cell, event), rows (species, kept, keep draw u, keep weight, proposals, inconsistent):
    what a structural mismatch between the device and the emulator is read from."""
    inp = O._Inputs(spec, surf, plasma[0], 1)
    pl = np.ascontiguousarray(plasma, dtype=np.float64)
    out = np.zeros((cap, 6))
    pd = C.POINTER(C.c_double)
    n = emulator().smp_trace(C.byref(inp.params), C.byref(inp.setup), C.byref(inp.surf), pl.ctypes.data_as(pd), seed, y_cut,
                             fast, cell, event, out.ctypes.data_as(pd), cap)
    assert n >= 0, "sampler emulator rc=%d" % n
    return out[:min(n, cap)]


# --- the derived bars ---------------------------------------------------------------------------------------
def ks_bar(n):
    return float(np.sqrt(np.log(2.0 / ALPHA) / (2.0 * n)))


def ks_distance(x, cdf):
    """sup |F_n - F| of the sample x against the callable cdf."""
    x = np.sort(np.asarray(x))
    n = len(x)
    F = cdf(x)
    return float(max(np.max(np.arange(1, n + 1) / n - F), np.max(F - np.arange(0, n) / n)))


def thermal_cdf(mbar, sign, chem, pmax=None, npts=400001):
    """CDF of p^2 / (exp(sqrt(p^2 + mbar^2) - chem) + sign) on [0, pmax] by the composite Simpson rule (the
    neglected tail beyond pmax = mbar + 80 is < 1e-30)."""
    pmax = pmax or (mbar + 80.0)
    p = np.linspace(0.0, pmax, npts)
    f = p * p / (np.exp(np.sqrt(p * p + mbar * mbar) - chem) + sign)
    h = p[1] - p[0]
    # Simpson on pairs of intervals: the cumulative at the even nodes
    pair = (f[0:-2:2] + 4.0 * f[1:-1:2] + f[2::2]) * (h / 3.0)
    cum_even = np.concatenate([[0.0], np.cumsum(pair)])
    pe = p[::2]
    total = cum_even[-1]

    def cdf(x):
        # between even nodes (4e-4 apart) the cumulative is interpolated linearly: an error of f' (2h)^2 / 8 ~ 1e-8 of
        # the total, far below the KS bars (7e-3 at n = 2e5)
        return np.interp(x, pe, cum_even) / total
    return cdf


def spectra_moments(spec, surf, y_cut, threads=1):
    """Per species (N of one event = 2 y_cut dN/dy, <pT>, v2 = <cos 2 phi>, std of pT) from the oracle's continuous
    spectra and the momentum tables' quadrature weights (2+1D: one y slot)."""
    npart = len(spec["species"]["mass"])
    dN = O.spectra(spec, surf, threads=threads).reshape(npart, len(spec["pT"]), len(spec["phi"]), -1)[..., 0]
    w = spec["pT_w"][:, None] * spec["phi_w"][None, :]
    pT = spec["pT"][:, None]
    n = (w * dN).sum(axis=(1, 2))
    m1 = (w * pT * dN).sum(axis=(1, 2)) / n
    m2 = (w * pT * pT * dN).sum(axis=(1, 2)) / n
    v2 = (w * np.cos(2.0 * spec["phi"])[None, :] * dN).sum(axis=(1, 2)) / n
    return 2.0 * y_cut * n, m1, v2, np.sqrt(m2 - m1 * m1)


# --- the physics cases: sampled moments against the oracle's continuous spectra -----------------------------------
# Shared by tests/test_sampler_cpu.py (the emulator) and tests/test_gpu_sampler_physics.py (Engine.sample).  Every
# case: pi, K, p; outflow = 1 and regulate_deltaf = 1 (the oracle's integrand is then the sampler's density term by
# term); y_cut = 0.5; synth.surface(300, seed = 37, ...).  Event counts: the largest at which the quadrature
# uncertainty of the reference (48 x 32 against 24 x 24 momentum tables) stays below a fifth of the statistical sigma.
#   baryon : synth's muB, nB, V with include_baryon = 1 and include_baryondiff_deltaf = 1
#   fast   : fast = 1 with (T, E, P) = (0.150, 0.28, 0.045) on every cell -- the Plasma-average densities of fast = 1
#            are exact only where the averages are the cells' own; synth's normals, pi and Pi are kept
#   route  : "boost": the 2+1D surface with eta ~ U(-2, 2) per cell sampled with dimension = 3.  Integrated over all y
#            a 3+1D cell emits what the 2+1D cell emits per unit rapidity, so N = n_events dN/dy, <pT> and v2 of the
#            2+1D spectra are the expectations, and y - eta_cell is distributed like y of the same cell at eta = 0.
#            "full3d": synth's full3d cells (un, pi^{x eta}, pi^{y eta} != 0, eta ~ U(-4, 4)) with dsigma_eta = 0
#            (the 2+1D integrand does not weight p_eta dsigma^eta by the eta weights).
Y_CUT = 0.5
BARYON_FLAGS = dict(include_baryon=1, include_baryondiff_deltaf=1)
PHYSICS_CASES = {
    "ptm-2d": dict(mode=3, n_events=300),
    "ptb-2d": dict(mode=4, n_events=200),
    "grad-2d-baryon": dict(mode=1, n_events=200, baryon=True),
    "ce-2d-baryon": dict(mode=2, n_events=150, baryon=True),
    "grad-2d-fast": dict(mode=1, n_events=300, fast=1),
    "ptm-2d-fast": dict(mode=3, n_events=300, fast=1),
    "ptb-2d-fast": dict(mode=4, n_events=200, fast=1),
    "ce-3d-boost": dict(mode=2, n_events=300, route="boost"),
    "ptb-3d-boost": dict(mode=4, n_events=150, route="boost"),
    "ce-3d-full": dict(mode=2, n_events=100, route="full3d"),
}
_physics = {}


def rapidity_moments(spec, surf, ny):
    """Per species (<y>, <y^2>, std of y^2) of the oracle's 3+1D spectra on ny rapidities in [-7, 7]: the trapezoid
    rule in y times the pT and phi weights."""
    spec = dict(spec)
    spec["y"] = np.linspace(-7.0, 7.0, ny)
    npart = len(spec["species"]["mass"])
    dN = O.spectra(spec, surf, threads=8).reshape(npart, len(spec["pT"]), len(spec["phi"]), ny)
    y = spec["y"]
    wy = np.full(ny, y[1] - y[0])
    wy[[0, -1]] *= 0.5
    f = ((spec["pT_w"][:, None] * spec["phi_w"][None, :])[None, :, :, None] * dN).sum(axis=(1, 2)) * wy[None, :]
    n = f.sum(axis=1)
    m1, m2, m4 = (f * y).sum(axis=1) / n, (f * y * y).sum(axis=1) / n, (f * y ** 4).sum(axis=1) / n
    return m1, m2, np.sqrt(m4 - m2 * m2)


def physics_inputs(name):
    """The inputs and the reference of one case, computed once: dict of spec (what is sampled), surf, plasma, fast,
    n_events, fine / coarse = (N of one event, <pT>, v2, std pT) per species and, for route = "boost" / "full3d",
    yfine / ycoarse = (<y - eta>, <(y - eta)^2>, std of (y - eta)^2)."""
    if name in _physics:
        return _physics[name]
    c = PHYSICS_CASES[name]
    baryon, route = c.get("baryon", False), c.get("route")
    n = 300
    if route == "full3d":
        s = synth.surface(n, seed=37, dimension=3, full3d=True)
        s["dan"][:] = 0.0
    else:
        s = synth.surface(n, seed=37, baryon=baryon)
    if c.get("fast"):
        s["T"][:] = 0.150
        s["E"][:] = 0.28
        s["P"][:] = 0.045
    if route == "boost":
        s["eta"] = np.random.default_rng(5).uniform(-2.0, 2.0, n)
    s = synth.as_read(s)
    at_rest = dict(s)
    at_rest["eta"] = np.zeros(n)              # what the oracle integrates: the same cells at eta = 0
    flags = dict(chosen="pikp", df_mode=c["mode"], outflow=1, regulate_deltaf=1)
    if baryon:
        flags.update(BARYON_FLAGS)
    fine2, coarse2 = make_spec(pT="pT48", phi="phi32", dimension=2, **flags), make_spec(pT="pT24", phi="phi24", dimension=2, **flags)
    out = dict(case=c, surf=s, n_events=c["n_events"], fast=c.get("fast", 0), plasma=O.averages(s, 1 if baryon else 0),
               fine=spectra_moments(fine2, at_rest, Y_CUT, threads=8), coarse=spectra_moments(coarse2, at_rest, Y_CUT, threads=8))
    out["spec"] = fine2
    if route:
        # the sampler's 3+1D y_max is 0.5 whatever y_cut: N of one event = dN/dy of the 2+1D spectra
        for k in ("fine", "coarse"):
            out[k] = (out[k][0] / (2.0 * Y_CUT),) + out[k][1:]
        fine3, coarse3 = make_spec(pT="pT48", phi="phi32", dimension=3, **flags), make_spec(pT="pT24", phi="phi24", dimension=3, **flags)
        out["spec"] = fine3
        out["yfine"], out["ycoarse"] = rapidity_moments(fine3, at_rest, 113), rapidity_moments(coarse3, at_rest, 57)
    _physics[name] = out
    return out


def check_moments(name, p, st, label):
    """p: the kept particles of the case's n_events events, st: the sampler's counters.  Per species and moment the
    condition on the input |fine - coarse| < sigma / 5 and then |sampled - fine| <= 5 sigma, with sigma = sqrt(mu) for
    a count and std / sqrt(mu) for a mean (the std from the spectra; for v2 = <cos 2 phi> the sampled one, as
    test_gpu_sampler.py does).  Returns (largest |pull|, largest quadrature / sigma)."""
    inp = physics_inputs(name)
    nev, fine, coarse, s = inp["n_events"], inp["fine"], inp["coarse"], inp["surf"]
    assert st["capped"] == 0 and st["kept"] == len(p)
    pT = np.hypot(p["px"], p["py"])
    c2 = np.cos(2.0 * np.arctan2(p["py"], p["px"]))
    rows = []
    for i, mcid in enumerate(inp["spec"]["species"]["mcid"]):
        k = p["species"] == i
        mu = nev * fine[0][i]
        rows += [(mcid, "N", int(k.sum()), mu, np.sqrt(mu), nev * abs(fine[0][i] - coarse[0][i])),
                 (mcid, "<pT>", pT[k].mean(), fine[1][i], fine[3][i] / np.sqrt(mu), abs(fine[1][i] - coarse[1][i])),
                 (mcid, "v2", c2[k].mean(), fine[2][i], c2[k].std() / np.sqrt(mu), abs(fine[2][i] - coarse[2][i]))]
        if "yfine" in inp:
            yf, yc = inp["yfine"], inp["ycoarse"]
            d = 0.5 * np.log((p["E"][k] + p["pz"][k]) / (p["E"][k] - p["pz"][k])) - s["eta"][p["cell"][k]]
            rows += [(mcid, "<y-eta>", d.mean(), yf[0][i], np.sqrt(yf[1][i] - yf[0][i] ** 2) / np.sqrt(mu), abs(yf[0][i] - yc[0][i])),
                     (mcid, "<(y-eta)^2>", (d * d).mean(), yf[1][i], yf[2][i] / np.sqrt(mu), abs(yf[1][i] - yc[1][i]))]
    worst = [0.0, 0.0]
    for mcid, what, g, w, sg, q in rows:
        print("%s %s mcid %d %s: sampled %.6g, spectra %.6g (%.2f sigma), quadrature / sigma %.3f" %
              (label, name, mcid, what, g, w, (g - w) / sg, q / sg))
        worst = [max(worst[0], abs(g - w) / sg), max(worst[1], q / sg)]
    print("%s %s: largest |pull| %.2f, largest quadrature / sigma %.3f" % (label, name, worst[0], worst[1]))
    for mcid, what, g, w, sg, q in rows:
        assert q < sg / 5, (name, int(mcid), what, "the reference's quadrature uncertainty is not below sigma / 5")
        assert abs(g - w) <= 5 * sg, (name, int(mcid), what, g, w, sg)
    return tuple(worst)
