"""Helpers of the particle-sampler tests: the host build of is3d2_amd/csrc/sampler_math.h
(tests/native/sampler_emulator.cpp), the derived statistical bars and the numerically integrated thermal CDF.

The bars are fixed by the issue, not tuned: a count with expectation mu passes within 5 sqrt(mu), a mean within 5
standard errors, a Kolmogorov-Smirnov distance below sqrt(ln(2 / alpha) / (2 n)) with alpha = 1e-9."""
import ctypes as C
import os
import subprocess

import numpy as np

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


def spectra_moments(spec, surf, y_cut):
    """Per species (N of one event = 2 y_cut dN/dy, <pT>, v2 = <cos 2 phi>, std of pT) from the oracle's continuous
    spectra and the momentum tables' quadrature weights (2+1D: one y slot)."""
    npart = len(spec["species"]["mass"])
    dN = O.spectra(spec, surf).reshape(npart, len(spec["pT"]), len(spec["phi"]), -1)[..., 0]
    w = spec["pT_w"][:, None] * spec["phi_w"][None, :]
    pT = spec["pT"][:, None]
    n = (w * dN).sum(axis=(1, 2))
    m1 = (w * pT * dN).sum(axis=(1, 2)) / n
    m2 = (w * pT * pT * dN).sum(axis=(1, 2)) / n
    v2 = (w * np.cos(2.0 * spec["phi"])[None, :] * dN).sum(axis=(1, 2)) / n
    return 2.0 * y_cut * n, m1, v2, np.sqrt(m2 - m1 * m1)
