"""Helpers of the Monte Carlo decay tests: the ctypes wrapper of the CPU emulator
(tests/native/decay_list_emulator.cpp = is3d2_amd/csrc/decay_mc_math.h compiled for the host), an independent numpy
Monte Carlo (draw_parents, boost_daughter: copies of tests/test_decay_cpu.py's, which a test module cannot import
from), and what the CPU and GPU tiers share: list builders, four-momentum sums per tree, pT-bin counts.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from is3d2_amd import _lib

import decay_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_SRC = os.path.join(HERE, "native", "decay_list_emulator.cpp")
EMU_LIB = os.path.join(HERE, "native", "libdecay_list_emulator.so")
CSRC = os.path.join(ROOT, "is3d2_amd", "csrc")
P_DTYPE = np.dtype(_lib.PARTICLE_DTYPE)
STAT_KEYS = ("primaries", "decays", "undecayed", "dropped_daughters", "capped", "final_particles", "passes")

T = 0.150
V2 = 0.10
PT_BINS = np.array([0.2, 0.5, 0.8, 1.2, 1.8])
PT_BINS_SOFT = np.array([0.1, 0.2, 0.3, 0.45, 0.6])
Y_MAX = 3.0


# pi+, pi-, N, rho, Delta, omega, and X whose channel X -> N pi is closed at the pole masses
MASS = np.array([0.138, 0.138, 0.938, 0.776, 1.232, 0.782, 1.07])
RHO = R.channel(3, [0, 1], 1.0, 0.776, [0.138, 0.138])
DELTA = R.channel(4, [2, 0], 1.0, 1.232, [0.938, 0.138])
OMEGA = R.channel(5, [0, 1, 0], 1.0, 0.782, [0.138, 0.138, 0.138])
# 1.07 < 0.938 + 0.138: one round of the closed-channel rule gives M = 1.095, m_N = 0.928
ADJUSTED = R.channel(6, [2, 0], 1.0, 1.07, [0.938, 0.138], width_parent=0.1, widths=[0.02, 0.0])
TABLE = [RHO, DELTA, OMEGA, ADJUSTED]
# the ulp bars of a tree's four-momentum sum (derived in tests/test_decay_list_cpu.py): 2-body, 3-body
BAR_2BODY, BAR_3BODY = 64, 128


def emulator():
    srcs = [EMU_SRC, os.path.join(ROOT, "include", "is3d_amd.h")] + \
           [os.path.join(CSRC, h) for h in ("decay_mc_math.h", "decay_math.h", "sampler_math.h", "cf_math.h")]
    if not os.path.exists(EMU_LIB) or any(os.path.getmtime(s) > os.path.getmtime(EMU_LIB) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-fopenmp", "-shared", "-o", EMU_LIB, EMU_SRC])
    lib = C.CDLL(EMU_LIB)
    pd = C.POINTER(C.c_double)
    lib.dl_emulate.restype = C.c_long
    lib.dl_emulate.argtypes = [C.c_int, pd, C.c_int, C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_void_p,
                               C.POINTER(C.c_long), C.POINTER(_lib.DecayStats), C.c_char_p, C.c_int]
    lib.dl_fetch.argtypes = [C.c_void_p, C.c_void_p]
    lib.dl_uniforms.argtypes = [C.c_long, C.c_long, C.c_long, C.c_long, C.c_int, pd]
    lib.dl_channels.argtypes = [C.c_int, pd, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.dl_particle_size() == P_DTYPE.itemsize == 96
    return lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def index_in_event(offsets):
    """prim[i]: the index of record i inside its event, for the list [offsets[0], offsets[-1])."""
    offsets = np.asarray(offsets, dtype=np.int64)
    n = int(offsets[-1] - offsets[0])
    start = np.repeat(offsets[:-1] - offsets[0], np.diff(offsets))
    return (np.arange(n) - start).astype(np.uint32)


def emulate(mass, channels, particles, offsets, seed):
    """(particles, offsets, origins, stats, plan_stats) of the emulator; the arguments of Engine.decay_particles."""
    lib = emulator()
    mass = np.ascontiguousarray(mass, dtype=np.float64)
    tab = R.channel_table(channels)
    offsets = np.asarray(offsets, dtype=np.int64)
    i0, n = int(offsets[0]), int(offsets[-1] - offsets[0])
    parts = np.ascontiguousarray(particles[i0:i0 + n], dtype=P_DTYPE)
    prim = index_in_event(offsets)
    st, pst, msg = (C.c_long * 8)(), _lib.DecayStats(), C.create_string_buffer(256)
    m = lib.dl_emulate(len(mass), _dp(mass), len(tab), C.c_void_p(tab.ctypes.data), int(seed), n,
                       C.c_void_p(parts.ctypes.data), C.c_void_p(prim.ctypes.data), st, C.byref(pst), msg, 256)
    if m < 0:
        raise ValueError(msg.value.decode())
    out, origin = np.zeros(m, dtype=P_DTYPE), np.zeros(m, dtype=np.int64)
    lib.dl_fetch(C.c_void_p(out.ctypes.data), C.c_void_p(origin.ctypes.data))
    new_off = np.searchsorted(origin, offsets - i0, side="left").astype(np.int64)
    stats = dict(zip(STAT_KEYS, list(st)[:7]))
    return out, new_off, origin + i0, stats, {k: getattr(pst, k) for k, _ in pst._fields_}


def uniforms(seed, prim, event, path, n):
    out = np.zeros(n)
    emulator().dl_uniforms(int(seed), int(prim), int(event), int(path), n, _dp(out))
    return out


def mc_channels(mass, channels):
    """(list of dicts of the kept channels as the Monte Carlo sees them, level[npart])."""
    lib = emulator()
    mass = np.ascontiguousarray(mass, dtype=np.float64)
    tab = R.channel_table(channels)
    cap = len(tab) + 1
    ints, dbls, level = np.zeros((cap, 5), dtype=np.int32), np.zeros((cap, 8)), np.zeros(len(mass), dtype=np.int32)
    n = lib.dl_channels(len(mass), _dp(mass), len(tab), C.c_void_p(tab.ctypes.data), cap, C.c_void_p(ints.ctypes.data),
                        C.c_void_p(dbls.ctypes.data), C.c_void_p(level.ctypes.data))
    assert n >= 0
    out = [dict(parent=int(ints[q, 0]), nbody=int(ints[q, 1]), d=[int(v) for v in ints[q, 2:5]], cum=dbls[q, 0],
                M=dbls[q, 1], m=list(dbls[q, 2:5]), k=list(dbls[q, 5:8])) for q in range(n)]
    return out, level


# ------------------------------------------------------------------------------------------
# lists
# ------------------------------------------------------------------------------------------
def make_list(species, mass, E=None, px=0.0, py=0.0, pz=0.0, pT=None, phi=None, y=None, event=0, seed=1):
    """A list of records on their pole mass shells with distinct positions and cells.  Give (px, py, pz) or (pT, phi, y)."""
    species = np.atleast_1d(np.asarray(species, dtype=np.int32))
    n = len(species)
    p = np.zeros(n, dtype=P_DTYPE)
    m = np.asarray(mass)[species]
    if pT is not None:
        px, py = pT * np.cos(phi), pT * np.sin(phi)
        mT = np.sqrt(m * m + px * px + py * py)
        p["pz"], p["E"] = mT * np.sinh(y), mT * np.cosh(y)
    else:
        p["pz"] = pz
        p["E"] = np.sqrt(m * m + px * px + py * py + np.asarray(pz, dtype=float) ** 2) if E is None else E
    p["species"], p["event"], p["px"], p["py"] = species, event, px, py
    rng = np.random.default_rng(seed)
    for k in ("tau", "x", "y", "eta", "t", "z"):
        p[k] = rng.uniform(-3, 3, n) if k != "tau" else rng.uniform(0.5, 10, n)
    p["cell"] = rng.integers(0, 1 << 40, n)
    return p


def draw_parents(rng, M, n):
    """(E, px, py, pz) of n parents from S_R = exp(-MT / T)(1 + 2 v2 cos 2 Phi), flat in |Y| < Y_MAX (a copy of
    tests/test_decay_cpu.py's)."""
    x = np.where(rng.uniform(size=n) < T / (T + M), rng.gamma(2.0, T, n), rng.exponential(T, n))
    MT = M + x
    PT = np.sqrt(MT ** 2 - M ** 2)
    Phi = np.empty(n)
    todo = np.arange(n)
    while len(todo):       # rejection under 1 + 2 v2
        p = rng.uniform(0, 2 * np.pi, len(todo))
        ok = rng.uniform(0, 1 + 2 * V2, len(todo)) < 1 + 2 * V2 * np.cos(2 * p)
        Phi[todo[ok]] = p[ok]
        todo = todo[~ok]
    Y = rng.uniform(-Y_MAX, Y_MAX, n)
    return MT * np.cosh(Y), PT * np.cos(Phi), PT * np.sin(Phi), MT * np.sinh(Y)


def boost_daughter(rng, parent, M, m1, p1):
    """Lab (pT, phi, y) of a daughter of mass m1 and rest-frame momentum p1, isotropic (a copy of
    tests/test_decay_cpu.py's)."""
    E, px, py, pz = parent
    n = len(E)
    ct = rng.uniform(-1, 1, n)
    st = np.sqrt(1 - ct ** 2)
    ph = rng.uniform(0, 2 * np.pi, n)
    q = np.stack([p1 * st * np.cos(ph), p1 * st * np.sin(ph), p1 * ct])
    e1 = np.sqrt(p1 ** 2 + m1 ** 2)
    beta = np.stack([px, py, pz]) / E
    gamma = E / M
    bq = np.sum(beta * q, axis=0)
    lab = q + beta * (gamma ** 2 / (gamma + 1) * bq + gamma * e1)
    elab = gamma * (e1 + bq)
    return np.hypot(lab[0], lab[1]), np.arctan2(lab[1], lab[0]), 0.5 * np.log((elab + lab[2]) / (elab - lab[2]))


def flat_dalitz_e1(rng, M, m, n):
    """E1 of n flat-Dalitz decays M -> 3 m by rejection on (E1, E2) (tests/test_decay_cpu.py's generator)."""
    emax = (M * M + m * m - 4 * m * m) / (2 * M)
    E1 = np.empty(n)
    todo = np.arange(n)
    while len(todo):
        e1, e2 = rng.uniform(m, emax, len(todo)), rng.uniform(m, emax, len(todo))
        e3 = M - e1 - e2
        p1, p2 = np.sqrt(e1 ** 2 - m * m), np.sqrt(e2 ** 2 - m * m)
        p3sq = e3 ** 2 - m * m
        ok = (e3 >= m) & (p3sq >= (p1 - p2) ** 2) & (p3sq <= (p1 + p2) ** 2)
        E1[todo[ok]] = e1[ok]
        todo = todo[~ok]
    return E1


def count_bins(pT, phi, y, bins):
    """Particles with |y| < 0.5 per pT bin, and their mean cos 2 phi."""
    sel = np.abs(y) < 0.5
    k = np.digitize(pT[sel], bins) - 1
    ok = (k >= 0) & (k < len(bins) - 1)
    N = np.bincount(k[ok], minlength=len(bins) - 1).astype(float)
    c2 = np.bincount(k[ok], weights=np.cos(2 * phi[sel][ok]), minlength=len(bins) - 1) / N
    return N, c2


def record_bins(p, bins):
    """count_bins of records."""
    return count_bins(np.hypot(p["px"], p["py"]), np.arctan2(p["py"], p["px"]),
                      np.arcsinh(p["pz"] / np.sqrt(p["E"] ** 2 - p["pz"] ** 2)), bins)


def thermal(MT, Phi, Y):
    return np.exp(-MT / T) * (1.0 + 2.0 * V2 * np.cos(2.0 * Phi)) + 0.0 * Y


def predict_bins(M, m1, others, n, bins):
    """The feed-down formula (decay_ref.slot_term) with the exact thermal parent, integrated over the bins, per parent:
    (fraction of the parents, v2) per bin -- tests/test_decay_cpu.py's predict_bins."""
    x, w = np.polynomial.legendre.leggauss(8)
    phi = np.arange(8) * (2 * np.pi / 8)
    norm = 2 * Y_MAX * 2 * np.pi * T * (M + T) * np.exp(-M / T)
    frac, v2 = [], []
    for lo, hi in zip(bins[:-1], bins[1:]):
        pT = 0.5 * (lo + hi) + 0.5 * (hi - lo) * x
        dS, _ = R.slot_term(thermal, 1.0, M, m1, others, pT, phi, [0.0], n)
        f = dS[:, :, 0] * (pT * w * 0.5 * (hi - lo))[:, None] * (2 * np.pi / 8)
        frac.append(f.sum() * 1.0 / norm)
        v2.append((f * np.cos(2 * phi)[None, :]).sum() / f.sum())
    return np.array(frac), np.array(v2)


def check_against_formula(N, c2, n_parents, M, m1, others, bins, label=""):
    """Counts and v2 of one daughter slot against the feed-down formula: 4 sigma of the counting error plus the
    |12 - 24 nodes| quadrature term (tests/test_decay_cpu.py's bound); every bin holds more than 1000."""
    f12, v12 = predict_bins(M, m1, others, 12, bins)
    f24, v24 = predict_bins(M, m1, others, 24, bins)
    quad_N, quad_v = np.abs(f12 - f24) * n_parents, np.abs(v12 - v24)
    pred = f12 * n_parents
    sig_N, sig_v = np.sqrt(pred), np.sqrt(0.5 / pred)
    print(label, "bins", bins, "\n N", N, "\n pred", pred, "\n pull", (N - pred) / sig_N, "\n v2", c2, "\n pred v2", v12,
          "\n pull", (c2 - v12) / sig_v)
    assert np.all(N > 1000)
    assert np.all(np.abs(N - pred) <= 4 * sig_N + quad_N)
    assert np.all(np.abs(c2 - v12) <= 4 * sig_v + quad_v)


def tree_sums(out, origins, n_primaries):
    """Sum of (E, px, py, pz) of the final records of every primary: [n_primaries][4]."""
    s = np.zeros((n_primaries, 4))
    for k, f in enumerate(("E", "px", "py", "pz")):
        s[:, k] = np.bincount(origins, weights=out[f], minlength=n_primaries)
    return s


def ulp(x):
    return np.spacing(np.abs(x))
