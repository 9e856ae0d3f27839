"""numpy restatement of the reference's delta-f coefficient generator (generate_delta_f_coefficients/*/
df_vh_dimensionless: deltaf_table.cpp, thermal_integrands.cpp, gauss_integration.cpp), written from those files in
their own form and loop order -- every integrand as thermal_integrands.cpp spells it, Gauss1D's sum over the nodes in
order, the prefactor applied to every hadron's term, the hadrons added in list order -- and evaluated in np.longdouble
(or any dtype).  Also the ctypes wrapper of the CPU emulator (tests/native/dfgen_emulator.cpp =
is3d2_amd/csrc/dfgen_math.h compiled for the host), the bars of DESIGN.md 7.9 and the small hadron lists the tests share.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from is3d2_amd import data, hrg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_SRC = os.path.join(HERE, "native", "dfgen_emulator.cpp")
EMU_LIB = os.path.join(HERE, "native", "libdfgen_emulator.so")
NAMES = ["c0", "c1", "c2", "c3", "c4", "F", "G", "betabulk", "betaV", "betapi"]
HBARC = 0.197327053
BAR_SHIPPED = 5.0e-7 * (1 + 1e-6)   # half a unit of the files' sixth decimal; the factor covers a value on a tie
BAR_REF = 1e-10                     # against the long-double restatement, of the table's largest entry at the same T
CODES = {1: "Bulk denominator is zero", 2: "Diffusion denominator is zero", 3: "Shear denominator is zero"}

# the grids of the acceptance tests
GRID_4x4 = ((0.1, 0.13, 0.155, 0.2), (0.0, 0.05, 0.4, 0.8))
GRID_WIDE = ((0.1, 0.155, 0.2, 0.3, 0.5), (0.0, 0.4, 0.8, 1.2))
GRID_5x3 = ((0.1, 0.125, 0.15, 0.175, 0.2), (0.0, 0.4, 0.8))      # nodes 0, 25, .. 100 x 0, 40, 80 of the shipped grid


# ------------------------------------------------------------------------------------------
# hadron lists: dicts of mass, gspin, baryon, sign (hrg.pdg_particles' form)
# ------------------------------------------------------------------------------------------
def hadrons(rows):
    a = np.array(rows, dtype=np.float64).reshape(-1, 4)
    return dict(mass=a[:, 0].copy(), gspin=a[:, 1].copy(), baryon=a[:, 2].copy(), sign=a[:, 3].copy())


THREE = hadrons([(0.138, 1, 0, -1), (0.938, 2, 1, 1), (0.938, 2, -1, 1)])     # a meson, a baryon, its antibaryon
MESONS = hadrons([(0.138, 3, 0, -1), (0.494, 4, 0, -1), (0.776, 9, 0, -1)])


@functools.lru_cache(maxsize=None)
def named_list(name):
    """'urqmd', 'smash', 'box': the shipped lists (hrg_eos 1, 2, 3); 'smash65': 65 rows of the SMASH list, the first
    33 and the 32 from the first baryon on, so that one row remains after 64."""
    if name == "smash65":
        p = hrg.pdg_particles(2)
        b0 = int(np.nonzero(p["baryon"] != 0)[0][0])
        idx = np.concatenate([np.arange(33), np.arange(max(b0, 33), max(b0, 33) + 32)])
        return {k: p[k][idx].copy() for k in ("mass", "gspin", "baryon", "sign")}
    return hrg.pdg_particles({"urqmd": 1, "smash": 2, "box": 3}[name])


def gl_rows(points):
    """(roots, weights)[4][points]: rows alpha = 1 .. 4 of the package's Gauss-Laguerre table."""
    r, w = data.gauss_laguerre(points)
    return np.ascontiguousarray(r[1:5]), np.ascontiguousarray(w[1:5])


# ------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------
def _gauss1d(integrand, root, weight):
    """Gauss1D: sum += weight[k] * integrand(root[k]) for k in order (the last axis), as a running sum."""
    return np.cumsum(weight * integrand(root), axis=-1)[..., -1]


def restate(parts, T, muB, points=64, dtype=np.longdouble):
    """(tab[10][nmuB][nT] in dtype, code[nmuB][nT]): deltaf_table.cpp on the grid T x muB for the hadron list `parts`;
    code = the exit(-1) check that fires first at a point (CODES), the 14-moment block's before the other's."""
    ft = dtype
    root, weight = [x.astype(ft) for x in gl_rows(points)]          # [0] is alpha = 1
    Tg, Bg = np.meshgrid(np.asarray(T, dtype=ft), np.asarray(muB, dtype=ft))     # [nmuB][nT]
    Tn, Bn = Tg[..., None], Bg[..., None]
    pi = ft(np.pi) if ft is np.float64 else np.arccos(ft(-1))
    two_pi2_hbarC3 = ft(2) * pi ** 2 * ft(HBARC) ** 3
    f = {k: Tg ** n / (d * two_pi2_hbarC3) for k, (n, d) in dict(
        J20=(4, 1), J21=(4, 3), J40=(6, 1), J41=(6, 3), N10=(3, 1), N30=(5, 1), N31=(5, 3), M20=(4, 1), M21=(4, 3),
        A20=(4, 1), A21=(4, 3), B10=(3, 1), nB=(3, 1), e=(4, 1), p=(4, 3), J30=(5, 1), J32=(5, 15), N20=(4, 1),
        M10=(3, 1), M11=(3, 3)).items()}
    S = {k: np.zeros(Tg.shape, dtype=ft) for k in f}
    for mass, dof, b, Theta in zip(parts["mass"], parts["gspin"], parts["baryon"], parts["sign"]):
        if mass == 0.0:
            continue
        mass, dof, b, Theta = ft(mass), ft(dof), ft(b), ft(Theta)
        mbar = mass / Tn
        mass2 = mass * mass

        def E(p):
            return np.sqrt(p * p + mbar * mbar)

        def ff(p):          # exp(pbar + Ebar - b muB / T) / qstat^2
            q = np.exp(E(p) - b * Bn / Tn) + Theta
            return np.exp(p + E(p) - b * Bn / Tn) / (q * q)

        def f1(p):          # exp(pbar) / (exp(Ebar - b muB / T) + Theta)
            return np.exp(p) / (np.exp(E(p) - b * Bn / Tn) + Theta)

        J20_int = lambda p: E(p) * ff(p)
        J21_int = lambda p: p * p / E(p) * ff(p)
        g2 = (root[1], weight[1])
        S["A20"] += mass2 * dof * f["A20"] * _gauss1d(J20_int, *g2)
        S["A21"] += mass2 * dof * f["A21"] * _gauss1d(J21_int, *g2)
        S["J20"] += dof * f["J20"] * _gauss1d(J20_int, *g2)
        S["J21"] += dof * f["J21"] * _gauss1d(J21_int, *g2)
        S["J40"] += dof * f["J40"] * _gauss1d(lambda p: E(p) * E(p) * E(p) / p / p * ff(p), root[3], weight[3])
        S["J41"] += dof * f["J41"] * _gauss1d(lambda p: E(p) * ff(p), root[3], weight[3])
        S["e"] += dof * f["e"] * _gauss1d(lambda p: E(p) * f1(p), *g2)
        S["p"] += dof * f["p"] * _gauss1d(lambda p: p * p / E(p) * f1(p), *g2)
        S["J30"] += dof * f["J30"] * _gauss1d(lambda p: E(p) * E(p) / p * ff(p), root[2], weight[2])
        S["J32"] += dof * f["J32"] * _gauss1d(lambda p: p * p * p / (E(p) * E(p)) * ff(p), root[2], weight[2])
        if b != 0:
            N10_int = lambda p: b * p * ff(p)
            S["B10"] += mass2 * dof * f["B10"] * _gauss1d(N10_int, root[0], weight[0])
            S["N10"] += dof * f["N10"] * _gauss1d(N10_int, root[0], weight[0])
            S["N30"] += dof * f["N30"] * _gauss1d(lambda p: b * E(p) * E(p) / p * ff(p), root[2], weight[2])
            S["N31"] += dof * f["N31"] * _gauss1d(lambda p: b * p * ff(p), root[2], weight[2])
            S["M20"] += dof * f["M20"] * _gauss1d(lambda p: b * b * E(p) * ff(p), *g2)
            S["M21"] += dof * f["M21"] * _gauss1d(lambda p: b * b * p * p / E(p) * ff(p), *g2)
            S["nB"] += dof * f["nB"] * _gauss1d(lambda p: b * p * f1(p), root[0], weight[0])
            S["N20"] += dof * f["N20"] * _gauss1d(lambda p: b * E(p) * ff(p), *g2)
            S["M10"] += dof * f["M10"] * _gauss1d(lambda p: b * b * p * ff(p), root[0], weight[0])
            S["M11"] += dof * f["M11"] * _gauss1d(lambda p: b * b * p * p * p / (E(p) * E(p)) * ff(p), root[0], weight[0])
    J20, J21, J40, J41, N10, N30, N31, M20, M21, A20, A21, B10 = [S[k] for k in (
        "J20", "J21", "J40", "J41", "N10", "N30", "N31", "M20", "M21", "A20", "A21", "B10")]
    T_ = Tg
    with np.errstate(divide="ignore", invalid="ignore"):
        # update 3/25
        bulk0 = (4 * N30 - B10) * N30 - M20 * (4 * J40 - A20)
        bulk1 = (B10 - N30) * (4 * J40 - A20) - (4 * N30 - B10) * (A20 - J40)
        bulk2 = M20 * (A20 - J40) - (B10 - N30) * N30
        denom = (A21 - J41) * bulk0 + N31 * bulk1 + (4 * J41 - A21) * bulk2
        c0, c1, c2 = bulk0 / denom, bulk1 / denom, bulk2 / denom
        c3 = J41 / (N31 * N31 - M21 * J41)
        c4 = -N31 / (N31 * N31 - M21 * J41)
        grad = np.where(J21 * bulk0 - N31 * bulk1 + J41 * bulk2 == 0, 1, np.where(N31 * N31 - M21 * J41 == 0, 2, 0))
        nB, e, p, J30, J32, N20, M10, M11 = [S[k] for k in ("nB", "e", "p", "J30", "J32", "N20", "M10", "M11")]
        # alphaB form
        G = ((e + p) * N20 - J30 * nB) / (J30 * M10 - N20 * N20)
        F = T_ * T_ * (N20 * nB - (e + p) * M10) / (J30 * M10 - N20 * N20)
        betabulk = G * nB * T_ + F * (e + p) / T_ + 5 * J32 / (3 * T_)
        betaV = M11 - nB * nB * T_ / (e + p)
        betapi = J32 / T_
        ce = np.where(betapi == 0, 3, np.where(betabulk == 0, 1, np.where(betaV == 0, 2, 0)))
        tab = np.stack([c0 * T_ ** 4, c1 * T_ ** 3, c2 * T_ ** 4, c3 * T_ ** 4, c4 * T_ ** 5, F / T_, G, betabulk / T_ ** 4,
                        betaV / T_ ** 3, betapi / T_ ** 4])
    return tab, np.where(grad != 0, grad, ce)


@functools.lru_cache(maxsize=None)
def restated(name, grid, points=64):
    """restate() of a named list on a grid ((T...), (muB...)), computed once per session and left unchanged."""
    tab, code = restate(named_list(name) if isinstance(name, str) else name, grid[0], grid[1], points)
    tab.setflags(write=False)
    return tab, code


# ------------------------------------------------------------------------------------------
# the emulator
# ------------------------------------------------------------------------------------------
def emulator():
    srcs = [EMU_SRC, os.path.join(ROOT, "is3d2_amd", "csrc", "dfgen_math.h")]
    if not os.path.exists(EMU_LIB) or any(os.path.getmtime(s) > os.path.getmtime(EMU_LIB) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-fopenmp", "-shared", "-o", EMU_LIB, EMU_SRC])
    lib = C.CDLL(EMU_LIB)
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int)
    lib.dfgen_emulate.argtypes = [C.c_int, pd, C.c_int, pd, pd, C.c_int, C.c_int, pd, pd, pd, pi]
    lib.dfgen_first_error.restype = C.c_long
    lib.dfgen_first_error.argtypes = [pi, C.c_long, pi]
    lib.dfgen_message.restype = C.c_char_p
    return lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def emulate(parts, T, muB, points=64):
    """(tab[10][nmuB][nT], first_error): dfgen_math.h on the host; first_error = None or (message, T, muB) of the
    first failing point in the reference's order."""
    lib = emulator()
    had = np.ascontiguousarray(np.stack([parts["mass"], parts["gspin"], parts["baryon"], parts["sign"]], axis=1), dtype=np.float64)
    r, w = gl_rows(points)
    T, muB = np.ascontiguousarray(T, dtype=np.float64), np.ascontiguousarray(muB, dtype=np.float64)
    tab = np.zeros((10, len(muB), len(T)))
    codes = np.zeros(len(muB) * len(T), dtype=np.int32)
    pc = codes.ctypes.data_as(C.POINTER(C.c_int))
    lib.dfgen_emulate(len(had), _dp(had), points, _dp(r), _dp(w), len(T), len(muB), _dp(T), _dp(muB), _dp(tab), pc)
    code = C.c_int(0)
    at = lib.dfgen_first_error(pc, len(codes), C.byref(code))
    err = None if at < 0 else (lib.dfgen_message(code.value).decode(), float(T[at % len(T)]), float(muB[at // len(T)]))
    return tab, err


# ------------------------------------------------------------------------------------------
# the bars
# ------------------------------------------------------------------------------------------
def ref_excess(got, ref):
    """max over the entries of |got - ref| / bar, per table (<= 1 passes): bar = BAR_REF x the largest |ref| of the same
    table at the same T; where that is 0 (c1, c4, G on a grid that holds muB = 0 only), BAR_REF x the table's largest
    |ref| over the grid -- and where that too is 0 the entry must be exactly 0."""
    ref = np.asarray(ref)
    err = np.abs(np.asarray(got, dtype=ref.dtype) - ref)
    scale = np.max(np.abs(ref), axis=1, keepdims=True) * np.ones_like(ref)          # [10][1][nT] -> same table, same T
    whole = np.max(np.abs(ref), axis=(1, 2), keepdims=True) * np.ones_like(ref)
    bar = BAR_REF * np.where(scale > 0, scale, whole)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bar > 0, err / bar, np.where(err == 0, 0.0, np.inf))
    return np.max(ratio.astype(np.float64), axis=(1, 2))


def assert_ref(got, ref, what=""):
    ex = ref_excess(got, ref)
    print("%s |got - restatement| / bar per table:" % what, " ".join("%s=%.2e" % kv for kv in zip(NAMES, ex)))
    assert np.all(ex <= 1.0), (what, dict(zip(NAMES, ex)))


def assert_shipped(got, shipped, what=""):
    err = np.max(np.abs(np.asarray(got) - np.asarray(shipped)), axis=(1, 2))
    print("%s max |got - shipped| per table:" % what, " ".join("%s=%.3e" % kv for kv in zip(NAMES, err)))
    assert np.all(err <= BAR_SHIPPED), (what, dict(zip(NAMES, err)))


def shipped_subgrid(hrg_eos, grid=GRID_5x3):
    """(T, muB, tab) of data.df_tables(hrg_eos) at the nodes of `grid` (which must be nodes of the shipped grid)."""
    T, muB, tab = data.df_tables(hrg_eos)
    iT = [int(np.argmin(np.abs(T - t))) for t in grid[0]]
    iB = [int(np.argmin(np.abs(muB - m))) for m in grid[1]]
    assert np.allclose(T[iT], grid[0], atol=1e-12) and np.allclose(muB[iB], grid[1], atol=1e-12)
    return T[iT], muB[iB], tab[:, iB][:, :, iT]
