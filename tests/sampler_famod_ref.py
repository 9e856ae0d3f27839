"""Helpers of the df_mode 5 (PTMA) particle-sampler tests: the host build of the sampler's famod math
(tests/native/sampler_famod_emulator.cpp over aniso_math.h and sampler_math.h), a Python restatement of the sampler's
chain rule (ParticleSampler.cpp:1330-1399) on the oracle's chain step, numpy restatements of the per-cell prologue
(:1181-1461) and of the species densities (:1467-1499), and the test surfaces U and Q."""
import ctypes as C
import os
import subprocess

import numpy as np

from is3d2_amd import synth
from oracle import oracle as O

from sampler_ref import PARTICLE_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_SRC = os.path.join(HERE, "native", "sampler_famod_emulator.cpp")
EMU_LIB = os.path.join(HERE, "native", "libsampler_famod_emulator.so")
HBARC = 0.197327053
PI_SCALE = 0.125


# --- the surfaces ------------------------------------------------------------------------------------------
def uniform_surface(n, dimension, seed=17):
    """U(dimension): uniform (T, E, P) = (0.150, 0.28, 0.045), timelike normals dsigma = (dat > 0, 0, 0, 0) and synth's
    pi and Pi scaled by 1/8 (test_gpu_sampler.py's uniform_surface, restated)."""
    s = synth.surface(n, seed=seed, dimension=dimension, full3d=(dimension == 3))
    for k in ("dax", "day", "dan"):
        s[k][:] = 0.0
    for k in ("pixx", "pixy", "pixn", "piyy", "piyn", "bulkPi"):
        s[k] *= PI_SCALE
    s["T"][:] = 0.150
    s["E"][:] = 0.28
    s["P"][:] = 0.045
    return synth.as_read(s)


def surface_q(baryon=False):
    """Q: 600 3+1D cells with every other bulk pressure x 10 (breakdown-heavy: pl / pt < 0 cells and reconstruction
    failures), and cell 36 -- which fails warm and cold -- a second time right after itself: 601 cells.  The copy then
    starts with no previous success and fails cold: the one case where the sampler's chain rule and the spectra's
    differ."""
    s = synth.surface(600, seed=31, dimension=3, baryon=baryon, full3d=True)
    s["bulkPi"][::2] *= 10.0
    s = {k: np.ascontiguousarray(np.insert(v, 37, v[36])) for k, v in s.items()}
    return synth.as_read(s)


# --- the emulator ------------------------------------------------------------------------------------------
def emulator():
    hdrs = [os.path.join(ROOT, "is3d2_amd", "csrc", h) for h in ("sampler_math.h", "aniso_math.h", "cf_math.h")]
    if not os.path.exists(EMU_LIB) or any(os.path.getmtime(s) > os.path.getmtime(EMU_LIB) for s in [EMU_SRC] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", EMU_LIB, EMU_SRC])
    lib = C.CDLL(EMU_LIB)
    pd, pl, pi = C.POINTER(C.c_double), C.POINTER(C.c_long), C.POINTER(C.c_int)
    lib.smpf_chain.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, pd, pd, pi, pi, pl]
    lib.smpf_chain.restype = None
    lib.smpf_cells.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, pd]
    lib.smpf_cells.restype = None
    lib.smpf_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_double, C.c_long,
                                C.c_long, pl, pl, pl, C.c_void_p, C.c_long]
    return lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def emu_chain(spec, surf, chains=1, srule=1):
    """aniso_cell over every cell: dict of sol [n][6] (lambda, aT, aL, broken, beta_pi_perp, beta_W_perp), sta [n][4]
    (the chain state after each cell), iters [n] (-1: not in the chain), flags [n] (1: pl/pt < 0, 2: failure) and the
    counters (plpt_negative, reconstruction_fail, iterations)."""
    inp = O._Inputs(spec, surf, None, 1)
    n = len(surf["tau"])
    sol, sta = np.zeros((n, 6)), np.zeros((n, 4))
    iters, flags = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    cnt = np.zeros(3, dtype=np.int64)
    emulator().smpf_chain(C.byref(inp.params), C.byref(inp.setup), C.byref(inp.surf), chains, srule, _dp(sol), _dp(sta),
                          iters.ctypes.data_as(C.POINTER(C.c_int)), flags.ctypes.data_as(C.POINTER(C.c_int)),
                          cnt.ctypes.data_as(C.POINTER(C.c_long)))
    return dict(sol=sol, sta=sta, iters=iters, flags=flags,
                counters=dict(plpt_negative=int(cnt[0]), reconstruction_fail=int(cnt[1]), iterations=int(cnt[2])))


CELL_COLS = ("live", "breaks", "Bxx", "Bxy", "Bxz", "Byy", "Byz", "Bzz", "detB", "lambda", "detA", "dn_tot")


def emu_cells(spec, surf, chains=1, y_cut=0.5):
    """cell_setup_famod + species_weight_famod of every cell from the sampler-rule prepass: dict of columns CELL_COLS."""
    inp = O._Inputs(spec, surf, None, 1)
    out = np.zeros((len(surf["tau"]), len(CELL_COLS)))
    emulator().smpf_cells(C.byref(inp.params), C.byref(inp.setup), C.byref(inp.surf), chains, y_cut, _dp(out))
    return {k: out[:, i] for i, k in enumerate(CELL_COLS)}


def emu_sample(spec, surf, seed, n_events, y_cut=0.5, chains=1, lo=0, hi=None, keep=0):
    """The serial famod sampler over cells [lo, hi): (kept per species, stats dict, first `keep` particles)."""
    inp = O._Inputs(spec, surf, None, 1)
    n = len(surf["tau"])
    counts = np.zeros(len(spec["species"]["mass"]), dtype=np.int64)
    stats, fam = np.zeros(8, dtype=np.int64), np.zeros(3, dtype=np.int64)
    parts = np.zeros(max(keep, 1), dtype=PARTICLE_DTYPE)
    lp = C.POINTER(C.c_long)
    rc = emulator().smpf_sample(C.byref(inp.params), C.byref(inp.setup), C.byref(inp.surf), chains, seed, n_events, y_cut,
                                lo, n if hi is None else hi, counts.ctypes.data_as(lp), stats.ctypes.data_as(lp),
                                fam.ctypes.data_as(lp), C.c_void_p(parts.ctypes.data if keep else 0), keep)
    assert rc == 0
    st = dict(zip(("live_cells", "breakdown", "candidates", "kept", "proposals", "acceptances", "capped"), [int(v) for v in stats]))
    st.update(plpt_negative=int(fam[0]), reconstruction_fail=int(fam[1]), iterations=int(fam[2]))
    return counts, st, parts[:min(keep, st["kept"])]


# --- numpy restatement of the prologue (ParticleSampler.cpp:1181-1320) ----------------------------------------------
def lrf(spec, s):
    """Per cell: u.dsigma, the LRF dsigma and its magnitude, the LRF pi, pl, pt, piT / WTz (under include_shear_deltaf),
    alphaB (muB under include_baryon alone)."""
    p = spec["params"]
    tau = s["tau"]; tau2 = tau * tau
    ux, uy, un = s["ux"], s["uy"], s["un"]
    dat, dax, day, dan = s["dat"], s["dax"], s["day"], s["dan"]
    ut = np.sqrt(1. + ux * ux + uy * uy + tau2 * un * un)
    uds = ut * dat + ux * dax + uy * day + un * dan
    ut2, ux2, uy2 = ut * ut, ux * ux, uy * uy
    uperp, utperp = np.sqrt(ux2 + uy2), np.sqrt(1. + ux2 + uy2)
    pixx, pixy, pixn, piyy, piyn = s["pixx"], s["pixy"], s["pixn"], s["piyy"], s["piyn"]
    pinn = (pixx * (ux2 - ut2) + piyy * (uy2 - ut2) + 2. * (pixy * ux * uy + tau2 * un * (pixn * ux + piyn * uy))) / (tau2 * utperp * utperp)
    pitn = (pixn * ux + piyn * uy + tau2 * pinn * un) / ut
    pity = (pixy * ux + piyy * uy + tau2 * piyn * un) / ut
    pitx = (pixx * ux + pixy * uy + tau2 * pixn * un) / ut
    pitt = (pitx * ux + pity * uy + tau2 * pitn * un) / ut
    # Milne basis (LocalRestFrame.cpp:12-41)
    sinhL, coshL = tau * un / utperp, ut / utperp
    big = uperp > 1.e-5
    safe = np.where(big, uperp, 1.0)
    Xt, Xn = uperp * coshL, uperp * sinhL / tau
    Xx, Xy = np.where(big, utperp * ux / safe, 1.0), np.where(big, utperp * uy / safe, 0.0)
    Yx, Yy = np.where(big, -uy / safe, 0.0), np.where(big, ux / safe, 1.0)
    Zt, Zn = sinhL, coshL / tau
    dst = dat * ut + dax * ux + day * uy + dan * un
    dsx = -(dat * Xt + dax * Xx + day * Xy + dan * Xn)
    dsy = -(dax * Yx + day * Yy)
    dsz = -(dat * Zt + dan * Zn)
    xx = (pitt * Xt * Xt + pixx * Xx * Xx + piyy * Xy * Xy + tau2 * tau2 * pinn * Xn * Xn
          + 2.0 * (-Xt * (pitx * Xx + pity * Xy) + pixy * Xx * Xy + tau2 * Xn * (pixn * Xx + piyn * Xy - pitn * Xt)))
    xy = Yx * (-pitx * Xt + pixx * Xx + pixy * Xy + tau2 * pixn * Xn) + Yy * (-pity * Xt + pixy * Xx + piyy * Xy + tau2 * piyn * Xn)
    xz = Zt * (pitt * Xt - pitx * Xx - pity * Xy - tau2 * pitn * Xn) - tau2 * Zn * (pitn * Xt - pixn * Xx - piyn * Xy - tau2 * pinn * Xn)
    yy = pixx * Yx * Yx + 2.0 * pixy * Yx * Yy + piyy * Yy * Yy
    yz = -Zt * (pitx * Yx + pity * Yy) + tau2 * Zn * (pixn * Yx + piyn * Yy)
    zz = -(xx + yy)
    sh = 1.0 if p["include_shear_deltaf"] else 0.0
    muB = s["muB"] if p["include_baryon"] else np.zeros_like(tau)
    return dict(uds=uds, dst=dst, dsx=dsx, dsy=dsy, dsz=dsz, ds_max=np.abs(dst) + np.sqrt(dsx * dsx + dsy * dsy + dsz * dsz),
                pl=s["P"] + s["bulkPi"] + zz, pt=s["P"] + s["bulkPi"] - zz / 2.,
                piTxx=sh * (xx - yy) / 2., piTxy=sh * xy, WTzx=sh * xz, WTzy=sh * yz, alphaB=muB / s["T"])


def prologue(spec, s, sol):
    """:1402-1461 from the cells' (lambda, aT, aL, broken, beta_pi_perp, beta_W_perp): dict of B (6 columns, the identity
    on breakdown), detB, detA, breaks."""
    L = lrf(spec, s)
    sol = np.where((L["uds"] > 0)[:, None], sol, 1.0)      # cells outside the chain have no row: keep the algebra finite
    aT, aL = sol[:, 1], sol[:, 2]
    sc, dc = 0.5 / sol[:, 4], 1. / sol[:, 5]
    piTxx, piTxy, piTyy, WTzx, WTzy = L["piTxx"], L["piTxy"], -L["piTxx"], L["WTzx"], L["WTzy"]
    detA = aT * aT * aL
    Cxx, Cxy, Cxz = 1. + sc * piTxx, sc * piTxy, dc * WTzx * aT / (aT + aL)
    Cyx, Cyy, Cyz = Cxy, 1. + sc * piTyy, dc * WTzy * aT / (aT + aL)
    Czx, Czy, Czz = dc * WTzx * aL / (aT + aL), dc * WTzy * aL / (aT + aL), 1.
    detC = Cxx * (Cyy * Czz - Cyz * Czy) - Cxy * (Cyx * Czz - Cyz * Czx) + Cxz * (Cyx * Czy - Cyy * Czx)
    detB = detC * detA
    breaks = (sol[:, 3] != 0) | (detB <= spec["params"]["deta_min"])
    B = dict(Bxx=aT + aT * sc * piTxx, Bxy=aT * sc * piTxy, Bxz=dc * WTzx * aT * aL / (aT + aL),
             Byy=aT + aT * sc * piTyy, Byz=dc * WTzy * aT * aL / (aT + aL), Bzz=aL)
    ident = dict(Bxx=1.0, Bxy=0.0, Bxz=0.0, Byy=1.0, Byz=0.0, Bzz=1.0)
    out = {k: np.where(breaks, ident[k], v) for k, v in B.items()}
    out.update(detB=detB, detA=detA, breaks=breaks)
    return out


def densities(spec, lam, detA, chem=0.0):
    """n_a [cell][species] = g lambda^3 detA / (2 pi^2 hbarc^3) sum_i pbar_i w_i e^pbar_i / (e^(Ebar_i + chem) + sign)
    with the alpha = 1 Gauss-Laguerre row (:1467-1499)."""
    sp = spec["species"]
    roots, weights = spec["gla"]
    r, w = np.asarray(roots)[1], np.asarray(weights)[1]
    mbar = sp["mass"][None, :, None] / lam[:, None, None]
    Ebar = np.sqrt(r[None, None, :] ** 2 + mbar * mbar)
    I = (r * w * np.exp(r) / (np.exp(Ebar + chem) + sp["sign"][None, :, None])).sum(axis=2)
    return sp["degen"][None, :] * (lam ** 3 * detA / (2.0 * np.pi ** 2 * HBARC ** 3))[:, None] * I


# --- the sampler's chain rule on the oracle's chain step (ParticleSampler.cpp:1330-1399) ----------------------------
def sampler_chain(spec, s, chains=1):
    """Walks the cells of each strided chain (chains = 0: every cell a chain of its own) one oracle step at a time.
    The oracle's step is the spectra's rule (MomentumSpectra.cpp:1288-1368); the sampler's differs only where a solved
    cell started with no previous success and the oracle's state after it is exactly (1, T, 1, 1) -- the failed cold
    solve the spectra accept -- where the sampler breaks the cell down, counts a failure and keeps prev_ok = 0.
    Returns dict: lam, aT, aL, broken, prev_ok, iters (-1: not in the chain) per cell, quirk (cells of that case) and
    the counters."""
    n = len(s["tau"])
    L = lrf(spec, s)
    ch = O.FamodChain(spec, s)
    lam, aT, aL = s["T"].copy(), np.ones(n), np.ones(n)
    broken, prev_ok, iters = np.zeros(n, dtype=bool), np.zeros(n), np.full(n, -1)
    quirk = []
    plpt = fail = 0
    C = min(chains, n) if chains > 0 else n
    for c0 in range(C):
        state = np.zeros(4)
        for c in range(c0, n, C):
            if L["uds"][c] > 0:
                if L["pl"][c] < 0 or L["pt"][c] < 0:
                    broken[c] = True
                    plpt += 1
                    iters[c] = 0
                else:
                    started_ok = state[0] != 0
                    _, it, end = ch.walk([c], state)
                    iters[c] = it[0]
                    cold_fail = (not started_ok) and tuple(end) == (1.0, s["T"][c], 1.0, 1.0)
                    if cold_fail:
                        quirk.append(c)
                    if cold_fail or (started_ok and end[0] == 0):
                        broken[c] = True
                        fail += 1
                        state = np.concatenate([[0.0], end[1:] if not cold_fail else state[1:]])
                    else:
                        state = end.copy()
                        lam[c], aT[c], aL[c] = end[1:]
            prev_ok[c] = state[0]
    live = iters >= 0
    return dict(lam=lam, aT=aT, aL=aL, broken=broken, prev_ok=prev_ok, iters=iters, quirk=quirk,
                counters=dict(plpt_negative=plpt, reconstruction_fail=fail, iterations=int(iters[live].sum())))
