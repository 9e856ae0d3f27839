"""Helpers of the four-body decay tests, written from the method's statement:
the case table, a flat four-body generator that shares no algebra with the engine's (massive RAMBO), the numpy form
of the feed-down density h(s), and the ctypes wrapper of the CPU emulator (tests/native/decay4_emulator.cpp =
is3d2_amd/csrc/decay_math.h and decay_mc_math.h compiled for the host behind the four-slot table).  Nothing here
includes or imports the headers' code.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from is3d2_amd import _lib

import decay_list_ref as L
import decay_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_SRC = os.path.join(HERE, "native", "decay4_emulator.cpp")
EMU_LIB = os.path.join(HERE, "native", "libdecay4_emulator.so")
CSRC = os.path.join(ROOT, "is3d2_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden")
P_DTYPE = L.P_DTYPE
FOUR_CAP = 1024          # tries of the four-body rejection loop
PHI3 = 24                # nodes of the inner rule of the plan

# ------------------------------------------------------------------------------------------
# the case table: a, b, c, R, H (and X, which is not chosen)
# ------------------------------------------------------------------------------------------
A_, B_, C_, R_, H_ = range(5)
MASS = np.array([0.14, 0.50, 0.94, 1.60, 2.40])
M_X = 0.30


def channel4(parent, daughters, branching, mass_parent, masses, n_body=None):
    """A channel dict with up to four daughters (Engine.set_decays' form; four daughters select the four-slot call)."""
    return dict(parent=parent, n_body=len(daughters) if n_body is None else n_body, daughter=list(daughters),
                branching=branching, mass_parent=mass_parent, width_parent=0.0, mass=list(masses),
                width=[0.0] * len(masses))


R_4A = channel4(R_, [A_, A_, A_, A_], 0.4, 1.60, [0.14] * 4)
R_ABXC = channel4(R_, [A_, B_, -1, C_], 0.3, 1.60, [0.14, 0.50, M_X, 0.94])
R_AA = channel4(R_, [A_, A_], 0.2, 1.60, [0.14, 0.14])                       # 0.1 of R is left undecayed
H_RAAB = channel4(H_, [R_, A_, A_, B_], 0.6, 2.40, [1.60, 0.14, 0.14, 0.50])  # slot 0 decays again: codes 4 c + 4 below c != 0
H_RC = channel4(H_, [R_, C_], 0.4, 2.40, [1.60, 0.94])
CHANNELS = [R_4A, R_ABXC, R_AA, H_RAAB, H_RC]
# With these masses R -> a b X c (sum m = 1.88 > 1.60) and H -> R c (2.54 > 2.40) are closed: in the table they are the
# rows that count in skipped_closed (R then stays undecayed with 0.4, H with 0.4), and the open channels still put the
# code 4 c + 4 below a nonzero c (H -> R a a b, then R -> a a a a).  The single-decay test of a dropped daughter
# needs an open channel with the same daughters: the heavier parent H.
H_ABXC = channel4(H_, [A_, B_, -1, C_], 1.0, 2.40, [0.14, 0.50, M_X, 0.94])


# ------------------------------------------------------------------------------------------
# the emulator
# ------------------------------------------------------------------------------------------
def emulator():
    srcs = [EMU_SRC, os.path.join(ROOT, "include", "is3d_amd.h")] + \
           [os.path.join(CSRC, h) for h in ("decay_mc_math.h", "decay_math.h", "sampler_math.h", "cf_math.h")]
    if not os.path.exists(EMU_LIB) or any(os.path.getmtime(s) > os.path.getmtime(EMU_LIB) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-fopenmp", "-shared", "-o", EMU_LIB, EMU_SRC])
    lib = C.CDLL(EMU_LIB)
    pd = C.POINTER(C.c_double)
    lib.dl4_emulate.restype = C.c_long
    lib.dl4_emulate.argtypes = [C.c_int, pd, C.c_int, C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_void_p, C.c_void_p,
                                C.POINTER(C.c_long), C.POINTER(_lib.DecayStats), C.c_char_p, C.c_int]
    lib.dl4_fetch.argtypes = [C.c_void_p, C.c_void_p]
    lib.dl4_channels.argtypes = [C.c_int, pd, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.POINTER(C.c_int)]
    lib.dl4_envelope.argtypes = [C.c_double, pd, C.c_long, C.c_long, pd]
    lib.decay4_slot_weights.argtypes = [C.c_double, C.c_double, pd, C.c_int, pd, pd]
    lib.decay4_phi3.restype = C.c_double
    lib.decay4_phi3.argtypes = [C.c_double] * 4 + [C.c_int]
    lib.decay4_emulate.argtypes = [C.c_int, pd, C.c_int, pd, C.c_int, pd, C.c_int, pd, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                   pd, pd, C.POINTER(_lib.DecayStats), C.POINTER(C.c_long), C.POINTER(C.c_long), C.c_char_p,
                                   C.c_int]
    assert lib.dl4_particle_size() == P_DTYPE.itemsize == 96
    assert lib.decay4_channel_size() == _lib.DECAY4_DTYPE.itemsize == C.sizeof(_lib.DecayChannel4)
    return lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def table4(channels):
    """A DECAY4_DTYPE array of a list of channel dicts, of a DECAY_DTYPE array (slot 3 empty) or of itself."""
    if isinstance(channels, np.ndarray) and channels.dtype == _lib.DECAY4_DTYPE:
        return np.ascontiguousarray(channels)
    a = np.zeros(len(channels), dtype=_lib.DECAY4_DTYPE)
    a["daughter"] = -1
    if isinstance(channels, np.ndarray):
        for k in ("parent", "n_body", "branching", "mass_parent", "width_parent"):
            a[k] = channels[k]
        for k in ("daughter", "mass", "width"):
            a[k][:, :3] = channels[k]
        return a
    for i, c in enumerate(channels):
        for k, v in c.items():
            if k in ("daughter", "mass", "width"):
                a[k][i, :len(v)] = v
            else:
                a[k][i] = v
    return a


def emulate_list(mass, channels, particles, offsets, seed, keep_four=True):
    """(particles, offsets, origins, stats, plan_stats) of the emulator: decay_list_ref.emulate over a four-slot table."""
    lib = emulator()
    mass = np.ascontiguousarray(mass, dtype=np.float64)
    tab = table4(channels)
    offsets = np.asarray(offsets, dtype=np.int64)
    i0, n = int(offsets[0]), int(offsets[-1] - offsets[0])
    parts = np.ascontiguousarray(particles[i0:i0 + n], dtype=P_DTYPE)
    prim = L.index_in_event(offsets)
    st, pst, msg = (C.c_long * 8)(), _lib.DecayStats(), C.create_string_buffer(256)
    m = lib.dl4_emulate(len(mass), _dp(mass), len(tab), C.c_void_p(tab.ctypes.data), int(keep_four), int(seed), n,
                        C.c_void_p(parts.ctypes.data), C.c_void_p(prim.ctypes.data), st, C.byref(pst), msg, 256)
    if m < 0:
        raise ValueError(msg.value.decode())
    out, origin = np.zeros(m, dtype=P_DTYPE), np.zeros(m, dtype=np.int64)
    lib.dl4_fetch(C.c_void_p(out.ctypes.data), C.c_void_p(origin.ctypes.data))
    new_off = np.searchsorted(origin, offsets - i0, side="left").astype(np.int64)
    stats = dict(zip(L.STAT_KEYS, list(st)[:7]))
    return out, new_off, origin + i0, stats, {k: getattr(pst, k) for k, _ in pst._fields_}


def mc_channels(mass, channels, keep_four=True):
    """(ints[n][6] = parent, nbody, d0 .. d3; doubles[n][9] = cum, M, m0 .. m3, k0, k1, k2; level[npart]; levels)."""
    lib = emulator()
    mass = np.ascontiguousarray(mass, dtype=np.float64)
    tab = table4(channels)
    cap = len(tab) + 1
    ints, dbls = np.zeros((cap, 6), dtype=np.int32), np.zeros((cap, 9))
    level, levels = np.zeros(len(mass), dtype=np.int32), C.c_int(0)
    n = lib.dl4_channels(len(mass), _dp(mass), len(tab), C.c_void_p(tab.ctypes.data), int(keep_four), cap,
                         C.c_void_p(ints.ctypes.data), C.c_void_p(dbls.ctypes.data), C.c_void_p(level.ctypes.data),
                         C.byref(levels))
    assert n >= 0
    return ints[:n], dbls[:n], level, levels.value


def emulate_feeddown(S, mass, pT, phi, y, channels, keep_four=True, phi3_points=PHI3):
    """(S + feed-down, sum |terms|, stats, slots, two-body terms) of the emulator; ValueError where the engine
    would return IS3D_ERR_ARG."""
    lib = emulator()
    arr = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    out = np.array(S, dtype=np.float64, order="C", copy=True)
    npart, npT, nphi, ny = out.shape
    ab = np.zeros_like(out)
    mass, pT, phi, y = arr(mass), arr(pT), arr(phi), arr(y if ny > 1 else [0.0])
    tab = table4(channels)
    st, slots, terms, msg = _lib.DecayStats(), C.c_long(0), C.c_long(0), C.create_string_buffer(256)
    rc = lib.decay4_emulate(npart, _dp(mass), npT, _dp(pT), nphi, _dp(phi), ny, _dp(y), len(tab), C.c_void_p(tab.ctypes.data),
                            int(keep_four), int(phi3_points), _dp(out), _dp(ab), C.byref(st), C.byref(slots),
                            C.byref(terms), msg, 256)
    if rc:
        raise ValueError(msg.value.decode())
    return out, ab, {k: getattr(st, k) for k, _ in st._fields_}, slots.value, terms.value


def slot_weights(M, m1, others, phi3_points=PHI3):
    """(s_j, w_j) of one slot of a four-body channel as the plan builds them."""
    s, w, mo = np.zeros(12), np.zeros(12), np.ascontiguousarray(others, dtype=np.float64)
    assert emulator().decay4_slot_weights(float(M), float(m1), _dp(mo), int(phi3_points), _dp(s), _dp(w)) == 1
    return s, w


def envelope(M, m, seed, draws):
    """(largest p1 p2 p3 / w_max, acceptance, w_max) of the engine's own draw over `draws` tries."""
    out, mm = np.zeros(3), np.ascontiguousarray(m, dtype=np.float64)
    emulator().dl4_envelope(float(M), _dp(mm), int(seed), int(draws), _dp(out))
    return out


# ------------------------------------------------------------------------------------------
# the density of the feed-down's s rule, from its statement
# ------------------------------------------------------------------------------------------
def kallen(x, y, z):
    return x * x + y * y + z * z - 2.0 * (x * y + y * z + z * x)


def phi3(s, a, b, c, n=400):
    """Phi3(s; a, b, c) = int dt sqrt(lambda(s, a^2, t) lambda(t, b^2, c^2)) / (s t) over [(b + c)^2, (sqrt s - a)^2]:
    the raw integrand, with t = t0 + (t1 - t0) sin^2(pi u / 2) (a substitution of its own that flattens both
    square-root ends), n-point Gauss-Legendre in u."""
    x, w = np.polynomial.legendre.leggauss(n)
    u = 0.5 * (1.0 + x)
    s = np.atleast_1d(np.asarray(s, dtype=float))[:, None]
    t0, t1 = (b + c) ** 2, (np.sqrt(s) - a) ** 2
    t = t0 + (t1 - t0) * np.sin(0.5 * np.pi * u) ** 2
    dt = (t1 - t0) * np.pi * np.sin(0.5 * np.pi * u) * np.cos(0.5 * np.pi * u)
    f = np.sqrt(np.maximum(kallen(s, a * a, t), 0.0) * np.maximum(kallen(t, b * b, c * c), 0.0)) / (s * t)
    return np.sum(0.5 * w * f * dt, axis=1)


def h_density(s, M, mk, others):
    """h(s) = sqrt(lambda(M^2, m_k^2, s)) Phi3(s; the other three)."""
    s = np.atleast_1d(np.asarray(s, dtype=float))
    return np.sqrt(np.maximum(kallen(M * M, mk * mk, s), 0.0)) * phi3(s, *others)


def four_body_nodes(M, mk, others, n=12):
    """(s_j, w_j): the n Gauss-Legendre nodes on [(sum others)^2, (M - m_k)^2] and the normalised weights x_j h(s_j)."""
    x, w = np.polynomial.legendre.leggauss(n)
    lo, hi = sum(others) ** 2, (M - mk) ** 2
    s = lo + 0.5 * (hi - lo) * (1.0 + x)
    f = w * h_density(s, M, mk, others)
    return s, f / f.sum()


def slot_term4(parent, b, M, mk, others, pT, phi, y, n=12):
    """One daughter slot of a four-body channel: sum_j w_j x (decay_ref.two_body with W^2 = s_j)."""
    s, w = four_body_nodes(M, mk, others, n)
    tot = ab = 0.0
    for sj, wj in zip(s, w):
        t, a = R.two_body(parent, b * wj, M, mk, sj, pT, phi, y, 12)
        tot, ab = tot + t, ab + a
    return tot, ab


# ------------------------------------------------------------------------------------------
# an independent flat four-body generator: massive RAMBO (Kleiss, Stirling, Ellis, CPC 40 (1986) 359)
# ------------------------------------------------------------------------------------------
def rambo(rng, W, masses, n):
    """n events of W -> len(masses) bodies at rest: (p[n][k][4] = (E, px, py, pz), weight[n]).  Massless momenta
    with isotropic directions and energies -ln(r r'), boosted and scaled to total (W, 0); then scaled by xi with
    sum_i sqrt(m_i^2 + xi^2 E_i^2) = W.  The weight of the massive event is
    (sum |k_i| / W)^(2 k - 3) prod(|k_i| / E_i) / sum(|k_i|^2 / E_i) up to a constant."""
    masses = np.asarray(masses, dtype=float)
    k = len(masses)
    ct, ph = rng.uniform(-1, 1, (n, k)), rng.uniform(0, 2 * np.pi, (n, k))
    e = -np.log(rng.uniform(size=(n, k)) * rng.uniform(size=(n, k)))
    st = np.sqrt(1 - ct * ct)
    q = np.stack([e, e * st * np.cos(ph), e * st * np.sin(ph), e * ct], axis=-1)
    Q = q.sum(axis=1)
    MQ = np.sqrt(Q[:, 0] ** 2 - np.sum(Q[:, 1:] ** 2, axis=1))
    bv = -Q[:, 1:] / MQ[:, None]
    xs, gam = W / MQ, Q[:, 0] / MQ
    av = 1.0 / (1.0 + gam)
    bq = np.einsum("nj,nkj->nk", bv, q[:, :, 1:])
    p = np.empty_like(q)
    p[:, :, 0] = xs[:, None] * (gam[:, None] * q[:, :, 0] + bq)
    p[:, :, 1:] = xs[:, None, None] * (q[:, :, 1:] + bv[:, None, :] * q[:, :, 0:1] + (av[:, None] * bq)[:, :, None] * bv[:, None, :])
    xi = np.full(n, np.sqrt(1.0 - (masses.sum() / W) ** 2))
    for _ in range(60):
        E = np.sqrt(masses[None, :] ** 2 + (xi[:, None] * p[:, :, 0]) ** 2)
        f = E.sum(axis=1) - W
        df = np.sum(xi[:, None] * p[:, :, 0] ** 2 / E, axis=1)
        xi = xi - f / df
    out = np.empty_like(p)
    out[:, :, 1:] = xi[:, None, None] * p[:, :, 1:]
    out[:, :, 0] = np.sqrt(masses[None, :] ** 2 + (xi[:, None] * p[:, :, 0]) ** 2)
    kk = xi[:, None] * p[:, :, 0]
    wt = (kk.sum(axis=1) / W) ** (2 * k - 3) * np.prod(kk / out[:, :, 0], axis=1) / np.sum(kk * kk / out[:, :, 0], axis=1)
    return out, wt


def boost_to(parent, M, p):
    """The rest-frame momenta p[n][k][4] of parents (E, px, py, pz)[n] of mass M, in the lab."""
    E, px, py, pz = parent
    P = np.stack([px, py, pz], axis=1)
    Pq = np.einsum("nj,nkj->nk", P, p[:, :, 1:])
    M = np.reshape(M, (-1, 1)) if np.ndim(M) else M          # one mass, or one per parent
    g = Pq / (M * (E[:, None] + M)) + p[:, :, 0] / M
    out = np.empty_like(p)
    out[:, :, 0] = (E[:, None] * p[:, :, 0] + Pq) / M
    out[:, :, 1:] = p[:, :, 1:] + g[:, :, None] * P[:, None, :]
    return out


# ------------------------------------------------------------------------------------------
# the inputs of the comparison with the parent commit (tests/golden/decay4_parent_*.npz, tools/record_decay_parent.py)
# ------------------------------------------------------------------------------------------
def parent_cases():
    """{name: (mass, three-slot channel table, S, pT, phi, y, primaries, offsets, seed)}: the SMASH fixture over its
    chosen list and the eight-species case of decay_ref, each with a small grid and a short primary list."""
    from is3d2_amd import hrg
    out = {}
    pT, phi, y = np.linspace(0.15, 2.4, 5), np.arange(4) * (2 * np.pi / 4), np.array([0.0])
    d = dict(np.load(os.path.join(GOLDEN, "decays_smash.npz")))
    mcids = hrg.chosen_mcids("smash")
    mass = hrg.chosen_species(hrg.pdg_particles(2), mcids)["mass"]
    for name, mass, ch in (("smash", mass, hrg.decay_channels(d, d, mcids)), ("case8", R.CASE_MASS, R.channel_table(R.CASE_CHANNELS))):
        S = np.exp(-np.sqrt(pT[None, :, None, None] ** 2 + mass[:, None, None, None] ** 2) / 0.15) * \
            (1 + 0.1 * np.cos(2 * phi))[None, None, :, None] * np.ones((1, 1, 1, 1))
        rng = np.random.default_rng(7)
        n = 400
        sp = rng.integers(0, len(mass), n) if name == "case8" else np.argsort(mass)[-n:][rng.permutation(n)]
        prim = L.make_list(sp, mass, pT=rng.uniform(0.1, 2.0, n), phi=rng.uniform(0, 2 * np.pi, n), y=rng.uniform(-2, 2, n),
                           event=np.repeat([0, 1], n // 2), seed=3)
        out[name] = (np.ascontiguousarray(mass, dtype=np.float64), ch, S, pT, phi, y, prim, np.array([0, n // 2, n]), 11)
    return out
