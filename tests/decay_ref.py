"""numpy restatement of the resonance-decay feed-down, written from the method's statement in its
direct, unfactorised form: every (pT, phi, y, v, zeta) point evaluates the parent on its own.  The parent is a grid
spectrum (interpolated as the method says) or an exact callable f(MT, Phi, Y).  Also the ctypes wrapper of the CPU
emulator (tests/native/decay_emulator.cpp = is3d2_amd/csrc/decay_math.h compiled for the host).
"""
import ctypes as C
import os
import subprocess

import numpy as np

from is3d2_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_SRC = os.path.join(HERE, "native", "decay_emulator.cpp")
EMU_LIB = os.path.join(HERE, "native", "libdecay_emulator.so")
BAR = 1e-8          # the project's parity bar: |got - ref| / sum |terms|
ADJUST_CAP = 100000


# ------------------------------------------------------------------------------------------
# the formula
# ------------------------------------------------------------------------------------------
def mt_interp(a, b, t):
    """Step 1: along MT between the bracket's values a, b at position t (outside [0, 1]: the line continues)."""
    pos = (a > 0) & (b > 0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        la, lb = np.log(np.where(pos, a, 1.0)), np.log(np.where(pos, b, 1.0))
        logv = np.exp(la + t * (lb - la))
    lin = a + t * (b - a)
    inside = (t >= 0) & (t <= 1)
    outside = np.where(pos & ~((t > 1) & (b >= a)), logv, 0.0)
    return np.where(inside, np.where(pos, logv, lin), outside)


def grid_parent(S, pT, phi, y, M):
    """S_R(MT, Phi, Y) of a grid spectrum S[pT][phi][y] of a parent of mass M, as a callable."""
    S = np.asarray(S, dtype=np.float64)
    npT, nphi, ny = S.shape
    a = np.sqrt(pT ** 2 + M ** 2)

    def f(MT, Phi, Y):
        MT, Phi, Y = np.broadcast_arrays(MT, Phi, Y)
        i0 = np.clip(np.searchsorted(a, MT, side="right") - 1, 0, npT - 2)
        t = (MT - a[i0]) / (a[i0 + 1] - a[i0])
        if ny == 1:
            rows = [(np.zeros(MT.shape, dtype=int), np.ones(MT.shape))]
        else:
            ok = (Y >= y[0]) & (Y <= y[-1])
            k0 = np.clip(np.searchsorted(y, Y, side="right") - 1, 0, ny - 2)
            ty = (Y - y[k0]) / (y[k0 + 1] - y[k0])
            rows = [(k0, np.where(ok, 1.0 - ty, 0.0)), (k0 + 1, np.where(ok, ty, 0.0))]
        if nphi == 1:
            cols = [(np.zeros(MT.shape, dtype=int), np.ones(MT.shape))]
        else:
            P = Phi - np.floor(Phi / (2 * np.pi)) * (2 * np.pi)
            j0 = np.searchsorted(phi, P, side="right") - 1          # -1: below phi_0 (the wrap interval)
            wrap = (j0 < 0) | (j0 >= nphi - 1)
            jl = np.where(wrap, nphi - 1, j0)
            jr = np.where(wrap, 0, j0 + 1)
            left = np.where(j0 < 0, phi[-1] - 2 * np.pi, phi[jl])
            right = np.where(wrap, np.where(j0 < 0, phi[0], phi[0] + 2 * np.pi), phi[jr])
            u = (P - left) / (right - left)
            cols = [(jl, 1.0 - u), (jr, u)]
        out = np.zeros(MT.shape)
        for j, wj in cols:
            for k, wk in rows:
                out = out + wj * wk * mt_interp(S[i0, j, k], S[i0 + 1, j, k], t)
        return out

    return f


def two_body(parent, b, M, m1, W2, pT, phi, y, n=12):
    """(dS1, sum |terms|)[pT][phi][y] of one daughter of mass m1 recoiling against invariant mass^2 W2."""
    x, w = np.polynomial.legendre.leggauss(n)
    pT_ = np.asarray(pT, dtype=float)[:, None, None, None, None]
    ph = np.asarray(phi, dtype=float)[None, :, None, None, None]
    yy = np.asarray(y, dtype=float)[None, None, :, None, None]
    v, wv = x[None, None, None, :, None], w[None, None, None, :, None]
    zeta, wz = (0.5 * np.pi * (1.0 + x))[None, None, None, None, :], (0.5 * np.pi * w)[None, None, None, None, :]
    Es = (M * M + m1 * m1 - W2) / (2.0 * M)
    ps = np.sqrt(Es * Es - m1 * m1)
    mT = np.sqrt(pT_ ** 2 + m1 ** 2)
    dY = np.arcsinh(ps / mT)
    c = np.cosh(v * dY)
    Y = yy + v * dY
    den = mT ** 2 * c ** 2 - pT_ ** 2
    MTbar = M * Es * mT * c / den
    dMT = M * pT_ * np.sqrt(np.maximum(Es ** 2 + pT_ ** 2 - mT ** 2 * c ** 2, 0.0)) / den
    MT = MTbar + dMT * np.cos(zeta)
    PT = np.sqrt(np.maximum(MT ** 2 - M ** 2, 0.0))
    d = PT * pT_
    with np.errstate(divide="ignore", invalid="ignore"):
        arg = np.where(d > 0, (MT * mT * c - M * Es) / np.where(d > 0, d, 1.0), 1.0)
    delta = np.arccos(np.clip(arg, -1.0, 1.0))
    val = parent(MT, ph + delta, Y) + parent(MT, ph - delta, Y)
    terms = b / (4.0 * np.pi * ps) * wv * dY * wz * M * MT / np.sqrt(den) * val
    return terms.sum(axis=(-1, -2)), np.abs(terms).sum(axis=(-1, -2))


def three_body_nodes(M, m1, m2, m3, n=12):
    """(s_k, w_k): the Gauss-Legendre nodes on [(m2 + m3)^2, (M - m1)^2] and the normalised phase-space weights."""
    x, w = np.polynomial.legendre.leggauss(n)
    lo, hi = (m2 + m3) ** 2, (M - m1) ** 2
    s = lo + 0.5 * (hi - lo) * (1.0 + x)
    f = np.sqrt(np.maximum(((M + m1) ** 2 - s) * (hi - s) * (s - lo) * (s - (m2 - m3) ** 2), 0.0)) / s
    return s, w * f / np.sum(w * f)


def slot_term(parent, b, M, m1, others, pT, phi, y, n=12):
    """One daughter slot of a 2- or 3-body channel: others = the masses of the other daughter(s)."""
    if len(others) == 1:
        return two_body(parent, b, M, m1, others[0] ** 2, pT, phi, y, n)
    s, w = three_body_nodes(M, m1, others[0], others[1], n)
    tot = ab = 0.0
    for sk, wk in zip(s, w):
        t, a = two_body(parent, b * wk, M, m1, sk, pT, phi, y, n)
        tot, ab = tot + t, ab + a
    return tot, ab


# ------------------------------------------------------------------------------------------
# the bookkeeping: which channels, which masses, which order
# ------------------------------------------------------------------------------------------
def channel(parent, daughters, branching, mass_parent, masses, width_parent=0.0, widths=None, n_body=None):
    """A channel dict in Engine.set_decays' form; daughters: chosen indices (-1: not chosen)."""
    n = len(daughters) if n_body is None else n_body
    return dict(parent=parent, n_body=n, daughter=list(daughters)[:3], branching=branching, mass_parent=mass_parent,
                width_parent=width_parent, mass=list(masses)[:3], width=list(widths or [0.0] * len(masses))[:3])


def open_two_body(M, m1, m2):
    """Open in floating point: both daughters get p*^2 > 0 (a channel a few ulp above threshold can round to <= 0)."""
    if not M > m1 + m2:
        return False
    e1, e2 = (M * M + m1 * m1 - m2 * m2) / (2 * M), (M * M + m2 * m2 - m1 * m1) / (2 * M)
    return e1 * e1 - m1 * m1 > 0 and e2 * e2 - m2 * m2 > 0


def open_three_body(M, m):
    """Open in floating point: for every slot the s rule has a positive norm and p*^2 > 0 at every node."""
    if not M > sum(m):
        return False
    for k in range(3):
        m1, (m2, m3) = m[k], [m[o] for o in range(3) if o != k]
        lo, hi = (m2 + m3) ** 2, (M - m1) ** 2
        x, wx = np.polynomial.legendre.leggauss(12)
        s = lo + 0.5 * (hi - lo) * (1.0 + x)
        f = np.sqrt(np.maximum(((M + m1) ** 2 - s) * (hi - s) * (s - lo) * (s - (m2 - m3) ** 2), 0.0)) / s
        es = (M * M + m1 * m1 - s) / (2 * M)
        if not np.sum(wx * f) > 0 or not np.all(es * es - m1 * m1 > 0):
            return False
    return True


def kept_channels(channels):
    """(kept, stats): the open 2- and 3-body channels with their (adjusted) masses, and the counts."""
    st = dict(channels=len(channels), kept=0, skipped_many_body=0, skipped_closed=0, adjusted=0, branching_skipped=0.0)
    kept = []
    for c in channels:
        nb = c["n_body"]
        if nb == 1:
            continue
        if nb >= 4:
            st["skipped_many_body"] += 1
            st["branching_skipped"] += c["branching"]
            continue
        M, m, g = c["mass_parent"], list(c["mass"][:nb]), list(c["width"][:nb])
        is_open = open_two_body(M, *m) if nb == 2 else open_three_body(M, m)
        if nb == 2 and not is_open and (c["width_parent"] > 0 or g[0] > 0 or g[1] > 0):
            for _ in range(ADJUST_CAP):
                M += 0.25 * c["width_parent"]
                m = [m[0] - 0.5 * g[0], m[1] - 0.5 * g[1]]
                if min(m) < 0:
                    break
                if open_two_body(M, *m):
                    is_open = True
                    st["adjusted"] += 1
                    break
        if not is_open:
            st["skipped_closed"] += 1
            st["branching_skipped"] += c["branching"]
            continue
        st["kept"] += 1
        kept.append(dict(c, M=M, m=m))
    return kept, st


def feeddown(S, mass, pT, phi, y, channels, n=12):
    """(S + feed-down, sum |terms|, stats) of the spectra S[species][pT][phi][y]: a species decays once every kept
    channel that feeds it has been applied."""
    S = np.array(S, dtype=np.float64)
    ab = np.zeros_like(S)
    kept, st = kept_channels(channels)
    npart = S.shape[0]
    feeds = [set() for _ in range(npart)]      # parents whose channels feed species d
    for c in kept:
        for d in c["daughter"][:c["n_body"]]:
            if d >= 0:
                feeds[d].add(c["parent"])
    todo = sorted({c["parent"] for c in kept})
    levels = 0
    while todo:
        ready = [p for p in todo if not (feeds[p] & set(todo))]
        if not ready:
            raise ValueError("cycle")
        levels += 1
        for p in ready:
            for c in kept:
                if c["parent"] != p:
                    continue
                par = grid_parent(S[p], pT, phi, y, c["M"])
                for k in range(c["n_body"]):
                    d = c["daughter"][k]
                    if d < 0:
                        continue
                    others = [c["m"][o] for o in range(c["n_body"]) if o != k]
                    t, a = slot_term(par, c["branching"], c["M"], c["m"][k], others, pT, phi, y, n)
                    S[d] += t
                    ab[d] += a
        todo = [p for p in todo if p not in ready]
    st["levels"] = levels
    return S, ab, st


# ------------------------------------------------------------------------------------------
# the small case of the parity tests (CPU: emulator against restatement; GPU: kernels against emulator)
# ------------------------------------------------------------------------------------------
T_CASE = 0.150
CASE_MASS = np.array([0.138, 0.138, 0.776, 1.232, 0.938, 0.782, 1.5, 1.3])
CASE_CHANNELS = [channel(2, [0, 1], 1.0, 0.776, [0.138, 0.138]),
                 channel(3, [4, 0], 0.9, 1.232, [0.938, 0.138]),
                 channel(5, [0, 1, 0], 0.89, 0.782, [0.138, 0.138, 0.138]),      # 3-body, a daughter that appears twice
                 channel(6, [2, 0], 0.5, 1.5, [0.776, 0.138]),                   # two generations: 6 -> 2 -> 0, 1
                 channel(6, [5, -1], 0.5, 1.5, [0.782, 0.138]),                  # a daughter that is not chosen
                 channel(7, [4, 0], 0.7, 1.3, [0.938, 0.138]),
                 channel(0, [0], 1.0, 0.138, [0.138])]                           # the stability marker
CASE_SLOTS = 12
UNFED = (3, 6, 7)        # parents no channel feeds: they decay from exactly the entries set below


def case_spectra(pT, phi, y):
    """Thermal spectra of the eight species with the four awkward parents, each on a parent that nothing feeds (a
    fed parent's awkward entries would be overwritten by an earlier level before its own logs are taken)."""
    S = np.zeros((len(CASE_MASS), len(pT), len(phi), len(y)))
    for s, m in enumerate(CASE_MASS):
        S[s] = (np.exp(-np.sqrt(pT ** 2 + m ** 2) / T_CASE))[:, None, None] * \
            (1 + 0.2 * np.cos(2 * phi))[None, :, None] * np.exp(-y ** 2 / 4)[None, None, :]
    S[3, 2, 5, 0] = 0.0                 # an exact zero inside the table
    S[3, 0, 3, 0] = 0.0                 # ... and at the first node: the lower extrapolation has an end value <= 0
    S[3, 4, 1, 0] = -1e-3               # a negative value
    S[7, -1] = 0.0                      # underflow zeros at the top pT node
    S[6, -1] = S[6, -2] * 1.5           # a last interval that does not fall
    return S


def check_awkward_parents(S, got, run):
    """The awkward entries are what the parents decayed from, and they matter: no channel feeds those parents, the
    output leaves them bit for bit, and replacing the non-positive entries by tiny positive ones changes the result
    (run(S) -> spectra with feed-down)."""
    for c in CASE_CHANNELS:
        assert c["n_body"] == 1 or not set(c["daughter"][:c["n_body"]]) & set(UNFED)
    for s in UNFED:
        assert np.array_equal(got[s], S[s])
    assert got[3, 2, 5, 0] == 0.0 and got[3, 0, 3, 0] == 0.0 and got[3, 4, 1, 0] < 0 and np.all(got[7, -1] == 0.0)
    assert np.all(got[6, -1] > got[6, -2])
    for idx in ((3, 2, 5, 0), (3, 0, 3, 0), (3, 4, 1, 0), (7, -1)):
        S2 = np.array(S)
        S2[idx] = 1e-300
        assert not np.array_equal(run(S2)[[0, 4]], got[[0, 4]]), idx
    S2 = np.array(S)
    S2[6, -1] = S2[6, -2] * 0.999        # a last interval that falls extrapolates instead of giving 0
    assert not np.array_equal(run(S2)[[0, 2]], got[[0, 2]])


# ------------------------------------------------------------------------------------------
# the emulator
# ------------------------------------------------------------------------------------------
def emulator():
    srcs = [EMU_SRC, os.path.join(ROOT, "is3d2_amd", "csrc", "decay_math.h"), os.path.join(ROOT, "include", "is3d_amd.h")]
    if not os.path.exists(EMU_LIB) or any(os.path.getmtime(s) > os.path.getmtime(EMU_LIB) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-fopenmp", "-shared", "-o", EMU_LIB, EMU_SRC])
    lib = C.CDLL(EMU_LIB)
    pd = C.POINTER(C.c_double)
    lib.decay_emulate.argtypes = [C.c_int, pd, C.c_int, pd, C.c_int, pd, C.c_int, pd, C.c_int, C.c_void_p, pd, pd,
                                  C.POINTER(_lib.DecayStats), C.POINTER(C.c_long), C.c_char_p, C.c_int]
    lib.decay_gauss_legendre.argtypes = [C.c_int, pd, pd]
    return lib


def channel_table(channels):
    """A DECAY_DTYPE array of a list of channel dicts (or the array itself)."""
    from is3d2_amd.engine import _decay_table
    return _decay_table(channels)[2]


def emulate(S, mass, pT, phi, y, channels):
    """(S + feed-down, sum |terms|, stats dict, slots) from the emulator; raises ValueError with its message where
    the engine would return IS3D_ERR_ARG."""
    lib = emulator()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    arr = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    out = np.array(S, dtype=np.float64, order="C", copy=True)
    npart, npT, nphi, ny = out.shape
    ab = np.zeros_like(out)
    mass, pT, phi, y = arr(mass), arr(pT), arr(phi), arr(y if ny > 1 else [0.0])
    tab = channel_table(channels)
    assert lib.decay_channel_size() == tab.dtype.itemsize == C.sizeof(_lib.DecayChannel)
    st, slots, msg = _lib.DecayStats(), C.c_long(0), C.create_string_buffer(256)
    rc = lib.decay_emulate(npart, dp(mass), npT, dp(pT), nphi, dp(phi), ny, dp(y), len(tab), C.c_void_p(tab.ctypes.data),
                           dp(out), dp(ab), C.byref(st), C.byref(slots), msg, 256)
    if rc:
        raise ValueError(msg.value.decode())
    return out, ab, {k: getattr(st, k) for k, _ in st._fields_}, slots.value


def parity(got, ref, ab):
    """max |got - ref| / sum |terms| over the outputs that received a term."""
    m = ab > 0
    return float(np.max(np.abs(got - ref)[m] / ab[m])) if m.any() else 0.0
