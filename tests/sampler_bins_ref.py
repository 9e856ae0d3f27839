"""Helpers of the binned-sampler tests: the host build of is3d2_amd/csrc/sampler_bins.h and of host_io.cpp's
results/sampled writers (tests/native/sampler_bins_emulator.cpp), the numpy restatement of the reference's binning
(BinSampledParticle.cpp:9-133) and of its writers (EmissionFunction.cpp:685-975), and the edge-ambiguity condition.

Quantum of the fixed-point vn sums: Q = 2^-32 (sampler_bins.h kVnQuantum)."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import oracle as O

import sampler_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "sampler_bins_emulator.cpp")
LIB = os.path.join(HERE, "native", "libsampler_bins_emulator.so")
HOST_IO = os.path.join(ROOT, "is3d2_amd", "csrc", "host", "host_io.cpp")
Q = 2.0 ** -32
TWO_PI = 6.283185307179586476925286766559
BIN_KEYS = ("pT_min", "pT_max", "pT_bins", "y_cut", "y_bins", "phip_bins", "eta_cut", "eta_bins", "tau_min", "tau_max",
            "tau_bins", "r_min", "r_max", "r_bins")
# the count parts in layout order: (name in Engine.sample_hist's dict, bins key)
PARTS = (("dN_dy", "y_bins"), ("dN_deta", "eta_bins"), ("dN_dphipdy", "phip_bins"), ("pT_count", "pT_bins"),
         ("dN_taudtaudy", "tau_bins"), ("dN_2pirdrdy", "r_bins"), ("dN_dphisdy", "phip_bins"))

# small bins whose ranges cut into what a synth surface populates (tau 0.6..10 fm, r 0.8..13.5 fm, |eta| < 4 in 3+1D,
# |y| up to the sampler's y_cut = 0.5 in 2+1D, pT from 0): every histogram drops particles at both ends
TEST_BINS = dict(pT_min=0.15, pT_max=1.6, pT_bins=12, y_cut=0.35, y_bins=10, phip_bins=8, eta_cut=1.4, eta_bins=14,
                 tau_min=2.0, tau_max=8.0, tau_bins=6, r_min=1.5, r_max=9.0, r_bins=5)


def lib():
    deps = [SRC, HOST_IO, os.path.join(HERE, "native", "sampler_emulator.cpp")] + \
           [os.path.join(ROOT, "is3d2_amd", "csrc", h) for h in ("sampler_bins.h", "sampler_math.h", "cf_math.h", "spline_host.h",
                                                                "host/host_io.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in deps):
        # no FMA contraction: the header's sums of squares and harmonics are then the device's bit for bit
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", LIB, SRC, HOST_IO])
    so = C.CDLL(LIB)
    pd, pl, pi, pll = C.POINTER(C.c_double), C.POINTER(C.c_long), C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    so.smpb_index.argtypes = [pd, C.c_long, C.c_double, C.c_double, C.c_int, pi]
    so.smpb_index.restype = None
    so.smpb_land.argtypes = [pd, C.c_long, pd, pd, pd, pd, pd, pd, pd, pi, pll]
    so.smpb_land.restype = None
    so.smpb_harmonics.argtypes = [pd, pd, C.c_long, pd]
    so.smpb_harmonics.restype = None
    so.smpb_fixed_sum.argtypes = [pd, C.c_long]
    so.smpb_fixed_sum.restype = C.c_double
    so.smpb_hist_words.argtypes = [pd, C.c_int, pl]
    so.smpb_hist_words.restype = C.c_long
    so.smpb_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, pd, C.c_long, C.c_long, C.c_double, C.c_int, C.c_long,
                               C.c_long, pd, pll, pl, C.c_void_p, pd, C.c_long]
    so.smpb_write.argtypes = [C.c_char_p, pd, C.c_int, C.c_long, pl, pd, pl]
    return so


def _d(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def b14(bins):
    return np.array([float(bins[k]) for k in BIN_KEYS])


def widths(bins):
    """EmissionFunction.cpp:223-247."""
    return dict(pT=(bins["pT_max"] - bins["pT_min"]) / float(bins["pT_bins"]), y=2.0 * bins["y_cut"] / float(bins["y_bins"]),
                phip=TWO_PI / float(bins["phip_bins"]), eta=2.0 * bins["eta_cut"] / float(bins["eta_bins"]),
                tau=(bins["tau_max"] - bins["tau_min"]) / float(bins["tau_bins"]), r=(bins["r_max"] - bins["r_min"]) / float(bins["r_bins"]))


# --- the header, element by element -------------------------------------------------------------------------
def c_index(v, lo, width, n):
    v = np.ascontiguousarray(v, dtype=np.float64)
    out = np.zeros(len(v), dtype=np.int32)
    lib().smpb_index(_d(v), len(v), lo, width, n, out.ctypes.data_as(C.POINTER(C.c_int)))
    return out


def c_land(bins, rapidity, eta, px, py, tau, x, y):
    a = [np.ascontiguousarray(v, dtype=np.float64) for v in (rapidity, eta, px, py, tau, x, y)]
    n = len(a[0])
    idx = np.zeros((n, 7), dtype=np.int32)
    vn = np.zeros((n, 14), dtype=np.int64)
    b = b14(bins)
    lib().smpb_land(_d(b), n, *[_d(v) for v in a], idx.ctypes.data_as(C.POINTER(C.c_int)), vn.ctypes.data_as(C.POINTER(C.c_longlong)))
    return idx, vn


def c_harmonics(px, py):
    px, py = np.ascontiguousarray(px, dtype=np.float64), np.ascontiguousarray(py, dtype=np.float64)
    out = np.zeros((len(px), 14))
    lib().smpb_harmonics(_d(px), _d(py), len(px), _d(out))
    return out


def c_fixed_sum(v):
    v = np.ascontiguousarray(v, dtype=np.float64)
    return lib().smpb_fixed_sum(_d(v), len(v))


# --- numpy restatement of BinSampledParticle.cpp ------------------------------------------------------------
def np_index(v, lo, width, n):
    """floor((v - lo) / width) where it is in [0, n), else -1."""
    f = np.floor((np.asarray(v, dtype=np.float64) - lo) / width)
    return np.where((f >= 0) & (f < n), f, -1).astype(np.int64)


def np_angle(b, a):
    phi = np.arctan2(b, a)
    return np.where(phi < 0.0, phi + TWO_PI, phi)


def coordinates(p, rapidity):
    """The seven binned coordinates of the particles p in layout order, with their (lo, width, bins key)."""
    return [rapidity, p["eta"], np_angle(p["py"], p["px"]), np.sqrt(p["px"] * p["px"] + p["py"] * p["py"]), p["tau"],
            np.sqrt(p["x"] * p["x"] + p["y"] * p["y"]), np_angle(p["y"], p["x"])]


def ranges(bins):
    w = widths(bins)
    return [(-bins["y_cut"], w["y"]), (-bins["eta_cut"], w["eta"]), (0.0, w["phip"]), (bins["pT_min"], w["pT"]),
            (bins["tau_min"], w["tau"]), (bins["r_min"], w["r"]), (0.0, w["phip"])]


def rapidity_from_momentum(p):
    return 0.5 * np.log((p["E"] + p["pz"]) / (p["E"] - p["pz"]))


def np_hist(p, rapidity, bins, npart):
    """Engine.sample_hist's dict from the list p: exact counts, and the vn sums as double sums of cos / sin (k phi)."""
    hist = {}
    co = coordinates(p, rapidity)
    sp = p["species"].astype(np.int64)
    for (name, key), v, (lo, w) in zip(PARTS, co, ranges(bins)):
        nb = int(bins[key])
        i = np_index(v, lo, w, nb)
        k = i >= 0
        hist[name] = np.bincount(sp[k] * nb + i[k], minlength=npart * nb).reshape(npart, nb)
    nb = int(bins["pT_bins"])
    i = np_index(co[3], bins["pT_min"], widths(bins)["pT"], nb)
    k = i >= 0
    flat = sp[k] * nb + i[k]
    phi = co[2][k]
    hist["vn_real"] = np.stack([np.bincount(flat, weights=np.cos((n + 1.0) * phi), minlength=npart * nb).reshape(npart, nb) for n in range(7)])
    hist["vn_imag"] = np.stack([np.bincount(flat, weights=np.sin((n + 1.0) * phi), minlength=npart * nb).reshape(npart, nb) for n in range(7)])
    return hist


def ambiguous(p, rapidity, bins, parts=(0, 2, 6)):
    """Number of (particle, histogram) pairs whose coordinate lies within 1e-12 max(1, |v|) of a bin edge or range end,
    over the histograms whose coordinate comes from atan2 or log (y, phip, phis): there the last bits of the device's
    and the host's libm may differ, everywhere else the index is exactly determined."""
    co, rg, total = coordinates(p, rapidity), ranges(bins), 0
    for part in parts:
        v, (lo, w), nb = co[part], rg[part], int(bins[PARTS[part][1]])
        edges = lo + w * np.arange(nb + 1)
        j = np.clip(np.searchsorted(edges, v), 1, nb)
        dist = np.minimum(np.abs(v - edges[j - 1]), np.abs(v - edges[j]))
        total += int((dist <= 1e-12 * np.maximum(1.0, np.abs(v))).sum())
    return total


def split(words, bins, npart):
    """The emulator's integer histogram as Engine.sample_hist's dict (vn converted once, as is3d_get_sample_hist)."""
    hist, at = {}, 0
    for name, key in PARTS:
        nb = int(bins[key])
        hist[name] = words[at:at + npart * nb].reshape(npart, nb).copy()
        at += npart * nb
    v = words[at:].astype(np.float64).reshape(2, 7, npart, int(bins["pT_bins"])) * Q
    hist["vn_real"], hist["vn_imag"] = v[0], v[1]
    return hist


def sample_binned(spec, surf, plasma, seed, n_events, bins, y_cut=0.5, fast=0, lo=0, hi=None, keep=1 << 20):
    """The serial sampler with every kept particle binned: (hist dict, stats dict, list, drawn rapidities)."""
    so = lib()
    inp = O._Inputs(spec, surf, plasma[0], 1)
    n = len(surf["tau"])
    npart = len(spec["species"]["mass"])
    pl = np.ascontiguousarray(plasma, dtype=np.float64)
    b = b14(bins)
    words = np.zeros(so.smpb_hist_words(_d(b), npart, None), dtype=np.int64)
    stats = np.zeros(8, dtype=np.int64)
    parts = np.zeros(keep, dtype=R.PARTICLE_DTYPE)
    drawn = np.zeros(keep)
    rc = so.smpb_sample(C.byref(inp.params), C.byref(inp.setup), C.byref(inp.surf), _d(pl), seed, n_events, y_cut, fast, lo,
                        n if hi is None else hi, _d(b), words.ctypes.data_as(C.POINTER(C.c_longlong)),
                        stats.ctypes.data_as(C.POINTER(C.c_long)), C.c_void_p(parts.ctypes.data), _d(drawn), keep)
    assert rc == 0, "sampler emulator rc=%d" % rc
    st = dict(zip(R.STATS, [int(v) for v in stats]))
    assert st["kept"] <= keep
    return split(words, bins, npart), st, parts[:st["kept"]], drawn[:st["kept"]]


def list_rapidity(p, dimension, drawn=None):
    """What the sampler bins as rapidity: 0.5 log((E + pz) / (E - pz)) in 3+1D; in 2+1D the drawn rapidity -- known to
    the emulator, and otherwise recomputed from (E, pz), which is the drawn one to rounding."""
    if dimension == 2 and drawn is not None:
        return drawn
    return rapidity_from_momentum(p)


# --- python restatement of the writers (EmissionFunction.cpp:685-975) ----------------------------------------
def expected_files(hist, bins, n_events, mcids):
    """{path under results/sampled: text}: %.6g for the default float format with precision 6, %.6e for scientific."""
    w = widths(bins)
    nev, ycut = float(n_events), bins["y_cut"]
    mid = lambda lo, width, nb: [lo + width * (float(i) + 0.5) for i in range(int(nb))]
    y_mid, eta_mid = mid(-ycut, w["y"], bins["y_bins"]), mid(-bins["eta_cut"], w["eta"], bins["eta_bins"])
    pT_mid, phi_mid = mid(bins["pT_min"], w["pT"], bins["pT_bins"]), mid(0.0, w["phip"], bins["phip_bins"])
    tau_mid, r_mid = mid(bins["tau_min"], w["tau"], bins["tau_bins"]), mid(bins["r_min"], w["r"], bins["r_bins"])
    out = {}
    for s, mc in enumerate(mcids):
        f = lambda sub, tail="_test.dat": "%s/%s_%d%s" % (sub, sub, mc, tail)
        c = {name: [float(v) for v in hist[name][s]] for name, _ in PARTS}
        out[f("dN_dy")] = "".join("%.6g\t%.6g\n" % (m, n / (w["y"] * nev)) for m, n in zip(y_mid, c["dN_dy"]))
        avg = 0.0
        for n in c["dN_dy"]:
            avg += n
        out[f("dN_dy", "_average_test.dat")] = "%.6g\n" % (avg / (2.0 * ycut * nev))
        out[f("dN_deta")] = "".join("%.6g\t%.6g\n" % (m, n / (w["eta"] * nev)) for m, n in zip(eta_mid, c["dN_deta"]))
        out[f("dN_2pipTdpTdy")] = "".join("%.6e\t%.6e\n" % (m, n / (TWO_PI * 2.0 * ycut * w["pT"] * m * nev)) for m, n in zip(pT_mid, c["pT_count"]))
        out[f("dN_dphipdy")] = "".join("%.6e\t%.6e\n" % (m, n / (2.0 * ycut * w["phip"] * nev)) for m, n in zip(phi_mid, c["dN_dphipdy"]))
        rows = []
        for i, m in enumerate(pT_mid):
            row = "%.6e" % m
            for k in range(7):
                n = c["pT_count"][i]
                v = abs(complex(hist["vn_real"][k][s][i], hist["vn_imag"][k][s][i])) / n if n != 0.0 else 0.0   # 0 / 0, x / 0 -> 0
                row += "\t%.6e" % v
            rows.append(row + "\n")
        out[f("vn")] = "".join(rows)
        out[f("dN_taudtaudy")] = "".join("%.6e\t%.6e\n" % (m, n / (m * w["tau"] * nev * 2.0 * ycut)) for m, n in zip(tau_mid, c["dN_taudtaudy"]))
        out[f("dN_2pirdrdy")] = "".join("%.6e\t%.6e\n" % (m, n / (TWO_PI * m * w["r"] * nev * 2.0 * ycut)) for m, n in zip(r_mid, c["dN_2pirdrdy"]))
        out[f("dN_dphisdy")] = "".join("%.6e\t%.6e\n" % (m, n / (w["phip"] * nev * 2.0 * ycut)) for m, n in zip(phi_mid, c["dN_dphisdy"]))
    return out


def read_tree(d):
    """{path under d: text} of every file below d."""
    out = {}
    for base, _, files in os.walk(d):
        for fn in files:
            full = os.path.join(base, fn)
            with open(full) as f:
                out[os.path.relpath(full, d).replace(os.sep, "/")] = f.read()
    return out


def write_files(d, hist, bins, n_events, mcids):
    """host_io.cpp's write_sampled_files on a histogram dict."""
    counts = np.ascontiguousarray(np.concatenate([np.asarray(hist[name], dtype=np.int64).ravel() for name, _ in PARTS]))
    vn = np.ascontiguousarray(np.concatenate([np.asarray(hist["vn_real"], dtype=np.float64).ravel(),
                                              np.asarray(hist["vn_imag"], dtype=np.float64).ravel()]))
    mc = np.ascontiguousarray(mcids, dtype=np.int64)
    b = b14(bins)
    pl = C.POINTER(C.c_long)
    rc = lib().smpb_write(d.encode(), _d(b), len(mc), int(n_events), counts.ctypes.data_as(pl), _d(vn), mc.ctypes.data_as(pl))
    assert rc == 0
