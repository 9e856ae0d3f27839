"""CPU tier of the spin polarization (mode 5): the kernel's math (is3d2_amd/csrc/polzn_math.h, run serially by
tests/native/polzn_emulator.cpp) against the numpy restatement of Polarization.cpp:98-255 (tests/polzn_ref.py),
and the mode-5 reader round trip.

Parity is |got - ref| / sum |term| (the spin components cancel to ~1e-6 of their terms); the bar is the
project's 1e-8.  At the issue's sizes (150 cells, pT24) no output is left out of the comparison; where a case has
outputs with sum |term| below 1e-290 (pT up to 40 GeV in 3+1D: every cell's term overflows) they are counted and
checked to be exactly 0, or below that floor (polzn_ref.check_left_out).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from is3d2_amd import host, make_spec, rundir, synth

import polzn_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_SRC = os.path.join(HERE, "native", "polzn_emulator.cpp")
EMU_LIB = os.path.join(HERE, "native", "libpolzn_emulator.so")
SPECIES = [211, 2212, 3122]
T_AVG = 0.150
BAR = 1e-8


def emulator():
    srcs = [EMU_SRC, os.path.join(ROOT, "is3d2_amd", "csrc", "polzn_math.h")]
    if not os.path.exists(EMU_LIB) or any(os.path.getmtime(s) > os.path.getmtime(EMU_LIB) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", EMU_LIB, EMU_SRC])
    lib = C.CDLL(EMU_LIB)
    pd = C.POINTER(C.c_double)
    lib.polzn_emulate.argtypes = [C.c_int, C.c_int, pd, pd, C.c_int, pd, C.c_int, pd, C.c_int, pd, pd, C.c_long, pd, pd,
                                  C.c_long, C.c_long, C.c_double, C.c_int, pd]
    return lib


def emulate(spec, surf, w, T_avg, kj=8, lo=0, hi=None):
    lib = emulator()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    arr = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    dim = spec["params"]["dimension"]
    mass, sign = arr(spec["species"]["mass"]), arr(spec["species"]["sign"])
    pT, phi = arr(spec["pT"]), arr(spec["phi"])
    if dim == 3:
        qv = arr(spec["y"]); qw = np.ones(len(qv))
    else:
        qv = arr(spec["eta"]); qw = arr(spec["eta_w"]) * (qv[1] - qv[0])
    n = len(surf["tau"])
    s25 = arr(np.stack([surf[k] for k in synth.FIELDS]))
    w6 = arr(w)
    ny = len(qv) if dim == 3 else 1
    out = np.zeros((5, len(mass), len(pT), len(phi), ny))
    rc = lib.polzn_emulate(dim, len(mass), dp(mass), dp(sign), len(pT), dp(pT), len(phi), dp(phi), len(qv), dp(qv),
                           dp(qw), n, dp(s25), dp(w6), lo, n if hi is None else hi, T_avg, kj, dp(out))
    assert rc == 0
    return out


def case(dimension, n=150, seed=21, pT="pT24", u_scale=1.0):
    spec = make_spec(chosen=SPECIES, pT=pT, phi="phi24", y="y21", eta="eta24", dimension=dimension)
    surf = synth.surface(n, seed=seed, dimension=dimension, full3d=(dimension == 3))
    surf["ux"] = surf["ux"] * u_scale
    surf["uy"] = surf["uy"] * u_scale
    return spec, surf, synth.vorticity(n, 5)


@pytest.mark.parametrize("dimension", [2, 3])
def test_kernel_math_matches_the_reference_loop(dimension):
    spec, surf, w = case(dimension)
    S, A = polzn_ref.polarization(spec, surf, w, T_AVG)
    got = emulate(spec, surf, w, T_AVG)
    err, left_out = polzn_ref.parity(got, S, A)
    print("polzn cpu parity d=%d: max |got-ref|/sum|term| = %.3e, smallest sum|term| = %.3e" % (dimension, err, float(A.min())))
    assert left_out == 0
    assert np.isfinite(got).all()
    assert err <= BAR


@pytest.mark.parametrize("dimension", [2, 3])
def test_large_exponents_in_both_factors(dimension):
    """u^x, u^y x 3 and pT up to the pT48 table's end: the (cell, phi) exponent pT B / T and the lane's mT A / T are
    both large; they are shifted, not dropped."""
    spec, surf, w = case(dimension, pT="pT48", u_scale=3.0)
    S, A = polzn_ref.polarization(spec, surf, w, T_AVG)
    got = emulate(spec, surf, w, T_AVG)
    err, left_out = polzn_ref.parity(got, S, A)
    print("polzn cpu parity (u x 3, pT48) d=%d: %.3e, %d outputs below the floor" % (dimension, err, left_out))
    assert np.isfinite(got).all()
    assert err <= BAR
    # 2+1D: every output is compared.  3+1D: at pT ~ 40 GeV and y = +-5 every one of the 150 cells (|eta| < 4)
    # overflows for the heavier species -- 300 of 362 880 outputs in the restatement; they are exactly 0 or below
    # the floor here too, and they stay under 0.1 % of the outputs
    assert polzn_ref.check_left_out(got, S, A) == left_out
    assert left_out == 0 if dimension == 2 else left_out <= got.size // 1000


@pytest.mark.parametrize("kj", [1, 4, 8])
def test_phi_block_sizes_agree(kj):
    """The three lane forms (1, 4, 8 phi points per lane; four points share one division) give the same sums."""
    spec, surf, w = case(3, n=13)
    S, A = polzn_ref.polarization(spec, surf, w, T_AVG)
    err, _ = polzn_ref.parity(emulate(spec, surf, w, T_AVG, kj=kj), S, A)
    assert err <= BAR


def test_overflowing_term_contributes_exactly_zero():
    """exp(u.p / T) = inf in the reference makes that term 1 / (inf + s) = 0 (Polarization.cpp:187).  Cell 1 sits at
    eta = 4 with a large u^eta: against the y21 table its terms overflow for part of the outputs, and there the sums
    over both cells must equal the sums over cell 0 alone, bit for bit."""
    spec, surf, w = case(3, n=2)
    surf["eta"] = np.array([0.3, 4.0])
    surf["un"] = np.array([surf["un"][0], -2.0 / surf["tau"][1]])
    both = emulate(spec, surf, w, T_AVG)
    first = emulate(spec, surf, w, T_AVG, lo=0, hi=1)
    _, A1 = polzn_ref.polarization(spec, surf, w, T_AVG, lo=1, hi=2)
    gone = np.asarray(A1[4] == 0)              # every term of cell 1 overflowed (Snorm's |term| is 0 only then)
    assert gone.any() and not gone.all()
    assert np.isfinite(both).all()
    for k in range(5):
        np.testing.assert_array_equal(both[k][gone], first[k][gone])
    S, A = polzn_ref.polarization(spec, surf, w, T_AVG)
    err, _ = polzn_ref.parity(both, S, A)
    assert err <= BAR


@pytest.mark.parametrize("dimension,baryon", [(2, 0), (3, 1)])
def test_mode5_reader_keeps_the_vorticity(tmp_path, dimension, baryon):
    n = 37
    surf = synth.surface(n, seed=3, dimension=dimension, baryon=bool(baryon), full3d=(dimension == 3))
    d5, d1 = str(tmp_path / "m5"), str(tmp_path / "m1")
    params = dict(dimension=dimension, df_mode=1, include_baryon=baryon)
    rundir.write_run_dir(d5, surf, params, surface_format=5)
    rundir.write_run_dir(d1, surf, params, surface_format=1)
    w = host.read_vorticity(d5, dimension, baryon)
    np.testing.assert_array_equal(w, synth.vorticity(n, 5))
    f5, avg5 = host.read_surface(d5, 5, dimension, baryon)
    f1, avg1 = host.read_surface(d1, 1, dimension, baryon)
    np.testing.assert_array_equal(f5, f1)
    np.testing.assert_array_equal(avg5, avg1)
