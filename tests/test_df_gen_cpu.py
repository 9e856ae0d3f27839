"""CPU tier of the delta-f coefficient generator: is3d2_amd/csrc/dfgen_math.h on the host
(tests/native/dfgen_emulator.cpp) against the shipped tables and against the long-double restatement of the reference's
generator (tests/df_gen_ref.py), the table writer, and the declared entry point."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import df_gen_ref as R
from is3d2_amd import _lib, data, host, hrg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("hrg_eos,name", [(1, "urqmd"), (2, "smash"), (3, "box")])
def test_emulator_reproduces_the_shipped_tables(hrg_eos, name):
    # the full 101 x 81 grid, 64 points: the shipped files are these values rounded to six decimals
    T, muB, tab = data.df_tables(hrg_eos)
    got, err = R.emulate(R.named_list(name), T, muB)
    assert err is None
    R.assert_shipped(got, tab, name)


@pytest.mark.parametrize("name", ["smash", "urqmd"])
@pytest.mark.parametrize("grid,points", [(R.GRID_4x4, 64), (R.GRID_WIDE, 64), (R.GRID_4x4, 32)])
def test_emulator_matches_the_long_double_restatement(name, grid, points):
    # 32 points: half the lanes hold no node (the strided-node path's bound)
    ref, code = R.restated(name, grid, points)
    assert not code.any()
    got, err = R.emulate(R.named_list(name), grid[0], grid[1], points)
    assert err is None
    R.assert_ref(got, ref, "%s %d points" % (name, points))


def test_baryon_tables_vanish_exactly_at_zero_muB():
    # baryon and antibaryon terms cancel pairwise: c1, c4 and G are exactly 0, as in the restatement
    ref, _ = R.restated("smash", R.GRID_4x4)
    got, _ = R.emulate(R.named_list("smash"), *R.GRID_4x4)
    for k in (1, 4, 6):
        assert np.all(ref[k, 0] == 0.0) and np.all(got[k, 0] == 0.0), R.NAMES[k]
        assert np.all(got[k, 1:] != 0.0)


def test_three_hadron_list():
    ref, code = R.restate(R.THREE, *R.GRID_4x4)
    got, err = R.emulate(R.THREE, *R.GRID_4x4)
    assert err is None and not code.any()
    R.assert_ref(got, ref, "three hadrons")


def test_sixty_five_hadron_list():
    ref, code = R.restated("smash65", R.GRID_4x4)
    got, err = R.emulate(R.named_list("smash65"), *R.GRID_4x4)
    assert err is None and not code.any()
    R.assert_ref(got, ref, "65 hadrons")


def test_photon_row_is_skipped():
    # UrQMD's first row is the photon (mass 0): the list without it gives the same bits
    p = R.named_list("urqmd")
    assert p["mass"][0] == 0.0
    rest = {k: v[1:] for k, v in p.items() if k != "mcid"}
    a, _ = R.emulate(p, *R.GRID_4x4)
    b, _ = R.emulate(rest, *R.GRID_4x4)
    assert a.tobytes() == b.tobytes()
    assert np.all(np.isfinite(a))


def test_meson_only_list_is_the_bulk_denominator_error():
    got, err = R.emulate(R.MESONS, [0.12, 0.15], [0.0, 0.3])
    assert err == ("Bulk denominator is zero", 0.12, 0.0)
    _, code = R.restate(R.MESONS, [0.12, 0.15], [0.0, 0.3])
    assert np.all(code == 1) and R.CODES[1] == err[0]


def test_a_point_does_not_depend_on_its_grid():
    T, muB = R.GRID_4x4
    whole, _ = R.emulate(R.THREE, T, muB)
    for iB, m in enumerate(muB):
        for iT, t in enumerate(T):
            one, _ = R.emulate(R.THREE, [t], [m])
            assert one[:, 0, 0].tobytes() == whole[:, iB, iT].tobytes()


def test_write_df_tables_round_trip(tmp_path):
    T, muB, tab = data.df_tables(2)
    d = str(tmp_path / "smash")
    hrg.write_df_tables(d, T, muB, tab)
    assert sorted(os.listdir(d)) == sorted(n + ".dat" for n in R.NAMES)
    # the rows of deltaf_coefficients/vh/smash/c0.dat: nT, nmuB, the label line, muB outer and T inner
    lines = open(os.path.join(d, "c0.dat")).read().split("\n")
    assert lines[:5] == ["101", "81", "T [GeV]\t\tmuB [GeV]\t\tc0_T4 [fm^3/GeV^3 * GeV^4]",
                         "0.100000\t\t0.000000\t\t-0.545933", "0.101000\t\t0.000000\t\t-0.519020"]
    assert lines[3 + 101].startswith("0.100000\t\t0.010000\t\t") and len([ln for ln in lines if ln]) == 3 + 101 * 81
    T2, muB2, tab2 = host.read_df_tables(d)
    np.testing.assert_array_equal(T2, T)
    np.testing.assert_array_equal(muB2, muB)
    np.testing.assert_array_equal(tab2, tab)           # the shipped values have six decimals: equal to the digit


def test_write_df_tables_digits(tmp_path):
    T, muB = np.array(R.GRID_5x3[0]), np.array(R.GRID_5x3[1])
    tab, _ = R.emulate(R.THREE, T, muB)
    for digits in (6, 12):
        d = str(tmp_path / ("d%d" % digits))
        hrg.write_df_tables(d, T, muB, tab, digits=digits)
        T2, muB2, tab2 = host.read_df_tables(d)
        np.testing.assert_array_equal(T2, T)
        assert tab2.shape == (10, 3, 5)
        written = np.array([float("%.*f" % (digits, v)) for v in tab.ravel()]).reshape(tab.shape)
        np.testing.assert_array_equal(tab2, written)                    # equal to the written digits
        assert np.max(np.abs(tab2 - tab)) <= 0.5 * 10.0 ** -digits * (1 + 1e-6)


def test_library_declares_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "is3d_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"int\s+is3d_generate_df_tables\s*\(([^)]*)\)\s*;", hdr)
    assert m, "is3d_generate_df_tables is not declared"
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert args == ["is3d_engine *e", "int nT", "int nmuB", "const double *T", "const double *muB", "double *tables"]
    assert "is3d_generate_df_tables" in _lib.EXPORTS
    assert hasattr(C.CDLL(_lib.LIB_PATH), "is3d_generate_df_tables")
    lib = _lib.load()
    pd = C.POINTER(C.c_double)
    assert list(lib.is3d_generate_df_tables.argtypes) == [C.c_void_p, C.c_int, C.c_int, pd, pd, pd]
