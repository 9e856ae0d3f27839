"""GPU tier of the delta-f coefficient generator (is3d_generate_df_tables, csrc/dfgen.hip): the kernel
against the shipped tables, the host build of its math and the long-double restatement of the reference's generator,
its bit guarantees, and the tables at work in the engine."""
import numpy as np
import pytest

import df_gen_ref as R
from helpers import parity
from is3d2_amd import Engine, IS3DError, _lib, build_engine, data, make_spec, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-8      # the spectra against the oracle (tests/test_gpu_parity.py)

SMALL_GRIDS = {"1x1": ((0.15,), (0.0,)), "3x1": ((0.1, 0.15, 0.2), (0.0,)), "4x3": ((0.1, 0.13, 0.155, 0.2), (0.0, 0.05, 0.4))}
SMALL_LISTS = {"three": R.THREE, "smash65": None}


def small_list(name):
    return R.named_list(name) if SMALL_LISTS[name] is None else SMALL_LISTS[name]


def gen_engine(parts, points=64, devices=None):
    e = Engine(devices=devices)
    e.set_pdg(parts["mass"], parts["sign"], parts["gspin"], parts["baryon"])
    e.set_gauss_laguerre(*data.gauss_laguerre(points))
    return e


@pytest.mark.parametrize("hrg_eos,name", [(1, "urqmd"), (2, "smash"), (3, "box")])
def test_real_lists_on_the_shipped_subgrid(hrg_eos, name):
    T, muB, shipped = R.shipped_subgrid(hrg_eos)
    e = gen_engine(R.named_list(name))
    got = e.generate_df_tables(T, muB)
    e.close()
    assert got.shape == (10, 3, 5)
    R.assert_shipped(got, shipped, name)
    emu, err = R.emulate(R.named_list(name), T, muB)
    assert err is None
    R.assert_ref(got, emu, name + " vs emulator")
    R.assert_ref(got, R.restated(name, R.GRID_5x3)[0], name + " vs restatement")


@pytest.mark.parametrize("name", ["smash", "urqmd"])
def test_wide_grid_matches_the_restatement(name):
    T, muB = R.GRID_WIDE
    e = gen_engine(R.named_list(name))
    got = e.generate_df_tables(T, muB)
    e.close()
    R.assert_ref(got, R.restated(name, R.GRID_WIDE)[0], name + " wide")


@pytest.mark.parametrize("points", [32, 64])
@pytest.mark.parametrize("lst", ["three", "smash65"])
@pytest.mark.parametrize("grid", ["1x1", "3x1", "4x3"])
def test_small_shapes(grid, lst, points):
    T, muB = SMALL_GRIDS[grid]
    parts = small_list(lst)
    e = gen_engine(parts, points)
    got = e.generate_df_tables(T, muB)
    e.close()
    emu, err = R.emulate(parts, T, muB, points)
    assert err is None
    R.assert_ref(got, emu, "vs emulator")
    ref, code = R.restate(parts, T, muB, points)
    assert not code.any()
    R.assert_ref(got, ref, "vs restatement")
    if lst == "three":                      # baryon and antibaryon cancel: c1, c4, G vanish exactly at muB = 0
        for k in (1, 4, 6):
            assert np.all(got[k, 0] == 0.0)


def test_bits_repeat_and_point_alone():
    T, muB = SMALL_GRIDS["4x3"]
    e = gen_engine(R.named_list("smash65"))
    a = e.generate_df_tables(T, muB)
    b = e.generate_df_tables(T, muB)
    assert a.tobytes() == b.tobytes()
    for iB, m in enumerate(muB):
        for iT, t in enumerate(T):
            one = e.generate_df_tables([t], [m])
            assert one[:, 0, 0].tobytes() == a[:, iB, iT].tobytes(), (t, m)
    e.close()


def test_bits_device_list_engine():
    T, muB = SMALL_GRIDS["4x3"]
    parts = R.named_list("smash65")
    e = gen_engine(parts)
    a = e.generate_df_tables(T, muB)
    e.close()
    g = gen_engine(parts, devices=[0, 0])
    b = g.generate_df_tables(T, muB)
    g.close()
    assert a.tobytes() == b.tobytes()


def test_generate_has_no_side_effect():
    s = synth.as_read(synth.surface(40, seed=3))
    spec = make_spec(hrg_eos=2, chosen="pikp", df_mode=1, dimension=2)
    e = build_engine(spec, s)
    before = e.calculate_spectra()
    plan = lambda: ({k: v for k, v in e.stats().items() if not k.startswith("ms_")},
                    e.get_tuning("splits"), e.get_tuning("phitab_chunks"))
    p0 = plan()
    tab = e.generate_df_tables(*R.GRID_5x3)
    assert np.all(np.isfinite(tab))
    assert plan() == p0
    after = e.calculate_spectra()
    assert plan() == p0
    e.close()
    assert before.tobytes() == after.tobytes()
    assert before.any()


@pytest.mark.parametrize("mode,baryon", [(1, 0), (2, 0), (1, 1), (2, 1)])
def test_installed_tables_evaluate_to_the_generated_values(mode, baryon):
    T, muB = np.array(R.GRID_5x3[0]), np.array(R.GRID_5x3[1])
    spec = make_spec(hrg_eos=2, chosen="pikp", df_mode=mode, dimension=2, include_baryon=baryon)
    e = build_engine(spec, None, T_avg=0.15)
    e.set_gauss_laguerre(*data.gauss_laguerre(64))
    tab = e.generate_df_tables(T, muB)
    e.set_gauss_laguerre(*spec["gla"])
    e.set_df_tables(T, muB, tab, 0.15)
    # out15 = c0 c1 c2 c3 c4 shear14 F G betabulk betaV betapi ...; the tables hold the coefficients scaled by T^n
    if mode == 1:
        cols = [(0, 0, -4), (2, 2, -4)] + ([(1, 1, -3), (3, 3, -4), (4, 4, -5)] if baryon else [])
    else:
        cols = [(6, 5, 1), (8, 7, 4), (10, 9, 4)] + ([(7, 6, 0), (9, 8, 3)] if baryon else [])
    # without baryon: the cubic spline in T of the muB = 0 row passes through its nodes; with: the bilinear cell's corner
    nodes = [(iT, iB) for iT in range(5) for iB in range(3)] if not baryon else [(iT, iB) for iT in range(4) for iB in range(2)]
    for iT, iB in nodes:
        if not baryon and iB > 0:
            continue
        out = e.evaluate_df_coefficients(T[iT], muB[iB], 0.3, 0.05, -0.001)
        for o, k, n in cols:
            want = tab[k, iB, iT] * T[iT] ** n
            assert abs(out[o] - want) <= 1e-13 * abs(want), (mode, baryon, R.NAMES[k], T[iT], muB[iB], out[o], want)
    e.close()


def hot_surface():
    s = synth.surface(13, seed=5)
    s["T"] = np.full(13, 0.25)
    s["E"] = 0.28 * (s["T"] / 0.15) ** 4
    s["P"] = 0.045 * (s["T"] / 0.15) ** 4
    return synth.as_read(s)


def test_surface_above_the_shipped_range():
    s = hot_surface()
    spec = make_spec(hrg_eos=2, chosen="pikp", df_mode=2, dimension=2)
    e = build_engine(spec, s)
    with pytest.raises(IS3DError) as ei:       # today's behaviour: T = 0.25 GeV is outside the shipped tables
        e.calculate_spectra()
    assert ei.value.code == _lib.IS3D_ERR_DF_RANGE
    e.close()
    spec = make_spec(hrg_eos=2, chosen="pikp", df_mode=2, dimension=2, df_tables="generate",
                     df_grid=(np.linspace(0.2, 0.3, 11), np.linspace(0.0, 0.1, 3)))
    e = build_engine(spec, s)
    got = e.calculate_spectra()
    e.close()
    assert spec["df"][2].shape == (10, 3, 11)
    ref = O.spectra(spec, s, threads=1)          # the oracle reads the same generated tables from the spec
    rel, zr, zg = parity(got, ref)
    print("T = 0.25 GeV surface, generated tables: max rel err vs oracle %.3e" % rel)
    assert rel < TOL and zr == zg and got.any()


def test_make_spec_generate_on_the_standard_surface():
    s = synth.as_read(synth.surface(200, seed=11))
    shipped = make_spec(hrg_eos=2, chosen="pikp", df_mode=1, dimension=2)
    e = build_engine(shipped, s)
    base = e.calculate_spectra()
    e.close()
    spec = make_spec(hrg_eos=2, chosen="pikp", df_mode=1, dimension=2, df_tables="generate")
    e = build_engine(spec, s)
    got = e.calculate_spectra()
    e.close()
    T, muB, tab = spec["df"]
    assert tab.shape == shipped["df"][2].shape and np.array_equal(T, shipped["df"][0])
    R.assert_shipped(tab, shipped["df"][2], "make_spec generate")
    assert not np.array_equal(got, base)          # unrounded coefficients: the spectra move
    rel = parity(got, O.spectra(spec, s, threads=1))[0]
    print("generated tables, standard surface: max rel err vs oracle %.3e" % rel)
    assert rel < TOL


def test_errors():
    T, muB = np.array([0.1, 0.15, 0.2]), np.array([0.0, 0.4])
    smash = R.named_list("smash")
    e = Engine()
    e.set_gauss_laguerre(*data.gauss_laguerre(64))
    with pytest.raises(IS3DError) as ei:                      # no PDG
        e.generate_df_tables(T, muB)
    assert ei.value.code == _lib.IS3D_ERR_STATE
    e.set_pdg(smash["mass"], smash["sign"], smash["gspin"], smash["baryon"])
    r, w = data.gauss_laguerre(64)
    e.set_gauss_laguerre(r[:4], w[:4])                        # rows 0 .. 3: alpha = 4 is missing
    with pytest.raises(IS3DError) as ei:
        e.generate_df_tables(T, muB)
    assert ei.value.code == _lib.IS3D_ERR_STATE
    e.set_gauss_laguerre(r, w)
    for bad in (T[::-1], np.array([0.0, 0.1, 0.2]), np.array([0.1, 0.1, 0.2])):
        with pytest.raises(IS3DError) as ei:
            e.generate_df_tables(bad, muB)
        assert ei.value.code == _lib.IS3D_ERR_ARG
    with pytest.raises(IS3DError) as ei:
        e.generate_df_tables(T, muB[::-1])
    assert ei.value.code == _lib.IS3D_ERR_ARG
    assert np.all(np.isfinite(e.generate_df_tables(T, muB)))  # the engine is still usable
    m = R.MESONS
    e.set_pdg(m["mass"], m["sign"], m["gspin"], m["baryon"])
    with pytest.raises(IS3DError, match="Bulk denominator is zero") as ei:
        e.generate_df_tables(T, muB)
    assert ei.value.code == _lib.IS3D_ERR_DF_RANGE
    assert "T = 0.1" in str(ei.value) and "muB = 0 " in str(ei.value)
    e.close()
