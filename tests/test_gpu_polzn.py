"""GPU tier of the spin polarization from thermal vorticity (mode 5): k_polzn / k_polzn_reduce (polzn.hip)
through the C ABI, the device-list engine, the Python binding and the run-directory workflow.

Reference: tests/polzn_ref.py, the numpy restatement of Polarization.cpp:98-255.  The four spin components
cancel (random vorticity sign: |sum| / sum |term| down to ~1e-6), so parity is |got - ref| / sum |term|; the bar
is the project's 1e-8 and at 150 cells no output is left out of the comparison (on the 1- and 13-cell surfaces the
outputs below the 1e-290 floor are checked to be exactly 0, or below it).  Independent of that restatement, Snorm is
tied to the oracle-pinned spectra: on a constant-T surface without delta-f it is the Cooper-Frye sum itself.
"""
import functools
import os

import numpy as np
import pytest

import polzn_ref
from helpers import parity
from is3d2_amd import Engine, IS3DError, _lib, build_engine, host, make_spec, rundir, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

T_AVG = 0.150
BAR = 1e-8            # of sum |term| (README parity bar)
ROUNDING = 1e-12      # of sum |term|: the same terms added in another order (<= 300 terms: ~300 eps = 7e-14)
HBARC = 0.197327053   # the project's constant (cf_math.h kHbarC, iS3D.h:14)
UNIQUE = [211, 2212, 3122]
SPECIES = [211, -211, 2212, 3122]        # pi+ and pi- share one (mass, sign) class


def polzn_engine(spec, surf, w=None, devices=None, classes=True):
    """An engine with only what the polarization needs: params, species, grid, surface, vorticity -- no PDG set,
    Gauss-Laguerre table or delta-f tables."""
    e = Engine(devices=devices)
    e.set_params(**spec["params"])
    sp = spec["species"]
    e.set_species(sp["mass"], sp["sign"], sp["degen"], sp["baryon"])
    if not classes:
        e.set_species_classes(False)
    e.set_momentum_grid(spec["pT"], spec["phi"], spec["y"], spec["eta"], spec["eta_w"])
    e.set_surface(surf)
    if w is not None:
        e.set_vorticity(w)
    return e


def run(spec, surf, w, T=T_AVG, **kw):
    e = polzn_engine(spec, surf, w, **kw)
    out = e.calculate_polarization(T)
    st = e.stats()
    e.close()
    return out, st


def cut(surf, lo, hi):
    return {k: v[lo:hi] for k, v in surf.items()}


def spec_for(dimension, phi, chosen):
    return make_spec(chosen=chosen, pT="pT24", phi=phi, y="y21", eta="eta24", dimension=dimension)


@functools.lru_cache(maxsize=None)
def case(dimension, phi, n=150, seed=21):
    """Surface, vorticity and the restatement's (sums, abs sums) of the first 1, 13 and n cells, for SPECIES
    (computed for the three distinct species; pi- copies pi+, whose (mass, sign) it shares)."""
    surf = synth.surface(n, seed=seed, dimension=dimension, full3d=(dimension == 3))
    w = synth.vorticity(n, 5)
    spec_u = spec_for(dimension, phi, UNIQUE)
    refs, S, A = {}, 0, 0
    lo = 0
    for hi in sorted({1, 13, n}):
        s, a = polzn_ref.polarization(spec_u, surf, w, T_AVG, lo=lo, hi=hi)
        S, A = S + s, A + a
        refs[hi] = (S[:, [0, 0, 1, 2]].copy(), A[:, [0, 0, 1, 2]].copy())
        lo = hi
    return surf, w, refs


@pytest.mark.parametrize("phi", ["phi24", "phi32", "phi48", "phi_default"])
@pytest.mark.parametrize("dimension", [2, 3])
def test_parity_with_the_reference_loop(dimension, phi):
    surf, w, refs = case(dimension, phi)
    spec = spec_for(dimension, phi, SPECIES)
    worst = 0.0
    for n, (S, A) in sorted(refs.items()):
        got, st = run(spec, cut(surf, 0, n), w[:, :n])
        assert got.shape == S.shape
        assert st["cells"] == n
        err, left_out = polzn_ref.parity(got, S, A)
        worst = max(worst, err)
        if n == max(refs):
            assert left_out == 0, "sum |term| below 1e-290: re-check the case on the CPU"
        # 1 and 13 cells in 3+1D: far from the cells' eta every term overflows (1 / (inf + s) = 0): those outputs
        # are exactly 0, and any other output left out is below the floor itself
        assert polzn_ref.check_left_out(got, S, A) == left_out
        assert np.isfinite(got).all()
        assert err <= BAR, (n, err)
        if n == max(refs):
            # classes (pi+ / pi- integrated once) against every species on its own lane
            each, _ = run(spec, cut(surf, 0, n), w[:, :n], classes=False)
            assert np.max(np.abs(each.astype(np.longdouble) - got) / A) < 1e-9
            np.testing.assert_array_equal(got[:, 0], got[:, 1])
    print("polzn gpu parity d=%d %s: max |got-ref|/sum|term| = %.3e" % (dimension, phi, worst))


@pytest.mark.parametrize("dimension", [2, 3])
def test_snorm_is_the_cooper_frye_sum_of_the_spectra_path(dimension):
    """Constant T, every delta-f flag off, Grad, only cells with u.dsigma > 0: dN = g (2 pi hbarc)^-3 sum p.dsigma f0,
    which is Snorm x g / (2 pi hbarc)^3 -- in 2+1D over (eta_2 - eta_1), the extra factor the reference's
    polarization loop carries (Polarization.cpp:58,68)."""
    s = synth.surface(300, seed=21, dimension=dimension, full3d=(dimension == 3))
    ut = np.sqrt(1.0 + s["ux"] ** 2 + s["uy"] ** 2 + (s["tau"] * s["un"]) ** 2)
    live = ut * s["dat"] + s["ux"] * s["dax"] + s["uy"] * s["day"] + s["un"] * s["dan"] > 0.0
    s = {k: np.ascontiguousarray(v[live]) for k, v in s.items()}
    n = len(s["tau"])
    assert n > 250
    s["T"] = np.full(n, T_AVG)
    spec = make_spec(chosen=UNIQUE, pT="pT24", phi="phi24", y="y21", eta="eta24", dimension=dimension, df_mode=1,
                     include_bulk_deltaf=0, include_shear_deltaf=0, include_baryondiff_deltaf=0, include_baryon=0,
                     regulate_deltaf=0, outflow=0)
    dN = O.spectra(spec, s, T_avg=T_AVG).reshape(3, 24, 24, -1)
    got, _ = run(spec, s, synth.vorticity(n, 5))
    g = np.asarray(spec["species"]["degen"], dtype=np.float64)[:, None, None, None]
    mine = got[4] * g / (2.0 * np.pi * HBARC) ** 3
    if dimension == 2:
        mine = mine / (spec["eta"][1] - spec["eta"][0])
    m = np.abs(dN) > 1e-280
    assert m.sum() > 0.9 * m.size
    rel = np.max(np.abs(mine[m] - dN[m]) / np.abs(dN[m]))
    print("Snorm vs oracle spectra d=%d: max rel %.3e over %d of %d outputs" % (dimension, rel, m.sum(), m.size))
    assert rel < 1e-9


def big_case():
    n = 100000
    surf = synth.surface(n, seed=77, dimension=3, full3d=True)
    spec = make_spec(chosen=[3122, -3122, 3312, 3334], pT="pT48", phi="phi32", y="y21", dimension=3)
    return n, surf, spec


def test_realistic_size_reproducible_and_snorm_independent_of_vorticity():
    """10^5 cells x 4 species x 48 x 32 x 21: two runs are bit-identical (fixed summation order, no atomics) and
    Snorm does not see the vorticity."""
    n, surf, spec = big_case()
    w1, w2 = synth.vorticity(n, 1), synth.vorticity(n, 2)
    e = polzn_engine(spec, surf, w1)
    a = e.calculate_polarization(T_AVG)
    b = e.calculate_polarization(T_AVG)
    assert e.stats()["cells"] == n
    e.set_vorticity(w2)
    c = e.calculate_polarization(T_AVG)
    e.close()
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a[4], c[4])
    assert np.isfinite(a).all() and np.isfinite(c).all()
    assert not np.array_equal(a[:4], c[:4])


# (nonzero vorticity components, all > 0) -> the outputs whose bracket then has one sign per momentum point:
#   S_t = wxy pn - wxn py + wyn px    S_x = wyn pt - wtn py + wty pn
#   S_y = -wxn pt + wtn px - wtx pn   S_n = wtx py + wxy pt - wty px
# pt > 0 and px, py depend on the momentum point only; pn changes sign from cell to cell, so its terms are left out
LINEAR_CASES = [((2, 3), (1, 2, 3)),    # wtn, wxy: S_x, S_y, S_n
                ((5,), (0, 1)),         # wyn: S_t, S_x
                ((4,), (0, 2)),         # wxn: S_t, S_y
                ((0,), (3,)),           # wtx: S_n
                ((1,), (3,))]           # wty: S_n


def test_realistic_size_linear_in_the_vorticity():
    """S(w1 + w2) = S(w1) + S(w2) at 10^5 cells, for every vorticity component and every output.  Without a reference
    the rounding scale must come from sums that cannot cancel (a run with |w| does not give sum |term|: the brackets
    also take their signs from pn and from p.dsigma, which differ from cell to cell).  So dsigma_tau is raised until
    p.dsigma > 0 in every cell -- p.dsigma >= pt (dat - |dax| - |day| - |dan| / tau), since |px|, |py| <= pt and
    |pn| <= pt / tau; dsigma_x, dsigma_y, dsigma_eta stay as drawn -- and each case switches on only vorticity
    components, all positive, for which the listed outputs' brackets have one sign per momentum point.  Those sums
    and Snorm are then sums of same-sign terms: each of the three runs is within n eps = 1.1e-11 of its exact sum
    (10^5 terms), hence the 1e-10 relative bound."""
    n, surf, spec = big_case()
    surf = dict(surf)
    margin = surf["dat"].copy()
    assert margin.min() > 0.0
    surf["dat"] = margin + np.abs(surf["dax"]) + np.abs(surf["day"]) + np.abs(surf["dan"]) / surf["tau"]
    assert np.all(surf["dat"] - np.abs(surf["dax"]) - np.abs(surf["day"]) - np.abs(surf["dan"]) / surf["tau"] > 0.0)
    assert np.abs(surf["dax"]).min() > 0.0 and np.abs(surf["dan"]).max() > 0.0
    rng = np.random.default_rng(9)
    e = polzn_engine(spec, surf, None)
    worst = 0.0
    for comps, outputs in LINEAR_CASES:
        ws = []
        for _ in range(2):
            w = np.zeros((6, n))
            for k in comps:
                w[k] = rng.uniform(0.01, 0.1, n)
            ws.append(w)
        res = []
        for w in (ws[0], ws[1], ws[0] + ws[1]):
            e.set_vorticity(w)
            res.append(e.calculate_polarization(T_AVG))
        s1, s2, s12 = res
        for c in outputs + (4,):
            m = np.abs(s12[c]) > 1e-280
            assert m.sum() > 0.5 * m.size
            total = s1[c][m] + s2[c][m] if c < 4 else s1[c][m]
            worst = max(worst, float(np.max(np.abs(s12[c][m] - total) / np.abs(s12[c][m]))))
        np.testing.assert_array_equal(s1[4], s12[4])
    e.close()
    print("polzn linearity at 1e5 cells: max rel %.3e" % worst)
    assert worst < 1e-10


@functools.lru_cache(maxsize=None)
def window_case():
    surf = synth.surface(300, seed=21, dimension=3, full3d=True)
    w = synth.vorticity(300, 5)
    spec = spec_for(3, "phi24", UNIQUE)
    part = polzn_ref.polarization(spec, surf, w, T_AVG, lo=37, hi=211)
    rest = [polzn_ref.polarization(spec, surf, w, T_AVG, lo=lo, hi=hi) for lo, hi in ((0, 37), (211, 300))]
    whole = tuple(part[k] + rest[0][k] + rest[1][k] for k in range(2))
    return surf, w, spec, part, whole


def test_cell_windows():
    surf, w, spec, (S, A), (S_all, A_all) = window_case()
    e = polzn_engine(spec, surf, w)
    whole = e.calculate_polarization(T_AVG)
    err, left_out = polzn_ref.parity(whole, S_all, A_all)
    assert left_out == 0 and err <= BAR
    e.set_cell_window(37, 211)
    part = e.calculate_polarization(T_AVG)
    assert e.stats()["cells"] == 211 - 37
    err, left_out = polzn_ref.parity(part, S, A)
    assert left_out == 0 and err <= BAR
    e.set_cell_window(0, 150)
    lo = e.calculate_polarization(T_AVG)
    e.set_cell_window(150, 300)
    hi = e.calculate_polarization(T_AVG)
    e.set_cell_window(-1, -1)
    again = e.calculate_polarization(T_AVG)
    e.close()
    np.testing.assert_array_equal(again, whole)
    assert np.max(np.abs((lo.astype(np.longdouble) + hi) - whole) / A_all) < ROUNDING


def test_split_knobs_change_only_the_summation_order():
    surf, w, spec, _, (S, A) = window_case()
    e = polzn_engine(spec, surf, w)
    base = e.calculate_polarization(T_AVG)
    n0 = e.get_tuning("splits")
    e.set_tuning("max_splits", 3)
    few = e.calculate_polarization(T_AVG)
    assert e.get_tuning("splits") == 3
    e.set_tuning("max_splits", -1)
    e.set_tuning("split_bytes", 120 * 16)      # 16 cells per split
    many = e.calculate_polarization(T_AVG)
    assert e.get_tuning("splits") >= max(n0, 300 // 16)
    e.close()
    for other in (few, many):
        assert np.max(np.abs(other.astype(np.longdouble) - base) / A) < ROUNDING


def check_device_list(devices):
    surf, w, spec, _, (S, A) = window_case()
    one, st1 = run(spec, surf, w)
    grp, stg = run(spec, surf, w, devices=devices)
    assert stg["cells"] == st1["cells"] == 300
    assert np.max(np.abs(grp.astype(np.longdouble) - one) / A) < ROUNDING


def test_device_list_engine_on_a_repeated_device():
    check_device_list([0, 0])


def test_device_list_engine_on_two_gpus():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    check_device_list([0, 1])


def test_minimal_state_and_errors():
    surf, w, spec, _, _ = window_case()
    e = polzn_engine(spec, surf, None)
    with pytest.raises(IS3DError) as ei:
        e.calculate_polarization(T_AVG)
    assert ei.value.code == _lib.IS3D_ERR_STATE
    with pytest.raises(IS3DError) as ei:
        e.set_vorticity(w[:, :299])
    assert ei.value.code == _lib.IS3D_ERR_ARG
    e.set_vorticity({k: w[i] for i, k in enumerate(_lib.VORTICITY_FIELDS)})
    with pytest.raises(IS3DError) as ei:
        e.calculate_polarization(0.0)
    assert ei.value.code == _lib.IS3D_ERR_ARG
    out = e.calculate_polarization(T_AVG)          # no PDG set, Gauss-Laguerre or delta-f tables on this engine
    assert out.shape == (5, 3, 24, 24, 21) and np.isfinite(out).all()
    e.set_surface(surf)                            # a new surface clears the vorticity
    with pytest.raises(IS3DError) as ei:
        e.calculate_polarization(T_AVG)
    assert ei.value.code == _lib.IS3D_ERR_STATE
    e.close()
    # a device-list engine reports the same
    g = polzn_engine(spec, surf, None, devices=[0, 0])
    with pytest.raises(IS3DError) as ei:
        g.calculate_polarization(T_AVG)
    assert ei.value.code == _lib.IS3D_ERR_STATE
    g.close()
    # vorticity before any surface: a missing step on both kinds of engine, whatever its length
    for devices in (None, [0, 0]):
        e = Engine(devices=devices)
        e.set_params(**spec["params"])
        with pytest.raises(IS3DError) as ei:
            e.set_vorticity(w)
        assert ei.value.code == _lib.IS3D_ERR_STATE
        e.close()


def test_spectra_unchanged_by_a_polarization_call():
    surf, w, spec, _, _ = window_case()
    s = synth.as_read(surf)
    full = make_spec(chosen=UNIQUE, pT="pT24", phi="phi24", y="y21", eta="eta24", dimension=3, df_mode=2)
    e = build_engine(full, dict(s, **{k: w[i] for i, k in enumerate(_lib.VORTICITY_FIELDS)}))
    before = e.calculate_spectra()
    pol = e.calculate_polarization(T_AVG)          # build_engine passed the wtx..wyn keys along
    after = e.calculate_spectra()
    e.close()
    np.testing.assert_array_equal(before, after)
    alone, _ = run(spec, s, w)
    np.testing.assert_array_equal(pol, alone)


def read_s_file(path):
    rows = [ln.split("\t") for ln in open(path).read().split("\n") if ln]
    return np.array([[float(v) for v in r] for r in rows])


@pytest.mark.parametrize("dimension", [2, 3])
def test_run_directory_writes_the_four_files(tmp_path, dimension):
    n = 150
    surf = synth.surface(n, seed=31, dimension=dimension, full3d=(dimension == 3))
    params = dict(dimension=dimension, df_mode=1, include_baryon=0, include_bulk_deltaf=1, include_shear_deltaf=1,
                  include_baryondiff_deltaf=0, regulate_deltaf=0, outflow=0, deta_min=1e-5, mass_pion0=0.138)
    d = rundir.write_run_dir(str(tmp_path / "m5"), surf, params, hrg_eos=2, chosen="pikp", surface_format=5)
    spec = make_spec(hrg_eos=2, chosen="pikp", pT="pT24", phi="phi24", **params)
    fields, avg = host.read_surface(d, 5, dimension, 0)
    rs = {k: fields[i] for i, k in enumerate(synth.FIELDS)}
    ref = O.spectra(spec, rs, T_avg=avg[0])
    got = host.run_particlization(d, len(ref))
    assert parity(got, ref)[0] < 1e-8
    npart, npT, nphi, ny = 3, 24, 24, (21 if dimension == 3 else 1)
    files = {c: read_s_file(os.path.join(d, "results", "S%s.dat" % c)) for c in "txyn"}
    os.remove(os.path.join(d, "results", "St.dat"))
    S = host.polarization(d, 5 * len(ref)).reshape(5, npart, npT, nphi, ny)
    assert os.path.exists(os.path.join(d, "results", "St.dat"))
    yv = spec["y"] if dimension == 3 else np.zeros(1)
    for k, c in enumerate("txyn"):
        rows = files[c]
        assert rows.shape == (npart * ny * nphi * npT, 4)
        # file order: species -> y -> phi -> pT; every row is looked up by its own labels
        ip = np.repeat(np.arange(npart), ny * nphi * npT)
        iy = np.abs(rows[:, 0][:, None] - yv[None, :]).argmin(axis=1)
        iphi = np.abs(rows[:, 1][:, None] - spec["phi"][None, :]).argmin(axis=1)
        ipT = np.abs(rows[:, 2][:, None] - spec["pT"][None, :]).argmin(axis=1)
        np.testing.assert_allclose(rows[:, 0], yv[iy], rtol=5e-9, atol=1e-300)
        np.testing.assert_allclose(rows[:, 1], spec["phi"][iphi], rtol=5e-9)
        np.testing.assert_allclose(rows[:, 2], spec["pT"][ipT], rtol=5e-9)
        assert len(set(zip(ip, iy, iphi, ipT))) == len(rows)
        np.testing.assert_allclose(rows[:, 3], S[k][ip, ipT, iphi, iy] / S[4][ip, ipT, iphi, iy], rtol=5e-9)
    w = host.read_vorticity(d, dimension, 0)
    np.testing.assert_array_equal(w, synth.vorticity(n, 5))
    Sr, Ar = polzn_ref.polarization(spec, rs, w, avg[0])
    err, left_out = polzn_ref.parity(S, Sr, Ar)
    assert left_out == 0 and err <= BAR
    # a mode-1 directory gets the spectra and nothing else
    d1 = rundir.write_run_dir(str(tmp_path / "m1"), surf, params, hrg_eos=2, chosen="pikp", surface_format=1)
    host.run_particlization(d1, len(ref))
    assert not any(os.path.exists(os.path.join(d1, "results", "S%s.dat" % c)) for c in "txyn")
    with pytest.raises(host.HostError):
        host.polarization(d1, 5 * len(ref))
    # the polarization alone does not depend on the directory's operation
    d2 = rundir.write_run_dir(str(tmp_path / "op2"), surf, dict(params, operation=2), hrg_eos=2, chosen="pikp",
                              surface_format=5)
    np.testing.assert_array_equal(host.polarization(d2, 5 * len(ref)).reshape(S.shape), S)


def test_polarization_error_keeps_the_operations_files(tmp_path):
    """The polarization runs after the operation's files are written: a 2+1D mode-5 directory whose eta table has one
    node (the reference reads eta_tab(2) - eta_tab(1), Polarization.cpp:58) still gets its spectra files."""
    surf = synth.surface(20, seed=31, dimension=2)
    params = dict(dimension=2, df_mode=1, include_baryon=0, include_bulk_deltaf=1, include_shear_deltaf=1,
                  include_baryondiff_deltaf=0, regulate_deltaf=0, outflow=0, deta_min=1e-5, mass_pion0=0.138)
    d = rundir.write_run_dir(str(tmp_path), surf, params, hrg_eos=2, chosen="pikp", surface_format=5,
                             eta=np.array([[0.0, 1.0]]))
    with pytest.raises(host.HostError) as ei:
        host.run_particlization(d, 3 * 24 * 24)
    assert "eta table" in str(ei.value)
    assert os.path.exists(os.path.join(d, "results/continuous/dN_pTdpTdphidy_211.dat"))
    assert not os.path.exists(os.path.join(d, "results/St.dat"))
