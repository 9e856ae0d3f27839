"""GPU tier: lane classes (is3d_lanes_integrated, include/is3d_amd.h; engine.hip baryon_blind / finalize_tables).

The integrand classes keep the documented key (mass, sign, baryon [, PTM: g == 0]) and their count is what
is3d_species_integrated reports (SMASH 193, UrQMD 124).  The kernels integrate the lane classes: the same key without
the baryon number when the run is baryon-blind -- include_baryon = 0 and the delta-f column that multiplies the baryon
number (Grad c1, RTA-CE / PTM G) identically zero on the table row such a run uses -- so a baryon and its antibaryon
of equal (mass, sign) share one lane (SMASH 135, UrQMD 75) and the reduction writes each with its own degeneracy.

Bars: 1e-8 maximum and 1e-11 at the 99th percentile against the oracle (test_gpu_parity.py), < 1e-9 against classes
off (test_gpu_classes.py), operation 0 at test_gpu_dndx.py's 1e-9, the polarization at test_gpu_polzn.py's 1e-9 of
sum |term|.  Shapes: one 12-cell tile and a remainder with skipped cells; 40 cells as four table chunks; 2+1D with 24
eta nodes."""
import functools

import numpy as np
import pytest

import polzn_ref
from helpers import parity, rel_quantile
from is3d2_amd import Engine, build_engine, make_spec, synth
from is3d2_amd.engine import surface_averages
from oracle import oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-8
P99 = 1e-11
OFF = 1e-9
SKIPPED = (1, 4, 12, 25, 39)      # cells given u.dsigma <= 0 (those below the surface's size)


def make_surface(n, seed=151, dimension=3, baryon=False):
    s = synth.surface(n, seed=seed, dimension=dimension, baryon=baryon, full3d=dimension == 3)
    for c in SKIPPED:
        if c < n:
            s["dat"][c] = -10.0 * abs(s["dat"][c])
    return synth.as_read(s)


def smash_spec(mode, **flags):
    # PTMA: every cell solved on its own (famod_chains = 0), which the oracle does with one thread per cell
    return make_spec(hrg_eos=2, chosen="smash", df_mode=mode, dimension=3, pT="pT24", phi="phi32", y="y21",
                     famod_chains=0, **flags)


def oracle_threads(spec, s):
    """The oracle's thread count is the reference's: for PTMA it sets the warm-start chains, so independent cells
    (famod_chains = 0) are one thread per cell; elsewhere it only spreads the work."""
    return len(s["tau"]) if spec["params"]["df_mode"] == 5 else 8


def run(spec, s, classes=True, tuning=None, devices=None, T_avg=None):
    e = build_engine(spec, s, T_avg=T_avg, species_classes=classes, devices=devices)
    for k, v in (tuning or {}).items():
        e.set_tuning(k, v)
    out = e.calculate_spectra()
    info = dict(classes=e.species_integrated(), lanes=e.lanes_integrated(), stats=e.stats(),
                chunks=e.get_tuning("phitab_chunks"))
    e.close()
    return out, info


def check_oracle(got, ref):
    rel, zr, zg = parity(got, ref)
    q = rel_quantile(got, ref)
    print("vs oracle: max rel %.3e  p99 %.3e  zeros %d / %d" % (rel, q, zr, zg))
    assert rel < TOL, (rel, zr, zg)
    assert q < P99, q
    assert zr == zg


def check_off(on, off):
    rel = parity(on, off, floor=1e-290)[0]
    print("vs classes off: max rel %.3e" % rel)
    assert rel < OFF, rel
    assert np.array_equal(np.isfinite(on), np.isfinite(off))


def baryon_pairs(sp):
    """Pairs of species with equal (mass, sign, g) and different baryon number."""
    first, pairs = {}, []
    for i, k in enumerate(zip(sp["mass"], sp["sign"], sp["degen"])):
        j = first.setdefault(k, i)
        if j != i and sp["baryon"][j] != sp["baryon"][i]:
            pairs.append((j, i))
    return pairs


@functools.lru_cache(maxsize=None)
def blind_case(mode):
    s = make_surface(13)
    spec = smash_spec(mode)
    return s, spec, O.spectra(spec, s, threads=oracle_threads(spec, s))


@pytest.mark.parametrize("mode", [1, 2, 3, 4, 5])
def test_blind_modes_merge_baryon_pairs(mode):
    s, spec, ref = blind_case(mode)
    on, io = run(spec, s)
    off, fo = run(spec, s, classes=False)
    assert io["classes"] == 193 and io["lanes"] == 135 and io["stats"]["lanes_integrated"] == 135
    assert fo["classes"] == 444 and fo["lanes"] == 444
    check_oracle(on, ref)
    check_off(on, off)
    sp = spec["species"]
    pairs = baryon_pairs(sp)
    assert len(pairs) >= 100
    rows = on.reshape(len(sp["mass"]), -1)
    for a, b in pairs:
        assert np.array_equal(rows[a], rows[b]), (a, b)
    assert io["stats"]["breakdown"] == fo["stats"]["breakdown"]
    assert io["stats"]["cells"] == 13


@pytest.mark.parametrize("mode", [1, 2])
def test_table_chunks_bit_equal(mode):
    """40 cells are four cell splits (12, 12, 12, 4): four table chunks, the last a remainder, give one chunk's bits."""
    s = make_surface(40)
    spec = smash_spec(mode)
    one, i1 = run(spec, s)
    many, ik = run(spec, s, tuning={"phitab_one_bytes": 0, "phitab_chunk_bytes": 1})
    assert i1["lanes"] == ik["lanes"] == 135
    assert i1["chunks"] == 1 and ik["chunks"] >= 3, (i1["chunks"], ik["chunks"])
    assert np.array_equal(many, one)


def test_baryon_terms_keep_the_class_key():
    """include_baryon = 1 with diffusion: no merge, and a proton differs from its antiproton."""
    s = make_surface(13, baryon=True)
    spec = smash_spec(1, include_baryon=1, include_baryondiff_deltaf=1)
    got, info = run(spec, s)
    assert info["classes"] == info["lanes"] == 193
    sp = spec["species"]
    a, b = baryon_pairs(sp)[0]
    rows = got.reshape(len(sp["mass"]), -1)
    assert not np.array_equal(rows[a], rows[b])
    check_oracle(got, O.spectra(spec, s, threads=8))


@pytest.mark.parametrize("mode,col", [(1, 1), (2, 6), (3, 6)])
def test_nonzero_baryon_column_keeps_the_class_key(mode, col):
    """include_baryon = 0, but the column that multiplies the baryon number (Grad c1, RTA-CE / PTM G) has one nonzero
    entry on the row the run uses: the lanes keep the full key.  The spectra are the oracle's all the same (neither
    reads the column without baryon terms)."""
    s, spec, ref = blind_case(mode)
    T, muB, tab = spec["df"]
    tab = np.array(tab, dtype=np.float64, copy=True)
    tab[col, 0, len(T) // 2] = 1e-3
    spec2 = dict(spec, df=(T, muB, tab))
    got, info = run(spec2, s)
    assert info["classes"] == info["lanes"] == 193
    check_oracle(got, ref)
    # ... and a nonzero entry on another row does not matter
    tab2 = np.array(spec["df"][2], dtype=np.float64, copy=True)
    tab2[col, 1, len(T) // 2] = 1e-3
    e = build_engine(dict(spec, df=(T, muB, tab2)), s)
    assert e.lanes_integrated() == 135
    e.close()


@pytest.mark.parametrize("mode", [1, 5])
def test_urqmd_boost_invariant(mode):
    """UrQMD (305 species, 124 classes, 75 lanes) in 2+1D with 24 eta nodes."""
    s = synth.as_read(synth.surface(30, seed=5, dimension=2))
    spec = make_spec(hrg_eos=1, chosen="urqmd", df_mode=mode, dimension=2, famod_chains=0)
    assert len(spec["eta"]) == 24
    on, io = run(spec, s)
    off, _ = run(spec, s, classes=False)
    assert io["classes"] == 124 and io["lanes"] == 75
    check_oracle(on, O.spectra(spec, s, threads=oracle_threads(spec, s)))
    check_off(on, off)


def test_ptm_zero_degeneracy_keeps_its_lane():
    """PTM: a baryon given g = 0 is skipped (its renormalisation is 0 / 0) while its antibaryon keeps g > 0: the
    two stay in separate lanes."""
    s = make_surface(13)
    spec = smash_spec(3)
    sp = dict(spec["species"])
    g = np.array(sp["degen"], dtype=float)
    z, anti = next((a, b) for a, b in baryon_pairs(sp) if sp["mass"][a] > 1.0)
    g[z] = 0.0
    sp["degen"] = g
    spec = dict(spec, species=sp)
    got, info = run(spec, s)
    assert info["lanes"] == len(set(zip(sp["mass"], sp["sign"], [v == 0 for v in g]))) == 136
    assert info["classes"] == len(set(zip(sp["mass"], sp["sign"], sp["baryon"], [v == 0 for v in g])))
    rows = got.reshape(len(g), -1)
    assert not np.any(rows[z])
    assert np.any(rows[anti])
    ref = O.spectra(spec, s, threads=8)
    check_oracle(got, ref)


@pytest.mark.parametrize("mode", [1, 3])
def test_dndx_and_cell_yields(mode):
    """operation = 0 on the lane classes: against the oracle at that operation's bar, bit-equal to classes off."""
    s = synth.as_read(synth.surface(200, seed=3, dimension=2))
    spec = make_spec(hrg_eos=2, chosen="smash", df_mode=mode, dimension=2)
    res = []
    for classes in (True, False):
        e = build_engine(spec, s, species_classes=classes)
        t, r, ph = e.calculate_dN_dX()
        res.append((t, r, ph, e.cell_yields()))
        assert e.lanes_integrated() == (135 if classes else 444)
        e.close()
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    # the oracle on a third of the list (it evaluates each species on its own, and 444 of them take 10 s): both
    # members of every fourth merged pair and every tenth species
    sp = spec["species"]
    idx = sorted({i for p in baryon_pairs(sp)[::4] for i in p} | set(range(0, len(sp["mass"]), 10)))
    sub = dict(spec, species={k: np.ascontiguousarray(np.asarray(v)[idx]) for k, v in sp.items()})
    ref = O.dndx(sub, s, threads=8, carry=0, omp_threads=8, return_cells=True)
    for g, f in zip(res[0], ref):
        g = g.reshape(len(sp["mass"]), -1)[idx]
        assert g.size == f.size
        rel, zr, zg = parity(g.ravel(), f.ravel())
        assert rel < 1e-9, rel
        assert zr == zg


def test_polarization_unchanged():
    """The polarization keys its own classes on (mass, sign) and reads none of the lane tables: a proton and an
    antiproton share its class as before, and classes on equals classes off to that suite's bar."""
    n = 13
    surf = synth.surface(n, seed=21, dimension=3, full3d=True)
    w = synth.vorticity(n, 5)
    spec = make_spec(chosen=[211, 2212, -2212], pT="pT24", phi="phi24", y="y21", eta="eta24", dimension=3)
    _, A = polzn_ref.polarization(make_spec(chosen=[211, 2212], pT="pT24", phi="phi24", y="y21", eta="eta24",
                                            dimension=3), surf, w, 0.150, lo=0, hi=n)
    A = A[:, [0, 1, 1]]
    out = []
    for classes in (True, False):
        e = Engine()
        e.set_params(**spec["params"])
        sp = spec["species"]
        e.set_species(sp["mass"], sp["sign"], sp["degen"], sp["baryon"])
        e.set_species_classes(classes)
        e.set_momentum_grid(spec["pT"], spec["phi"], spec["y"], spec["eta"], spec["eta_w"])
        e.set_surface(surf)
        e.set_vorticity(w)
        out.append(e.calculate_polarization(0.150))
        e.close()
    on, each = out
    m = A > 1e-290
    assert np.max(np.abs(each.astype(np.longdouble) - on)[m] / A[m]) < 1e-9
    np.testing.assert_array_equal(on[:, 1], on[:, 2])


def test_device_list_forwards_the_lane_count():
    """A device list that repeats GPU 0, on the surface tests/test_gpu_classes.py::test_classes_device_group uses (60
    cells, seed 9, RTA-CE).  The first version of this case took that seed with full 3+1D flow and five cells turned
    inward: that surface has one output whose cells cancel to -8.1e-13 in a row that peaks at 8.2e-5, where the sum's
    rounding alone is 2.5e-8 of the value -- the same 2.525e-8 from the parent build, with classes off and on one
    device (absolute error 2e-20).  It measured the oracle's summation order, not the lanes, so the case runs on the
    suite's own device-list surface; the bar is unchanged."""
    s = synth.as_read(synth.surface(60, seed=9, dimension=3))
    spec = smash_spec(2)
    e = build_engine(spec, s, devices=[0, 0])
    assert e.species_integrated() == 193 and e.lanes_integrated() == 135
    got = e.calculate_spectra()
    assert e.stats()["lanes_integrated"] == 135
    e.close()
    check_oracle(got, O.spectra(spec, s, threads=8))


def test_switching_baryon_terms_and_classes_on_one_engine():
    """include_baryon 0 -> 1 -> 0 and classes on -> off -> on: the lane count follows each switch and the spectra are
    a fresh engine's, bit for bit."""
    s = make_surface(13, baryon=True)
    T_avg = surface_averages(s, 0)[0]
    blind = smash_spec(1)
    full = smash_spec(1, include_baryon=1, include_baryondiff_deltaf=1)
    fresh = {k: run(sp, s, T_avg=T_avg)[0] for k, sp in (("blind", blind), ("full", full))}
    fresh_off = run(blind, s, classes=False, T_avg=T_avg)[0]
    e = build_engine(blind, s, T_avg=T_avg)
    for spec, key, lanes in ((blind, "blind", 135), (full, "full", 193), (blind, "blind", 135)):
        e.set_params(**spec["params"])
        assert e.lanes_integrated() == lanes and e.species_integrated() == 193
        assert np.array_equal(e.calculate_spectra(), fresh[key])
    e.set_species_classes(False)
    assert e.lanes_integrated() == 444 and e.species_integrated() == 444
    assert np.array_equal(e.calculate_spectra(), fresh_off)
    e.set_species_classes(True)
    assert e.lanes_integrated() == 135 and e.species_integrated() == 193
    assert np.array_equal(e.calculate_spectra(), fresh["blind"])
    e.close()
