"""GPU tier of operation = 0 for df_mode 5 (is3d_calculate_dN_dX_famod, Engine.calculate_dN_dX_famod).  The reference
has no routine; DESIGN 7.1 defines the per-cell yields as the per-cell decomposition of the PTMA spectra, binned as the
other modes'.  References: the emulator's PTMA cell yields (tests/native/cf_emulator.cpp, pinned to the oracle's PTMA
spectra by tests/test_dndx_famod_cpu.py), the oracle's spectra folded with the pT / phi weights, the same engine's
calculate_spectra (pinned to the oracle by tests/test_gpu_configs.py) and a numpy restatement of the binning."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from helpers import emu_spectra, emulator, parity
from is3d2_amd import Engine, IS3DError, _lib, build_engine, host, make_spec, rundir, synth
from is3d2_amd.engine import surface_averages
from oracle import oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-9        # cell yields: tests/test_gpu_dndx.py's TOL (FP64 sums in another order than the reference)
TOL_BIN = 1e-12   # binning against numpy: tests/test_dndx_cpu.py

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REC_SRC = os.path.join(HERE, "native", "famod_records.cpp")
REC_LIB = os.path.join(HERE, "native", "libfamod_records.so")


def famod_records(spec, surf, chains):
    """{R_KIND, det B, R_NARROW} of the cells after the PTMA prepass on the host (tests/native/famod_records.cpp)."""
    emulator()
    srcs = [REC_SRC, os.path.join(HERE, "native", "cf_emulator.cpp")] + [os.path.join(ROOT, "is3d2_amd", "csrc", h)
                                                                         for h in ("cf_math.h", "aniso_math.h")]
    if not os.path.exists(REC_LIB) or any(os.path.getmtime(s) > os.path.getmtime(REC_LIB) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", REC_LIB, REC_SRC])
    lib = C.CDLL(REC_LIB)
    inp = O._Inputs(spec, surf, None, 1)
    n = len(surf["tau"])
    out = np.zeros(3 * n)
    assert lib.emu_famod_records(C.byref(inp.params), C.byref(inp.setup), C.byref(inp.surf), int(chains), 0, O._p(out)) == 0
    return out.reshape(n, 3).T


def heavy(n, seed, dim, full3d=None):
    s = synth.as_read(synth.surface(n, seed=seed, dimension=dim, full3d=(dim == 3) if full3d is None else full3d))
    s["bulkPi"] = s["bulkPi"].copy()
    s["bulkPi"][::2] *= 10.0          # breakdown-heavy, as tests/test_gpu_configs.py::test_modified_fallback_launch
    return s


def folded(spec, spectra):
    a = np.asarray(spectra).reshape(len(spec["species"]["mass"]), len(spec["pT"]), len(spec["phi"]), -1)
    return np.einsum("sijk,i,j->s", a, spec["pT_w"], spec["phi_w"])


def one_cell(s, c):
    return {k: (v[c:c + 1].copy() if v is not None else None) for k, v in s.items()}


def narrow_lanes(spec, s, rec):
    """(cell, y) pairs of the narrow-window fallback: non-broken cells with det B < 0.01 and |y - eta| < det B."""
    kind, det, nar = rec
    return [(c, k) for c in np.nonzero((kind == 2.0) & (nar != 0.0) & (det < 0.01))[0]
            for k in np.nonzero(np.abs(spec["y"] - s["eta"][c]) < det[c])[0]]


@functools.lru_cache(maxsize=None)
def case1(dim):
    """Case 1's surface (200 cells, seed 31, every other bulk pressure x 10, pi K p) with its references, computed
    once: emulator yields and counters for one chain and cold, the oracle's spectra folded, its counters.  3+1D: the
    non-broken cells with det B < 0.01 are moved to within det B of a y node, so the narrow (cell, y) fallback runs."""
    s = heavy(200, 31, dim)
    spec = make_spec(hrg_eos=2, chosen="pikp", df_mode=5, dimension=dim, famod_chains=1)
    np_ = len(spec["species"]["mass"])
    if dim == 3:
        kind, det, nar = famod_records(spec, s, 1)
        s["eta"] = s["eta"].copy()
        for c in np.nonzero((kind == 2.0) & (nar != 0.0))[0]:      # eta enters 3+1D only through y - eta
            s["eta"][c] = spec["y"][np.argmin(np.abs(spec["y"] - s["eta"][c]))] + 0.25 * det[c]
    ref = {}
    for chains in (1, 0):
        cy, st = emu_spectra(spec, s, chains=chains, op=0)
        ref[chains] = (cy.reshape(np_, -1), st)
    spectra, rst = O.spectra(spec, s, threads=1, return_stats=True)
    _, rst_cold = O.spectra(spec, s, threads=len(s["tau"]), return_stats=True)     # one chain per cell: cold starts
    for v in s.values():
        if v is not None:
            v.setflags(write=False)
    return dict(s=s, spec=spec, emu=ref, folded=folded(spec, spectra), rst=rst, rst_cold=rst_cold)


def cold_spec(spec):
    out = dict(spec)
    out["params"] = dict(spec["params"], famod_chains=0)
    return out


def run(spec, s, devices=None):
    e = build_engine(spec, s, devices=devices)
    out = e.calculate_dN_dX_famod()
    cy, st = e.cell_yields(), e.stats()
    e.close()
    return out, cy, st


def check_cells(cy, ref):
    rel, zr, zg = parity(cy.ravel(), ref.ravel())
    print("cell yields against the reference: %.3e" % rel)
    assert rel < TOL, rel
    assert np.array_equal(cy == 0.0, ref == 0.0)


@functools.lru_cache(maxsize=None)
def one_device(dim, chains):
    c = case1(dim)
    return run(c["spec"] if chains else cold_spec(c["spec"]), c["s"])


# --- 1. parity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_parity(dim):
    c = case1(dim)
    if dim == 3:      # a condition on the input: the narrow (cell, y) fallback has lanes
        assert narrow_lanes(c["spec"], c["s"], famod_records(c["spec"], c["s"], 1))
    _, cy, st = one_device(dim, 1)
    emu, est = c["emu"][1]
    check_cells(cy, emu)
    rel = parity(cy.sum(axis=1), c["folded"])[0]
    print("sum over cells against the oracle's folded spectra: %.3e" % rel)
    assert rel < TOL, rel
    assert st["breakdown"] == c["rst"][0] > 0
    assert st["iterations"] == c["rst"][3]


# --- 2. cold cells ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_cold_cells(dim):
    c = case1(dim)
    _, cy, st = one_device(dim, 0)
    emu, est = c["emu"][0]
    check_cells(cy, emu)
    assert st["iterations"] == c["rst_cold"][3] == est[3]
    assert st["iterations"] != c["rst"][3]           # the chain that ran shows in the count, not in the yields
    assert st["breakdown"] == c["rst_cold"][0]
    ref = np.stack([folded(c["spec"], O.spectra(c["spec"], one_cell(c["s"], k), threads=1)) for k in range(12)], axis=1)
    rel, zr, zg = parity(cy[:, :12].ravel(), ref.ravel())
    print("first 12 cells against the oracle's one-cell spectra: %.3e" % rel)
    assert rel < TOL, rel
    assert np.array_equal(cy[:, :12] == 0.0, ref == 0.0)


# --- 3. closure on the device at SMASH width ---------------------------------------------------------------------------
def test_closure_smash_width():
    # 444 species: 7 lane groups; 70 cells: ragged tails of the 8-cell (F_FB) and the 4-cell (modified) record tiles
    s = heavy(70, 34, 3, full3d=True)
    spec = make_spec(hrg_eos=2, chosen="smash", df_mode=5, dimension=3, pT="pT48", phi="phi32", y="y21", famod_chains=1)
    assert len(spec["species"]["mass"]) > 6 * 64 and len(spec["y"]) == 21
    e = build_engine(spec, s)
    e.calculate_dN_dX_famod()
    cy = e.cell_yields()
    spectra = e.calculate_spectra()
    e.close()
    rel = parity(cy.sum(axis=1), folded(spec, spectra))[0]
    print("SMASH width: sum over cells against the engine's folded spectra: %.3e" % rel)
    assert rel < TOL, rel


def test_smash_width_cells_against_emulator():
    s = heavy(8, 34, 3, full3d=True)
    spec = make_spec(hrg_eos=2, chosen="smash", df_mode=5, dimension=3, pT="pT48", phi="phi32", y="y21", famod_chains=1)
    emu, est = emu_spectra(spec, s, chains=1, op=0)
    _, cy, st = run(spec, s)
    check_cells(cy, emu.reshape(cy.shape))
    assert st["breakdown"] == est[0] and st["iterations"] == est[3]


# --- 4. binning ------------------------------------------------------------------------------------------------------
def _bin_sums(spec, s, cy):
    """Independent numpy binning of dN_dy_cell (reference bin formulas, no thread slices): tests/test_dndx_cpu.py's."""
    b = spec["bins"]
    tw = (b["tau_max"] - b["tau_min"]) / b["tau_bins"]
    rw = (b["r_max"] - b["r_min"]) / b["r_bins"]
    pw = 2 * np.pi / b["phip_bins"]
    r = np.sqrt(s["x"] ** 2 + s["y"] ** 2)
    phi = np.arctan2(s["y"], s["x"])
    phi = np.where(phi < 0, phi + 2 * np.pi, phi)
    out = []
    for key, nb, norm in ((np.floor((s["tau"] - b["tau_min"]) / tw), b["tau_bins"],
                           (b["tau_min"] + tw * (np.arange(b["tau_bins"]) + 0.5)) * tw),
                          (np.floor((r - b["r_min"]) / rw), b["r_bins"],
                           2 * np.pi * (b["r_min"] + rw * (np.arange(b["r_bins"]) + 0.5)) * rw),
                          (np.floor(phi / pw), b["phip_bins"], np.full(b["phip_bins"], pw))):
        key = key.astype(np.int64)
        m = (key >= 0) & (key < nb)
        h = np.zeros((cy.shape[0], nb))
        for i in range(cy.shape[0]):
            h[i] = np.bincount(key[m], weights=cy[i][m], minlength=nb)
        out.append(h / norm)
    return out


@pytest.mark.parametrize("dim", [2, 3])
def test_binning_matches_numpy(dim):
    c = case1(dim)
    s, spec = c["s"], c["spec"]
    b = spec["bins"]
    (t, r, ph), cy, _ = one_device(dim, 1)
    rr = np.sqrt(s["x"] ** 2 + s["y"] ** 2)
    assert (rr >= b["r_max"]).any()                                                  # cells the r histogram leaves out
    assert ((s["tau"] >= b["tau_min"]) & (s["tau"] < b["tau_max"])).all()            # none left out of the tau one
    for got, ref in zip((t, r, ph), _bin_sums(spec, s, cy)):
        np.testing.assert_allclose(got, ref, rtol=TOL_BIN, atol=0)
    tw = (b["tau_max"] - b["tau_min"]) / b["tau_bins"]
    norm = (b["tau_min"] + tw * (np.arange(b["tau_bins"]) + 0.5)) * tw
    np.testing.assert_allclose((t * norm).sum(axis=1), cy.sum(axis=1), rtol=TOL_BIN)


# --- 5. many tasks ---------------------------------------------------------------------------------------------------
def test_many_tasks_and_phi_blocks():
    # 70 y x 4 phi blocks (100-point phi grid, padded to 128) = 280 tasks per species over 4 x 21 slots
    s = heavy(20, 35, 3, full3d=False)
    spec = make_spec(hrg_eos=2, chosen="pikp", df_mode=5, dimension=3, famod_chains=1)
    spec["y"] = np.linspace(-5.0, 5.0, 70)
    spec["phi"] = 2 * np.pi * (np.arange(100) + 0.5) / 100
    spec["phi_w"] = np.full(100, 2 * np.pi / 100)
    emu, est = emu_spectra(spec, s, chains=1, op=0)
    _, cy, st = run(spec, s)
    check_cells(cy, emu.reshape(cy.shape))
    assert st["iterations"] == est[3]


# --- 6. device list --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chains", [1, 0])
def test_device_list(chains):
    c = case1(3)
    spec = c["spec"] if chains else cold_spec(c["spec"])
    out1, cy1, st1 = one_device(3, chains)
    outg, cyg, stg = run(spec, c["s"], devices=[0, 0])
    for a, b in zip(outg, out1):
        assert parity(a, b, floor=1e-300)[0] < TOL_BIN
        assert np.array_equal(a == 0.0, b == 0.0)
    assert np.array_equal(cyg, cy1)
    for k in ("cells", "breakdown", "pl_negative", "recon_fail", "iterations"):
        assert stg[k] == st1[k], k
    # one engine with a cell window (what a shard runs): the window's cells of the whole-surface result, the same bits
    e = build_engine(spec, c["s"])
    e.set_cell_window(50, 130)
    tw, rw, pw = e.calculate_dN_dX_famod()
    cyw, stw = e.cell_yields(), e.stats()
    e.close()
    assert cyw.shape == (cy1.shape[0], 80) and np.array_equal(cyw, cy1[:, 50:130])
    sw = {k: (v[50:130] if v is not None else None) for k, v in c["s"].items()}
    for got, ref in zip((tw, rw, pw), _bin_sums(spec, sw, cyw)):
        np.testing.assert_allclose(got, ref, rtol=TOL_BIN, atol=0)
    assert stw["cells"] == 80 and (not chains or stw["iterations"] == st1["iterations"])
    tspec = dict(spec, bins=dict(spec["bins"], threads=2))
    e = build_engine(tspec, c["s"], devices=[0, 0])
    with pytest.raises(IS3DError, match="threads > 0") as ei:
        e.calculate_dN_dX_famod()
    e.close()
    assert ei.value.code == _lib.IS3D_ERR_UNSUPPORTED


# --- 7. errors and edges ---------------------------------------------------------------------------------------------
def _engine_without(spec, surf, weights=True, bins=True):
    e = Engine(0)
    e.set_params(**spec["params"])
    sp, pdg = spec["species"], spec["pdg"]
    e.set_species(sp["mass"], sp["sign"], sp["degen"], sp["baryon"])
    e.set_pdg(pdg["mass"], pdg["sign"], pdg["gspin"], pdg["baryon"])
    e.set_momentum_grid(spec["pT"], spec["phi"], spec["y"], spec["eta"], spec["eta_w"])
    if weights:
        e.set_momentum_weights(spec["pT_w"], spec["phi_w"])
    if bins:
        e.set_spacetime_bins(**spec["bins"])
    e.set_gauss_laguerre(*spec["gla"])
    e.set_df_tables(*spec["df"], surface_averages(surf, 0)[0])
    e.set_surface(surf)
    return e


def test_errors_and_edges():
    s = heavy(40, 36, 2)
    spec = make_spec(hrg_eos=2, chosen="pikp", df_mode=5, dimension=2, famod_chains=1)
    e = build_engine(make_spec(hrg_eos=2, chosen="pikp", df_mode=1), s)
    with pytest.raises(IS3DError, match="calculate_dN_dX") as ei:
        e.calculate_dN_dX_famod()
    assert ei.value.code == _lib.IS3D_ERR_UNSUPPORTED
    e.close()
    for kw in (dict(weights=False), dict(bins=False)):
        e = _engine_without(spec, s, **kw)
        with pytest.raises(IS3DError) as ei:
            e.calculate_dN_dX_famod()
        assert ei.value.code == _lib.IS3D_ERR_STATE
        # ... and the library's own check (the Python method needs the bins for its output shapes)
        buf = np.zeros(8)
        pb = buf.ctypes.data_as(C.POINTER(C.c_double))
        assert e.lib.is3d_calculate_dN_dX_famod(e._e, pb, pb, pb) == _lib.IS3D_ERR_STATE
        e.close()
    e = build_engine(spec, s)
    with pytest.raises(IS3DError, match="no spacetime distribution routine for famod yet") as ei:
        e.calculate_dN_dX()
    assert ei.value.code == _lib.IS3D_ERR_UNSUPPORTED and "is3d_calculate_dN_dX_famod" in str(ei.value)
    sp0 = e.calculate_spectra()
    a = e.calculate_dN_dX_famod()
    cya, sta = e.cell_yields(), e.stats()
    b = e.calculate_dN_dX_famod()
    cyb, stb = e.cell_yields(), e.stats()
    sp1 = e.calculate_spectra()
    for x, y in zip(a + (cya,), b + (cyb,)):
        assert x.tobytes() == y.tobytes()
    assert cya.any() and sta["iterations"] == stb["iterations"] > 0 and sta["breakdown"] == stb["breakdown"]
    assert sp0.tobytes() == sp1.tobytes()
    e.set_surface({k: (v[:0] if v is not None else None) for k, v in s.items()})
    t, r, ph = e.calculate_dN_dX_famod()
    assert not t.any() and not r.any() and not ph.any()
    assert e.cell_yields().shape == (3, 0) and e.stats()["iterations"] == 0
    e.close()


# --- 8. run directory ------------------------------------------------------------------------------------------------
def test_run_directory(tmp_path):
    dim = 3
    s = synth.surface(60, seed=41, dimension=dim, full3d=True)
    s["bulkPi"] = np.asarray(s["bulkPi"]).copy()
    s["bulkPi"][::2] *= 10.0
    params = dict(operation=0, dimension=dim, df_mode=5, include_baryon=0, include_bulk_deltaf=1, include_shear_deltaf=1,
                  include_baryondiff_deltaf=0, regulate_deltaf=0, outflow=0, deta_min=1e-5, mass_pion0=0.138,
                  famod_chains=1, tau_min=0.0, tau_max=12.0, tau_bins=60, r_min=0.0, r_max=15.0, r_bins=30, phip_bins=50,
                  spacetime_threads=0)
    d = rundir.write_run_dir(str(tmp_path), s, params, hrg_eos=2, chosen="pikp", surface_format=1)
    exe = os.path.join(ROOT, "is3d2_amd", "bin", "iS3D_amd")
    p = subprocess.run([exe], cwd=d, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    spec = make_spec(hrg_eos=2, chosen="pikp", pT="pT24", phi="phi24", **{k: v for k, v in params.items() if k != "operation"})
    fields, avg = host.read_surface(d, 1, dim, 0)
    surf = {k: fields[i] for i, k in enumerate(synth.FIELDS)}
    e = build_engine(spec, surf, T_avg=avg[0])
    t, r, ph = e.calculate_dN_dX_famod()
    e.close()
    assert t.any() and r.any() and ph.any()
    for k, mc in enumerate(spec["species"]["mcid"]):
        for name, arr, mid in (("dN_taudtaudy", t, 0.1 + 0.2 * np.arange(60)), ("dN_2pirdrdy", r, 0.25 + 0.5 * np.arange(30)),
                               ("dN_dphidy", ph, (np.arange(50) + 0.5) * 2 * np.pi / 50)):
            rows = np.loadtxt(os.path.join(d, "results/continuous/%s_%d.dat" % (name, mc)))
            assert rows.shape == (len(mid), 2)
            # the writer prints setprecision(6) scientific: seven digits
            np.testing.assert_allclose(rows[:, 0], mid, rtol=1e-6)
            np.testing.assert_allclose(rows[:, 1], arr[k], rtol=1e-6, atol=1e-300)
