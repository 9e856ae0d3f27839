"""GPU tier: the y-term rows of the scalar-table (F_TS) k_spectra launches.  k_ytab builds them once per pass, rows
[cell][q][11] behind the chunk's k_phitab rows; k_spectra copies the rows of its next tile into LDS with that tile's
records (a cell's rows r0 .. r0 + nqw - 1 are one segment) and builds its T1 rows from them with a fixed phi slot per
thread.  The shapes here are the smallest where that path can go wrong, each against the oracle at the bars
test_gpu_parity.py uses for these launches (1e-8 max, 1e-11 at P99):
 - tiles of 12 cells: 5 cells (less than a tile), 13 (a tile and one cell), 40 (three tiles and four cells: the copy's
   prologue, its steady state and a partial last tile), with a few skipped cells (u.dsigma <= 0);
 - row ranges: SMASH as 193 classes (a workgroup's 256 tasks span 2-3 rows) and as 444 species (1-2 rows), rapidity
   grids of 1, 2, 3 and 21 points, a 2+1D run (q = y x eta node, 24 rows), phi blocks of 24 and of 32 points;
 - Grad, RTA-CE and Grad with baryon terms (F_BY);
 - several table chunks with a remainder, a cell window, a surface set anew on a used engine.
Every case asserts the launch was an F_TS one: "phitab_chunks" is 0 for any other plan (the device-side fallback to
the F_TB kernels needs |mu_B| / T > ~300, which these surfaces do not have).  The pT grid is cut to five points: the
rows do not depend on pT, and the oracle's time does."""
import numpy as np
import pytest

from helpers import parity, rel_quantile
from is3d2_amd import build_engine, make_spec, synth
from is3d2_amd.engine import surface_averages
from oracle import oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-8
P99 = 1e-11
SKIPPED = (1, 4, 12, 25, 39)      # cells given u.dsigma <= 0 (those below the surface's size)


def make_surface(n, seed=131, dimension=3, baryon=False):
    s = synth.surface(n, seed=seed, dimension=dimension, baryon=baryon, full3d=dimension == 3)
    for c in SKIPPED:
        if c < n:
            s["dat"][c] = -10.0 * abs(s["dat"][c])
    return synth.as_read(s)


def spec_of(mode, phi="phi32", dimension=3, ny=21, **flags):
    spec = make_spec(hrg_eos=2, chosen="smash", df_mode=mode, dimension=dimension, pT="pT24", phi=phi, y="y21", **flags)
    spec["pT"] = np.ascontiguousarray(spec["pT"][2::5])
    spec["pT_w"] = np.ascontiguousarray(spec["pT_w"][2::5])
    if ny != 21:
        spec["y"] = np.linspace(-1.5, 2.0, ny) if ny > 1 else np.array([0.5])
    return spec


def run(spec, s, tuning=None, window=None, T_avg=None, classes=True):
    e = build_engine(spec, s, T_avg=T_avg, species_classes=classes)
    for k, v in (tuning or {}).items():
        e.set_tuning(k, v)
    if window:
        e.set_cell_window(*window)
    out = e.calculate_spectra()
    chunks = e.get_tuning("phitab_chunks")
    e.close()
    assert chunks >= 1, chunks       # the scalar-table (F_TS) launch ran
    return out, chunks


def check(got, spec, s, T_avg=None):
    ref = O.spectra(spec, s, threads=8) if T_avg is None else O.spectra(spec, s, threads=8, T_avg=T_avg)
    rel, zr, zg = parity(got, ref)
    print("max rel %.3e  p99 %.3e  zeros %d / %d" % (rel, rel_quantile(got, ref), zr, zg))
    assert rel < TOL, (rel, zr, zg)
    assert rel_quantile(got, ref) < P99
    assert zr == zg


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("n", [5, 13, 40])
def test_tile_shapes(mode, n):
    s = make_surface(n)
    spec = spec_of(mode)
    got, _ = run(spec, s)
    check(got, spec, s)


@pytest.mark.parametrize("ny", [1, 2, 3, 21])
def test_row_ranges_species(ny):
    """444 lane species: a workgroup's tasks span one or two rows; phi blocks of 24 points."""
    s = make_surface(13)
    spec = spec_of(1, phi="phi24", ny=ny)
    got, _ = run(spec, s, classes=False)
    check(got, spec, s)


@pytest.mark.parametrize("mode,ny", [(2, 1), (2, 2), (1, 3), (2, 21)])
def test_row_ranges_classes_phi24(mode, ny):
    """193 classes (2-3 rows per workgroup) with phi blocks of 24 points: 240 of the 256 threads build the T1 rows."""
    s = make_surface(13)
    spec = spec_of(mode, phi="phi24", ny=ny)
    got, _ = run(spec, s)
    check(got, spec, s)


@pytest.mark.parametrize("mode", [1, 2])
def test_boost_invariant_eta_rows(mode):
    """2+1D: q = y x eta node, 24 rows whose eta and weight come from the grid."""
    s = make_surface(13, dimension=2)
    spec = spec_of(mode, dimension=2)
    got, _ = run(spec, s)
    check(got, spec, s)


@pytest.mark.parametrize("phi", ["phi24", "phi32"])
def test_baryon_rows(phi):
    """Grad with include_baryon (F_BY): the lanes read Y_S1 and the record's baryon terms as well."""
    s = make_surface(40, baryon=True)
    spec = spec_of(1, phi=phi, include_baryon=1, include_baryondiff_deltaf=1)
    got, _ = run(spec, s)
    check(got, spec, s)


@pytest.mark.parametrize("mode", [1, 2])
def test_chunks_and_window(mode):
    """40 cells are four cell splits (12, 12, 12, 4); chunks of one split each are four table chunks, the last a
    remainder: the same bits as one chunk.  A window with a non-zero start reads rows [cell - window start]."""
    s = make_surface(40)
    spec = spec_of(mode)
    one, n1 = run(spec, s)
    many, nk = run(spec, s, {"phitab_one_bytes": 0, "phitab_chunk_bytes": 1})
    assert n1 == 1 and nk >= 3, (n1, nk)
    assert np.array_equal(many, one)
    check(many, spec, s)
    lo, hi = 7, 33
    T_avg = surface_averages(s, 0)[0]
    part = {k: np.ascontiguousarray(v[lo:hi]) for k, v in s.items()}
    win, _ = run(spec, s, window=(lo, hi), T_avg=T_avg)
    win_many, nw = run(spec, s, {"phitab_one_bytes": 0, "phitab_chunk_bytes": 1}, window=(lo, hi), T_avg=T_avg)
    assert nw >= 3, nw
    assert np.array_equal(win_many, win)
    check(win_many, spec, part, T_avg=T_avg)


def test_surface_set_anew():
    """One engine on 40 cells, then on 13 other cells: both equal fresh engines bit for bit (no row of the first
    surface's table is read for the second)."""
    a, b = make_surface(40, seed=131), make_surface(13, seed=137)
    spec = spec_of(1)
    T_avg = surface_averages(a, 0)[0]
    e = build_engine(spec, a, T_avg=T_avg)
    first = e.calculate_spectra()
    e.set_surface(b)
    second = e.calculate_spectra()
    assert e.get_tuning("phitab_chunks") >= 1
    e.close()
    assert np.array_equal(first, run(spec, a, T_avg=T_avg)[0])
    fresh_b, _ = run(spec, b, T_avg=T_avg)
    assert np.array_equal(second, fresh_b)
    check(second, spec, b, T_avg=T_avg)
