"""CPU tier for operation = 0 with df_mode 5 (is3d_calculate_dN_dX_famod).  The reference has no routine, so the
per-cell yields are defined as the per-cell decomposition of the PTMA spectra; this file pins the
reference the GPU tier leans on -- the emulator's PTMA cell yields (tests/native/cf_emulator.cpp, op = 0) -- to the
oracle's PTMA spectra: summed over the cells they are the spectra folded with the pT / phi weights, and the yields of
one cell are the folded spectra of that one-cell surface (cold Newton starts)."""
import numpy as np
import pytest

from helpers import emu_spectra, parity
from is3d2_amd import make_spec, synth
from oracle import oracle as O

TOL = 1e-12     # tests/test_dndx_cpu.py's bar for the emulator against the oracle


def surface(n, dim, seed=31):
    s = synth.as_read(synth.surface(n, seed=seed, dimension=dim, full3d=(dim == 3)))
    s["bulkPi"] = s["bulkPi"].copy()
    s["bulkPi"][::2] *= 10.0          # breakdown-heavy, as tests/test_gpu_configs.py::test_modified_fallback_launch
    return s


def folded(spec, spectra):
    """sum_ipT,iphi,iy w_pT w_phi dN_pTdpTdphidy[s][ipT][iphi][iy] per species (2+1D: the one y = 0 entry)."""
    a = np.asarray(spectra).reshape(len(spec["species"]["mass"]), len(spec["pT"]), len(spec["phi"]), -1)
    return np.einsum("sijk,i,j->s", a, spec["pT_w"], spec["phi_w"])


def one_cell(s, c):
    return {k: (v[c:c + 1].copy() if v is not None else None) for k, v in s.items()}


@pytest.fixture(scope="module", params=[2, 3])
def case(request):
    dim = request.param
    s = surface(40, dim)
    spec = make_spec(hrg_eos=2, chosen="pikp", df_mode=5, dimension=dim, famod_chains=1)
    return dim, s, spec


def test_cell_yields_sum_to_folded_spectra(case):
    dim, s, spec = case
    ref, rst = O.spectra(spec, s, threads=1, return_stats=True)
    cy, st = emu_spectra(spec, s, chains=1, op=0)
    cy = cy.reshape(len(spec["species"]["mass"]), -1)
    rel = parity(cy.sum(axis=1), folded(spec, ref))[0]
    print("dim %d: sum over cells against the folded spectra %.2e; breakdown %d, iterations %d" % (dim, rel, st[0], st[3]))
    assert rel < TOL, rel
    assert st[0] == rst[0] > 0 and st[3] == rst[3]      # breakdown cells, Newton iterations of the one chain


def test_cold_cell_yields_are_one_cell_spectra(case):
    dim, s, spec = case
    n = len(s["tau"])
    cy, st = emu_spectra(spec, s, chains=0, op=0)
    cy = cy.reshape(len(spec["species"]["mass"]), n)
    ref = np.stack([folded(spec, O.spectra(spec, one_cell(s, c), threads=1)) for c in range(n)], axis=1)
    rel, zr, zg = parity(cy.ravel(), ref.ravel())
    print("dim %d: cold cell yields against one-cell spectra %.2e" % (dim, rel))
    assert rel < TOL, rel
    assert np.array_equal(cy == 0.0, ref == 0.0)
    # cold starts are the oracle's n chains; they differ from the one chain in the iteration count
    _, rst = O.spectra(spec, s, threads=n, return_stats=True)
    _, st1 = emu_spectra(spec, s, chains=1, op=0)
    assert st[3] == rst[3] and st[3] != st1[3]
