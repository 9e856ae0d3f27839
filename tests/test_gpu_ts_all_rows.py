"""GPU tier: F_TS launches whose workgroups cover every rapidity row.  k_spectra keeps its y-terms per q instead of
per row once a workgroup's rows cover every q (several phi blocks); the F_TS launches have one phi block, where the
two forms coincide, and are compiled with the per-row form alone (kernels.h allq).  With SMASH's 193 classes a
workgroup's 256 tasks span two rows, so a rapidity grid of one point (one row, one workgroup) and of two points (the
first workgroup holds both rows, the second only row 1) are the shapes where the per-q form used to run; three points
are the smallest grid where no workgroup covers every row (rows 0-1, 1-2, 2), the neighbouring case that always took
the per-row form.  All must meet the oracle within the suite's bars."""
import numpy as np
import pytest

from helpers import parity, rel_quantile
from is3d2_amd import build_engine, make_spec, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-8
P99 = 1e-11


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("ny", [1, 2, 3])
def test_few_rapidity_rows(mode, ny):
    s = synth.as_read(synth.surface(40, seed=97, dimension=3, full3d=True))
    spec = make_spec(hrg_eos=2, chosen="smash", df_mode=mode, dimension=3, pT="pT24", phi="phi32", y="y21")
    spec["y"] = np.linspace(-1.5, 2.0, ny) if ny > 1 else np.array([0.5])
    e = build_engine(spec, s)
    got = e.calculate_spectra()
    chunks = e.get_tuning("phitab_chunks")
    e.close()
    assert chunks >= 1, chunks       # the scalar-table (F_TS) launch ran
    ref = O.spectra(spec, s, threads=8)
    rel, zr, zg = parity(got, ref)
    assert rel < TOL, (rel, zr, zg)
    assert rel_quantile(got, ref) < P99
    assert zr == zg
