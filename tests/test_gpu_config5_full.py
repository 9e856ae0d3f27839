"""BASELINE config 5 at full size: 5 x 10^6 3+1D cells, UrQMD HRG, PTMA + baryon diffusion,
64-pt Gauss-Laguerre, the drop-in default of one warm-start Newton chain over every cell (famod_chains = 1,
MomentumSpectra.cpp:1132-1135, 1308-1364) -- the bench's config-5 line, where the oracle's serial chain would take
days.  test_gpu_configs.py::test_config5_miniature pins the same physics to the oracle on 8 cells; here the full
path is held to size-independent properties:

* the segmented chain solve (engine_kernels.h k_chain_pass: up to 24 passes, then the serial finisher) reaches the serial
  chain's fixed point whatever the pass count: with IS3D_CHAIN_PASSES=2 the finisher carries whatever ripple the
  later passes of the default schedule would have resolved, and the Newton iteration /
  breakdown / p_L < 0 counts are the default schedule's exactly (one pass would leave every one of the ~16k
  segments' ~10-cell ripple to the one-workgroup finisher: minutes at full size);
* the Newton solve does not see dsigma_mu and p.dsigma enters the integrand linearly, so that run, on the surface
  with dsigma_mu doubled, returns twice the default run's spectra bit for bit in the normal range -- which holds
  only if all 5 x 10^6 Newton solutions are identical between the two schedules;
* every entry is finite (the miniature's entries are) and the spectra are not empty.
"""
import os

import numpy as np
import pytest

from is3d2_amd import build_engine, make_spec, synth

pytestmark = pytest.mark.gpu


def test_config5_full_size_chain_schedule_and_linearity():
    n = 5_000_000
    s = synth.as_read(synth.surface(n, seed=7, dimension=3, baryon=True, full3d=True))
    spec = make_spec(hrg_eos=1, chosen="urqmd", df_mode=5, dimension=3, pT="pT48", phi="phi32", y="y21",
                     gla_points=64, include_baryon=1, include_baryondiff_deltaf=1, famod_chains=1)
    assert spec["params"]["famod_chains"] == 1
    e = build_engine(spec, s)
    full = e.calculate_spectra()
    st = e.stats()
    s2 = dict(s)
    for k in ("dat", "dax", "day", "dan"):
        s2[k] = 2.0 * s[k]
    del s
    e.set_surface(s2)
    old = os.environ.get("IS3D_CHAIN_PASSES")
    os.environ["IS3D_CHAIN_PASSES"] = "2"
    try:
        d = e.calculate_spectra()
        st1 = e.stats()
    finally:
        if old is None:
            os.environ.pop("IS3D_CHAIN_PASSES")
        else:
            os.environ["IS3D_CHAIN_PASSES"] = old
    e.close()
    assert st["iterations"] > n // 2, st               # >= one Newton step per live cell
    for key in ("iterations", "breakdown", "pl_negative", "recon_fail"):
        assert st1[key] == st[key], (key, st1[key], st[key])
    assert np.isfinite(full).all() and np.isfinite(d).all()
    assert (full != 0).sum() > 0.5 * full.size
    m = np.abs(full) > 1e-290
    assert np.array_equal(d[m], 2.0 * full[m])
    assert np.abs(d[~m] - 2.0 * full[~m]).max(initial=0.0) <= 1e-300
