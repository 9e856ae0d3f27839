"""GPU tier of the sampler's physics checks: Engine.sample on the cases of tests/sampler_ref.py (PHYSICS_CASES) -- PTM
and PTB momenta, baryon chemical potential and diffusion in Grad and RTA-CE, fast = 1, and 3+1D by boost invariance --
against the oracle's continuous Cooper-Frye spectra: per species N, <pT>, v2 and, in 3+1D, <y - eta_cell> and
<(y - eta_cell)^2> with y from the record's (E, pz).

The bars are derived, none tuned: 5 sqrt(mu) for a count, 5 std / sqrt(mu) for a mean (std from the spectra), after the
condition on the input that the reference's own quadrature uncertainty (48 x 32 against 24 x 24 momentum tables, 113
against 57 rapidities) is below a fifth of that sigma.  300 cells and at most 300 events; tests/test_sampler_cpu.py
runs the same cases through the serial emulator.  Measured figures: DESIGN.md 7.5."""
import pytest

from is3d2_amd import build_engine

import sampler_ref as R

pytestmark = pytest.mark.gpu
SEED = 43          # not the CPU tier's 41: the two tiers draw independent samples


@pytest.mark.parametrize("name", sorted(R.PHYSICS_CASES))
def test_sampled_moments_against_the_continuous_spectra(name):
    inp = R.physics_inputs(name)
    plasma = inp["plasma"]
    e = build_engine(inp["spec"], inp["surf"], T_avg=plasma[0])
    p, off, st = e.sample(SEED, inp["n_events"], R.Y_CUT, inp["fast"], plasma)
    e.close()
    assert off[-1] == len(p) == st["kept"] and st["cells"] == len(inp["surf"]["tau"])
    R.check_moments(name, p, st, "gpu")
