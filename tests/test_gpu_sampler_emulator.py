"""Engine.sample / Engine.sample_famod against the serial CPU emulator of the same sampler_math.h
(tests/native/sampler_emulator.cpp, sampler_famod_emulator.cpp), record for record.

What differs between the two is everything sampler.hip adds to the math: k_cells' lanes over species and its sum,
k_count's thread per (event, cell), k_sample's running sum in LDS, its 64-event prefix sum that maps a lane to an
(event, candidate) pair, the slots, the scans and the compaction, and the Plasma-average densities of fast = 1 -- and the
device's exp / log / sin / cos against the host's.  So the structure of the list (which candidates exist, their
species, which are kept) must be equal with allowance 0, and the momenta within the project's host-against-device bar
of 1e-8.  Measured maxima: DESIGN.md 7.5.

A keep or species draw u that falls within rounding of its threshold can flip between host and device libm; with
~1e5 draws of 53-bit uniforms against thresholds that differ by a few ulp this has probability ~1e-11 per case.  Should
it happen, the message below shows |u - weight| < 1e-12 for the first differing candidate: that is a property of the
seed -- change the seed of that case, never the allowance."""
import numpy as np
import pytest

from is3d2_amd import build_engine, make_spec, synth
from oracle import oracle as O

import sampler_famod_ref as F
import sampler_ref as R

pytestmark = pytest.mark.gpu
BAR = 1e-8          # host against device, DESIGN.md 7.1
NEV, Y_CUT, SEED = 20, 0.8, 3
EXACT = ("species", "cell", "event", "tau", "x", "y")


def harsh_surface(dimension, baryon):
    """test_gpu_sampler.py's invariants surface (300 cells, seed 29) made harsher: every seventh normal reversed
    (u.dsigma <= 0: skipped cells) and every other bulk pressure x 10 (PTM and PTB cells that break down next to cells
    that do not; clamped delta-f weights in Grad and RTA-CE)."""
    s = synth.surface(300, seed=29, dimension=dimension, baryon=baryon, full3d=(dimension == 3))
    s["dat"][::7] *= -1.0
    s["bulkPi"][::2] *= 10.0
    return synth.as_read(s)


def by_event(ref, n_events):
    """The emulator's (cell, event, candidate) order as the engine's (event, cell, candidate), and its offsets."""
    ref = ref[np.argsort(ref["event"], kind="stable")]
    return ref, np.concatenate([[0], np.cumsum(np.bincount(ref["event"], minlength=n_events))])


def compare(got, off, ref, off_r, dimension, explain):
    """Allowance 0 for the structure and the copied positions, BAR for the computed fields; returns the largest
    relative difference per field.  explain(cell, event, got, ref) prints the candidates of the first pair that differs."""
    k = min(len(got), len(ref))
    same = (got["cell"][:k] == ref["cell"][:k]) & (got["event"][:k] == ref["event"][:k]) & (got["species"][:k] == ref["species"][:k])
    if len(got) != len(ref) or not same.all():
        i = int(np.argmin(same)) if not same.all() else k - 1
        print("first structural mismatch at record %d: device %s, emulator %s" % (i, got[i:i + 1], ref[i:i + 1]))
        first = min((int(q["event"][i]), int(q["cell"][i])) for q in (got, ref))     # the list is ordered by (event, cell)
        explain(first[1], first[0], got, ref)
    assert len(got) == len(ref)
    exact = EXACT + (("eta",) if dimension == 3 else ())
    for f in exact:
        assert np.array_equal(got[f], ref[f]), f
    assert np.array_equal(off, off_r)
    E, tau = ref["E"], ref["tau"]
    err = {f: float(np.max(np.abs(got[f] - ref[f]) / E)) for f in ("E", "px", "py", "pz")}
    err.update({f: float(np.max(np.abs(got[f] - ref[f]) / tau)) for f in ("t", "z")})
    if dimension == 2:
        err["eta"] = float(np.max(np.abs(got["eta"] - ref["eta"]) / np.maximum(1.0, np.abs(ref["eta"]))))
    return err


CASES = [(mode, dimension, fast, False, "pikp") for mode in (1, 2, 3, 4) for dimension in (2, 3) for fast in (0, 1)] + \
        [(mode, 3, 0, True, "pikp") for mode in (1, 2, 3)] + [(3, 3, 0, False, "smash")]


@pytest.mark.parametrize("mode,dimension,fast,baryon,chosen", CASES)
def test_engine_sample_equals_the_emulator(mode, dimension, fast, baryon, chosen):
    """df_mode 1-4, 2+1D and 3+1D (full3d), fast 0 / 1; Grad, RTA-CE and PTM once more with synth's muB, nB, V and
    include_baryon = include_baryondiff_deltaf = 1; PTM once with SMASH's 444 species (its negative species weights enter
    dn_tot and count as zero in the draw)."""
    flags = dict(R.BARYON_FLAGS) if baryon else {}
    spec = make_spec(chosen=chosen, df_mode=mode, dimension=dimension, **flags)
    s = harsh_surface(dimension, baryon)
    plasma = O.averages(s, 1 if baryon else 0)
    e = build_engine(spec, s, T_avg=plasma[0])
    got, off, st = e.sample(SEED, NEV, Y_CUT, fast, plasma)
    e.close()
    cap = 4 * len(got) + 1000
    _, st_r, ref = R.sample(spec, s, plasma, SEED, NEV, Y_CUT, fast, keep=cap)
    assert st_r["kept"] <= cap
    ref, off_r = by_event(ref, NEV)

    def explain(cell, event, got, ref):
        rows = R.trace(spec, s, plasma, SEED, cell, event, Y_CUT, fast)
        dev = got[(got["cell"] == cell) & (got["event"] == event)]
        print("(cell %d, event %d): the emulator draws %d candidates; the device kept species %s" % (cell, event, len(rows), list(dev["species"])))
        for n, (sp, kept, u, w, prop, odd) in enumerate(rows):
            print("  candidate %d: species %d, kept %d, keep draw u = %.17g, weight = %.17g, |u - w| = %.3e, proposals %d%s" %
                  (n, sp, kept, u, w, abs(u - w), prop, "  (restated weight disagrees with candidate())" if odd else ""))

    err = compare(got, off, ref, off_r, dimension, explain)
    print("mode %d %dD fast %d baryon %d %s: %d records, %d candidates, breakdown %d of %d live cells, clamped %d; max relative "
          "difference %s" % (mode, dimension, fast, baryon, chosen, len(got), st["candidates"], st["breakdown"], st_r["live_cells"],
                             st["clamped"], ", ".join("%s %.2e" % kv for kv in sorted(err.items()))))
    # conditions on the input: skipped cells, and for PTM / PTB both branches in one launch
    assert len(got) > 1000 and st["cells"] == 300 and 200 < st_r["live_cells"] < 300
    if mode in (3, 4):
        assert 0 < st["breakdown"] < st_r["live_cells"]
    if chosen == "smash":
        assert len(spec["species"]["mass"]) == 444
    for k in ("candidates", "kept", "proposals", "acceptances", "capped", "clamped", "breakdown"):
        assert st[k] == st_r[k], (k, st[k], st_r[k])
    # the engine counts the cells of the window, not the live ones: those are the emulator's, and every cell in the
    # device's list is one of them by the equality of the lists
    assert st["capped"] == 0 and st["kept"] == len(got)
    assert max(err.values()) < BAR


def test_engine_sample_famod_equals_the_emulator():
    """df_mode 5 on the breakdown-heavy surface Q with the reference's one chain: the list and the sampler's and the
    reconstruction's counters."""
    spec = make_spec(chosen="pikp", df_mode=5, dimension=3, famod_chains=1)
    s = F.surface_q()
    e = build_engine(spec, s)
    got, off, st = e.sample_famod(SEED, NEV, Y_CUT)
    fst = e.sample_famod_stats()
    e.close()
    cap = 4 * len(got) + 1000
    _, st_r, ref = F.emu_sample(spec, s, SEED, NEV, Y_CUT, chains=1, keep=cap)
    assert st_r["kept"] <= cap
    ref, off_r = by_event(ref, NEV)

    def explain(cell, event, got, ref):
        for name, q in (("device", got), ("emulator", ref)):
            print("(cell %d, event %d) %s: %s" % (cell, event, name, q[(q["cell"] == cell) & (q["event"] == event)]))

    err = compare(got, off, ref, off_r, 3, explain)
    print("mode 5 Q: %d records, %d candidates, breakdown %d of %d live cells, %s; max relative difference %s" %
          (len(got), st["candidates"], st["breakdown"], st_r["live_cells"], fst, ", ".join("%s %.2e" % kv for kv in sorted(err.items()))))
    assert len(got) > 1000 and 0 < st["breakdown"] < st_r["live_cells"] < len(s["tau"]) == st["cells"]
    for k in ("candidates", "kept", "proposals", "acceptances", "capped", "breakdown"):
        assert st[k] == st_r[k], (k, st[k], st_r[k])
    assert fst == {k: st_r[k] for k in ("plpt_negative", "reconstruction_fail", "iterations")} and fst["plpt_negative"] > 10
    assert st["capped"] == 0 and st["kept"] == len(got)
    assert max(err.values()) < BAR
