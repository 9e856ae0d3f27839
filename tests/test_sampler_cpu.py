"""CPU tier of the operation = 2 particle sampler: is3d2_amd/csrc/sampler_math.h, run serially by
tests/native/sampler_emulator.cpp -- the Philox generator, the Poisson draw, sample_momentum and whole cells.

Every seed is fixed and every bar is derived (tests/sampler_ref.py): 5 sqrt(mu) for a count, 5 standard errors for a
mean, sqrt(ln(2 / 1e-9) / (2 n)) for a Kolmogorov-Smirnov distance."""
import numpy as np
import pytest

from is3d2_amd import make_spec, synth
from oracle import oracle as O

import sampler_ref as R

N = 200000

# Philox4x32-10 known answers (Random123's kat_vectors)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert tuple(R.philox(ctr, key)) == want


def test_uniforms_are_53_bit_fractions_in_the_unit_interval():
    u = R.uniforms(12345, 2, 7, 3, 1, 100000)
    assert (u >= 0.0).all() and (u < 1.0).all()
    assert (u * 2.0 ** 53 == np.floor(u * 2.0 ** 53)).all()          # multiples of 2^-53
    assert (np.floor(u * 2.0 ** 53) % 2 == 1).any()                   # ... and the last of the 53 bits is used
    assert abs(u.mean() - 0.5) <= 5 * np.sqrt(1 / 12 / len(u))
    # a stream is a function of every coordinate: changing one gives other numbers, repeating gives the same
    base = R.uniforms(12345, 2, 7, 3, 1, 8)
    assert (base == u[:8]).all()
    for other in [(12346, 2, 7, 3, 1), (12345, 1, 7, 3, 1), (12345, 2, 8, 3, 1), (12345, 2, 7, 4, 1), (12345, 2, 7, 3, 2),
                  (12345, 2, 7 + 2 ** 32, 3, 1)]:
        assert not (R.uniforms(*other, 8) == base).any()


@pytest.mark.parametrize("mean", [0.05, 3.0, 16.5, 40.0, 400.0])
def test_poisson_mean_and_variance(mean):
    x, capped = R.poisson(99, mean, N)
    assert capped == 0
    x = x.astype(np.float64)
    se_mean = np.sqrt(mean / N)
    # Var[(x - mean)^2] = mu4 - mean^2 with the Poisson mu4 = mean (1 + 3 mean)
    se_var = np.sqrt((mean * (1 + 3 * mean) - mean * mean) / N)
    var = np.mean((x - mean) ** 2)
    print("poisson mean %g: sample mean %.6g (se %.3g), variance %.6g (se %.3g)" % (mean, x.mean(), se_mean, var, se_var))
    assert abs(x.mean() - mean) <= 5 * se_mean
    assert abs(var - mean) <= 5 * se_var


CASES = [(0.5, -1, 0.0), (0.9, -1, 0.0), (0.9, 1, 0.0), (1.5, -1, 0.0), (6.0, 1, 0.0), (6.0, 1, 0.8), (15.0, 1, 0.0)]
_momenta = {}


def momenta(case):
    if case not in _momenta:
        _momenta[case] = R.momentum(2024, case[0], float(case[1]), case[2], N)
    return _momenta[case]


@pytest.mark.parametrize("case", CASES)
def test_sample_momentum_radial_distribution(case):
    out, capped = momenta(case)
    assert capped == 0
    d = R.ks_distance(out[:, 0], R.thermal_cdf(*case))
    print("sample_momentum mbar=%g sign=%+d chem=%g: KS %.3e (bar %.3e), efficiency %.3f" %
          (case + (d, R.ks_bar(N), N / out[:, 4].sum())))
    assert d < R.ks_bar(N)


@pytest.mark.parametrize("case", CASES)
def test_sample_momentum_direction_is_isotropic(case):
    out, _ = momenta(case)
    dc = R.ks_distance(out[:, 1], lambda c: (c + 1.0) / 2.0)
    dp = R.ks_distance(out[:, 2], lambda p: p / (2 * np.pi))
    print("direction mbar=%g: KS costheta %.3e, phi %.3e (bar %.3e)" % (case[0], dc, dp, R.ks_bar(N)))
    assert dc < R.ks_bar(N) and dp < R.ks_bar(N)


def test_every_proposal_branch_is_taken():
    """0: light without the pion rescale, 4: with it (bosons below 0.8554); 1, 2, 3: the three K-distributions."""
    seen = set()
    for case in CASES:
        out, _ = momenta(case)
        seen |= set(int(b) for b in np.unique(out[:, 3]))
    assert seen == {0, 1, 2, 3, 4}
    assert set(np.unique(momenta(CASES[0])[0][:, 3])) == {4}
    assert set(np.unique(momenta(CASES[1])[0][:, 3])) == {0}
    for case in CASES[3:]:
        assert set(np.unique(momenta(case)[0][:, 3])) == {1, 2, 3}


def one_cell(dimension):
    """One cell with a timelike normal (dsigma = (dat, 0, 0, 0): p.dsigma > 0 for every momentum) and small pi, Pi."""
    s = synth.surface(4, seed=31, dimension=dimension, full3d=(dimension == 3))
    s = {k: v[1:2].copy() for k, v in s.items()}
    for k in ("dax", "day", "dan"):
        s[k][:] = 0.0
    for k in ("pixx", "pixy", "pixn", "piyy", "piyn"):
        s[k] *= 0.05
    s["bulkPi"] *= 0.1
    return synth.as_read(s)


@pytest.mark.parametrize("mode,dimension,fast", [(1, 2, 0), (2, 3, 0), (3, 2, 0), (4, 3, 0), (1, 3, 1), (3, 3, 1), (4, 2, 1)])
def test_exact_yield_of_one_cell(mode, dimension, fast):
    """Thinning a Poisson draw leaves a Poisson: the kept count of 2e5 events has the mean
    Nevents x estimate_mean_particle_number at the cell's own densities (the oracle's total yield with the cell's
    (T, E, P) as the Plasma averages), exactly, as long as the delta-f clamp is never hit."""
    spec = make_spec(hrg_eos=2, chosen="pikp", df_mode=mode, dimension=dimension)
    s = one_cell(dimension)
    plasma = np.array([s["T"][0], s["E"][0], s["P"][0], 0.0, 0.0])
    y_cut = 0.7
    mu1, _ = O.total_yield(spec, s, plasma, y_cut=y_cut)
    counts, st, _ = R.sample(spec, s, plasma, seed=5, n_events=N, y_cut=y_cut, fast=fast)
    mu = N * mu1
    print("mode %d %dD fast %d: kept %d, expected %.1f (5 sigma %.1f), candidates %d, clamped %d, breakdown %d" %
          (mode, dimension, fast, st["kept"], mu, 5 * np.sqrt(mu), st["candidates"], st["clamped"], st["breakdown"]))
    assert st["capped"] == 0 and st["clamped"] == 0 and st["breakdown"] == 0
    assert counts.sum() == st["kept"]
    assert abs(st["kept"] - mu) <= 5 * np.sqrt(mu)
    for i, mcid in enumerate(spec["species"]["mcid"]):      # and per species, the oracle with that one species chosen
        spec1 = make_spec(hrg_eos=2, chosen=[int(mcid)], df_mode=mode, dimension=dimension)
        mus = N * O.total_yield(spec1, s, plasma, y_cut=y_cut)[0]
        assert abs(counts[i] - mus) <= 5 * np.sqrt(mus)


def test_particle_list_writers_match_the_reference_format(tmp_path):
    """write_particle_list_OSC / write_particle_list_toFile (EmissionFunction.cpp:611-678): the header line, the
    column order, setprecision(16) / setprecision(8) scientific, the row index restarting in every event and the
    MCID right-aligned in five columns (setw(5)) in the CSV form."""
    from is3d2_amd import host
    rng = np.random.default_rng(8)
    n, off = 7, np.array([0, 3, 3, 7])
    p = np.zeros(n, dtype=R.PARTICLE_DTYPE)
    for k in ("tau", "x", "y", "eta", "t", "z", "E", "px", "py", "pz"):
        p[k] = rng.normal(0.0, 3.0, n) * 10.0 ** rng.integers(-3, 4, n)
    mcid = np.array([211, -211, 2212, 321, -3122, 111, 9000221])
    mass = rng.uniform(0.1, 2.0, n)
    d = str(tmp_path)
    host.write_particle_lists(d, p, off, mcid, mass, write_csv=True)
    for ev in range(3):
        rows = range(off[ev], off[ev + 1])
        osc = "n pid px py pz E m x y z t\n" + "".join(
            "%d %d " % (i - off[ev], mcid[i]) + " ".join("%.16e" % v for v in (p["px"][i], p["py"][i], p["pz"][i], p["E"][i], mass[i],
                                                                               p["x"][i], p["y"][i], p["z"][i], p["t"][i])) + "\n"
            for i in rows)
        csv = "mcid,tau,x,y,eta,E,px,py,pz\n" + "".join(
            "%5d," % mcid[i] + ",".join("%.8e" % p[k][i] for k in ("tau", "x", "y", "eta", "E", "px", "py", "pz")) + "\n" for i in rows)
        assert open("%s/results/particle_list_osc_%d.dat" % (d, ev + 1)).read() == osc
        assert open("%s/results/particle_list_%d.dat" % (d, ev + 1)).read() == csv
