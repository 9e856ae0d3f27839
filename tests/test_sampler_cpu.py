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


@pytest.mark.parametrize("name", sorted(R.PHYSICS_CASES))
def test_momentum_distribution_against_the_continuous_spectra(name):
    """The serial emulator on the cases of tests/sampler_ref.py (PHYSICS_CASES): N, <pT>, v2 per species -- and in
    3+1D <y - eta_cell>, <(y - eta_cell)^2> -- against the oracle's Cooper-Frye spectra.  5 sigma, after the condition
    on the input that the reference's own quadrature uncertainty is below sigma / 5.  tests/test_gpu_sampler_physics.py
    runs the same cases through Engine.sample."""
    inp = R.physics_inputs(name)
    mu = inp["n_events"] * inp["fine"][0].sum()
    _, st, parts = R.sample(inp["spec"], inp["surf"], inp["plasma"], seed=41, n_events=inp["n_events"], y_cut=R.Y_CUT,
                            fast=inp["fast"], keep=int(mu + 10 * np.sqrt(mu)))
    R.check_moments(name, parts, st, "emulator")


HBARC = 0.197327053


def cell_at_rest(baryon):
    """One 3+1D cell with u = 0, dsigma = (dat, 0, 0, 0) and eta = 0: the LRF axes are the lab's, w_flux = 1 and every
    candidate is kept.  pi^{mu nu} has every component different (tau pi^{x eta} != pi^{xy}: a transposed or mis-signed
    term in rescale_momentum moves the distribution), Pi < 0, and with baryon: muB, nB and V^mu with three different
    components."""
    s = synth.surface(4, seed=31, dimension=3, baryon=baryon, full3d=True)
    s = {k: v[1:2].copy() for k, v in s.items()}
    for k in ("dax", "day", "dan", "ux", "uy", "un", "eta"):
        s[k][:] = 0.0
    tau = s["tau"][0]
    s["dat"][:] = 40.0
    s["T"][:], s["E"][:], s["P"][:] = 0.150, 0.28, 0.045
    s["pixx"][:], s["pixy"][:], s["pixn"][:], s["piyy"][:], s["piyn"][:] = 0.009, 0.006, -0.004 / tau, -0.003, 0.002 / tau
    s["bulkPi"][:] = -0.004
    if baryon:
        s["muB"][:], s["nB"][:] = 0.21, 0.06
        s["Vx"][:], s["Vy"][:], s["Vn"][:] = 0.012, -0.007, 0.004 / tau
    return synth.as_read(s)


@pytest.mark.parametrize("mode,baryon", [(3, False), (4, False), (3, True)])
def test_modified_momenta_of_one_cell_at_rest(mode, baryon):
    """PTM and PTB: the kept momentum is p = A p' (+ the diffusion shift), p' thermal at T_mod (PTM) or T (PTB).  A, T_mod
    and alphaB_mod are rebuilt here in numpy from the surface fields and the oracle's delta-f coefficients
    (ParticleSampler.cpp:407-426, :790-830), not taken from the emulator's Cell:
        A_ij = (1 + bulk_mod) delta_ij + pi_ij / (2 beta_pi),  bulk_mod = Pi / (3 beta_Pi) (PTM), lambda (PTB),
        T_mod = T + Pi F / beta_Pi,  alphaB_mod = alphaB + Pi G / beta_Pi  (PTM).
    A^-1 p / T_mod is then the thermal distribution: the radial KS test against thermal_cdf and the two angular ones per
    species, bar ks_bar(n); the kept count is Poisson with the oracle's total yield at the cell's own densities.

    PTM with baryon diffusion: p = A p' + (T / beta_V)(E' nB / (E + P) + b) V with E' = sqrt(p'^2 + m^2)
    (ParticleSampler.cpp:407-422) is inverted by fixed-point iteration on p' and tested at (T_mod, b alphaB_mod).  This
    is the only check this case can have: the reference's continuous PTM spectra leave the diffusion shift out of the
    momentum map (MomentumSpectra.cpp:694-696, "leave for future work") while its sampler applies it, so the two
    disagree -- with synth's baryon surface the sampled proton <pT> is 1.383 GeV against 1.209 GeV from the spectra,
    19 sigma at 200 events.  The sampler here follows the reference's sampler; it is not to be "fixed" to match the
    spectra."""
    nev = 200000
    flags = dict(R.BARYON_FLAGS) if baryon else {}
    spec = make_spec(hrg_eos=2, chosen="pikp", df_mode=mode, dimension=3, **flags)
    s = cell_at_rest(baryon)
    T, E, P, Pi, tau = s["T"][0], s["E"][0], s["P"][0], s["bulkPi"][0], s["tau"][0]
    muB, nB = (s["muB"][0], s["nB"][0]) if baryon else (0.0, 0.0)
    plasma = np.array([T, E, P, muB, nB])
    rc, df = O.df_coefficients(spec, T, muB, E, P, Pi, T)
    assert rc == 0
    F, G, betabulk, betaV, betapi, lam = df[6], df[7], df[8], df[9], df[10], df[11]
    xx, xy, xz, yy, yz = s["pixx"][0], s["pixy"][0], tau * s["pixn"][0], s["piyy"][0], tau * s["piyn"][0]
    pi = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, -(xx + yy)]])
    if mode == 3:
        A = (1.0 + Pi / (3.0 * betabulk)) * np.eye(3) + pi / (2.0 * betapi)
        T_mod, alpha_mod = T + Pi * F / betabulk, muB / T + Pi * G / betabulk
    else:
        A = (1.0 + lam) * np.eye(3) + pi / (2.0 * betapi)
        T_mod, alpha_mod = T, 0.0
    # conditions on the input: A is far from breakdown, its xy and xz terms differ, and PTM's T_mod is not T
    assert np.linalg.det(A) > 0.1 and abs(A[0, 1] - A[0, 2]) > 0.05 and (mode == 4 or abs(T_mod - T) > 1e-4)
    mu = nev * O.total_yield(spec, s, plasma)[0]
    counts, st, parts = R.sample(spec, s, plasma, seed=13, n_events=nev, keep=int(mu + 10 * np.sqrt(mu)))
    print("mode %d baryon %d: kept %d of %d candidates, mu %.1f (%.2f sigma)" %
          (mode, baryon, st["kept"], st["candidates"], mu, (st["kept"] - mu) / np.sqrt(mu)))
    assert st["capped"] == 0 and st["breakdown"] == 0 and st["clamped"] == 0
    assert st["kept"] == st["candidates"] == len(parts)
    assert mu > 1e5 and abs(st["kept"] - mu) <= 5 * np.sqrt(mu)
    p = np.stack([parts["px"], parts["py"], parts["pz"]], axis=1)
    sp = spec["species"]
    m, b = sp["mass"][parts["species"]], sp["baryon"][parts["species"]]
    q = np.linalg.solve(A, p.T).T
    if baryon:
        V = np.array([s["Vx"][0], s["Vy"][0], tau * s["Vn"][0]])
        shift = lambda q: (T / betaV) * (np.sqrt((q * q).sum(axis=1) + m * m) * (nB / (E + P)) + b)[:, None] * V[None, :]
        assert np.abs(shift(q)).max() > 1e-3            # the shift is there to be inverted
        for _ in range(60):
            q = np.linalg.solve(A, (p - shift(q)).T).T
        res = np.abs(q @ A.T + shift(q) - p).max()
        print("fixed point of p = A p' + shift(p'): residual %.2e GeV" % res)
        assert res < 1e-14
    for i, mcid in enumerate(sp["mcid"]):
        k = parts["species"] == i
        n = int(k.sum())
        qb = np.linalg.norm(q[k], axis=1)
        phi = np.arctan2(q[k, 1], q[k, 0]) % (2 * np.pi)
        d = (R.ks_distance(qb / T_mod, R.thermal_cdf(sp["mass"][i] / T_mod, sp["sign"][i], sp["baryon"][i] * alpha_mod)),
             R.ks_distance(q[k, 2] / qb, lambda c: (c + 1.0) / 2.0), R.ks_distance(phi, lambda a: a / (2 * np.pi)))
        print("mcid %d: %d particles, KS radial %.3e costheta %.3e phi %.3e (bar %.3e)" % ((int(mcid), n) + d + (R.ks_bar(n),)))
        assert n > 10000 and max(d) < R.ks_bar(n)


@pytest.mark.parametrize("mode", [1, 4])
def test_lab_momentum_of_a_3d_cell_is_the_boost_of_the_cell_at_rest_in_eta(mode):
    """The streams are functions of (seed, cell, event, candidate), not of eta, and the flux and viscous weights are
    boost invariant: the same full-3D cells (u^eta, dsigma_eta, pi^{x eta}, pi^{y eta} != 0) at eta = 0 and at eta = eta0
    keep the same candidates, and (E, pz) at eta0 is the Lorentz boost by eta0 of (E, pz) at eta = 0, where
    pz = tau p^eta alone.  Bar: 64 ulp of E cosh(eta0) -- the record's E is a rounded square root of sums that the
    boost restates in another order."""
    eps = np.finfo(np.float64).eps
    spec = make_spec(hrg_eos=2, chosen="pikp", df_mode=mode, dimension=3)
    s0 = synth.as_read(synth.surface(300, seed=29, dimension=3, full3d=True))
    plasma = O.averages(s0, 0)
    s0["eta"] = np.zeros(300)
    assert (np.abs(s0["un"] * s0["tau"]) > 0.02).sum() > 150
    _, st0, a = R.sample(spec, s0, plasma, seed=3, n_events=20, keep=100000)
    for eta0 in (1.3, -2.6):
        s1 = dict(s0)
        s1["eta"] = np.full(300, eta0)
        _, st1, b = R.sample(spec, s1, plasma, seed=3, n_events=20, keep=100000)
        assert st1 == st0 and len(a) == len(b) == st0["kept"] > 2000
        for k in ("species", "cell", "event", "px", "py"):
            np.testing.assert_array_equal(a[k], b[k])
        ch, sh = np.cosh(eta0), np.sinh(eta0)
        bar = 64 * eps * a["E"] * ch
        assert (np.abs(b["E"] - (a["E"] * ch + a["pz"] * sh)) <= bar).all()
        assert (np.abs(b["pz"] - (a["pz"] * ch + a["E"] * sh)) <= bar).all()
        np.testing.assert_array_equal(b["eta"], s1["eta"][b["cell"]])


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
