"""CPU tier of the Monte Carlo decays of a particle list: the kernels' math
(is3d2_amd/csrc/decay_mc_math.h, run on the host by tests/native/decay_list_emulator.cpp) -- single-decay kinematics,
the flat Dalitz plot, an independent numpy Monte Carlo, the channel draw -- and the channel plan it shares with the
feed-down, which must be what it was.
"""
import numpy as np
import pytest

import decay_list_ref as L
import decay_ref as R

MASS, RHO, DELTA, OMEGA, ADJUSTED, TABLE = L.MASS, L.RHO, L.DELTA, L.OMEGA, L.ADJUSTED, L.TABLE

# (pT, y) of the parents of the kinematics test: at rest, pT = 0 with rapidity, |y| = 4, and a generic one
CONFIGS = [(0.0, 0.0), (0.0, 1.5), (0.7, 4.0), (0.7, -4.0), (2.5, 0.3)]
N_EACH = 2000


def decay_configs(species, table=TABLE):
    """N_EACH decays of a parent of `species` at every CONFIGS point: (parents, finals, origins, stats)."""
    pT = np.repeat([c[0] for c in CONFIGS], N_EACH)
    y = np.repeat([c[1] for c in CONFIGS], N_EACH)
    phi = np.random.default_rng(3).uniform(0, 2 * np.pi, len(pT))
    par = L.make_list(np.full(len(pT), species), MASS, pT=pT, phi=phi, y=y)
    out, off, orig, st, _ = L.emulate(MASS, table, par, [0, len(par)], 11)
    return par, out, orig, st


def mass_shell_ulps(p):
    """|E^2 - p^2 - m^2| in ulp of E^2."""
    m = MASS[p["species"]]
    return np.abs(p["E"] ** 2 - p["px"] ** 2 - p["py"] ** 2 - p["pz"] ** 2 - m * m) / L.ulp(p["E"] ** 2)


@pytest.mark.parametrize("species,nbody,bar", [(3, 2, 64), (4, 2, 64), (5, 3, 128)], ids=["rho", "Delta", "omega"])
def test_single_decay_conserves_four_momentum(species, nbody, bar):
    """Unadjusted channels: the daughters sit on their mass shells and sum to the parent's (MT cosh y, px, py,
    MT sinh y), for parents at rest, at pT = 0, at y = +-4 and at a generic point.

    Mass shell: E = sqrt(m^2 + px^2 + py^2 + pz^2) is the last operation, so E^2 - p^2 - m^2 carries the rounding of
    four squares, three additions, the square root and the test's own five operations, each at most half an ulp of
    E^2 or (the root, squared) one ulp: 8 ulp of E^2, the sampler tests' bar.

    Sum: in units of ulp(E_R), E_R the parent's energy.  One boost (decay_mc_math.h boost) is 11 roundings per
    component -- P.q 5, g 4, the component 2 -- of values bounded by 2 E_R, so at most 11 ulp(E_R) per daughter; the
    rest-frame vector q enters the two daughters with exactly opposite signs and E1* + E2* = M to one ulp, so nothing
    else of the rest frame survives in the sum.  parent_p4 (two square roots, a division, three products) adds 6, and
    re-deriving E from the mass shell moves it by at most the three components' errors, another 11 per daughter.  Two
    daughters: 2 x (11 + 11) + 6 = 50, rounded up to 64.  A 3-body decay boosts daughters 2 and 3 twice, and the
    outer boost carries the inner one's error over with a factor bounded by 2 in these units: 128."""
    par, out, orig, st = decay_configs(species)
    assert st["decays"] == len(par) and st["capped"] == 0 and st["undecayed"] == 0
    assert len(out) == nbody * len(par) and np.array_equal(orig, np.repeat(np.arange(len(par)), nbody))
    assert mass_shell_ulps(out).max() <= 8
    sums = L.tree_sums(out, orig, len(par))
    want = np.stack([par[f] for f in ("E", "px", "py", "pz")], axis=1)
    err = np.abs(sums - want) / L.ulp(par["E"])[:, None]
    print("max |sum p - P| in ulp(E_R) per config:", err.reshape(len(CONFIGS), N_EACH, 4).max(axis=(1, 2)))
    assert err.max() <= bar
    # positions, cell and event are the parent's
    for f in ("tau", "x", "y", "eta", "t", "z", "cell", "event"):
        assert np.array_equal(out[f], par[f][orig])
    # isotropy at rest: the mean direction of daughter 0 vanishes within 5 sigma of 1 / sqrt(3 N)
    first = out[::nbody][:N_EACH]
    p = np.sqrt(first["px"] ** 2 + first["py"] ** 2 + first["pz"] ** 2)
    for f in ("px", "py", "pz"):
        assert abs(np.mean(first[f] / p)) < 5 / np.sqrt(3 * N_EACH)


def test_adjusted_channel_keeps_px_py_and_rapidity():
    """X(1.07) -> N pi is closed at the pole masses; the rule opens it at M = 1.095, m_N = 0.928.  The parent enters at
    its (pT, phi, y) on M, the daughters are written on their pole masses at the (px, py, y) they were produced with:
    the mass shells hold at 8 ulp of E^2 and px, py are conserved at the 2-body bar; E and pz are not."""
    par, out, orig, st = decay_configs(6)
    ch, _ = L.mc_channels(MASS, TABLE)
    adj = [c for c in ch if c["parent"] == 6][0]
    assert adj["M"] == pytest.approx(1.095) and adj["m"][0] == pytest.approx(0.928)
    assert st["decays"] == len(par) and len(out) == 2 * len(par)
    assert mass_shell_ulps(out).max() <= 8
    sums = L.tree_sums(out, orig, len(par))
    scale = L.ulp(np.sqrt(adj["M"] ** 2 + par["px"] ** 2 + par["py"] ** 2) * np.cosh(np.arcsinh(par["pz"] / np.sqrt(
        par["E"] ** 2 - par["pz"] ** 2))))
    assert np.max(np.abs(sums[:, 1] - par["px"]) / scale) <= 64
    assert np.max(np.abs(sums[:, 2] - par["py"]) / scale) <= 64
    assert np.max(np.abs(sums[:, 0] - par["E"]) / par["E"]) > 1e-3        # energy is not: M is not the pole mass
    # the nucleon's rapidity is the one it was produced with: rebuild it on the channel mass and the pair's energy
    # and pz sum to the parent's on M
    N, pi = out[0::2], out[1::2]
    yN = np.arcsinh(N["pz"] / np.sqrt(MASS[2] ** 2 + N["px"] ** 2 + N["py"] ** 2))
    mT = np.sqrt(adj["m"][0] ** 2 + N["px"] ** 2 + N["py"] ** 2)
    yR = np.arcsinh(par["pz"] / np.sqrt(par["E"] ** 2 - par["pz"] ** 2))
    MT = np.sqrt(adj["M"] ** 2 + par["px"] ** 2 + par["py"] ** 2)
    assert np.allclose(mT * np.sinh(yN) + pi["pz"], MT * np.sinh(yR), rtol=1e-12, atol=1e-12)
    assert np.allclose(mT * np.cosh(yN) + pi["E"], MT * np.cosh(yR), rtol=1e-12, atol=1e-12)


def test_flat_dalitz_plot():
    """10^6 omega -> 3 pi decays at rest: (s12, s23) counted in a 6 x 6 grid of cells wholly inside the Dalitz
    boundary.  A flat plot puts mu = N x cell area / plot area in each (the plot's area is the integral of the s12
    range f(s23) of DESIGN.md 7.6); counts within 5 sqrt(mu), the sampler tests' bar."""
    n, M, m = 1_000_000, 0.782, 0.138
    par = L.make_list(np.full(n, 5), MASS, pT=np.zeros(n), phi=np.zeros(n), y=np.zeros(n))
    out, off, orig, st, _ = L.emulate(MASS, [OMEGA], par, [0, n], 2024)
    assert st["decays"] == n and st["capped"] == 0 and len(out) == 3 * n
    d = [out[k::3] for k in range(3)]

    def inv(a, b):
        return (a["E"] + b["E"]) ** 2 - (a["px"] + b["px"]) ** 2 - (a["py"] + b["py"]) ** 2 - (a["pz"] + b["pz"]) ** 2

    s12, s23 = inv(d[0], d[1]), inv(d[1], d[2])

    def s12_range(s):      # of a flat plot at fixed s23
        e2 = s / (2 * np.sqrt(s))            # equal masses: E2* = sqrt(s) / 2 in the (23) frame
        e1 = (M * M - s - m * m) / (2 * np.sqrt(s))
        p2, p1 = np.sqrt(np.maximum(e2 ** 2 - m * m, 0)), np.sqrt(np.maximum(e1 ** 2 - m * m, 0))
        return (e1 + e2) ** 2 - (p1 + p2) ** 2, (e1 + e2) ** 2 - (p1 - p2) ** 2

    lo, hi = 4 * m * m, (M - m) ** 2
    x, w = np.polynomial.legendre.leggauss(200)
    sq = lo + 0.5 * (hi - lo) * (1 + x)
    a, b = s12_range(sq)
    area = np.sum(0.5 * (hi - lo) * w * (b - a))
    c, h = (M * M + 3 * m * m) / 3, 0.05            # a square around the plot's centre
    edges = np.linspace(c - h, c + h, 7)
    fine = np.linspace(edges[0], edges[-1], 601)
    a, b = s12_range(fine)
    assert a.max() < edges[0] and b.min() > edges[-1]          # every cell is wholly inside
    H, _, _ = np.histogram2d(s12, s23, bins=[edges, edges])
    mu = n * (edges[1] - edges[0]) ** 2 / area
    print("mu %.1f, counts %d .. %d, largest pull %.2f" % (mu, H.min(), H.max(), np.abs(H - mu).max() / np.sqrt(mu)))
    assert mu > 1000 and np.all(np.abs(H - mu) <= 5 * np.sqrt(mu))


@pytest.mark.parametrize("case", ["rho-pipi", "Delta-N", "Delta-pi", "omega-3pi"])
def test_emulator_against_numpy_monte_carlo(case):
    """2 x 10^6 thermal parents decayed by the emulator against 2 x 10^6 others decayed by the independent numpy Monte Carlo of
    tests/test_decay_cpu.py (isotropic boost_daughter; omega: E1 from rejection on (E1, E2), not through f(s)):
    |y| < 0.5 counts of one daughter slot in that file's pT bins, and v2.  Two samples: 4 sigma of the combined
    counting error, sqrt(N1 + N2) and sqrt(0.5 / N1 + 0.5 / N2); every bin holds more than 1000."""
    n = 2_000_000
    sp, chan, slot, M, m1, m2, bins = {"rho-pipi": (3, RHO, 0, 0.776, 0.138, 0.138, L.PT_BINS),
                                       "Delta-N": (4, DELTA, 0, 1.232, 0.938, 0.138, L.PT_BINS),
                                       "Delta-pi": (4, DELTA, 1, 1.232, 0.138, 0.938, L.PT_BINS_SOFT),
                                       "omega-3pi": (5, OMEGA, 1, 0.782, 0.138, 0.138, L.PT_BINS_SOFT)}[case]
    rng = np.random.default_rng(20260301 + sp + slot)
    E, px, py, pz = L.draw_parents(rng, M, n)
    par = L.make_list(np.full(n, sp), MASS, E=E, px=px, py=py, pz=pz)
    out, off, orig, st, _ = L.emulate(MASS, [chan], par, [0, n], 77)
    nb = chan["n_body"]
    assert len(out) == nb * n and st["capped"] == 0
    N1, c1 = L.record_bins(out[slot::nb], bins)
    parent = L.draw_parents(rng, M, n)
    if nb == 2:
        Es = (M * M + m1 * m1 - m2 * m2) / (2 * M)
        p1 = np.sqrt(Es ** 2 - m1 * m1)
    else:
        p1 = np.sqrt(L.flat_dalitz_e1(rng, M, m1, n) ** 2 - m1 * m1)
    N2, c2 = L.count_bins(*L.boost_daughter(rng, parent, M, m1, p1), bins)
    print(case, "\n emulator", N1, c1, "\n numpy", N2, c2, "\n pulls", (N1 - N2) / np.sqrt(N1 + N2),
          (c1 - c2) / np.sqrt(0.5 / N1 + 0.5 / N2))
    assert np.all(N1 > 1000) and np.all(N2 > 1000)
    assert np.all(np.abs(N1 - N2) <= 4 * np.sqrt(N1 + N2))
    assert np.all(np.abs(c1 - c2) <= 4 * np.sqrt(0.5 / N1 + 0.5 / N2))


def test_channel_draw():
    """Species 6 of decay_ref.CASE_CHANNELS takes its two channels 0.5 / 0.5, and species 3, 5 and 7 stay undecayed
    with the shares 0.1, 0.11 and 0.3 their branchings leave: multinomial counts within 5 sqrt(mu)."""
    n = 200_000
    mass = R.CASE_MASS
    six = [c for c in R.CASE_CHANNELS if c["parent"] == 6]          # daughters 2 and 5 then stay: one generation
    par = L.make_list(np.full(n, 6), mass, pT=np.full(n, 0.5), phi=np.zeros(n), y=np.zeros(n))
    out, off, orig, st, _ = L.emulate(mass, six, par, [0, n], 9)
    a, b = np.sum(out["species"] == 2), np.sum(out["species"] == 5)
    print("species 6: %d / %d of %d" % (a, b, n))
    assert a + b == n and st["undecayed"] == 0 and st["dropped_daughters"] == b
    assert abs(a - n / 2) <= 5 * np.sqrt(n / 2)
    for sp, share in ((3, 0.1), (5, 0.11), (7, 0.3)):
        par = L.make_list(np.full(n, sp), mass, pT=np.full(n, 0.5), phi=np.zeros(n), y=np.zeros(n))
        out, off, orig, st, _ = L.emulate(mass, R.CASE_CHANNELS, par, [0, n], 10 + sp)
        stay = int(np.sum(out["species"] == sp))
        print("species %d: %d undecayed of %d" % (sp, stay, n))
        assert stay == st["undecayed"] and st["capped"] == 0
        assert abs(stay - share * n) <= 5 * np.sqrt(share * n)
        # the channel draw is the first uniform of the node's stream
        u = np.array([L.uniforms(10 + sp, i, 0, 0, 1)[0] for i in range(200)])
        kept = np.bincount(orig[out["species"] != sp], minlength=n)[:200] > 0
        assert np.array_equal(u < 1 - share, kept)


def test_plan_of_the_feed_down_is_unchanged():
    """build_plan now also hands out the kept list (with M and m[3]), the channel ranges and the levels.  The
    feed-down's statistics and results on the case table are what the numpy restatement gives, at the existing parity
    bar, and both consumers see one plan."""
    pT = np.linspace(0.1, 3.0, 10) ** 1.3
    phi = np.sort(np.random.default_rng(19).uniform(0, 2 * np.pi, 8))
    y = np.zeros(1)
    S = R.case_spectra(pT, phi, y)
    got, ab, st, slots = R.emulate(S, R.CASE_MASS, pT, phi, y, R.CASE_CHANNELS)
    ref, ab_ref, st_ref = R.feeddown(S, R.CASE_MASS, pT, phi, y, R.CASE_CHANNELS)
    assert R.parity(got, ref, ab_ref) < R.BAR
    assert slots == R.CASE_SLOTS
    for k, v in st_ref.items():
        assert st[k] == pytest.approx(v), k
    par = L.make_list([6], R.CASE_MASS, pT=np.array([0.5]), phi=np.zeros(1), y=np.zeros(1))
    _, _, _, _, plan = L.emulate(R.CASE_MASS, R.CASE_CHANNELS, par, [0, 1], 1)
    assert {k: plan[k] for k in st if k != "ms_total"} == {k: st[k] for k in st if k != "ms_total"}
    ch, level = L.mc_channels(R.CASE_MASS, R.CASE_CHANNELS)
    kept, _ = R.kept_channels(R.CASE_CHANNELS)
    assert sorted((c["parent"], c["nbody"], tuple(c["d"][:c["nbody"]])) for c in ch) == \
        sorted((c["parent"], c["n_body"], tuple(c["daughter"][:c["n_body"]])) for c in kept)
    assert list(level) == [-1, -1, 1, 0, -1, 1, 0, 0]


def chain(n):
    """n species, species k -> (k - 1) + (k - 1): n - 1 levels."""
    mass = 0.1 * 2.5 ** np.arange(n)
    return mass, [R.channel(k, [k - 1, k - 1], 1.0, mass[k], [mass[k - 1], mass[k - 1]]) for k in range(1, n)]


def test_a_plan_of_more_than_16_levels_is_refused():
    """The path code of a node's random stream has the 32 bits of the Philox counter's candidate word: 4^16 - 1 is the
    largest code, so 16 levels decay (2^16 leaves of one primary) and 17 are refused, never wrapped."""
    mass, ch = chain(17)
    par = L.make_list([16], mass, pT=np.array([0.3]), phi=np.zeros(1), y=np.zeros(1))
    out, off, orig, st, plan = L.emulate(mass, ch, par, [0, 1], 3)
    assert plan["levels"] == 16 and st["passes"] == 16 and len(out) == 2 ** 16 and (out["species"] == 0).all()
    assert st["decays"] == 2 ** 16 - 1
    mass, ch = chain(18)
    par = L.make_list([17], mass, pT=np.array([0.3]), phi=np.zeros(1), y=np.zeros(1))
    with pytest.raises(ValueError, match="17 levels"):
        L.emulate(mass, ch, par, [0, 1], 3)
