"""CPU tier of the resonance-decay feed-down: the formula against Monte Carlo decays, the kernel's
math (is3d2_amd/csrc/decay_math.h, run on the host by tests/native/decay_emulator.cpp) against the numpy restatement
(tests/decay_ref.py), yield conservation and the channel bookkeeping.

Parity is |got - ref| / sum |terms| with the project's bar 1e-8; measured 2.7e-13 (10 x 8 x 1 and 10 x 8 x 5).
"""
import os

import numpy as np
import pytest

from is3d2_amd import data as _data
from is3d2_amd import hrg

import decay_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
T = 0.150
V2 = 0.10
PT_BINS = np.array([0.2, 0.5, 0.8, 1.2, 1.8])
PT_BINS_SOFT = np.array([0.1, 0.2, 0.3, 0.45, 0.6])      # the pion of Delta -> N pi and of omega -> 3 pi is soft
N_PARENTS = 2_000_000
Y_MAX = 3.0           # parents flat in |Y| < Y_MAX: 0.5 + the largest dY = asinh(p* / m_pi) = 1.7 (rho), 2.0 (omega)


def thermal(MT, Phi, Y):
    return np.exp(-MT / T) * (1.0 + 2.0 * V2 * np.cos(2.0 * Phi)) + 0.0 * Y


# ------------------------------------------------------------------------------------------
# 1, 2: the formula against Monte Carlo decays (no shared algebra: draw parents, decay, boost, count)
# ------------------------------------------------------------------------------------------
def draw_parents(rng, M, n):
    """(E, px, py, pz) of n parents from S_R = exp(-MT / T)(1 + 2 v2 cos 2 Phi), flat in |Y| < Y_MAX."""
    # MT - M = x with density (x + M) exp(-x / T): Gamma(2, T) with weight T^2, Exp(T) with weight M T
    x = np.where(rng.uniform(size=n) < T / (T + M), rng.gamma(2.0, T, n), rng.exponential(T, n))
    MT = M + x
    PT = np.sqrt(MT ** 2 - M ** 2)
    Phi = np.empty(n)
    todo = np.arange(n)
    while len(todo):       # rejection under 1 + 2 v2
        p = rng.uniform(0, 2 * np.pi, len(todo))
        ok = rng.uniform(0, 1 + 2 * V2, len(todo)) < 1 + 2 * V2 * np.cos(2 * p)
        Phi[todo[ok]] = p[ok]
        todo = todo[~ok]
    Y = rng.uniform(-Y_MAX, Y_MAX, n)
    return MT * np.cosh(Y), PT * np.cos(Phi), PT * np.sin(Phi), MT * np.sinh(Y)


def boost_daughter(rng, parent, M, m1, p1):
    """Lab (pT, phi, y) of a daughter of mass m1 and rest-frame momentum p1 (array or scalar), isotropic."""
    E, px, py, pz = parent
    n = len(E)
    ct = rng.uniform(-1, 1, n)
    st = np.sqrt(1 - ct ** 2)
    ph = rng.uniform(0, 2 * np.pi, n)
    q = np.stack([p1 * st * np.cos(ph), p1 * st * np.sin(ph), p1 * ct])
    e1 = np.sqrt(p1 ** 2 + m1 ** 2)
    beta = np.stack([px, py, pz]) / E
    gamma = E / M
    bq = np.sum(beta * q, axis=0)
    lab = q + beta * (gamma ** 2 / (gamma + 1) * bq + gamma * e1)
    elab = gamma * (e1 + bq)
    return np.hypot(lab[0], lab[1]), np.arctan2(lab[1], lab[0]), 0.5 * np.log((elab + lab[2]) / (elab - lab[2]))


def count_bins(pT, phi, y, bins):
    """Daughters with |y| < 0.5 per pT bin, and their mean cos 2 phi."""
    sel = np.abs(y) < 0.5
    k = np.digitize(pT[sel], bins) - 1
    ok = (k >= 0) & (k < len(bins) - 1)
    N = np.bincount(k[ok], minlength=len(bins) - 1).astype(float)
    c2 = np.bincount(k[ok], weights=np.cos(2 * phi[sel][ok]), minlength=len(bins) - 1) / N
    return N, c2


def predict_bins(M, m1, others, n, bins):
    """The restatement with the exact parent, integrated over the bins (8 Gauss-Legendre points in pT, 8 uniform phi
    points: the daughters carry harmonics 0 and 2 only), per parent: (fraction of the parents, v2) per bin."""
    x, w = np.polynomial.legendre.leggauss(8)
    phi = np.arange(8) * (2 * np.pi / 8)
    norm = 2 * Y_MAX * 2 * np.pi * T * (M + T) * np.exp(-M / T)        # int dY PT dPT dPhi S_R
    frac, v2 = [], []
    for lo, hi in zip(bins[:-1], bins[1:]):
        pT = 0.5 * (lo + hi) + 0.5 * (hi - lo) * x
        dS, _ = R.slot_term(thermal, 1.0, M, m1, others, pT, phi, [0.0], n)
        f = dS[:, :, 0] * (pT * w * 0.5 * (hi - lo))[:, None] * (2 * np.pi / 8)
        frac.append(f.sum() * 1.0 / norm)          # x 1.0: the y window |y| < 0.5
        v2.append((f * np.cos(2 * phi)[None, :]).sum() / f.sum())
    return np.array(frac), np.array(v2)


def check_against_mc(N, c2, M, m1, others, bins):
    f12, v12 = predict_bins(M, m1, others, 12, bins)
    f24, v24 = predict_bins(M, m1, others, 24, bins)
    quad_N, quad_v = np.abs(f12 - f24) * N_PARENTS, np.abs(v12 - v24)
    pred = f12 * N_PARENTS
    sig_N, sig_v = np.sqrt(pred), np.sqrt(0.5 / pred)
    print("bins", bins, "\n MC N", N, "\n pred", pred, "\n pull", (N - pred) / sig_N, "\n quad/N", quad_N / pred,
          "\n MC v2", c2, "\n pred v2", v12, "\n pull", (c2 - v12) / sig_v, "\n quad v2", quad_v)
    assert np.all(np.abs(N - pred) <= 4 * sig_N + quad_N)
    assert np.all(np.abs(c2 - v12) <= 4 * sig_v + quad_v)
    assert np.all(N > 1000)


@pytest.mark.parametrize("M,m1,m2,bins", [(0.776, 0.138, 0.138, PT_BINS), (1.232, 0.938, 0.138, PT_BINS),
                                          (1.232, 0.138, 0.938, PT_BINS_SOFT)], ids=["rho-pipi", "Delta-N", "Delta-pi"])
def test_two_body_formula_against_monte_carlo(M, m1, m2, bins):
    """2 x 10^6 parents decayed isotropically; daughters with |y| < 0.5 counted in four pT bins, and their v2.
    Agreement within 4 sigma of the counting error plus the quadrature term |12 - 24 nodes|.  Measured quadrature
    term per bin: rho -> pi pi up to 1.7e-3 of the yield and 7e-4 in v2; Delta -> N below 2e-10 and 6e-6; Delta -> pi
    (softer bins) up to 1.5e-4 and 6e-4.  Largest pull of the three cases: 1.4."""
    rng = np.random.default_rng(20260101)
    parent = draw_parents(rng, M, N_PARENTS)
    Es = (M * M + m1 * m1 - m2 * m2) / (2 * M)
    N, c2 = count_bins(*boost_daughter(rng, parent, M, m1, np.sqrt(Es ** 2 - m1 ** 2)), bins)
    check_against_mc(N, c2, M, m1, [m2], bins)


def test_three_body_formula_against_monte_carlo():
    """omega(0.782) -> 3 pi with a flat Dalitz plot generated by rejection on (E1, E2) -- not through w(s).  Measured:
    quadrature term (12 against 24 nodes in all three rules) up to 1e-4 of a bin's yield and 8e-5 in v2; largest
    pull 2.1."""
    M, m = 0.782, 0.138
    rng = np.random.default_rng(20260102)
    emax = (M * M + m * m - 4 * m * m) / (2 * M)
    E1 = np.empty(N_PARENTS)
    todo = np.arange(N_PARENTS)
    while len(todo):
        e1, e2 = rng.uniform(m, emax, len(todo)), rng.uniform(m, emax, len(todo))
        e3 = M - e1 - e2
        p1, p2 = np.sqrt(e1 ** 2 - m * m), np.sqrt(e2 ** 2 - m * m)
        p3sq = e3 ** 2 - m * m
        ok = (e3 >= m) & (p3sq >= (p1 - p2) ** 2) & (p3sq <= (p1 + p2) ** 2)
        E1[todo[ok]] = e1[ok]
        todo = todo[~ok]
    parent = draw_parents(rng, M, N_PARENTS)
    N, c2 = count_bins(*boost_daughter(rng, parent, M, m, np.sqrt(E1 ** 2 - m * m)), PT_BINS_SOFT)
    check_against_mc(N, c2, M, m, [m, m], PT_BINS_SOFT)


# ------------------------------------------------------------------------------------------
# 3: the emulator against the restatement on grid parents
# ------------------------------------------------------------------------------------------
MASS, CHANNELS = R.CASE_MASS, R.CASE_CHANNELS


def small_case(ny, seed=1):
    """10 pT x 8 phi x ny spectra of decay_ref's eight species, with the four awkward parents of the issue."""
    rng = np.random.default_rng(seed)
    pT = np.linspace(0.1, 3.0, 10) ** 1.3
    phi = np.sort(rng.uniform(0, 2 * np.pi, 8))
    y = np.linspace(-2, 2, ny) if ny > 1 else np.zeros(1)
    return R.case_spectra(pT, phi, y), pT, phi, y


@pytest.mark.parametrize("ny", [1, 5])
def test_emulator_against_restatement(ny):
    S, pT, phi, y = small_case(ny)
    ref, ab, st = R.feeddown(S, MASS, pT, phi, y, CHANNELS)
    got, ab2, st2, slots = R.emulate(S, MASS, pT, phi, y, CHANNELS)
    err = R.parity(got, ref, ab)
    print("ny = %d: parity %.3e, sum |terms| parity %.3e" % (ny, err, R.parity(ab2, ab, ab)))
    assert err < R.BAR
    assert R.parity(ab2, ab, ab) < R.BAR
    assert slots == R.CASE_SLOTS
    assert {k: st2[k] for k in st} == st
    assert not np.array_equal(got[0], S[0]) and np.all(np.isfinite(got))
    # the zero, the negative value, the top-node zeros and the rising last interval reach the interpolation
    R.check_awkward_parents(S, got, lambda S2: R.emulate(S2, MASS, pT, phi, y, CHANNELS)[0])
    R.check_awkward_parents(S, ref, lambda S2: R.feeddown(S2, MASS, pT, phi, y, CHANNELS)[0])


def test_gauss_legendre_nodes_are_computed():
    import ctypes as C
    x, w = np.zeros(12), np.zeros(12)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    R.emulator().decay_gauss_legendre(12, dp(x), dp(w))
    xr, wr = np.polynomial.legendre.leggauss(12)
    # nodes to an ulp; a weight 2 / ((1 - x^2) P'^2) carries the node's ulp amplified by up to ~50 near the ends
    assert np.max(np.abs(x - xr)) < 4e-16 and np.max(np.abs(w - wr)) < 2e-15


# ------------------------------------------------------------------------------------------
# 4: yield conservation, 2+1D, on the pT48 x phi32 Gauss tables
# ------------------------------------------------------------------------------------------
def test_yield_conservation():
    """sum w_pT w_phi dS_1 = b x multiplicity x sum w_pT w_phi S_R for a thermal parent (the pT weights carry the pT
    of pT dpT).  The deficit of the restatement with the exact callable parent is quadrature error (the inner 12-point
    rules and the outer tables); the grid parent adds the interpolation and may have 3 x that.  Measured, rho -> pi pi
    / Delta -> N pi (N) / omega -> 3 pi: see the printed lines (recorded in DESIGN.md 7.6)."""
    (pT, pTw), (phi, phiw) = _data.grid("pT48"), _data.grid("phi32")
    W = pTw[:, None] * phiw[None, :]
    for name, M, b, dau, mult in (("rho", 0.776, 1.0, [0.138, 0.138], 2), ("Delta", 1.232, 0.9, [0.938, 0.138], 1),
                                  ("omega", 0.782, 0.89, [0.138, 0.138, 0.138], 3)):
        mass = np.array([dau[0], M])
        iso = lambda MT, Phi, Y: np.exp(-MT / T) + 0.0 * Phi + 0.0 * Y
        S = np.zeros((2, len(pT), len(phi), 1))
        S[1, :, :, 0] = np.exp(-np.sqrt(pT ** 2 + M ** 2) / T)[:, None]
        want = b * mult * np.sum(W * S[1, :, :, 0])
        exact = sum(R.slot_term(iso, b, M, dau[k], [m for o, m in enumerate(dau) if o != k], pT, phi, [0.0])[0]
                    for k in range(mult))
        deficit_exact = abs(np.sum(W * exact[:, :, 0]) / want - 1.0)
        ch = [R.channel(1, [0 if k < mult else -1 for k in range(len(dau))], b, M, dau)]
        got, _, _, _ = R.emulate(S, mass, pT, phi, [0.0], ch)
        deficit_grid = abs(np.sum(W * (got[0] - S[0])[:, :, 0]) / want - 1.0)
        print("%s: yield deficit exact parent %.3e, grid parent %.3e" % (name, deficit_exact, deficit_grid))
        assert deficit_exact < 1e-2
        assert deficit_grid <= 3 * deficit_exact


# ------------------------------------------------------------------------------------------
# 5: bookkeeping
# ------------------------------------------------------------------------------------------
def flat_case(npart):
    pT = np.linspace(0.2, 2.0, 6)
    phi = np.arange(4) * (np.pi / 2) + 0.1
    S = np.ones((npart, 6, 4, 1)) * np.exp(-pT)[None, :, None, None]
    return S, pT, phi, np.zeros(1)


def test_mass_adjustment_opens_a_closed_channel():
    S, pT, phi, y = flat_case(2)
    mass = np.array([0.5, 0.875])
    # binary fractions, so the rounds are exact: after one round M = 0.9375 = 0.5 + 0.4375 is still closed
    closed = R.channel(1, [0, 0], 1.0, 0.875, [0.5, 0.5], width_parent=0.25, widths=[0.0, 0.125])
    got, _, st, _ = R.emulate(S, mass, pT, phi, y, [closed])
    assert st["adjusted"] == 1 and st["kept"] == 1 and st["skipped_closed"] == 0
    assert np.all(got[0] > S[0])
    # the same channel with the masses the rule ends at: M = 0.875 + 2 x 0.0625, m = (0.5, 0.5 - 2 x 0.0625)
    ref, _, st2, _ = R.emulate(S, mass, pT, phi, y, [R.channel(1, [0, 0], 1.0, 1.0, [0.5, 0.375])])
    assert st2["adjusted"] == 0 and got.tobytes() == ref.tobytes()
    # channels a few ulp above their threshold: p*^2 rounds to <= 0 (closed, counted) or p* is tiny -- never a NaN
    for M in (np.nextafter(1.0, 2.0), 0.95 + 2 ** -52, 1.0 + 1e-12):
        for m in ([0.5, 0.5], [0.5, 0.45]):
            got, _, st, _ = R.emulate(S, mass, pT, phi, y, [R.channel(1, [0, 0], 1.0, M, m)])
            assert np.all(np.isfinite(got)) and st["kept"] + st["skipped_closed"] == 1


def test_zero_widths_are_skipped_not_looped():
    S, pT, phi, y = flat_case(2)
    closed = R.channel(1, [0, 0], 0.7, 0.9, [0.5, 0.5])
    negative = R.channel(1, [0, 0], 0.2, 0.9, [0.5, 5.0], widths=[0.9, 0.0])      # m_1 goes negative first
    got, _, st, _ = R.emulate(S, np.array([0.5, 0.9]), pT, phi, y, [closed, negative])
    assert st["skipped_closed"] == 2 and st["kept"] == 0 and st["adjusted"] == 0
    assert st["branching_skipped"] == pytest.approx(0.9)
    assert np.array_equal(got, S)


def test_many_body_rows_are_counted_with_their_branching():
    S, pT, phi, y = flat_case(2)
    rows = [R.channel(1, [0, 0, 0], 0.25, 1.5, [0.1, 0.1, 0.1], n_body=4), R.channel(1, [0, 0, 0], 0.125, 1.5, [0.1] * 3, n_body=5),
            R.channel(1, [0, 0, 0], 0.5, 0.25, [0.1, 0.1, 0.1])]                  # a closed 3-body channel
    got, _, st, _ = R.emulate(S, np.array([0.1, 1.5]), pT, phi, y, rows)
    assert st["skipped_many_body"] == 2 and st["skipped_closed"] == 1 and st["kept"] == 0
    assert st["branching_skipped"] == pytest.approx(0.875)
    assert np.array_equal(got, S)


def test_chain_gives_both_generations_and_order_does_not_matter():
    S, pT, phi, y = flat_case(3)
    mass = np.array([0.14, 0.6, 1.4])                     # C, B, A
    ab = R.channel(2, [1, 0], 1.0, 1.4, [0.6, 0.14])      # A -> B C
    bc = R.channel(1, [0, 0], 1.0, 0.6, [0.14, 0.14])     # B -> C C
    got, _, st, _ = R.emulate(S, mass, pT, phi, y, [ab, bc])
    assert st["levels"] == 2
    only_b, _, _, _ = R.emulate(S, mass, pT, phi, y, [bc])
    only_a, _, _, _ = R.emulate(S, mass, pT, phi, y, [ab])
    assert np.all(got[0] > only_b[0] + (only_a[0] - S[0]) * (1 - 1e-12))     # C also got A's Bs' daughters
    ref, _, _ = R.feeddown(S, mass, pT, phi, y, [ab, bc])
    assert np.allclose(got, ref, rtol=1e-9)
    rev, _, _, _ = R.emulate(S, mass, pT, phi, y, [bc, ab])
    assert got.tobytes() == rev.tobytes()
    many = [R.channel(2, [1, 0], 0.5, 1.4, [0.6, 0.14]), R.channel(2, [0, 0], 0.3, 1.4, [0.14, 0.14]), bc,
            R.channel(2, [0, 1, 0], 0.2, 1.4, [0.14, 0.6, 0.14])]
    a, _, _, _ = R.emulate(S, mass, pT, phi, y, many)
    b, _, _, _ = R.emulate(S, mass, pT, phi, y, many[::-1])
    assert a.tobytes() == b.tobytes()


def test_cycle_and_bad_rows_are_refused():
    S, pT, phi, y = flat_case(2)
    mass = np.array([0.5, 1.2])
    with pytest.raises(ValueError, match="cycle"):
        R.emulate(S, mass, pT, phi, y, [R.channel(1, [0, 0], 1.0, 1.2, [0.5, 0.5]), R.channel(0, [1, -1], 1.0, 3.0, [1.2, 0.1])])
    with pytest.raises(ValueError, match="cycle"):
        R.emulate(S, mass, pT, phi, y, [R.channel(1, [1, 0], 1.0, 1.2, [0.1, 0.5])])
    with pytest.raises(ValueError, match="n_body"):
        R.emulate(S, mass, pT, phi, y, [R.channel(1, [0, 0], 1.0, 1.2, [0.5, 0.5], n_body=0)])
    with pytest.raises(ValueError, match="out of range"):
        R.emulate(S, mass, pT, phi, y, [R.channel(1, [0, 2], 1.0, 1.2, [0.5, 0.5])])
    with pytest.raises(ValueError, match="out of range"):
        R.emulate(S, mass, pT, phi, y, [R.channel(2, [0, 0], 1.0, 1.2, [0.5, 0.5])])
    with pytest.raises(ValueError, match="pT"):
        R.emulate(S, mass, np.concatenate([[0.0], pT[1:]]), phi, y, [])
    with pytest.raises(ValueError, match="phi"):
        R.emulate(S, mass, pT, phi[::-1].copy(), y, [])


def test_three_body_channel_at_its_threshold_is_closed_not_nan():
    """A 3-body channel a few ulp above M = m1 + m2 + m3 has no positive s-rule norm or p* in floating point: it is
    skipped and counted like a closed one; a little further up it is kept and finite."""
    S, pT, phi, y = flat_case(2)
    mass = np.array([0.25, 0.75])
    for M in (0.75, np.nextafter(0.75, 1.0), 0.75 + 2 ** -50, 0.75 + 1e-13, 0.75 + 1e-9, 0.76):
        for m in ([0.25, 0.25, 0.25], [0.25, 0.125, 0.375]):
            ch = [R.channel(1, [0, 0, 0], 0.5, M, m)]
            got, _, st, _ = R.emulate(S, mass, pT, phi, y, ch)
            assert np.all(np.isfinite(got)), (M, m)
            assert st["kept"] + st["skipped_closed"] == 1
            assert R.kept_channels(ch)[1]["kept"] == st["kept"]
            if st["kept"] == 0:
                assert np.array_equal(got, S) and st["branching_skipped"] == 0.5
            else:
                assert np.all(got[0] > S[0])
    assert R.emulate(S, mass, pT, phi, y, [R.channel(1, [0, 0, 0], 0.5, 0.75, [0.25] * 3)])[2]["skipped_closed"] == 1
    assert R.emulate(S, mass, pT, phi, y, [R.channel(1, [0, 0, 0], 0.5, 0.76, [0.25] * 3)])[2]["kept"] == 1


def test_unused_slots_of_a_two_body_row_do_not_matter():
    """daughter[2], mass[2] and width[2] of a 2-body row are the caller's leftovers: any values, in range or not, give
    the same bytes, in either listing order."""
    S, pT, phi, y = flat_case(3)
    mass = np.array([0.14, 0.3, 1.4])
    rows = [R.channel(2, [0, 1], 0.5, 1.4, [0.14, 0.3]), R.channel(2, [0, 1], 0.3, 1.4, [0.14, 0.3]),
            R.channel(2, [1, 1], 0.25, 1.4, [0.3, 0.3])]
    clean = R.channel_table(rows)
    want = R.emulate(S, mass, pT, phi, y, clean)[0]
    for fill in ((7, 99, -5), (-3, 2, 12345)):
        dirty = clean.copy()
        dirty["daughter"][:, 2] = fill
        dirty["mass"][:, 2] = (3.0, 0.5, -1.0)
        dirty["width"][:, 2] = (0.1, 9.0, 0.0)
        assert R.emulate(S, mass, pT, phi, y, dirty)[0].tobytes() == want.tobytes()
        assert R.emulate(S, mass, pT, phi, y, dirty[::-1].copy())[0].tobytes() == want.tobytes()


def smash_rows():
    d = dict(np.load(os.path.join(HERE, "golden", "decays_smash.npz")))
    return d


def test_antibaryon_rule():
    """readindata.cpp:1035-1056: the antibaryon's daughters are negated, except neutral non-strange mesons."""
    d = smash_rows()
    rows, parts = hrg.decay_rows_with_antibaryons(d, d)
    assert len(d["row_mcid"]) == 1706 and set(d["row_n_body"].tolist()) == {1, 2}

    def channels_of(mcid):
        return sorted(tuple(int(v) for v in ds[:2]) for m, nb, ds in zip(rows["row_mcid"], rows["row_n_body"], rows["row_daughters"])
                      if m == mcid and nb == 2)

    delta_pp, delta_0 = channels_of(2224), channels_of(2114)          # Delta++ -> p pi+, Delta0 -> n pi0 | p pi-
    assert (211, 2212) in [tuple(sorted(c)) for c in delta_pp]
    assert sorted(tuple(sorted(c)) for c in channels_of(-2224)) == sorted(tuple(sorted((-a, -b))) for a, b in delta_pp)
    anti0 = [tuple(sorted(c)) for c in channels_of(-2114)]
    assert (-2112, 111) in anti0 and (-2212, 211) in anti0            # pi0 stays, pi- -> pi+
    assert (111, 2112) in [tuple(sorted(c)) for c in delta_0]
    lam = [tuple(sorted(c)) for c in channels_of(3124)]               # Lambda(1520) -> N Kbar
    alam = [tuple(sorted(c)) for c in channels_of(-3124)]
    assert (-321, 2212) in lam and (-2212, 321) in alam               # p K-  ->  pbar K+
    assert (-311, 2112) in lam and (-2112, 311) in alam               # n Kbar0 -> nbar K0: a neutral strange meson flips
    # and through the chosen list: indices, masses and widths
    mcids = hrg.chosen_mcids("smash")
    ch = hrg.decay_channels(d, d, mcids)
    i = {int(m): k for k, m in reversed(list(enumerate(mcids)))}
    sel = ch[(ch["parent"] == i[-2224]) & (ch["n_body"] == 2)]
    assert len(sel) == len(delta_pp) and sorted(sel[0]["daughter"][:2].tolist()) == sorted([i[-2212], i[-211]])
    assert sel[0]["mass_parent"] == pytest.approx(1.232) and sel[0]["width_parent"] > 0.1


# ------------------------------------------------------------------------------------------
# 6: the host reader
# ------------------------------------------------------------------------------------------
def test_host_reader_returns_the_fixture_channels(tmp_path):
    """A run directory written with the fixture's decay rows: read_pdg (through is3d_host_read_decays) returns the
    rows of the fixture with the antibaryon rows generated, i.e. what hrg.decay_rows_with_antibaryons builds."""
    from is3d2_amd import host, rundir, synth
    d = smash_rows()
    run = rundir.write_run_dir(str(tmp_path), synth.surface(4, seed=1), dict(dimension=2, df_mode=1), hrg_eos=2,
                               chosen="pikp", decays=d)
    got = host.read_decays(run, 2)
    want, _ = hrg.decay_rows_with_antibaryons(d, d)
    assert len(got["row_mcid"]) == len(want["row_mcid"]) > 1706
    for k in ("row_mcid", "row_n_body", "row_daughters"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["row_branching"], want["row_branching"])
    # the particle list itself is what it was without the rows
    plain = rundir.write_run_dir(str(tmp_path / "plain"), synth.surface(4, seed=1), dict(dimension=2, df_mode=1), hrg_eos=2,
                                 chosen="pikp")
    a, b = host.read_pdg(run, 2), host.read_pdg(plain, 2)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert len(host.read_decays(plain, 2)["row_mcid"]) == 0


def test_urqmd_subset_has_three_and_four_body_rows():
    """The UrQMD rows (parents below 1.45 GeV) through the builder and the emulator on a tiny grid: 3-body channels
    are kept, 4-body rows are skipped and counted with their branching, the negative body counts of that table read
    as their magnitude."""
    d = dict(np.load(os.path.join(HERE, "golden", "decays_urqmd_subset.npz")))
    assert {3, 4} <= set(np.abs(d["row_n_body"]).tolist()) and (d["row_n_body"] < 0).any()
    mcids = hrg.chosen_mcids("urqmd")
    ch = hrg.decay_channels(d, d, mcids)
    assert ch["n_body"].min() >= 1
    parts = hrg.pdg_particles(1)
    mass = hrg.chosen_species(parts, mcids)["mass"]
    S, pT, phi, y = flat_case(len(mcids))
    got, ab, st, slots = R.emulate(S, mass, pT, phi, y, ch)
    many = ch["n_body"] >= 4
    assert st["skipped_many_body"] == many.sum() > 0
    assert st["kept"] + st["skipped_closed"] == ((ch["n_body"] == 2) | (ch["n_body"] == 3)).sum()
    assert st["kept"] >= (ch["n_body"] == 3).sum() - st["skipped_closed"] > 0
    assert st["branching_skipped"] >= ch["branching"][many].sum() * (1 - 1e-12)
    assert np.all(np.isfinite(got)) and slots > 0
    pip = int(np.nonzero(mcids == 211)[0][0])
    assert np.all(got[pip] > S[pip])
