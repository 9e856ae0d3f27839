"""CPU tier of the four-body decay channels (is3d_set_decays4): the changed headers run on the
host (tests/native/decay4_emulator.cpp and the two older emulators) against the parent commit's recorded results, an
independent flat four-body generator (massive RAMBO) and the density h(s) written from its statement
(tests/decay4_ref.py).
"""
import os

import numpy as np
import pytest

import decay4_ref as D
import decay_list_ref as L
import decay_ref as R
from is3d2_amd import hrg

HERE = os.path.dirname(os.path.abspath(__file__))
MASS = D.MASS
PULL = 5.0


def fourbody_rows():
    return dict(np.load(os.path.join(HERE, "golden", "decays_urqmd_fourbody.npz")))


def row_masses(d):
    """[(M, m[4])] of the 21 rows of the UrQMD fixture."""
    mass = {int(m): float(v) for m, v in zip(d["p_mcid"], d["p_mass"])}
    return [(mass[int(p)], [mass[int(x)] for x in ds[:4]]) for p, ds in zip(d["row_mcid"], d["row_daughters"])]


def at_rest(species, n, event=0):
    return L.make_list(np.full(n, species), MASS, pT=np.zeros(n), phi=np.zeros(n), y=np.zeros(n), event=event)


def only(channel):
    return [dict(channel, branching=1.0)]


# ------------------------------------------------------------------------------------------
# 1: nothing changes without a four-body row
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["smash", "case8"])
def test_without_four_body_rows_everything_is_the_parents(name):
    """The three-slot call (the two older emulators over the changed headers, and the four-slot table with the
    keep-four-body flag off), and the four-slot call on a table without a 4-body row: the Monte Carlo channel table,
    the plan statistics, the feed-down and the decayed list are, byte for byte, what the parent commit's emulators
    gave (tests/golden/decay4_parent_*.npz, tools/record_decay_parent.py)."""
    mass, ch, S, pT, phi, y, prim, offsets, seed = D.parent_cases()[name]
    g = np.load(os.path.join(HERE, "golden", "decay4_parent_%s.npz" % name))
    keys = [str(k) for k in g["plan_stat_keys"]]
    assert (np.abs(ch["n_body"]) < 4).all()
    # the older emulators: is3d_set_decays' build_plan
    fd, ab, st, slots = R.emulate(S, mass, pT, phi, y, ch)
    out, off, origins, lst, pst = L.emulate(mass, ch, prim, offsets, seed)
    kept, level = L.mc_channels(mass, ch)
    assert fd.tobytes() == g["feeddown"].tobytes() and ab.tobytes() == g["sum_abs"].tobytes() and slots == int(g["slots"])
    assert np.array_equal([float(st[k]) for k in keys], g["plan_stats"])
    assert out.tobytes() == g["list"].tobytes() and np.array_equal(off, g["offsets"]) and np.array_equal(origins, g["origins"])
    assert np.array_equal([lst[k] for k in L.STAT_KEYS], g["list_stats"])
    assert np.array_equal(np.array([[c["parent"], c["nbody"]] + c["d"] for c in kept]).reshape(-1, 5), g["chan_ints"])
    assert np.array([[c["cum"], c["M"]] + c["m"] + c["k"] for c in kept]).reshape(-1, 8).tobytes() == g["chan_dbls"].tobytes()
    assert np.array_equal(level, g["level"])
    # the four-slot table, flag off and flag on
    for keep_four in (False, True):
        fd4, ab4, st4, slots4, terms = D.emulate_feeddown(S, mass, pT, phi, y, ch, keep_four=keep_four)
        assert fd4.tobytes() == g["feeddown"].tobytes() and ab4.tobytes() == g["sum_abs"].tobytes() and slots4 == slots
        assert np.array_equal([float(st4[k]) for k in keys], g["plan_stats"])
        out4, off4, origins4, lst4, _ = D.emulate_list(mass, ch, prim, offsets, seed, keep_four=keep_four)
        assert out4.tobytes() == g["list"].tobytes() and np.array_equal(off4, g["offsets"]) and np.array_equal(origins4, g["origins"])
        assert np.array_equal([lst4[k] for k in L.STAT_KEYS], g["list_stats"])
        ints, dbls, level4, _ = D.mc_channels(mass, ch, keep_four=keep_four)
        assert np.array_equal(ints[:, :5], g["chan_ints"]) and np.all(ints[:, 5] == -1)
        assert dbls[:, [0, 1, 2, 3, 4, 6, 7, 8]].tobytes() == g["chan_dbls"].tobytes() and np.all(dbls[:, 5] == 0)
        assert np.array_equal(level4, g["level"])


# ------------------------------------------------------------------------------------------
# 2: single four-body decays
# ------------------------------------------------------------------------------------------
CONFIGS = [(0.0, 0.0), (0.0, 1.5), (0.7, 4.0), (0.7, -4.0), (2.5, 0.3)]
N_EACH = 20000


@pytest.mark.parametrize("channel,emitted", [(D.R_4A, 4), (D.H_ABXC, 3)], ids=["R-4a", "H-abXc"])
def test_single_four_body_decay(channel, emitted):
    """10^5 decays each of R -> a a a a and of a parent -> a b X c (X not chosen; the parent is H, because with the
    case table's masses R -> a b X c is closed: 0.14 + 0.50 + 0.30 + 0.94 > 1.60), parents at rest, at pT = 0, at y = +-4 and
    at a generic point.  Mass shell: 8 ulp of E^2 (tests/test_decay_list_cpu.py's argument: E is the last operation).

    Sum of the four daughters against the parent, in ulp(E_R): tests/test_decay_list_cpu.py derives 64 for a 2-body
    decay (two daughters, one boost each) and 128 for a 3-body one, whose daughters 2 and 3 are boosted twice, the
    outer boost carrying the inner one's error with a factor bounded by 2.  The four-body chain nests once more
    (daughters 3 and 4 are boosted three times: out of the (34) frame, out of the (234) frame, into the lab), so the
    same factor gives 256.  Measured here: 4 (R -> 4a) and 3 (H -> a b X c), summed with X kept as a sixth species.
    The -1 daughter is dropped and counted: with the table as given the same decays leave three records each, the
    same bytes, and dropped_daughters = decays."""
    pT, y = np.repeat([c[0] for c in CONFIGS], N_EACH), np.repeat([c[1] for c in CONFIGS], N_EACH)
    phi = np.random.default_rng(3).uniform(0, 2 * np.pi, len(pT))
    par = L.make_list(np.full(len(pT), channel["parent"]), MASS, pT=pT, phi=phi, y=y)
    # X chosen as a sixth species: the same decays with every daughter kept give the full sum
    mass6 = np.append(MASS, D.M_X)
    full = dict(channel, branching=1.0, daughter=[5 if d < 0 else d for d in channel["daughter"]])
    out, off, orig, st, _ = D.emulate_list(mass6, [full], par, [0, len(par)], 11)
    assert st["decays"] == len(par) and st["capped"] == 0 and st["undecayed"] == 0 and st["dropped_daughters"] == 0
    assert len(out) == 4 * len(par) and np.array_equal(orig, np.repeat(np.arange(len(par)), 4))
    assert np.array_equal(out["species"].reshape(-1, 4), np.tile(full["daughter"], (len(par), 1)))
    m = mass6[out["species"]]
    shell = np.abs(out["E"] ** 2 - out["px"] ** 2 - out["py"] ** 2 - out["pz"] ** 2 - m * m) / L.ulp(out["E"] ** 2)
    assert shell.max() <= 8
    sums = L.tree_sums(out, orig, len(par))
    want = np.stack([par[f] for f in ("E", "px", "py", "pz")], axis=1)
    err = np.abs(sums - want) / L.ulp(par["E"])[:, None]
    print("max |sum p - P| in ulp(E_R) per config:", err.reshape(len(CONFIGS), N_EACH, 4).max(axis=(1, 2)))
    assert err.max() <= 256
    for f in ("tau", "x", "y", "eta", "t", "z", "cell", "event"):
        assert np.array_equal(out[f], par[f][orig])
    # the table as given: the daughter that is not chosen is dropped and counted, the others are the same bytes
    got, off, orig2, st2, _ = D.emulate_list(MASS, only(channel), par, [0, len(par)], 11)
    keep = out["species"] != 5
    assert st2["decays"] == len(par) and st2["dropped_daughters"] == (4 - emitted) * len(par) and len(got) == emitted * len(par)
    assert got.tobytes() == out[keep].tobytes() and np.array_equal(orig2, orig[keep])


# ------------------------------------------------------------------------------------------
# 3, 4: flat four-body phase space
# ------------------------------------------------------------------------------------------
def pair_mass(a, b):
    return np.sqrt((a["E"] + b["E"]) ** 2 - (a["px"] + b["px"]) ** 2 - (a["py"] + b["py"]) ** 2 - (a["pz"] + b["pz"]) ** 2)


def two_sample(x1, x2, edges, w2=None):
    """Per-bin pulls of two samples' histograms (the second may be weighted and is scaled to the first's total):
    (n1 - s n2) / sqrt(n1 + s^2 sum w2^2)."""
    n1 = np.histogram(x1, bins=edges)[0].astype(float)
    w2 = np.ones(len(x2)) if w2 is None else w2
    n2, v2 = np.histogram(x2, bins=edges, weights=w2)[0], np.histogram(x2, bins=edges, weights=w2 * w2)[0]
    s = n1.sum() / n2.sum()
    return (n1 - s * n2) / np.sqrt(n1 + s * s * v2)


def chain_generator(rng, M, m, n, weighted):
    """A sequential generator in numpy: (M234, M34) uniform over the allowed triangle, three isotropic two-body
    splits; weighted = True keeps a decay with probability p1 p2 p3 / w_max (flat phase space), False keeps every
    one (the wrong weight).  Returns the rest-frame momenta [k][4][4] = (E, px, py, pz)."""
    def pstar(W, a, b):
        return np.sqrt(np.maximum((W * W - (a + b) ** 2) * (W * W - (a - b) ** 2), 0.0)) / (2 * W)

    K = M - sum(m)
    u = np.sort(rng.uniform(size=(n, 2)), axis=1)
    w34, w234 = m[2] + m[3] + u[:, 0] * K, m[1] + m[2] + m[3] + u[:, 1] * K
    p1, p2, p3 = pstar(M, m[0], w234), pstar(w234, m[1], w34), pstar(w34, m[2], m[3])
    if weighted:
        wmax = pstar(M, m[0], m[1] + m[2] + m[3]) * pstar(M - m[0], m[1], m[2] + m[3]) * pstar(M - m[0] - m[1], m[2], m[3])
        ok = rng.uniform(size=n) * wmax < p1 * p2 * p3
        w34, w234, p1, p2, p3 = w34[ok], w234[ok], p1[ok], p2[ok], p3[ok]

    def split(P, W, ma, p):       # P[k][4] of mass W -> (a, rest)
        k = len(p)
        ct, ph = rng.uniform(-1, 1, k), rng.uniform(0, 2 * np.pi, k)
        st = np.sqrt(1 - ct * ct)
        q = np.stack([p * st * np.cos(ph), p * st * np.sin(ph), p * ct], axis=1)
        ea = np.sqrt(ma * ma + p * p)
        a = D.boost_to((P[:, 0], P[:, 1], P[:, 2], P[:, 3]), W, np.concatenate([ea[:, None], q], axis=1)[:, None, :])[:, 0]
        return a, P - a

    k = len(p1)
    P0 = np.zeros((k, 4))
    P0[:, 0] = M
    d1, S = split(P0, M, m[0], p1)
    d2, T = split(S, w234, m[1], p2)
    d3, d4 = split(T, w34, m[2], p3)
    return np.stack([d1, d2, d3, d4], axis=1)


def test_four_body_decays_are_flat():
    """2 x 10^5 R -> 4a decays at rest from the emulator.  In flat phase space of four equal masses the six pair
    masses m_ij have one distribution and the four energies one spectrum; the chain R -> 1 (234), (234) -> 2 (34),
    (34) -> 3 4 treats the daughters differently, so only the right weight p1 p2 p3 makes them agree.
    (12) against (34) and against (14): two-sample pulls in 20 bins; the four energy spectra against each other and
    against the weighted histogram of massive RAMBO, which has no sequential masses at all.  Every pull below 5 of
    the counting error.  Measured largest pulls: pair masses 2.05, energies among themselves 2.71, against RAMBO 2.14.
    The same chain in numpy with every (M234, M34) kept (the wrong weight) fails (12) against (34): pull 63.5, while
    with the right weight it passes too (1.74)."""
    n, M, m = 200_000, 1.60, 0.14
    out, off, orig, st, _ = D.emulate_list(MASS, only(D.R_4A), at_rest(D.R_, n), [0, n], 2024)
    assert st["decays"] == n and st["capped"] == 0 and len(out) == 4 * n
    d = [out[k::4] for k in range(4)]
    edges = np.linspace(2 * m, M - 2 * m, 21)
    m12, m34, m14 = pair_mass(d[0], d[1]), pair_mass(d[2], d[3]), pair_mass(d[0], d[3])
    pm = max(np.abs(two_sample(m12, m34, edges)).max(), np.abs(two_sample(m12, m14, edges)).max())
    e_edges = np.linspace(m, (M * M + m * m - 9 * m * m) / (2 * M), 21)
    pe = max(np.abs(two_sample(d[a]["E"], d[b]["E"], e_edges)).max() for a in range(4) for b in range(a + 1, 4))
    p, wt = D.rambo(np.random.default_rng(5), M, [m] * 4, 400_000)
    assert np.allclose(p.sum(axis=1), [M, 0, 0, 0], atol=1e-12)
    pr = max(np.abs(two_sample(d[k]["E"], p[:, k, 0], e_edges, wt)).max() for k in range(4))
    # the generators of this file against RAMBO, so that the failing case below is the weight's doing
    good = chain_generator(np.random.default_rng(6), M, [m] * 4, 3 * n, True)
    bad = chain_generator(np.random.default_rng(6), M, [m] * 4, n, False)

    def m_of(q, i, j):
        s = q[:, i] + q[:, j]
        return np.sqrt(s[:, 0] ** 2 - np.sum(s[:, 1:] ** 2, axis=1))

    pg = np.abs(two_sample(m_of(good, 0, 1), m_of(good, 2, 3), edges)).max()
    pb = np.abs(two_sample(m_of(bad, 0, 1), m_of(bad, 2, 3), edges)).max()
    print("largest pulls: pair masses %.2f, energies %.2f, against RAMBO %.2f; numpy chain right weight %.2f, wrong weight %.2f"
          % (pm, pe, pr, pg, pb))
    assert pm < PULL and pe < PULL and pr < PULL and pg < PULL
    assert pb > 2 * PULL


def test_recoil_mass_follows_the_feeddown_density():
    """The M234^2 = M^2 + m1^2 - 2 M E1 histogram of the emulator's R -> 4a decays against the feed-down's density
    h(s) = sqrt(lambda(M^2, m1^2, s)) Phi3(s) (decay4_ref.h_density, from its statement), normalised over the s range
    and integrated over each of 20 bins: every pull below 5.  This ties the list decays and the plan together.
    Measured largest pull: 1.97."""
    n, M, m = 200_000, 1.60, 0.14
    out, off, orig, st, _ = D.emulate_list(MASS, only(D.R_4A), at_rest(D.R_, n), [0, n], 77)
    s = M * M + m * m - 2 * M * out[0::4]["E"]
    lo, hi = 9 * m * m, (M - m) ** 2
    edges = np.linspace(lo, hi, 21)
    x, w = np.polynomial.legendre.leggauss(16)
    mu = np.array([np.sum(0.5 * (b - a) * w * D.h_density(a + 0.5 * (b - a) * (1 + x), M, m, [m] * 3)) for a, b in zip(edges[:-1], edges[1:])])
    mu *= n / mu.sum()
    H = np.histogram(s, bins=edges)[0]
    pull = (H - mu) / np.sqrt(mu)
    print("M234^2 pulls", np.round(pull, 2))
    assert H.sum() == n and np.abs(pull).max() < PULL
    # and the other slots of the chain see the same density
    for k in (1, 3):
        sk = M * M + m * m - 2 * M * out[k::4]["E"]
        assert np.abs((np.histogram(sk, bins=edges)[0] - mu) / np.sqrt(mu)).max() < PULL


# ------------------------------------------------------------------------------------------
# 5, 6: the feed-down's s rule
# ------------------------------------------------------------------------------------------
def bin_terms(M, mk, s_nodes, bins=L.PT_BINS):
    """T[j][bin]: the two-body term with W^2 = s_j (unit branching, the exact thermal parent with v2) integrated
    over each pT bin and phi, per parent -- tests/decay_list_ref.predict_bins for one s node at a time."""
    x, w = np.polynomial.legendre.leggauss(8)
    phi = np.arange(8) * (2 * np.pi / 8)
    norm = 2 * L.Y_MAX * 2 * np.pi * L.T * (M + L.T) * np.exp(-M / L.T)
    T = np.zeros((len(s_nodes), len(bins) - 1))
    V = np.zeros_like(T)
    for j, sj in enumerate(s_nodes):
        for b, (lo, hi) in enumerate(zip(bins[:-1], bins[1:])):
            pT = 0.5 * (lo + hi) + 0.5 * (hi - lo) * x
            dS, _ = R.two_body(L.thermal, 1.0, M, mk, sj, pT, phi, [0.0], 12)
            f = dS[:, :, 0] * (pT * w * 0.5 * (hi - lo))[:, None] * (2 * np.pi / 8)
            T[j, b] = f.sum() / norm
            V[j, b] = (f * np.cos(2 * phi)[None, :]).sum() / norm
    return T, V


def test_phi3_rule_is_converged_for_every_urqmd_row():
    """The plan's weights w_j of every slot of the 21 UrQMD four-body rows with the inner rule of 24 nodes against
    the same with 48, and against the numpy statement (400 nodes, another substitution).  The bar is the change of
    the slot's summed term (thermal parent, four pT bins) that the weights' difference causes: it must stay below the
    slot's own 12-against-24-node term of the s rule, the error scale of DESIGN.md 7.6.
    Measured: largest |w_24 - w_48| = 5.5e-14 (the rule is converged to rounding; against numpy 5.5e-14), its
    effect on a term at most 1.1e-13 of the term, against a 12 / 24 quadrature term of 1.4e-4 .. 1.7e-4 of the term."""
    rows = row_masses(fourbody_rows())
    assert len(rows) == 21
    worst_w = worst_np = 0.0
    seen = {}
    for M, m in rows:
        for k in range(4):
            others = [m[o] for o in range(4) if o != k]
            key = (M, m[k], tuple(others))
            if key in seen:         # the same masses give the same weights: all four pions weigh 0.138
                continue
            s24, w24 = D.slot_weights(M, m[k], others, 24)
            s48, w48 = D.slot_weights(M, m[k], others, 48)
            sn, wn = D.four_body_nodes(M, m[k], others, 12)
            assert np.array_equal(s24, s48) and np.allclose(s24, sn, rtol=1e-13) and abs(w24.sum() - 1) < 1e-14
            worst_w, worst_np = max(worst_w, np.abs(w24 - w48).max()), max(worst_np, np.abs(w24 - wn).max())
            T12, _ = bin_terms(M, m[k], s24)
            s2, w2 = D.four_body_nodes(M, m[k], others, 24)
            T24, _ = bin_terms(M, m[k], s2)
            term, quad = w24 @ T12, np.abs(w24 @ T12 - w2 @ T24)
            effect = np.abs((w24 - w48) @ T12)
            seen[key] = (effect / term, quad / term)
            assert np.all(effect < quad), key
    print("largest |w24 - w48| %.3g, |w24 - numpy| %.3g" % (worst_w, worst_np))
    for key, (e, q) in seen.items():
        print(" M %.3f: effect / term %s, 12|24 quadrature / term %s" % (key[0], ["%.2g" % v for v in e], ["%.2g" % v for v in q]))
    assert worst_np < 1e-10


def test_feeddown_formula_against_monte_carlo():
    """Thermal R (T = 0.15, v2 = 0.1) -> a a a a: 2 x 10^6 parents decayed by massive RAMBO (weighted events), slot-0
    daughters counted in |y| < 0.5 in four pT bins with their v2, against the feed-down terms with the emulator's own
    weights (plan nodes s_j, w_j): within 4 sigma of the weighted counting error plus the 12-against-24-node term."""
    M, m, n = 1.60, 0.14, 2_000_000
    rng = np.random.default_rng(12)
    bins = L.PT_BINS_SOFT          # the pions of a four-body decay are soft: above 1.2 GeV too few arrive to count
    N, C2, V = np.zeros(4), np.zeros(4), np.zeros(4)
    wsum = 0.0
    for _ in range(8):
        k = n // 8
        p, wt = D.rambo(rng, M, [m] * 4, k)
        lab = D.boost_to(L.draw_parents(rng, M, k), M, p[:, :1])[:, 0]
        pT, phi = np.hypot(lab[:, 1], lab[:, 2]), np.arctan2(lab[:, 2], lab[:, 1])
        y = 0.5 * np.log((lab[:, 0] + lab[:, 3]) / (lab[:, 0] - lab[:, 3]))
        wsum += wt.sum()
        sel = np.abs(y) < 0.5
        b = np.digitize(pT[sel], bins) - 1
        ok = (b >= 0) & (b < 4)
        N += np.bincount(b[ok], weights=wt[sel][ok], minlength=4)
        V += np.bincount(b[ok], weights=wt[sel][ok] ** 2, minlength=4)
        C2 += np.bincount(b[ok], weights=wt[sel][ok] * np.cos(2 * phi[sel][ok]), minlength=4)
    frac, sig, v2 = N / wsum, np.sqrt(V) / wsum, C2 / N
    sig_v = np.sqrt(0.5 * V) / N
    s12, w12 = D.slot_weights(M, m, [m] * 3)
    T12, V12 = bin_terms(M, m, s12, bins)
    s24, w24 = D.four_body_nodes(M, m, [m] * 3, 24)
    T24, V24 = bin_terms(M, m, s24, bins)
    f12, f24 = w12 @ T12, w24 @ T24
    v12, v24 = (w12 @ V12) / f12, (w24 @ V24) / f24
    print("fraction per bin", frac, "\n formula", f12, "\n pull", (frac - f12) / sig, "\n quadrature", np.abs(f12 - f24),
          "\n v2", v2, "\n formula", v12, "\n pull", (v2 - v12) / sig_v)
    assert np.all(N * N / V > 1000)          # effective counts
    assert np.all(np.abs(frac - f12) <= 4 * sig + np.abs(f12 - f24))
    assert np.all(np.abs(v2 - v12) <= 4 * sig_v + np.abs(v12 - v24))


# ------------------------------------------------------------------------------------------
# 7: statistics and the level bound
# ------------------------------------------------------------------------------------------
def test_statistics_of_the_four_slot_call():
    """The UrQMD subset fixture through hrg.decay_channels(four_body=True): no row is skipped as many-body, kept
    grows by the open 4-body rows and branching_skipped falls by their branching; a 5-body row is still skipped and
    counted; the default of decay_channels is the three-slot table it was."""
    d = dict(np.load(os.path.join(HERE, "golden", "decays_urqmd_subset.npz")))
    mcids = hrg.chosen_mcids("urqmd")
    mass = hrg.chosen_species(hrg.pdg_particles(1), mcids)["mass"]
    ch3, ch4 = hrg.decay_channels(d, d, mcids), hrg.decay_channels(d, d, mcids, four_body=True)
    from is3d2_amd import _lib
    assert ch3.dtype == _lib.DECAY_DTYPE and ch4.dtype == _lib.DECAY4_DTYPE and len(ch3) == len(ch4)
    for k in ("parent", "n_body", "branching", "mass_parent", "width_parent"):
        assert np.array_equal(ch3[k], ch4[k])
    assert all(np.array_equal(ch3[k], ch4[k][:, :3]) for k in ("daughter", "mass", "width"))
    four = ch4["n_body"] == 4
    assert four.sum() == 9 and np.all(ch4["daughter"][four, 3] >= 0) and np.all(ch4["mass"][four, 3] > 0)
    assert np.all(ch4["daughter"][~four, 3] == -1)
    S = np.ones((len(mass), 3, 2, 1))
    grid = (np.array([0.3, 1.0, 2.0]), np.array([0.0, np.pi]), np.array([0.0]))
    _, _, st3, slots3, terms3 = D.emulate_feeddown(S, mass, *grid, ch4, keep_four=False)
    _, _, st4, slots4, terms4 = D.emulate_feeddown(S, mass, *grid, ch4, keep_four=True)
    assert st3["skipped_many_body"] == 9 and st4["skipped_many_body"] == 0
    assert st4["skipped_closed"] == st3["skipped_closed"]          # every one of the nine is open
    assert st4["kept"] == st3["kept"] + 9
    assert st4["branching_skipped"] == pytest.approx(st3["branching_skipped"] - ch4["branching"][four].sum(), abs=1e-12)
    assert slots4 == slots3 + 36 and terms4 == terms3 + 36 * 12
    # a 5-body row is skipped and counted whatever its first four daughters are; a closed 4-body row counts as closed
    five = D.channel4(D.R_, [D.A_] * 4, 0.05, 1.60, [0.14] * 4, n_body=5)
    closed = D.channel4(D.R_, [D.C_, D.B_, D.A_, D.A_], 0.05, 1.60, [0.94, 0.50, 0.14, 0.14])
    _, _, st, _, _ = D.emulate_feeddown(np.ones((5, 3, 2, 1)), MASS, *grid, D.CHANNELS + [five, closed])
    assert (st["kept"], st["skipped_many_body"], st["skipped_closed"]) == (3, 1, 3)      # R -> a b X c and H -> R c are closed
    assert st["branching_skipped"] == pytest.approx(0.05 + 0.05 + 0.3 + 0.4)
    _, _, st, _, _ = D.emulate_feeddown(np.ones((5, 3, 2, 1)), MASS, *grid, D.CHANNELS + [five, closed], keep_four=False)
    assert (st["kept"], st["skipped_many_body"], st["skipped_closed"]) == (1, 5, 1)


def deep_table(levels):
    """A chain of `levels` species, k -> (k - 1) (k - 1), whose top decays to four of the next: (mass, channels)."""
    mass = 0.1 * 4.5 ** np.arange(levels + 1)
    ch = [D.channel4(k, [k - 1, k - 1], 1.0, mass[k], [mass[k - 1]] * 2) for k in range(1, levels)]
    ch.append(D.channel4(levels, [levels - 1] * 4, 1.0, mass[levels], [mass[levels - 1]] * 4))
    return mass, ch


def test_level_bound_with_a_four_body_channel():
    """Slot 3 of node c has the code 4 c + 4: at depth 16 the largest code passes 2^32, so a plan that holds a
    four-body channel has at most 15 levels; without one the bound stays 16."""
    assert 4 * (4 ** 15 - 1) // 3 < 2 ** 32 < 4 * (4 ** 16 - 1) // 3
    for levels, ok in ((15, True), (16, False)):
        mass, ch = deep_table(levels)
        par = L.make_list(np.array([0]), mass, pT=np.array([0.5]), phi=np.array([0.0]), y=np.array([0.0]))
        if ok:
            out, _, _, st, pst = D.emulate_list(mass, ch, par, [0, 1], 1)
            assert pst["levels"] == 15 and st["decays"] == 0
        else:
            with pytest.raises(ValueError, match="4-body channel and has 16 levels"):
                D.emulate_list(mass, ch, par, [0, 1], 1)
            # the same 16 levels without the four-body channel pass
            ch2 = ch[:-1] + [D.channel4(16, [15, 15], 1.0, mass[16], [mass[15]] * 2)]
            assert D.emulate_list(mass, ch2, par, [0, 1], 1)[4]["levels"] == 16


# ------------------------------------------------------------------------------------------
# 8: the envelope
# ------------------------------------------------------------------------------------------
def test_envelope_holds_for_every_urqmd_row():
    """All 21 four-body rows of the UrQMD table: over 10^6 tries of the engine's own draw no weight p1 p2 p3 exceeds
    w_max, and over 10^6 decays no rejection loop reaches its cap of 1024 tries.  Rows with the same masses see the
    same random streams (a stream is keyed by the primary, not by the channel), so each distinct (M, m) is run once
    and stands for its rows.  Measured acceptance / largest weight ratio: M = 1.275: 0.0762 / 0.129, 1.282: 0.0760 /
    0.129, 1.37: 0.0741 / 0.127, 1.465: 0.0723 / 0.124, 1.72: 0.0685 / 0.120; capped 0 everywhere."""
    rows = row_masses(fourbody_rows())
    distinct = sorted({(M, tuple(m)) for M, m in rows})
    assert len(rows) == 21 and len(distinct) == 5
    n = 1_000_000
    for M, m in distinct:
        worst, acc, wmax = D.envelope(M, m, 5, n)
        mass = np.array([m[0], M])
        ch = [D.channel4(1, [0, 0, 0, 0], 1.0, M, list(m))]
        par = L.make_list(np.full(n, 1), mass, pT=np.zeros(n), phi=np.zeros(n), y=np.zeros(n))
        out, _, _, st, _ = D.emulate_list(mass, ch, par, [0, n], 9)
        print("M %.3f: acceptance %.4f, largest p1 p2 p3 / w_max %.4f, capped %d" % (M, acc, worst, st["capped"]))
        assert wmax > 0 and worst <= 1.0
        assert acc > 0.05 and (1 - acc) ** D.FOUR_CAP < 1e-20
        assert st["decays"] == n and st["capped"] == 0 and len(out) == 4 * n
