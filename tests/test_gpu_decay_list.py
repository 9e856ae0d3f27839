"""GPU tier of the Monte Carlo decays of a sampled particle list (decay_list.hip through the C ABI and the Python
binding): the decayed list is a pure function of (seed, list); invariants of every record; the kernels
against the CPU emulator (the same decay_mc_math.h on the host); the decayed spectra against the feed-down formula of
7.6, which shares no algebra with them; the whole SMASH table; the operation = 2 run directory; the errors.

Statistical bars are derived: 5 sqrt(mu) for a count with expectation mu, 4 sigma plus the quadrature term against the
formula (tests/test_decay_cpu.py's bound); seeds are fixed."""
import ctypes as C
import functools
import glob
import os

import numpy as np
import pytest

import decay_list_ref as L
import decay_ref as R
import sampler_bins_ref as B
from is3d2_amd import Engine, IS3DError, _lib, build_engine, hrg, make_spec, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MASS, CHANNELS = R.CASE_MASS, R.CASE_CHANNELS
POSITION = ("tau", "x", "y", "eta", "t", "z", "cell", "event")
BINS = dict(pT_min=0.0, pT_max=3.0, pT_bins=12, y_cut=2.0, y_bins=10, phip_bins=12, eta_cut=3.0, eta_bins=12,
            tau_min=0.0, tau_max=12.0, tau_bins=6, r_min=0.0, r_max=12.0, r_bins=6)


def case_spec():
    """The 8 species of decay_ref's case table as the chosen species of a 2+1D sampler run."""
    spec = make_spec(chosen="pikp", df_mode=1, dimension=2)
    n = len(MASS)
    spec["species"] = dict(mass=MASS.copy(), sign=np.where(np.isin(np.arange(n), (3, 4, 7)), 1.0, -1.0), degen=np.ones(n),
                           baryon=np.zeros(n), mcid=np.arange(1, n + 1))
    return spec


def sampler_engine(spec, s, plasma=None, **kw):
    plasma = O.averages(s, spec["params"]["include_baryon"]) if plasma is None else plasma
    return build_engine(spec, s, T_avg=plasma[0], **kw), plasma


def list_engine(mass, channels, devices=None):
    """An engine with only what decay_particles needs: params, species, a grid, the channels."""
    e = Engine(devices=devices)
    e.set_params(dimension=3)
    n = len(mass)
    e.set_species(mass, -np.ones(n), np.ones(n), np.zeros(n))
    e.set_momentum_grid(np.linspace(0.1, 3.0, 4), np.array([0.5, 2.0, 4.0]), np.zeros(1), np.zeros(1), np.ones(1))
    if channels is not None:
        e.set_decays(channels)
    return e


def same_hist(a, b):
    return sorted(a) == sorted(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)


@functools.lru_cache(maxsize=None)
def sampled_case():
    """50 events of a 300-cell surface with the case species, decayed once: everything tests 1 and 2 share."""
    spec = case_spec()
    s = synth.as_read(synth.surface(300, seed=23))
    e, plasma = sampler_engine(spec, s)
    e.set_decays(CHANNELS)
    e.set_sample_bins(**BINS)
    prim, off0, st0 = e.sample(11, 50, 0.5, 0, plasma)
    out, off, orig, st = e.decay_sampled(5, binned=True)
    hist = e.sample_hist()
    e.close()
    for a in (prim, off0, out, off, orig):
        a.setflags(write=False)
    return spec, s, plasma, prim, off0, out, off, orig, st, hist


# ------------------------------------------------------------------------------------------
# 1. bytes depend on (seed, list) only
# ------------------------------------------------------------------------------------------
def test_the_decayed_list_depends_on_the_seed_and_the_list_only():
    spec, s, plasma, prim, off0, out, off, orig, st, hist = sampled_case()
    assert len(prim) > 1000 and len(out) > len(prim) and st["capped"] == 0 and st["batches"] == 1
    e, _ = sampler_engine(spec, s, plasma)
    e.set_decays(CHANNELS)
    e.set_sample_bins(**BINS)

    def again(seed, binned=True):
        p, o, _ = e.sample(11, 50, 0.5, 0, plasma)
        assert p.tobytes() == prim.tobytes()
        return e.decay_sampled(seed, binned=binned)

    b, off_b, orig_b, st_b = again(5)
    assert b.tobytes() == out.tobytes() and (off_b == off).all() and (orig_b == orig).all()
    assert same_hist(e.sample_hist(), hist)
    # several batches of primaries
    e.set_tuning("sample_bytes", 150000)
    c, off_c, orig_c, st_c = again(5)
    assert st_c["batches"] > 3
    assert c.tobytes() == out.tobytes() and (off_c == off).all() and (orig_c == orig).all()
    assert same_hist(e.sample_hist(), hist)
    for k in ("primaries", "decays", "undecayed", "dropped_daughters", "capped", "final_particles", "passes"):
        assert st_c[k] == st[k], k
    e.set_tuning("sample_bytes", -1)
    # events [10, 20) decayed alone
    d, off_d, orig_d, st_d = e.decay_particles(prim, off0[10:21], 5)
    assert d.tobytes() == out[off[10]:off[20]].tobytes()
    assert (off_d == off[10:21] - off[10]).all() and (orig_d == orig[off[10]:off[20]]).all()
    assert st_d["primaries"] == off0[20] - off0[10]
    # the list decay_particles leaves in the engine is what the getters return
    assert e.lib.is3d_sample_count(e._e) == len(d)
    # another seed
    f, _, _, _ = again(6, binned=False)
    assert f.tobytes() != out.tobytes()
    e.close()
    # two shards on one device: the decays run on the first over the merged list
    g, _ = sampler_engine(spec, s, plasma, devices=[0, 0])
    g.set_decays(CHANNELS)
    g.set_sample_bins(**BINS)
    p, o, _ = g.sample(11, 50, 0.5, 0, plasma)
    assert p.tobytes() == prim.tobytes()
    h, off_h, orig_h, st_h = g.decay_sampled(5, binned=True)
    hist_h = g.sample_hist()
    g.close()
    assert h.tobytes() == out.tobytes() and (off_h == off).all() and (orig_h == orig).all() and same_hist(hist_h, hist)


def test_binned_histograms_are_the_numpy_binning_of_the_decayed_list():
    """bin = 1: the counts are the numpy binning of the list the same call returns (rapidity from (E, pz)); the fixed
    seed has no particle within 1e-12 of an edge of a histogram whose coordinate comes from atan2 or log."""
    spec, s, plasma, prim, off0, out, off, orig, st, hist = sampled_case()
    rap = B.rapidity_from_momentum(out)
    assert B.ambiguous(out, rap, BINS) == 0
    want = B.np_hist(out, rap, BINS, len(MASS))
    for name, _ in _lib.SAMPLE_BIN_PARTS:
        np.testing.assert_array_equal(hist[name], want[name], err_msg=name)
    assert hist["dN_deta"].sum() > 0.9 * len(out)


# ------------------------------------------------------------------------------------------
# 2. invariants of every record
# ------------------------------------------------------------------------------------------
def test_invariants_of_every_record():
    """Mass shell at 8 ulp of E^2 (E is the rounded root of a sum of four rounded squares, as in the sampler tests);
    four-momentum of the complete unadjusted trees at the CPU tier's derived ulp bars."""
    spec, s, plasma, prim, off0, out, off, orig, st, hist = sampled_case()
    _, level = L.mc_channels(MASS, CHANNELS)
    residual = level[out["species"]] >= 0
    assert st["capped"] == 0 and residual.sum() == st["undecayed"] + st["capped"] and st["undecayed"] > 0
    m = MASS[out["species"]]
    E2 = out["E"] ** 2
    assert np.max(np.abs(E2 - out["px"] ** 2 - out["py"] ** 2 - out["pz"] ** 2 - m * m) / L.ulp(E2)) <= 8
    for f in POSITION:
        assert np.array_equal(out[f], prim[f][orig]), f
    assert (np.diff(orig) >= 0).all() and orig[0] >= 0 and orig[-1] < len(prim)
    assert off[0] == 0 and off[-1] == len(out) and len(off) == len(off0)
    assert (off == np.searchsorted(orig, off0, side="left")).all()
    for ev in range(50):
        assert (out["event"][off[ev]:off[ev + 1]] == ev).all()
    # the counters against the list: tree sizes are fixed by the primary's species in this table
    assert st["final_particles"] == len(out) and st["primaries"] == len(prim) and st["passes"] == 2
    size = np.bincount(orig, minlength=len(prim))
    sp = prim["species"]
    allowed = {0: (1,), 1: (1,), 4: (1,), 2: (2,), 3: (1, 2), 5: (1, 3), 6: (1, 3), 7: (1, 2)}
    for k, ok in allowed.items():
        assert np.isin(size[sp == k], ok).all(), k
    decays = np.where(np.isin(sp, (0, 1, 4)), 0, np.where(sp == 6, np.where(size == 3, 2, 1), (size > 1).astype(int)))
    assert decays.sum() == st["decays"]
    # sum over trees of (records gained) = sum over decays of (bodies - 1) - dropped daughters
    assert len(out) - len(prim) <= 2 * st["decays"] and st["dropped_daughters"] > 0
    # every decay of 6 -> 5 + (not chosen) drops one daughter; trees of 6 of size 1 took it and 5 stayed
    assert st["dropped_daughters"] >= int(((sp == 6) & (size == 1)).sum())
    sums = L.tree_sums(out, orig, len(prim))
    want = np.stack([prim[f] for f in ("E", "px", "py", "pz")], axis=1)
    err = np.abs(sums - want) / L.ulp(prim["E"])[:, None]
    for k, bar in ((2, L.BAR_2BODY), (3, L.BAR_2BODY), (7, L.BAR_2BODY), (5, L.BAR_3BODY)):
        sel = sp == k
        assert sel.sum() > 20
        print("species %d: %d trees, max |sum p - P| = %.1f ulp(E)" % (k, sel.sum(), err[sel].max()))
        assert err[sel].max() <= bar


def test_adjusted_channel_conserves_px_and_py():
    """The table of the CPU tier with X(1.07) -> N pi opened by the mass adjustment: sum px and sum py of every tree at
    the 2-body bar, in ulp of the parent's energy on the adjusted mass; mass shells at 8 ulp of E^2."""
    n = 20000
    rng = np.random.default_rng(8)
    par = L.make_list(np.full(n, 6), L.MASS, pT=rng.exponential(0.5, n), phi=rng.uniform(0, 2 * np.pi, n), y=rng.uniform(-4, 4, n))
    e = list_engine(L.MASS, L.TABLE)
    assert e.decay_stats()["adjusted"] == 1
    out, off, orig, st = e.decay_particles(par, [0, n], 3)
    e.close()
    assert st["decays"] == n and len(out) == 2 * n and st["capped"] == 0
    sums = L.tree_sums(out, orig, n)
    ER = np.sqrt(1.095 ** 2 + par["px"] ** 2 + par["py"] ** 2) * par["E"] / np.sqrt(par["E"] ** 2 - par["pz"] ** 2)
    assert np.max(np.abs(sums[:, 1] - par["px"]) / L.ulp(ER)) <= L.BAR_2BODY
    assert np.max(np.abs(sums[:, 2] - par["py"]) / L.ulp(ER)) <= L.BAR_2BODY
    m = L.MASS[out["species"]]
    E2 = out["E"] ** 2
    assert np.max(np.abs(E2 - out["px"] ** 2 - out["py"] ** 2 - out["pz"] ** 2 - m * m) / L.ulp(E2)) <= 8


# ------------------------------------------------------------------------------------------
# 3. GPU against the emulator
# ------------------------------------------------------------------------------------------
def test_gpu_against_emulator():
    """2 x 10^5 primaries of the eight case species in four events: species, origins and offsets equal the emulator's
    exactly (a flipped channel or rejection draw would show there: allowance 0), momenta within the project's
    host-against-device bar 1e-8 of the primary's energy.  Measured on MI355X: 6.3e-16."""
    n, seed = 200_000, 17
    rng = np.random.default_rng(4)
    sp = rng.integers(0, len(MASS), n)
    par = L.make_list(sp, MASS, pT=rng.exponential(0.6, n), phi=rng.uniform(0, 2 * np.pi, n), y=rng.uniform(-4, 4, n))
    offsets = np.array([0, 50_000, 50_001, 120_000, n])
    par["event"] = np.repeat([3, 4, 9, 10], np.diff(offsets))
    e = list_engine(MASS, CHANNELS)
    out, off, orig, st = e.decay_particles(par, offsets, seed)
    e.close()
    ref, off_r, orig_r, st_r, _ = L.emulate(MASS, CHANNELS, par, offsets, seed)
    if len(out) != len(ref) or not np.array_equal(out["species"], ref["species"]) or not np.array_equal(orig, orig_r):
        k = min(len(orig), len(orig_r))
        bad = np.nonzero((orig[:k] != orig_r[:k]) | (out["species"][:k] != ref["species"][:k]))[0]
        o = int(orig_r[bad[0]]) if len(bad) else int(orig_r[k - 1])
        prim = int(L.index_in_event(offsets)[o])
        ch, _ = L.mc_channels(MASS, CHANNELS)
        print("first structural mismatch in the tree of primary %d (species %d, event %d): root channel draw u = %.17g, "
              "thresholds %s" % (o, par["species"][o], par["event"][o], L.uniforms(seed, prim, par["event"][o], 0, 1)[0],
                                 [c["cum"] for c in ch if c["parent"] == par["species"][o]]))
    assert len(out) == len(ref)
    assert np.array_equal(out["species"], ref["species"]) and np.array_equal(orig, orig_r) and np.array_equal(off, off_r)
    for f in POSITION:
        assert np.array_equal(out[f], ref[f]), f
    assert {k: st[k] for k in L.STAT_KEYS} == st_r and st["capped"] == 0 and st["ms_total"] > 0
    scale = par["E"][orig]
    err = max(float(np.max(np.abs(out[f] - ref[f]) / scale)) for f in ("E", "px", "py", "pz"))
    print("GPU vs emulator: %d final records, max |dp| / E_primary = %.3e" % (len(out), err))
    assert err < R.BAR


# ------------------------------------------------------------------------------------------
# 4. against the feed-down formula
# ------------------------------------------------------------------------------------------
FORMULA_CASES = {"rho-pipi": (3, L.RHO, 0, 0.776, 0.138, [0.138], L.PT_BINS[:4]),          # 10^6 parents: the 1.2-1.8 bin holds < 1000
                 "Delta-N": (4, L.DELTA, 0, 1.232, 0.938, [0.138], L.PT_BINS),
                 "Delta-pi": (4, L.DELTA, 1, 1.232, 0.138, [0.938], L.PT_BINS_SOFT),
                 "omega-3pi": (5, L.OMEGA, 1, 0.782, 0.138, [0.138, 0.138], L.PT_BINS_SOFT)}


@pytest.mark.parametrize("case", sorted(FORMULA_CASES))
def test_decayed_spectra_against_the_feed_down_formula(case):
    """10^6 primaries of one parent species drawn in numpy from exp(-MT / T)(1 + 2 v2 cos 2 Phi), flat in |Y| < 3, and
    decayed on the GPU: the daughters of one slot with |y| < 0.5 per pT bin, and their v2, against decay_ref.slot_term
    on the exact parent -- 4 sigma of the counting error plus the |12 - 24 nodes| quadrature term
    (tests/test_decay_cpu.py's bound); every bin holds more than 1000.  The CPU emulator with the same lists stays inside
    the bound (largest pull 2.6)."""
    sp, chan, slot, M, m1, others, bins = FORMULA_CASES[case]
    n = 1_000_000
    rng = np.random.default_rng(7 + sp + slot)
    E, px, py, pz = L.draw_parents(rng, M, n)
    par = L.make_list(np.full(n, sp), L.MASS, E=E, px=px, py=py, pz=pz)
    e = list_engine(L.MASS, [chan])
    out, off, orig, st = e.decay_particles(par, [0, n], 5)
    e.close()
    nb = chan["n_body"]
    assert len(out) == nb * n and st["capped"] == 0 and st["decays"] == n
    N, c2 = L.record_bins(out[slot::nb], bins)
    L.check_against_formula(N, c2, n, M, m1, others, bins, case)


def test_chain_yields():
    """Per primary of species 6 of the case table the mean final counts of species 0 and 1 are the sums over the paths
    of branching x multiplicity: 6 -> 2 + 0 -> (0 + 1) + 0 with 0.5, 6 -> 5 -> 0 + 1 + 0 with 0.5 x 0.89: 1.89 and
    0.945.  Counts within 5 sqrt(mu)."""
    n = 200_000
    par = L.make_list(np.full(n, 6), MASS, pT=np.full(n, 0.4), phi=np.zeros(n), y=np.zeros(n))
    e = list_engine(MASS, CHANNELS)
    out, off, orig, st = e.decay_particles(par, [0, n], 21)
    e.close()
    for sp, per in ((0, 0.5 * 2 + 0.5 * 0.89 * 2), (1, 0.5 + 0.5 * 0.89)):
        got, mu = int((out["species"] == sp).sum()), per * n
        print("species %d: %d, expected %.0f (%.2f sqrt(mu))" % (sp, got, mu, (got - mu) / np.sqrt(mu)))
        assert abs(got - mu) <= 5 * np.sqrt(mu)
    assert st["passes"] == 2 and st["dropped_daughters"] > 0


# ------------------------------------------------------------------------------------------
# 5. the whole SMASH table
# ------------------------------------------------------------------------------------------
def test_whole_smash_table():
    """444 species, a 64-cell surface, 20 events: every final species has no kept channel or is a counted residual; one
    pass per level; charge and baryon number of every complete tree (no daughter outside the chosen list anywhere
    below the primary's species) equal the primary's, from the table's own quantum numbers."""
    d = dict(np.load(os.path.join(HERE, "golden", "decays_smash.npz")))
    spec = make_spec(hrg_eos=2, chosen="smash", df_mode=2, dimension=2)
    mcids = spec["species"]["mcid"]
    ch = hrg.decay_channels(d, d, mcids)
    s = synth.as_read(synth.surface(64, seed=7))
    e, plasma = sampler_engine(spec, s)
    e.set_decays(ch)
    prim, off0, _ = e.sample(3, 20, 0.8, 0, plasma)
    out, off, orig, st = e.decay_sampled(3)
    levels = e.decay_stats()["levels"]
    e.close()
    mass = spec["species"]["mass"]
    kept, level = L.mc_channels(mass, ch)
    print("SMASH: %d primaries -> %d final hadrons, %s" % (len(prim), len(out), st))
    assert len(prim) > 1000 and len(out) > len(prim)
    assert st["capped"] == 0 and st["passes"] == levels and levels > 3
    assert (level[out["species"]] >= 0).sum() == st["undecayed"]
    assert st["final_particles"] == len(out) and (np.diff(orig) >= 0).all()
    for f in POSITION:
        assert np.array_equal(out[f], prim[f][orig]), f
    # complete species: every kept channel has chosen daughters that are complete themselves
    complete = np.ones(len(mass), dtype=bool)
    for _ in range(levels + 1):
        for c in kept:
            ds = c["d"][:c["nbody"]]
            if any(x < 0 or not complete[x] for x in ds):
                complete[c["parent"]] = False
    _, parts = hrg.decay_rows_with_antibaryons(d, d)
    q = {int(m): (int(b), int(c)) for m, b, c in zip(parts["p_mcid"], parts["p_baryon"], parts["p_charge"])}
    baryon = np.array([q[int(m)][0] for m in mcids])
    charge = np.array([q[int(m)][1] for m in mcids])
    sel = complete[prim["species"]]
    assert sel.sum() > 0.5 * len(prim)
    for name, v in (("baryon", baryon), ("charge", charge)):
        tot = np.bincount(orig, weights=v[out["species"]], minlength=len(prim))
        assert np.array_equal(tot[sel], v[prim["species"]][sel].astype(float)), name


# ------------------------------------------------------------------------------------------
# 6. drop-in: do_resonance_decays with operation = 2
# ------------------------------------------------------------------------------------------
DROPIN_CHOSEN = [211, -211, 111, 2212, -2212, 2112, 113, 213, 223, 2224, -2224, 2214, 321, 313]
DROPIN_PARAMS = dict(operation=2, dimension=2, df_mode=1, include_baryon=0, include_bulk_deltaf=1, include_shear_deltaf=1,
                     include_baryondiff_deltaf=0, regulate_deltaf=0, outflow=0, deta_min=1e-5, mass_pion0=0.138,
                     oversample=1, min_num_hadrons=2000.0, max_num_samples=100.0, y_cut=0.75, sampler_seed=77, fast=0)


def read_results(d):
    out = {}
    for base, _, files in os.walk(os.path.join(d, "results")):
        for fn in files:
            with open(os.path.join(base, fn), "rb") as f:
                out[os.path.relpath(os.path.join(base, fn), d)] = f.read()
    return out


def dropin_engine(d, spec):
    from is3d2_amd import host
    fields, avg = host.read_surface(d, 1, 2, 0)
    return build_engine(spec, {k: fields[i] for i, k in enumerate(synth.FIELDS)}, T_avg=avg[0]), avg


def test_dropin_run_directory(tmp_path):
    """operation = 2 with do_resonance_decays = 1: host.sample returns Engine.sample -> decay_sampled (the sampler's
    seed) byte for byte, with origins and the decay counters, and the OSCAR files hold that list at the writer's
    precision; with the key 0 every file is the file of a run without the key."""
    from is3d2_amd import host, rundir
    dec = dict(np.load(os.path.join(HERE, "golden", "decays_smash.npz")))
    s = synth.surface(200, seed=43)
    params = dict(DROPIN_PARAMS, test_sampler=0)
    runs = {}
    for name, extra in (("on", dict(do_resonance_decays=1, lightest_particle=111)), ("off", dict(do_resonance_decays=0)),
                        ("absent", {})):
        d = rundir.write_run_dir(str(tmp_path / name), s, dict(params, **extra), hrg_eos=2, chosen=DROPIN_CHOSEN,
                                 surface_format=1, decays=dec)
        runs[name] = (d, host.sample(d, write_files=True, write_csv=True))
    off_files, absent_files = read_results(runs["off"][0]), read_results(runs["absent"][0])
    assert off_files == absent_files and len(off_files) > 2
    assert runs["off"][1]["particles"].tobytes() == runs["absent"][1]["particles"].tobytes()
    assert "origins" not in runs["off"][1] and "origins" not in runs["absent"][1]
    d, got = runs["on"]
    spec = make_spec(hrg_eos=2, chosen=DROPIN_CHOSEN, **{k: v for k, v in params.items() if k != "operation"})
    e, avg = dropin_engine(d, spec)
    nev = got["n_events"]
    prim, off0, st0 = e.sample(77, nev, 0.75, 0, avg)
    assert prim.tobytes() == runs["off"][1]["particles"].tobytes()
    e.set_decays(hrg.decay_channels(dec, dec, DROPIN_CHOSEN))
    p, off, orig, st = e.decay_sampled(77)
    e.close()
    assert len(p) > len(prim) > 500 and st["decays"] > 100
    assert got["particles"].tobytes() == p.tobytes() and (got["offsets"] == off).all() and (got["origins"] == orig).all()
    assert {k: got["decay_stats"][k] for k in L.STAT_KEYS} == {k: st[k] for k in L.STAT_KEYS}
    mcids, mass = spec["species"]["mcid"], spec["species"]["mass"]
    assert (got["mcid"] == mcids[p["species"]]).all()
    names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(d, "results", "particle_list_osc_*")))
    assert names == sorted("particle_list_osc_%d.dat" % (k + 1) for k in range(nev))
    for ev in range(nev):
        with open(os.path.join(d, "results", "particle_list_osc_%d.dat" % (ev + 1))) as f:
            assert f.readline() == "n pid px py pz E m x y z t\n"
            rows = np.array([[float(v) for v in ln.split()] for ln in f]).reshape(-1, 11)
        q = p[off[ev]:off[ev + 1]]
        assert len(rows) == len(q)
        assert (rows[:, 0] == np.arange(len(q))).all() and (rows[:, 1] == mcids[q["species"]]).all()
        want = np.stack([q["px"], q["py"], q["pz"], q["E"], mass[q["species"]], q["x"], q["y"], q["z"], q["t"]], axis=1)
        np.testing.assert_array_equal(rows[:, 2:], want)      # 17 significant digits round-trip a double exactly
    assert read_results(d) != off_files


def test_dropin_run_directory_with_test_sampler(tmp_path):
    """test_sampler = 1 with do_resonance_decays = 1: the written results/sampled counts are the numpy binning of the
    decayed list exactly (rapidity from (E, pz)), no list is written; with the key 0 the tree is the tree without it."""
    from is3d2_amd import host, rundir
    dec = dict(np.load(os.path.join(HERE, "golden", "decays_smash.npz")))
    s = synth.surface(200, seed=43)
    params = dict(DROPIN_PARAMS, test_sampler=1)
    d = rundir.write_run_dir(str(tmp_path / "on"), s, dict(params, do_resonance_decays=1), hrg_eos=2, chosen=DROPIN_CHOSEN,
                             surface_format=1, decays=dec)
    got = host.sample(d, write_files=True)
    assert len(got["particles"]) == 0 and (got["offsets"] == 0).all()
    assert glob.glob(os.path.join(d, "results", "particle_list*")) == []
    spec = make_spec(hrg_eos=2, chosen=DROPIN_CHOSEN, **{k: v for k, v in params.items() if k != "operation"})
    e, avg = dropin_engine(d, spec)
    sb, npart = _lib.SampleBins(), len(DROPIN_CHOSEN)
    nc, nv, npp = C.c_long(), C.c_long(), C.c_int()
    assert host.load().is3d_host_sample_hist_size(d.encode(), C.byref(sb), C.byref(npp), C.byref(nc), C.byref(nv)) == 0
    bins = {k: getattr(sb, k) for k, _ in sb._fields_}
    e.set_sample_bins(**bins)
    e.set_decays(hrg.decay_channels(dec, dec, DROPIN_CHOSEN))
    nev = got["n_events"]
    e.sample(77, nev, 0.75, 0, avg)
    p, off, orig, st = e.decay_sampled(77, binned=True)
    hist = e.sample_hist()
    e.close()
    assert same_hist(got["hist"], hist)
    assert {k: got["decay_stats"][k] for k in L.STAT_KEYS} == {k: st[k] for k in L.STAT_KEYS} and len(got["origins"]) == 0
    rap = B.rapidity_from_momentum(p)
    assert B.ambiguous(p, rap, bins) == 0
    want = B.np_hist(p, rap, bins, npart)
    for name, _ in _lib.SAMPLE_BIN_PARTS:
        np.testing.assert_array_equal(hist[name], want[name], err_msg=name)
    mcids = [int(m) for m in spec["species"]["mcid"]]
    files = B.expected_files(hist, bins, nev, mcids)
    tree = B.read_tree(os.path.join(d, "results", "sampled"))
    assert sorted(tree) == sorted(files)
    for name in sorted(files):
        assert tree[name] == files[name], name
    off_dir = rundir.write_run_dir(str(tmp_path / "off"), s, dict(params, do_resonance_decays=0), hrg_eos=2,
                                   chosen=DROPIN_CHOSEN, surface_format=1, decays=dec)
    absent = rundir.write_run_dir(str(tmp_path / "absent"), s, params, hrg_eos=2, chosen=DROPIN_CHOSEN, surface_format=1,
                                  decays=dec)
    host.sample(off_dir, write_files=True)
    host.sample(absent, write_files=True)
    a, b = read_results(off_dir), read_results(absent)
    assert a == b and len(a) == 9 * npart and a != read_results(d)


# ------------------------------------------------------------------------------------------
# 7. errors
# ------------------------------------------------------------------------------------------
def expect(code, f, *a, **kw):
    with pytest.raises(IS3DError) as ei:
        f(*a, **kw)
    assert ei.value.code == code, str(ei.value)


def test_errors():
    par = L.make_list(np.array([2, 3, 6, 0]), MASS, pT=np.full(4, 0.5), phi=np.zeros(4), y=np.zeros(4))
    # state: no channels; no sampled list; no bins for bin = 1
    e = list_engine(MASS, None)
    expect(_lib.IS3D_ERR_STATE, e.decay_particles, par, [0, 4], 1)
    expect(_lib.IS3D_ERR_STATE, e.decay_sampled, 1)
    expect(_lib.IS3D_ERR_STATE, e.decay_list_stats)
    e.set_decays(CHANNELS)
    expect(_lib.IS3D_ERR_STATE, e.decay_sampled, 1)
    expect(_lib.IS3D_ERR_STATE, e.decay_particles, par, [0, 4], 1, binned=True)
    # arguments: a negative seed, a species out of range, events that are not contiguous or decrease
    expect(_lib.IS3D_ERR_ARG, e.decay_particles, par, [0, 4], -1)
    for bad in (len(MASS), -1):
        q = par.copy()
        q["species"][1] = bad
        expect(_lib.IS3D_ERR_ARG, e.decay_particles, q, [0, 4], 1)
    q = par.copy()
    q["event"] = [0, 1, 0, 1]
    expect(_lib.IS3D_ERR_ARG, e.decay_particles, q, [0, 4], 1)               # one event, two values
    q["event"] = [1, 1, 0, 0]
    expect(_lib.IS3D_ERR_ARG, e.decay_particles, q, [0, 2, 4], 1)            # the event field decreases
    expect(_lib.IS3D_ERR_ARG, e.decay_particles, par, [0, 3, 2], 1)          # offsets that decrease
    q["event"] = [1, 1, 1, 1]
    expect(_lib.IS3D_ERR_ARG, e.decay_particles, q, [0, 2, 4], 1)            # two events, one value: one set of streams
    # a plan of more than 16 levels: the path code has 32 bits
    mass17 = 0.1 * 2.5 ** np.arange(18)
    deep = list_engine(mass17, [R.channel(k, [k - 1, k - 1], 1.0, mass17[k], [mass17[k - 1], mass17[k - 1]]) for k in range(1, 18)])
    assert deep.decay_stats()["levels"] == 17
    expect(_lib.IS3D_ERR_ARG, deep.decay_particles, L.make_list([0], mass17, pT=np.array([0.3]), phi=np.zeros(1), y=np.zeros(1)),
           [0, 1], 1)
    deep.close()
    # a refused call leaves no list behind; a good one does
    expect(_lib.IS3D_ERR_STATE, e.decay_list_stats)
    out, off, orig, st = e.decay_particles(par, [0, 4], 1)
    assert st["primaries"] == 4 and len(out) >= 4 and e.decay_list_stats()["final_particles"] == len(out)
    # a single primary that cannot fit the "sample_bytes" bound: the size needed, never a truncation
    e.set_tuning("sample_bytes", 64)
    with pytest.raises(IS3DError) as ei:
        e.decay_particles(par, [0, 4], 1)
    assert ei.value.code == _lib.IS3D_ERR_ARG and "sample_bytes" in str(ei.value) and "needs" in str(ei.value)
    e.set_tuning("sample_bytes", -1)
    # an empty list and an empty event are lists
    out, off, orig, st = e.decay_particles(par, [0, 0, 4, 4], 1)
    assert off[0] == 0 and off[1] == 0 and off[2] == off[3] == len(out)
    out, off, orig, st = e.decay_particles(par[:0], [0, 0], 1)
    assert len(out) == 0 and st["primaries"] == 0
    # a binned-only sample keeps no list to decay
    e.close()
    spec = make_spec(chosen="pikp", df_mode=1, dimension=2)
    s = synth.as_read(synth.surface(40, seed=5))
    g, plasma = sampler_engine(spec, s)
    g.set_decays([])
    g.set_sample_bins(**BINS)
    g.sample_binned(1, 3, 0.5, 0, plasma, keep_list=False)
    expect(_lib.IS3D_ERR_STATE, g.decay_sampled, 1)
    g.sample_binned(1, 3, 0.5, 0, plasma, keep_list=True)
    p0, _, _ = g.sample(1, 3, 0.5, 0, plasma)
    out, off, orig, st = g.decay_sampled(1)
    assert out.tobytes() == p0.tobytes() and (orig == np.arange(len(p0))).all() and st["decays"] == 0    # no channels: nothing decays
    g.close()
