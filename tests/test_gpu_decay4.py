"""GPU tier of the four-body decay channels (is3d_set_decays4 through the C ABI and the Python binding; DESIGN.md 7.6
and 7.7): the list kernels and the feed-down against the CPU emulator (the same headers on the host,
tests/native/decay4_emulator.cpp), the invariances of the decayed list, the UrQMD rows, is3d_sample_decayed, the run
directory and the errors.  The case table is tests/decay4_ref.py's."""
import os

import numpy as np
import pytest

import decay4_ref as D
import decay_list_ref as L
import decay_ref as R
from is3d2_amd import Engine, IS3DError, _lib, build_engine, hrg, make_spec, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MASS, CHANNELS = D.MASS, D.CHANNELS
POSITION = ("tau", "x", "y", "eta", "t", "z", "cell", "event")
BINS = dict(pT_min=0.0, pT_max=3.0, pT_bins=12, y_cut=2.0, y_bins=10, phip_bins=12, eta_cut=3.0, eta_bins=12,
            tau_min=0.0, tau_max=12.0, tau_bins=6, r_min=0.0, r_max=12.0, r_bins=6)


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


def primaries(n, species, seed=4):
    rng = np.random.default_rng(seed)
    sp = rng.choice(species, n)
    return L.make_list(sp, MASS, pT=rng.exponential(0.6, n), phi=rng.uniform(0, 2 * np.pi, n), y=rng.uniform(-4, 4, n))


# ------------------------------------------------------------------------------------------
# 1. the list kernels against the emulator
# ------------------------------------------------------------------------------------------
def test_gpu_against_emulator():
    """2 x 10^5 primaries of R and H in four events through the case table: species, origins and offsets equal the
    emulator's exactly, momenta within 1e-8 of the primary's energy.  H -> R a a b followed by
    R -> a a a a puts slot 3 (code 4 c + 4) below a nonzero c.  Measured on MI355X: 603 840 final records, 7.5e-15."""
    n, seed = 200_000, 17
    par = primaries(n, [D.R_, D.H_])
    offsets = np.array([0, 50_000, 50_001, 120_000, n])
    par["event"] = np.repeat([3, 4, 9, 10], np.diff(offsets))
    e = list_engine(MASS, CHANNELS)
    assert e.decay_stats()["kept"] == 3 and e.decay_stats()["skipped_closed"] == 2 and e.decay_stats()["skipped_many_body"] == 0
    out, off, orig, st = e.decay_particles(par, offsets, seed)
    e.close()
    ref, off_r, orig_r, st_r, _ = D.emulate_list(MASS, CHANNELS, par, offsets, seed)
    assert len(out) == len(ref)
    assert np.array_equal(out["species"], ref["species"]) and np.array_equal(orig, orig_r) and np.array_equal(off, off_r)
    for f in POSITION:
        assert np.array_equal(out[f], ref[f]), f
    assert {k: st[k] for k in L.STAT_KEYS} == st_r and st["capped"] == 0 and st["passes"] == 2
    # some H went H -> R a a b -> (a a a a) a a b: seven records of one primary, the four-body daughters of a daughter
    assert np.bincount(orig).max() == 7
    err = max(float(np.max(np.abs(out[f] - ref[f]) / par["E"][orig])) for f in ("E", "px", "py", "pz"))
    print("GPU vs emulator: %d final records, max |dp| / E_primary = %.3e" % (len(out), err))
    assert err <= 1e-8


# ------------------------------------------------------------------------------------------
# 2. the bytes depend on (seed, list) only
# ------------------------------------------------------------------------------------------
def test_same_bytes_for_every_batching_subrange_and_device_list():
    n, seed = 40_000, 5
    par = primaries(n, [D.H_], seed=9)          # 3.64 final records per H on average: more than the first guess of 3
    offsets = np.array([0, 9_000, 20_000, 31_000, n])
    par["event"] = np.repeat([0, 1, 2, 3], np.diff(offsets))
    e = list_engine(MASS, CHANNELS)
    out, off, orig, st = e.decay_particles(par, offsets, seed)
    assert st["batches"] == 1 and len(out) > 3.3 * n
    # a bound that plans ranges of 10 000 primaries, whose products do not fit: the ranges halve (8 batches, not 4)
    e.set_tuning("sample_bytes", 10_000 * (100 + 3 * 340))
    a, off_a, orig_a, st_a = e.decay_particles(par, offsets, seed)
    assert st_a["batches"] >= 8
    # ... and a smaller one (any bound below the whole list halves here: the guess of three records is always short)
    e.set_tuning("sample_bytes", 2_500 * (100 + 3 * 340))
    b, off_b, orig_b, st_b = e.decay_particles(par, offsets, seed)
    assert st_b["batches"] >= 32
    for got, o, g, s in ((a, off_a, orig_a, st_a), (b, off_b, orig_b, st_b)):
        assert got.tobytes() == out.tobytes() and np.array_equal(o, off) and np.array_equal(g, orig)
        assert {k: s[k] for k in L.STAT_KEYS} == {k: st[k] for k in L.STAT_KEYS}
    e.set_tuning("sample_bytes", -1)
    # events 1 and 2 decayed alone
    c, off_c, orig_c, st_c = e.decay_particles(par, offsets[1:4], seed)
    assert c.tobytes() == out[off[1]:off[3]].tobytes() and np.array_equal(off_c, off[1:4] - off[1])
    assert np.array_equal(orig_c, orig[off[1]:off[3]])
    e.close()
    g = list_engine(MASS, CHANNELS, devices=[0, 0])
    d, off_d, orig_d, st_d = g.decay_particles(par, offsets, seed)
    assert g.decay_stats()["kept"] == 3
    g.close()
    assert d.tobytes() == out.tobytes() and np.array_equal(off_d, off) and np.array_equal(orig_d, orig)


# ------------------------------------------------------------------------------------------
# 3. the UrQMD rows
# ------------------------------------------------------------------------------------------
def test_urqmd_subset_trees():
    """The UrQMD subset fixture (nine four-body rows: f2(1270), f1(1285), f0(1370)) over the whole UrQMD particle list
    as the chosen list, so that no daughter is dropped and every tree is complete; 200 primaries of every species with
    a kept channel: every tree conserves charge and baryon number, no record of a decaying species remains beyond the
    undecayed count (none: with the four-body rows the branchings of f2, f1 and f0 sum to 1), no rejection loop is
    capped; with the three-slot call some f2, f1 and f0 remain."""
    d = dict(np.load(os.path.join(HERE, "golden", "decays_urqmd_subset.npz")))
    pdg = hrg.pdg_particles(1)
    mcids, mass = pdg["mcid"], pdg["mass"]
    ch3, ch4 = hrg.decay_channels(d, d, mcids), hrg.decay_channels(d, d, mcids, four_body=True)
    ints, dbls, level, levels = D.mc_channels(mass, ch4)
    parents = np.nonzero(level >= 0)[0]
    rng = np.random.default_rng(2)
    sp = np.repeat(parents, 200)
    n = len(sp)
    par = L.make_list(sp, mass, pT=rng.exponential(0.6, n), phi=rng.uniform(0, 2 * np.pi, n), y=rng.uniform(-3, 3, n))
    left = {}
    for name, ch in (("three", ch3), ("four", ch4)):
        e = list_engine(mass, ch)
        gst = e.decay_stats()
        out, off, orig, st = e.decay_particles(par, [0, n], 3)
        e.close()
        left[name] = {m: int((mcids[out["species"]] == m).sum()) for m in (225, 20223, 10221)}
        if name == "three":
            assert gst["skipped_many_body"] == 9
            continue
        assert gst["skipped_many_body"] == 0 and gst["levels"] == levels == st["passes"]
        assert st["capped"] == 0 and (level[out["species"]] >= 0).sum() == st["undecayed"]
        assert st["dropped_daughters"] == 0 and st["undecayed"] == 0
        _, parts = hrg.decay_rows_with_antibaryons(d, d)
        q = {int(m): (int(b), int(c)) for m, b, c in zip(parts["p_mcid"], parts["p_baryon"], parts["p_charge"])}
        assert np.isin(mcids[par["species"]], (225, 20223, 10221)).sum() == 600
        for k, label in ((0, "baryon"), (1, "charge")):
            v = np.array([q[int(m)][k] for m in mcids])
            tot = np.bincount(orig, weights=v[out["species"]], minlength=n)
            assert np.array_equal(tot, v[par["species"]].astype(float)), label
        assert st["final_particles"] == len(out)
    print("f2, f1, f0 left: three-slot call %s, four-slot call %s" % (left["three"], left["four"]))
    assert all(left["four"][m] == 0 < left["three"][m] for m in left["four"])


# ------------------------------------------------------------------------------------------
# 4. is3d_sample_decayed
# ------------------------------------------------------------------------------------------
def test_sample_decayed_equals_the_two_calls():
    """A 300-cell surface with the case table's five species (R and H with large degeneracies, so that they are
    sampled): the one-pass call gives the list, the offsets, the origins and the histograms of sample followed by
    decay_sampled, and its binned-only form the same histograms."""
    spec = make_spec(chosen="pikp", df_mode=1, dimension=2)
    spec["species"] = dict(mass=MASS.copy(), sign=-np.ones(5), degen=np.array([1.0, 1.0, 1.0, 3e4, 3e6]), baryon=np.zeros(5),
                           mcid=np.arange(1, 6))
    s = synth.as_read(synth.surface(300, seed=23))
    plasma = O.averages(s, 0)
    e = build_engine(spec, s, T_avg=plasma[0])
    e.set_decays(CHANNELS)
    e.set_sample_bins(**BINS)
    prim, off0, _ = e.sample(11, 20, 0.5, 0, plasma)
    want, off, orig, st = e.decay_sampled(5, binned=True)
    hist = e.sample_hist()
    assert (prim["species"] == D.H_).sum() > 100 and (prim["species"] == D.R_).sum() > 100 and st["decays"] > 300
    assert np.bincount(orig).max() == 7
    got, off_g, orig_g, st_g = e.sample_decayed(11, 20, 5, 0.5, 0, plasma, keep_list=True, binned=True)
    assert got.tobytes() == want.tobytes() and np.array_equal(off_g, off) and np.array_equal(orig_g, orig)
    assert {k: st_g[k] for k in L.STAT_KEYS} == {k: st[k] for k in L.STAT_KEYS}
    assert same_hist(e.sample_hist(), hist)
    e.sample_decayed(11, 20, 5, 0.5, 0, plasma, keep_list=False, binned=True)
    assert same_hist(e.sample_hist(), hist)
    e.close()


# ------------------------------------------------------------------------------------------
# 5. the feed-down
# ------------------------------------------------------------------------------------------
def decay_engine(mass, pT, phi, y, dimension, channels):
    e = Engine()
    e.set_params(dimension=dimension)
    n = len(mass)
    e.set_species(mass, -np.ones(n), np.ones(n), np.zeros(n))
    e.set_momentum_grid(pT, phi, y, np.zeros(1), np.ones(1))
    e.set_decays(channels)
    return e


@pytest.mark.parametrize("shape", [(10, 8, 1), (10, 8, 5), (6, 32, 21)], ids=lambda s: "%dx%dx%d" % s)
def test_feeddown_against_emulator(shape):
    """The case table (two four-body channels, one of them feeding a parent that decays again) on tests/test_gpu_decay.py's
    grids: |got - emulator| / sum |terms| <= 1e-8, the plan statistics equal the emulator's, and the reversed channel
    list gives the same bytes.  Measured on MI355X: 1.7e-13, 1.9e-13 and 1.5e-10."""
    npT, nphi, ny = shape
    rng = np.random.default_rng(npT + nphi + ny)
    pT = np.linspace(0.1, 3.0, npT) ** 1.3
    phi = np.sort(rng.uniform(0, 2 * np.pi, nphi))
    y = np.linspace(-2.5, 2.5, ny) if ny > 1 else np.zeros(1)
    S = np.exp(-np.sqrt(pT[None, :, None, None] ** 2 + MASS[:, None, None, None] ** 2) / 0.15) * \
        (1 + 0.2 * np.cos(2 * phi))[None, None, :, None] * np.exp(-y ** 2 / 4)[None, None, None, :]
    ref, ab, st, slots, terms = D.emulate_feeddown(S, MASS, pT, phi, y, CHANNELS)
    assert st["kept"] == 3 and slots == 10 and terms == 8 * 12 + 2
    e = decay_engine(MASS, pT, phi, y, 3 if ny > 1 else 2, CHANNELS)
    got = e.feeddown(S)
    err = R.parity(got, ref, ab)
    print("%s: GPU vs emulator %.3e of sum |terms|" % (shape, err))
    assert err <= 1e-8
    assert np.all(got[D.A_] > S[D.A_]) and np.all(got[D.R_] > S[D.R_]) and np.array_equal(got[D.H_], S[D.H_])
    gst = e.decay_stats()
    assert {k: gst[k] for k in st if k != "ms_total"} == {k: st[k] for k in st if k != "ms_total"}
    e.set_decays(CHANNELS[::-1])
    assert e.feeddown(S).tobytes() == got.tobytes()
    e.close()


# ------------------------------------------------------------------------------------------
# 6. the run directory
# ------------------------------------------------------------------------------------------
RUN_CHOSEN = [211, -211, 111, 2212, -2212, 113, 213, 223, 225, 20223, 10221, 221, 331]
RUN_PARAMS = dict(operation=2, dimension=2, df_mode=1, include_baryon=0, include_bulk_deltaf=1, include_shear_deltaf=1,
                  include_baryondiff_deltaf=0, regulate_deltaf=0, outflow=0, deta_min=1e-5, mass_pion0=0.138,
                  oversample=1, min_num_hadrons=3000.0, max_num_samples=100.0, y_cut=0.75, sampler_seed=77, fast=0,
                  test_sampler=0, do_resonance_decays=1, lightest_particle=111)


def read_results(d):
    out = {}
    for base, _, files in os.walk(os.path.join(d, "results")):
        for fn in files:
            with open(os.path.join(base, fn), "rb") as f:
                out[os.path.relpath(os.path.join(base, fn), d)] = f.read()
    return out


def test_run_directory(tmp_path):
    """operation = 2 with the UrQMD subset rows: four_body_decays = 1 gives what Engine.sample, set_decays with
    hrg.decay_channels(four_body=True) and decay_sampled give; without the key, and with the key 0, the run is the
    three-slot run (the Python calls with the default table, which the older tests pin to the run directory), file
    for file."""
    from is3d2_amd import host, rundir
    dec = dict(np.load(os.path.join(HERE, "golden", "decays_urqmd_subset.npz")))
    s = synth.surface(200, seed=43)
    runs = {}
    for name, extra in (("four", dict(four_body_decays=1)), ("zero", dict(four_body_decays=0)), ("absent", {})):
        d = rundir.write_run_dir(str(tmp_path / name), s, dict(RUN_PARAMS, **extra), hrg_eos=1, chosen=RUN_CHOSEN,
                                 surface_format=1, decays=dec)
        runs[name] = (d, host.sample(d, write_files=True))
    assert read_results(runs["zero"][0]) == read_results(runs["absent"][0])
    assert runs["zero"][1]["particles"].tobytes() == runs["absent"][1]["particles"].tobytes()
    spec = make_spec(hrg_eos=1, chosen=RUN_CHOSEN, **{k: v for k, v in RUN_PARAMS.items()
                                                       if k not in ("operation", "do_resonance_decays", "lightest_particle")})
    d, got = runs["four"]
    fields, avg = host.read_surface(d, 1, 2, 0)
    e = build_engine(spec, {k: fields[i] for i, k in enumerate(synth.FIELDS)}, T_avg=avg[0])
    nev = got["n_events"]
    for name, four in (("four", True), ("absent", False)):
        prim, off0, _ = e.sample(77, nev, 0.75, 0, avg)
        e.set_decays(hrg.decay_channels(dec, dec, RUN_CHOSEN, four_body=four))
        p, off, orig, st = e.decay_sampled(77)
        g = runs[name][1]
        assert g["particles"].tobytes() == p.tobytes() and (g["offsets"] == off).all() and (g["origins"] == orig).all()
        assert {k: g["decay_stats"][k] for k in L.STAT_KEYS} == {k: st[k] for k in L.STAT_KEYS}
    e.close()
    mcids = np.array(RUN_CHOSEN)
    left = {name: int(np.isin(mcids[runs[name][1]["particles"]["species"]], (225, 20223, 10221)).sum()) for name in runs}
    print("f2 + f1 + f0 left in the lists:", left)
    assert left["four"] < left["absent"] and read_results(runs["four"][0]) != read_results(runs["absent"][0])


# ------------------------------------------------------------------------------------------
# 7. errors
# ------------------------------------------------------------------------------------------
def test_errors():
    e = list_engine(MASS, None)
    with pytest.raises(IS3DError) as ei:
        e.set_decays([D.channel4(D.R_, [D.A_, D.A_, D.A_, 5], 1.0, 1.60, [0.14] * 4)])       # slot 3 out of range
    assert ei.value.code == _lib.IS3D_ERR_ARG
    with pytest.raises(IS3DError) as ei:
        e.set_decays([D.channel4(D.R_, [D.A_, D.A_, D.A_, -2], 1.0, 1.60, [0.14] * 4)])
    assert ei.value.code == _lib.IS3D_ERR_ARG
    with pytest.raises(IS3DError) as ei:        # a failed call leaves no decays
        e.decay_stats()
    assert ei.value.code == _lib.IS3D_ERR_STATE
    # the three-slot call does not look at a fourth daughter: a 4-body row is skipped whatever it holds
    e.set_decays([R.channel(D.R_, [D.A_, D.A_, D.A_], 1.0, 1.60, [0.14] * 3, n_body=4)])
    assert e.decay_stats()["skipped_many_body"] == 1
    e.close()
    for levels, ok in ((15, True), (16, False)):
        mass = 0.1 * 4.5 ** np.arange(levels + 1)
        ch = [D.channel4(k, [k - 1, k - 1], 1.0, mass[k], [mass[k - 1]] * 2) for k in range(1, levels)]
        ch.append(D.channel4(levels, [levels - 1] * 4, 1.0, mass[levels], [mass[levels - 1]] * 4))
        par = L.make_list(np.array([levels, 0]), mass, pT=np.array([0.5, 0.5]), phi=np.zeros(2), y=np.zeros(2))
        deep = list_engine(mass, ch)
        assert deep.decay_stats()["levels"] == levels         # the feed-down takes the plan
        if ok:
            out, off, orig, st = deep.decay_particles(par[1:], [0, 1], 1)
            assert len(out) == 1 and st["passes"] == 15
        else:
            with pytest.raises(IS3DError) as ei:
                deep.decay_particles(par[1:], [0, 1], 1)
            assert ei.value.code == _lib.IS3D_ERR_ARG and "4-body" in str(ei.value)
        deep.close()
