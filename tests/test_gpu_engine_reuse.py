"""GPU tier: one engine used again and again.  Every device buffer, stream and event in csrc -- the engine's, the
sampler's, the device group's -- has one owner (csrc/devbuf.h) that makes it on demand and keeps it otherwise, and the entry points share their host sequences (the launch prologue, the
prepass, the error mapping), so a call must not depend on what the engine did before: each result here equals, bit for
bit, the same call on a fresh engine."""
import numpy as np
import pytest

from helpers import parity
from is3d2_amd import IS3DError, _lib, build_engine, make_spec, surface_averages, synth

pytestmark = pytest.mark.gpu

T_AVG = 0.15      # the same delta-f tables on every engine of a test, whatever surface it was built with


def surf(n, seed):
    return synth.as_read(synth.surface(n, seed=seed))


def fresh_spectra(spec, s):
    e = build_engine(spec, s, T_avg=T_AVG)
    out = e.calculate_spectra()
    e.close()
    return out


@pytest.mark.parametrize("flags,sizes", [(dict(df_mode=3), (64, 8, 0, 64)),
                                         (dict(df_mode=5, famod_chains=4), (64, 8, 64))], ids=["ptm", "ptma_chains"])
def test_grow_shrink_grow(flags, sizes):
    """Surfaces of 64, 8, (0,) 64 cells through one engine: PTM sizes the records, aux, renormalisation rows, fallback
    list and slabs by the surface, PTMA with chains the Newton solutions and the chain state."""
    spec = make_spec(hrg_eos=2, chosen="pikp", dimension=2, **flags)
    big = surf(64, 31)
    surfaces = {64: big, 8: surf(8, 32), 0: {k: v[:0] for k, v in big.items()}}
    ref = {n: fresh_spectra(spec, s) for n, s in surfaces.items() if n in sizes}
    assert np.any(ref[64] != 0.0) and np.any(ref[8] != 0.0)
    e = build_engine(spec, surfaces[sizes[0]], T_avg=T_AVG)
    for n in sizes:
        e.set_surface(surfaces[n])
        assert np.array_equal(e.calculate_spectra(), ref[n]), n
    e.close()


def test_operations_interleaved_on_one_engine():
    """Spectra, dN/dX, the yield estimate, the sampler and the spectra again share the records, the aux rows, the error
    word and the counters of one engine."""
    spec = make_spec(hrg_eos=2, chosen="pikp", df_mode=1, dimension=2)
    s = surf(64, 33)
    plasma = surface_averages(s)
    calls = [("spectra", lambda e: e.calculate_spectra()),
             ("dN_dX", lambda e: e.calculate_dN_dX()),
             ("yield", lambda e: e.total_yield(plasma)),
             ("sample", lambda e: e.sample(1, 2, fast=1, plasma=plasma)[0]),
             ("spectra", lambda e: e.calculate_spectra())]
    ref = {}
    for name, call in calls[:4]:
        f = build_engine(spec, s, T_avg=T_AVG)
        ref[name] = call(f)
        f.close()
    assert len(ref["sample"]) > 0

    def same(a, b):
        if isinstance(a, tuple):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        return np.array_equal(a, b)

    e = build_engine(spec, s, T_avg=T_AVG)
    for i, (name, call) in enumerate(calls):
        assert same(call(e), ref[name]), (i, name)
    e.close()


def test_one_error_mapping_and_engine_usable_afterwards():
    """A cell temperature outside the delta-f table: every operation reports IS3D_ERR_DF_RANGE with the reference's
    message, and the engine computes the good surface's spectra afterwards as a fresh one does."""
    spec = make_spec(hrg_eos=2, chosen="pikp", df_mode=2, dimension=2)
    good = surf(16, 1)
    bad = dict(good)
    bad["T"] = good["T"].copy()
    bad["T"][3] = 0.3
    plasma = surface_averages(good)
    ref = fresh_spectra(spec, good)
    calls = [("spectra", lambda e: e.calculate_spectra()),
             ("dN_dX", lambda e: e.calculate_dN_dX()),
             ("yield", lambda e: e.total_yield(plasma)),
             ("sample", lambda e: e.sample(1, 2, fast=0, plasma=plasma))]
    e = build_engine(spec, good, T_avg=T_AVG)
    for name, call in calls:
        e.set_surface(bad)
        with pytest.raises(IS3DError) as ei:
            call(e)
        print(name, ei.value)
        assert ei.value.code == _lib.IS3D_ERR_DF_RANGE, name
        assert "interpolation" in str(ei.value) or "outside df coefficient table" in str(ei.value), name
        e.set_surface(good)
        assert np.array_equal(e.calculate_spectra(), ref), name
    e.close()


def test_device_list_engine_spectra_and_polarization():
    """devices = [0, 0] (two shards, the copy reduction): the spectra and the polarization, which share the group's
    launch-and-download path, against the one-device engine (tests/test_gpu_group.py's bound: summation order only)."""
    spec = make_spec(hrg_eos=2, chosen="pikp", df_mode=1, dimension=2)
    s = dict(surf(64, 34))
    s.update(zip(_lib.VORTICITY_FIELDS, synth.vorticity(64, 5)))
    res = []
    for devices in (None, [0, 0]):
        e = build_engine(spec, s, T_avg=T_AVG, devices=devices)
        res.append((e.calculate_spectra(), e.calculate_polarization(T_AVG), e.calculate_spectra()))
        e.close()
    (one, pol1, again1), (grp, polg, againg) = res
    print("spectra", parity(grp, one)[0], "polarization", parity(polg, pol1)[0])
    assert parity(grp, one)[0] < 1e-12
    assert parity(polg, pol1)[0] < 1e-12
    assert np.array_equal(again1, one) and np.array_equal(againg, grp)


def same(a, b):
    """Bit equality of two results: arrays (structured ones too), dicts and tuples of them, numbers."""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


# "sample_bytes" of tests/test_gpu_sampler_bins.py's batch-window cases.  A call that keeps the list: 100000 ("the list
# path's own batches"; this surface draws 683 candidates an event at 204 bytes each).  A binned-only call: its batches of
# (event, cell) pairs at 12 bytes each, 24 pairs for this 64-cell surface where that test has 100 for 300 cells, so one
# event alone takes three windows of cells
SMALL_SAMPLE_BYTES = {"list": 100000, "binned+list": 100000, "binned": 12 * 24}


def test_sampler_buffers_across_calls():
    """sample and sample_binned with and without the list, 1, 8 and 1 events, "sample_bytes" default, small and default
    again on one engine: the call's working buffers (sampler.hip Buffers: pairs, candidates, scan scratch) grow batch
    by batch and die with the call, so the lists, offsets, histograms and stats are a fresh engine's."""
    spec = make_spec(hrg_eos=2, chosen="pikp", df_mode=1, dimension=2)
    s = surf(64, 33)
    plasma = surface_averages(s)
    calls = {"list": lambda e, nev: e.sample(3, nev, 2, 0, plasma),
             "binned+list": lambda e, nev: e.sample_binned(3, nev, 2, 0, plasma, keep_list=True),
             "binned": lambda e, nev: e.sample_binned(3, nev, 2, 0, plasma)}

    def engine():
        e = build_engine(spec, s, T_avg=T_AVG)
        e.set_sample_bins()
        return e

    ref = {}
    for small in (False, True):
        for nev in (1, 8):
            for name, call in calls.items():
                f = engine()
                if small:
                    f.set_tuning("sample_bytes", SMALL_SAMPLE_BYTES[name])
                ref[small, nev, name] = (call(f, nev), f.sample_stats())
                batches = f.get_tuning("sample_batches")
                f.close()
                print(small, nev, name, ref[small, nev, name][1])
                assert ref[small, nev, name][1]["kept"] > 0
                assert batches > 1 if small else batches == 1, (small, nev, name, batches)
    e = engine()
    for small in (False, True, False):
        for nev in (1, 8, 1):
            for name, call in calls.items():
                e.set_tuning("sample_bytes", SMALL_SAMPLE_BYTES[name] if small else -1)
                got = (call(e, nev), e.sample_stats())
                assert same(got, ref[small, nev, name]), (small, nev, name)
                assert (e.get_tuning("sample_batches") > 1) == small
    e.close()


def test_lazy_streams_and_events_survive_reuse_and_teardown():
    """The side / fold streams and their events exist from the first chunked F_TS launch on (3+1D, folded slabs: the
    smallest case of tests/test_gpu_north_star.py's chunked test).  Chunked, one chunk, chunked on one engine, then a
    second engine in the same process after the first is closed: each result is a fresh engine's with that tuning."""
    spec = make_spec(hrg_eos=2, chosen="smash", df_mode=2, dimension=3, pT="pT48", phi="phi32", y="y21")
    s = synth.as_read(synth.surface(200, seed=41, dimension=3, full3d=True))
    chunked = {"phitab_one_bytes": 0, "phitab_chunk_bytes": 1}
    one_chunk = {"phitab_one_bytes": -1, "phitab_chunk_bytes": 1}

    def call(e, tuning):
        for k, v in tuning.items():
            e.set_tuning(k, v)
        out = e.calculate_spectra()
        n = e.get_tuning("phitab_chunks")
        assert (n > 1) if tuning is chunked else (n == 1), n
        if tuning is chunked:     # the folded plan: an accumulator slab and two buffers of one chunk's splits
            assert e.get_tuning("slabs") == 1 + 2 * -(-e.get_tuning("splits") // n)
        return out

    ref = {}
    for name, tuning in (("chunked", chunked), ("one", one_chunk)):
        f = build_engine(spec, s, T_avg=T_AVG)
        ref[name] = call(f, tuning)
        f.close()
    assert np.any(ref["one"] != 0.0)
    e = build_engine(spec, s, T_avg=T_AVG)
    for name, tuning in (("chunked", chunked), ("one", one_chunk), ("chunked", chunked)):
        assert np.array_equal(call(e, tuning), ref[name]), name
    e.close()
    e2 = build_engine(spec, s, T_avg=T_AVG)
    assert np.array_equal(call(e2, chunked), ref["chunked"])
    e2.close()


def test_device_list_engine_operations_interleaved():
    """devices = [0, 0] (the copy reduction, a fixed order): polarization, spectra, the binned sampler, dN/dX and the
    polarization again on one group engine -- the shard outputs and the device-0 output take five spectra sizes, one
    and five again -- each bit-equal to the same call on a fresh [0, 0] engine."""
    spec = make_spec(hrg_eos=2, chosen="pikp", df_mode=1, dimension=2)
    s = dict(surf(64, 34))
    s.update(zip(_lib.VORTICITY_FIELDS, synth.vorticity(64, 5)))
    plasma = surface_averages(s)

    def engine():
        e = build_engine(spec, s, T_avg=T_AVG, devices=[0, 0])
        e.set_sample_bins()
        return e

    calls = [("polarization", lambda e: e.calculate_polarization(T_AVG)),
             ("spectra", lambda e: e.calculate_spectra()),
             ("sample_binned", lambda e: e.sample_binned(3, 2, 2, 0, plasma, keep_list=True)),
             ("dN_dX", lambda e: e.calculate_dN_dX()),
             ("polarization", lambda e: e.calculate_polarization(T_AVG))]
    ref = {}
    for name, call in calls[:4]:
        f = engine()
        ref[name] = call(f)
        f.close()
    assert np.any(ref["polarization"] != 0.0) and np.any(ref["spectra"] != 0.0) and len(ref["sample_binned"][2]) > 0
    e = engine()
    for i, (name, call) in enumerate(calls):
        assert same(call(e), ref[name]), (i, name)
    e.close()


# a decay table over pikp: K -> pi pi (open in floating point) and the pion's stability marker
PIKP_CHANNELS = [dict(parent=1, n_body=2, daughter=[0, 0], branching=1.0, mass_parent=0.494, width_parent=0.0,
                      mass=[0.138, 0.138], width=[0.0, 0.0]),
                 dict(parent=0, n_body=1, daughter=[0], branching=1.0, mass_parent=0.138, width_parent=0.0,
                      mass=[0.138], width=[0.0])]


def test_changed_inputs_match_a_fresh_engine():
    """One input of a live engine changed at a time -- the species list, the classes switch, the momentum grid, the
    params (df_mode, dimension), the PDG, the Gauss-Laguerre table, the delta-f tables, the decay table -- and after
    each change every operation that applies: what an input invalidates (engine.h kInvalidates) must leave the engine
    computing, bit for bit, what a fresh engine given the same final inputs computes.  A new species list drops the
    decay channels, as on a fresh engine that never had any (tests/test_gpu_decay.py)."""
    from is3d2_amd import data as D

    s = dict(surf(64, 35))
    s.update(zip(_lib.VORTICITY_FIELDS, synth.vorticity(64, 5)))
    plasma = surface_averages(s)
    spec0 = make_spec(hrg_eos=2, chosen="pikp", df_mode=1, dimension=2, pT="pT24", phi="phi24", eta="eta24")
    state = dict(spec=spec0, classes=True, T_avg=T_AVG, decays=None)

    def fresh(st):
        e = build_engine(st["spec"], s, T_avg=st["T_avg"], species_classes=st["classes"])
        e.set_sample_bins()
        if st["decays"] is not None:
            e.set_decays(st["decays"])
        return e

    def attempt(f):
        try:
            return f()
        except IS3DError as err:       # an error is a result too: the live engine must give the fresh one's
            return ("error", err.code)

    def failed(r):
        return isinstance(r, tuple) and len(r) == 2 and isinstance(r[0], str) and r[0] == "error"

    def operations(e, st):
        out = {"spectra": attempt(e.calculate_spectra),
               "polarization": attempt(lambda: e.calculate_polarization(T_AVG)),
               "sample_binned": attempt(lambda: e.sample_binned(3, 2, 2, 0, plasma)),
               "sample": attempt(lambda: e.sample(3, 2, 2, 0, plasma))}
        out["decay_sampled"] = attempt(lambda: e.decay_sampled(5)[:3])      # the stats carry a device time
        out["feeddown"] = attempt(lambda: e.feeddown(out["spectra"]))
        out["decay_stats"] = attempt(lambda: {k: v for k, v in e.decay_stats().items() if k != "ms_total"})
        return out

    def respec(**kw):
        sp = dict(state["spec"])
        sp.update(kw)
        return sp

    sp3 = spec0["species"]
    sp2 = {k: v[:2].copy() for k, v in sp3.items()}
    species = lambda e, sp: e.set_species(sp["mass"], sp["sign"], sp["degen"], sp["baryon"])
    phi32, phi32_w = D.grid("phi32")
    pdg = spec0["pdg"]
    pdg_cut = {k: v[:-7].copy() for k, v in pdg.items()}
    gla64 = D.gauss_laguerre(64)

    def grid(e, sp):
        e.set_momentum_grid(sp["pT"], sp["phi"], sp["y"], sp["eta"], sp["eta_w"])
        e.set_momentum_weights(sp["pT_w"], sp["phi_w"])      # the weights are the grid's

    def params(**kw):
        return dict(state["spec"]["params"], **kw)

    # (name, the new state's entries, the one setter call on the live engine)
    steps = [
        ("species: two of three", dict(spec=lambda: respec(species=sp2)), lambda e, st: species(e, sp2)),
        ("species: back", dict(spec=lambda: respec(species=sp3)), lambda e, st: species(e, sp3)),
        ("classes off", dict(classes=lambda: False), lambda e, st: e.set_species_classes(False)),
        ("grid phi32", dict(spec=lambda: respec(phi=phi32, phi_w=phi32_w)), lambda e, st: grid(e, st["spec"])),
        ("df_mode 2", dict(spec=lambda: respec(params=params(df_mode=2))), lambda e, st: e.set_params(**st["spec"]["params"])),
        ("dimension 3", dict(spec=lambda: respec(params=params(dimension=3))), lambda e, st: e.set_params(**st["spec"]["params"])),
        ("dimension 2", dict(spec=lambda: respec(params=params(dimension=2))), lambda e, st: e.set_params(**st["spec"]["params"])),
        ("pdg", dict(spec=lambda: respec(pdg=pdg_cut)),
         lambda e, st: e.set_pdg(pdg_cut["mass"], pdg_cut["sign"], pdg_cut["gspin"], pdg_cut["baryon"])),
        ("gauss-laguerre 64", dict(spec=lambda: respec(gla=gla64)), lambda e, st: e.set_gauss_laguerre(*gla64)),
        ("df tables at another T_avg", dict(T_avg=lambda: 0.16), lambda e, st: e.set_df_tables(*st["spec"]["df"], 0.16)),
        ("decays", dict(decays=lambda: PIKP_CHANNELS), lambda e, st: e.set_decays(PIKP_CHANNELS)),
        ("species with decays set", dict(spec=lambda: respec(species=sp2), decays=lambda: None), lambda e, st: species(e, sp2)),
    ]
    live = fresh(state)
    got = operations(live, state)
    assert np.any(got["spectra"] != 0.0) and np.any(got["polarization"] != 0.0) and len(got["sample"][0]) > 0
    assert got["feeddown"] == ("error", _lib.IS3D_ERR_STATE) and got["decay_sampled"] == ("error", _lib.IS3D_ERR_STATE)
    for name, change, setter in steps:
        state.update({k: v() for k, v in change.items()})
        setter(live, state)
        got = operations(live, state)
        f = fresh(state)
        want = operations(f, state)
        f.close()
        print(name, {op: r if failed(r) else "ok" for op, r in want.items()})
        for op in want:
            assert same(got[op], want[op]), (name, op)
        # the operations ran: no error stands in for a result, except where no decay channels are set
        for op in ("spectra", "polarization", "sample", "sample_binned"):
            assert not failed(want[op]), (name, op, want[op])
        assert np.any(want["spectra"] != 0.0) and want["sample"][2]["kept"] > 0, name
        for op in ("feeddown", "decay_sampled", "decay_stats"):
            if state["decays"] is None:     # the channels are gone with the species they indexed
                assert want[op] == ("error", _lib.IS3D_ERR_STATE), (name, op, want[op])
            else:
                assert not failed(want[op]), (name, op, want[op])
        if state["decays"] is not None:
            assert not np.array_equal(want["feeddown"], want["spectra"]) and len(want["decay_sampled"][0]) > len(want["sample"][0])
    live.close()
