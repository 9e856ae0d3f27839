"""GPU tier of is3d_sample_decayed: the sampler's compacted batches decayed where they lie, against the
two calls it replaces -- is3d_sample / is3d_sample_famod followed by is3d_decay_sampled -- computed in the same test on
the same engine.  Everything compared is compared for equality: records, offsets, origins, histogram words and every
stats field that does not say how the work was cut (`batches`, `ms_total`).  The base case is
tests/test_gpu_decay_list.py's sampled_case(): 8 case species, decay_ref.CASE_CHANNELS, synth.surface(300, seed=23),
50 events, seed 11, decay seed 5."""
import functools

import numpy as np
import pytest

import decay_list_ref as L
import decay_ref as R
import sampler_famod_ref as F
from is3d2_amd import Engine, IS3DError, _lib, build_engine, make_spec, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

MASS, CHANNELS = R.CASE_MASS, R.CASE_CHANNELS
BINS = dict(pT_min=0.0, pT_max=3.0, pT_bins=12, y_cut=2.0, y_bins=10, phip_bins=12, eta_cut=3.0, eta_bins=12,
            tau_min=0.0, tau_max=12.0, tau_bins=6, r_min=0.0, r_max=12.0, r_bins=6)
NEV, SEED, DSEED = 50, 11, 5
RECORD = np.dtype(_lib.PARTICLE_DTYPE).itemsize


def case_spec(**kw):
    """The 8 species of decay_ref's case table as the chosen species of a sampler run (2+1D, df_mode 1 by default)."""
    kw = dict(dict(df_mode=1, dimension=2), **kw)
    spec = make_spec(chosen="pikp", **kw)
    n = len(MASS)
    spec["species"] = dict(mass=MASS.copy(), sign=np.where(np.isin(np.arange(n), (3, 4, 7)), 1.0, -1.0), degen=np.ones(n),
                           baryon=np.zeros(n), mcid=np.arange(1, n + 1))
    return spec


def case_engine(spec, s, devices=None):
    plasma = O.averages(s, spec["params"]["include_baryon"])
    e = build_engine(spec, s, T_avg=plasma[0], devices=devices)
    e.set_decays(CHANNELS)
    e.set_sample_bins(**BINS)
    return e, plasma


def result(e, out, off, orig, st, binned):
    return dict(out=out, off=off, orig=orig, st=st, st0=e.sample_stats(), hist=e.sample_hist() if binned else None,
                xfer=e.list_transfer_bytes())


def two_step(e, plasma, nev=NEV, dseed=DSEED, binned=True, fast=0, famod=False):
    prim, off0, _ = e.sample_famod(SEED, nev) if famod else e.sample(SEED, nev, 0.5, fast, plasma)
    got = result(e, *e.decay_sampled(dseed, binned=binned), binned)
    got["prim"], got["off0"] = prim, off0
    return got


def fused(e, plasma, nev=NEV, dseed=DSEED, binned=True, fast=0, keep_list=True):
    return result(e, *e.sample_decayed(SEED, nev, dseed, 0.5, fast, plasma, keep_list=keep_list, binned=binned), binned)


def same_hist(a, b):
    return sorted(a) == sorted(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)


def same_stats(got, want):
    for k in L.STAT_KEYS:
        assert got["st"][k] == want["st"][k], k
    for k in want["st0"]:
        if k != "batches":
            assert got["st0"][k] == want["st0"][k], k


def assert_same(got, want, hist=True):
    assert got["out"].tobytes() == want["out"].tobytes()
    assert (got["off"] == want["off"]).all() and (got["orig"] == want["orig"]).all()
    same_stats(got, want)
    if hist:
        assert same_hist(got["hist"], want["hist"])


@functools.lru_cache(maxsize=None)
def base():
    """The two-step result of the base case, once."""
    spec = case_spec()
    s = synth.as_read(synth.surface(300, seed=23))
    e, plasma = case_engine(spec, s)
    want = two_step(e, plasma)
    e.close()
    for k in ("prim", "off0", "out", "off", "orig"):
        want[k].setflags(write=False)
    assert len(want["prim"]) > 1000 and len(want["out"]) > len(want["prim"]) and want["st"]["passes"] == 2
    assert set(L.STAT_KEYS) == {"primaries", "decays", "undecayed", "dropped_daughters", "capped", "final_particles", "passes"}
    return spec, s, plasma, want


# ------------------------------------------------------------------------------------------
# 1. equality with the two calls
# ------------------------------------------------------------------------------------------
def test_one_call_gives_the_bytes_of_the_two_calls():
    spec, s, plasma, want = base()
    e, _ = case_engine(spec, s)
    again = two_step(e, plasma)                                 # the expectation on this engine
    assert_same(again, want)
    got = fused(e, plasma)                                      # list = 1, bin = 1
    assert_same(got, want)
    assert e.lib.is3d_sample_count(e._e) == len(want["out"]) and got["st"]["ms_total"] > 0
    nobin = fused(e, plasma, binned=False)                      # list = 1, bin = 0: the same list
    assert_same(nobin, want, hist=False)
    with pytest.raises(IS3DError) as ei:                        # ... and no histogram, as after is3d_sample
        e.sample_hist()
    assert ei.value.code == _lib.IS3D_ERR_STATE
    other = fused(e, plasma, dseed=6)
    assert other["out"].tobytes() != want["out"].tobytes() and other["st"]["primaries"] == want["st"]["primaries"]
    assert_same(two_step(e, plasma, dseed=6), other)
    e.close()


# ------------------------------------------------------------------------------------------
# 2. batching regimes
# ------------------------------------------------------------------------------------------
def test_every_batching_regime_gives_the_same_bytes():
    """"sample_bytes" bounds from several events a batch down to one event in several cell windows.  What a bound
    reached is read from the stats: the sampler's batches against the events, the decay stage's ranges against the
    sampler's batches.  Every regime has to be reached by some bound, and every bound gives the default bound's bytes."""
    spec, s, plasma, want = base()
    e, _ = case_engine(spec, s)
    reached = set()
    for bound in (6000000, 2500000, 900000, 400000, 120000):
        e.set_tuning("sample_bytes", bound)
        got = fused(e, plasma)
        sb, db = e.get_tuning("sample_batches"), got["st"]["batches"]
        assert sb == got["st0"]["batches"]
        regime = "several events" if 1 < sb < NEV else "one event" if sb == NEV else "cell windows" if sb > NEV else "one batch"
        reached.add(regime)
        if db > sb:
            reached.add("sub-ranges")
        print("sample_bytes %7d: %3d sampler batches of %d events (%s), %3d decay ranges" % (bound, sb, NEV, regime, db))
        assert_same(got, want)
        hist_only = fused(e, plasma, keep_list=False)
        assert same_hist(hist_only["hist"], want["hist"])
        same_stats(hist_only, want)
    assert {"several events", "one event", "cell windows", "sub-ranges"} <= reached, reached
    e.set_tuning("sample_bytes", -1)
    assert e.get_tuning("sample_bytes") == 1 << 30
    got = fused(e, plasma)
    assert_same(got, want)
    assert got["st0"]["batches"] == 1 and got["st"]["batches"] == 1
    e.close()


# ------------------------------------------------------------------------------------------
# 3. binned only: no record crosses to the host
# ------------------------------------------------------------------------------------------
def test_binned_only_moves_no_record():
    spec, s, plasma, want = base()
    e, _ = case_engine(spec, s)
    got = fused(e, plasma, keep_list=False)
    assert same_hist(got["hist"], want["hist"])
    assert e.lib.is3d_sample_count(e._e) == 0 and len(got["out"]) == 0 and len(got["orig"]) == 0
    assert len(got["off"]) == NEV + 1 and (got["off"] == 0).all()
    same_stats(got, want)
    assert got["xfer"] == (0, 0)
    one = np.zeros(1, dtype=np.int64)
    ptr = one.ctypes.data_as(_lib.C.POINTER(_lib.C.c_long))
    assert e.lib.is3d_get_particle_origins(e._e, 0, 0, ptr) == _lib.IS3D_OK
    assert e.lib.is3d_get_particle_origins(e._e, 0, 1, ptr) == _lib.IS3D_ERR_ARG
    with pytest.raises(IS3DError) as ei:                        # nothing for is3d_decay_sampled to decay again
        e.decay_sampled(DSEED)
    assert ei.value.code == _lib.IS3D_ERR_STATE
    listed = fused(e, plasma)
    assert listed["xfer"] == (0, len(want["out"]) * (RECORD + 8)) and RECORD == 96
    e.sample(SEED, NEV, 0.5, 0, plasma)
    assert e.list_transfer_bytes() == (0, len(want["prim"]) * RECORD)
    e.decay_sampled(DSEED)
    assert e.list_transfer_bytes() == (len(want["prim"]) * (RECORD + 4), len(want["out"]) * (RECORD + 8))
    assert want["xfer"][0] > 0
    e.close()


# ------------------------------------------------------------------------------------------
# 4. the other methods, each against its own two calls
# ------------------------------------------------------------------------------------------
def method_case(name):
    if name == "3+1D mode 2 fast":
        return case_spec(df_mode=2, dimension=3), synth.as_read(synth.surface(300, seed=23, dimension=3, full3d=True)), 1, 20
    if name == "mode 4 breakdown":
        return case_spec(df_mode=4, dimension=3, deta_min=1e9), synth.as_read(synth.surface(300, seed=23, dimension=3, full3d=True)), 0, 20
    return case_spec(df_mode=5, dimension=2), F.uniform_surface(300, 2), 0, 16


@pytest.mark.parametrize("name", ["3+1D mode 2 fast", "mode 4 breakdown", "famod"])
def test_other_methods(name):
    spec, s, fast, nev = method_case(name)
    famod = name == "famod"
    e, plasma = case_engine(spec, s)
    want = two_step(e, plasma, nev=nev, fast=fast, famod=famod)
    fst = e.sample_famod_stats() if famod else None
    assert len(want["prim"]) > 300 and want["st"]["decays"] > 50
    if name == "mode 4 breakdown":
        assert want["st0"]["breakdown"] > 0
    got = fused(e, None if famod else plasma, nev=nev, fast=fast)
    assert_same(got, want)
    if famod:
        assert e.sample_famod_stats() == fst and fst["iterations"] > 0
    else:
        with pytest.raises(IS3DError):
            e.sample_famod_stats()
    e.set_tuning("sample_bytes", 60000)
    cut = fused(e, plasma, nev=nev, fast=fast)
    assert cut["st0"]["batches"] > 1
    assert_same(cut, want)
    hist_only = fused(e, plasma, nev=nev, fast=fast, keep_list=False)
    assert same_hist(hist_only["hist"], want["hist"]) and hist_only["xfer"] == (0, 0)
    if famod:
        assert e.sample_famod_stats() == fst
    e.close()


# ------------------------------------------------------------------------------------------
# 5. edges
# ------------------------------------------------------------------------------------------
def test_cell_window_small_and_empty_surfaces_and_a_device_list():
    spec, s, plasma, want = base()
    e, _ = case_engine(spec, s)
    e.set_cell_window(40, 170)
    w = two_step(e, plasma)
    assert 0 < len(w["prim"]) < len(want["prim"])
    assert_same(fused(e, plasma), w)
    e.set_cell_window(-1, -1)
    # two cells: several events hold nothing, and the empty events of a batch share their bound with the next
    e.set_surface({k: v[:2] for k, v in s.items()})
    few = two_step(e, plasma)
    empty = int((np.diff(few["off0"]) == 0).sum())
    assert 2 <= empty < NEV and len(few["prim"]) > 0
    assert_same(fused(e, plasma), few)
    e.set_tuning("sample_bytes", 40000)
    cut = fused(e, plasma)
    assert cut["st0"]["batches"] > 1
    assert_same(cut, few)
    e.set_tuning("sample_bytes", -1)
    # no cell: no primary at all
    e.set_surface({k: v[:0] for k, v in s.items()})
    none = two_step(e, plasma)
    got = fused(e, plasma)
    assert len(none["out"]) == 0 and none["st"]["primaries"] == 0
    assert_same(got, none)
    assert (got["off"] == 0).all() and len(got["off"]) == NEV + 1 and got["st"]["passes"] == 2
    e.close()
    # two shards on one device: the present sequence underneath
    g, _ = case_engine(spec, s, devices=[0, 0])
    got = fused(g, plasma)
    assert_same(got, want)
    assert got["xfer"][0] == len(want["prim"]) * (RECORD + 4)
    hist_only = fused(g, plasma, keep_list=False)
    assert same_hist(hist_only["hist"], want["hist"]) and len(hist_only["out"]) == 0 and (hist_only["off"] == 0).all()
    same_stats(hist_only, want)
    assert g.lib.is3d_sample_count(g._e) == 0
    g.close()


# ------------------------------------------------------------------------------------------
# 6. errors
# ------------------------------------------------------------------------------------------
def test_errors_leave_no_list_and_a_usable_engine():
    spec, s, plasma, want = base()
    e, _ = case_engine(spec, s)

    def refused(code, *words, **kw):
        a = dict(seed=SEED, n_events=NEV, decay_seed=DSEED, y_cut=0.5, fast=0, plasma=plasma, keep_list=True, binned=True)
        a.update(kw)
        with pytest.raises(IS3DError) as ei:
            e.sample_decayed(**a)
        assert ei.value.code == code, str(ei.value)
        for word in words:
            assert word in str(ei.value), str(ei.value)
        assert e.lib.is3d_sample_count(e._e) == -1

    fused(e, plasma)
    refused(_lib.IS3D_ERR_ARG, keep_list=False, binned=False)
    refused(_lib.IS3D_ERR_ARG, seed=-1)
    refused(_lib.IS3D_ERR_ARG, decay_seed=-1)
    refused(_lib.IS3D_ERR_ARG, n_events=0)
    refused(_lib.IS3D_ERR_ARG, plasma=None)
    e.set_tuning("sample_bytes", 64)
    refused(_lib.IS3D_ERR_ARG, "sample_bytes", "bytes")
    e.set_tuning("sample_bytes", -1)
    assert_same(fused(e, plasma), want)
    e.close()
    # no decays set; bin = 1 without bins
    plain = build_engine(spec, s, T_avg=plasma[0])
    e = plain
    refused(_lib.IS3D_ERR_STATE, "is3d_set_decays", binned=False)
    e.set_decays(CHANNELS)
    refused(_lib.IS3D_ERR_STATE, "is3d_set_sample_bins")
    assert_same(fused(e, plasma, binned=False), want, hist=False)
    e.close()
    # df_mode 5 without a PDG table
    e = Engine()
    e.set_params(**case_spec(df_mode=5)["params"])
    sp = spec["species"]
    e.set_species(sp["mass"], sp["sign"], sp["degen"], sp["baryon"])
    e.set_momentum_grid(spec["pT"], spec["phi"], spec["y"], spec["eta"], spec["eta_w"])
    e.set_decays(CHANNELS)
    refused(_lib.IS3D_ERR_STATE, "is3d_set_pdg", binned=False)
    e.close()
    # a plan of more than 16 levels: the path code has 32 bits
    mass17 = 0.1 * 2.5 ** np.arange(18)
    deep = case_spec()
    deep["species"] = dict(mass=mass17, sign=-np.ones(18), degen=np.ones(18), baryon=np.zeros(18), mcid=np.arange(1, 19))
    e = build_engine(deep, s, T_avg=plasma[0])
    e.set_decays([R.channel(k, [k - 1, k - 1], 1.0, mass17[k], [mass17[k - 1], mass17[k - 1]]) for k in range(1, 18)])
    refused(_lib.IS3D_ERR_ARG, "16", binned=False)
    e.close()
