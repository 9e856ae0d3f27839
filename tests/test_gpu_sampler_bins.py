"""GPU tier of the sampler's test_sampler = 1 binned distributions (is3d_sample_binned: k_sample's binned variants in
is3d2_amd/csrc/sampler.hip, the binning math of sampler_bins.h).

The histograms are a pure function of (seed, inputs, bins): the counts are the numpy binning of the list the same call
returns, and the same bits whatever the batches, the cell windows, the devices or whether a list is kept.

Edge-ambiguous particles.  The index of a coordinate that comes from atan2 or log (y, phip, phis) is only determined
when the coordinate is not within 1e-12 max(1, |v|) of a bin edge or range end: there the last bits of the device's and
numpy's libm may differ.  ~1e5 coordinates x 1e-12 / bin width ~ 1e-6 such particles are expected per test; the tests
assert that their fixed seeds have none -- a condition on the inputs, not a tolerance on the kernel.  Every other
coordinate (eta, pT, tau, r) is exactly determined and compared without condition.

vn: the fixed-point sums carry at most q / 2 = 2^-33 per particle and the harmonics 1e-13 (recurrence against
cos / sin (k atan2), tests/test_sampler_bins_cpu.py), so a bin of n particles agrees within n (q / 2 + 1e-13)."""
import glob
import os

import numpy as np
import pytest

from is3d2_amd import IS3DError, build_engine, make_spec, synth
from is3d2_amd import _lib
from oracle import oracle as O

import sampler_bins_ref as B

pytestmark = pytest.mark.gpu

N_CELLS = 300
PI_SCALE = 0.125          # synth's pi and Pi scaled as tests/test_gpu_sampler.py's uniform_surface does
BINS = B.TEST_BINS        # 12 pT / 10 y / 8 phi / 14 eta / 6 tau / 5 r, ranges cutting into the populated region
COUNT_PARTS = [name for name, _ in B.PARTS]


def surface(dimension, n=N_CELLS, seed=23, volume=1.0):
    s = synth.surface(n, seed=seed, dimension=dimension, full3d=(dimension == 3))
    for k in ("pixx", "pixy", "pixn", "piyy", "piyn", "bulkPi"):
        s[k] *= PI_SCALE
    for k in ("dat", "dax", "day", "dan"):
        s[k] *= volume
    return synth.as_read(s)


def setup(dimension, mode, **kw):
    """(engine with BINS set, spec, surface, plasma, n_events, y_cut): pikp in 2+1D, the SMASH list in 3+1D."""
    spec = make_spec(chosen="pikp" if dimension == 2 else "smash", df_mode=mode, dimension=dimension)
    s = surface(dimension)
    plasma = O.averages(s, 0)
    e = build_engine(spec, s, T_avg=plasma[0], **kw)
    e.set_sample_bins(**BINS)
    return e, spec, s, plasma, (8 if dimension == 2 else 4), 0.5


def same_hist(a, b):
    return all(a[k].tobytes() == b[k].tobytes() and a[k].shape == b[k].shape for k in COUNT_PARTS + ["vn_real", "vn_imag"])


def add_hist(a, b):
    return {k: a[k] + b[k] for k in a}


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("mode", [1, 4])
@pytest.mark.parametrize("dimension", [2, 3])
def test_the_histogram_is_the_binning_of_the_list(dimension, mode, fast):
    e, spec, s, plasma, nev, y_cut = setup(dimension, mode)
    hist, st, p, off = e.sample_binned(5, nev, y_cut, fast, plasma, keep_list=True)
    q, off_q, st_q = e.sample(5, nev, y_cut, fast, plasma)
    e.close()
    npart = len(spec["species"]["mass"])
    # the list keeps its bytes
    assert p.tobytes() == q.tobytes() and (off == off_q).all() and len(p) > 1000
    assert st == st_q and st["kept"] == len(p) and st["capped"] == 0
    # 2+1D: the sampler bins the drawn rapidity, which is the one of (E, pz) to rounding
    rap = B.rapidity_from_momentum(p)
    assert B.ambiguous(p, rap, BINS) == 0
    want = B.np_hist(p, rap, BINS, npart)
    for name in COUNT_PARTS:
        assert hist[name].dtype == np.int64 and hist[name].shape == want[name].shape
        np.testing.assert_array_equal(hist[name], want[name], err_msg=name)
        if "dphi" in name:
            assert hist[name].sum() == len(p)
        else:
            assert 0 < hist[name].sum() < len(p), name          # the drop logic is exercised
    nbin = hist["pT_count"][None, :, :]
    for name in ("vn_real", "vn_imag"):
        err = np.abs(hist[name] - want[name])
        print("%dD mode %d fast %d %s: %d particles, max |delta| %.3e, max |delta| / bound %.3f" %
              (dimension, mode, fast, name, len(p), err.max(), (err / np.maximum(nbin * (B.Q / 2 + 1e-13), 1e-300)).max()))
        assert (err <= nbin * (B.Q / 2 + 1e-13)).all(), name
        assert (hist[name][:, hist["pT_count"] == 0] == 0.0).all()


@pytest.mark.parametrize("dimension,mode,fast", [(2, 1, 0), (3, 4, 1)])
def test_binned_only_equals_binned_with_list_for_every_batch_window_and_device_list(dimension, mode, fast):
    e, spec, s, plasma, nev, y_cut = setup(dimension, mode)
    ref, st_l, p, off = e.sample_binned(5, nev, y_cut, fast, plasma, keep_list=True)
    hist, st = e.sample_binned(5, nev, y_cut, fast, plasma)
    assert same_hist(hist, ref)
    assert e.lib.is3d_sample_count(e._e) == 0
    off0 = np.ones(nev + 1, dtype=np.int64)
    e._chk(e.lib.is3d_sample_offsets(e._e, off0.ctypes.data_as(_lib.C.POINTER(_lib.C.c_long))))
    assert (off0 == 0).all()
    assert st["kept"] == st_l["kept"] == len(p) and st["candidates"] == st_l["candidates"]
    assert {k: st[k] for k in st if k != "batches"} == {k: st_l[k] for k in st_l if k != "batches"}
    assert st["batches"] == 1
    # repeated calls
    again, st_a = e.sample_binned(5, nev, y_cut, fast, plasma)
    assert same_hist(again, ref) and st_a == st
    other, _ = e.sample_binned(6, nev, y_cut, fast, plasma)
    assert not same_hist(other, ref)
    # batches of cells: 100 (event, cell) pairs at 12 bytes each
    e.set_tuning("sample_bytes", 1200)
    hb, st_b = e.sample_binned(5, nev, y_cut, fast, plasma)
    assert st_b["batches"] == 3 * nev >= 4 and same_hist(hb, ref) and st_b["kept"] == st["kept"]
    # batches of events: two events a batch
    e.set_tuning("sample_bytes", 12 * 2 * N_CELLS + 8)
    hb, st_b = e.sample_binned(5, nev, y_cut, fast, plasma)
    assert st_b["batches"] == nev // 2 >= 2 and same_hist(hb, ref)
    # the list path's own batches, binned
    e.set_tuning("sample_bytes", 100000)
    hb, st_b, pb, _ = e.sample_binned(5, nev, y_cut, fast, plasma, keep_list=True)
    assert st_b["batches"] >= 4 and same_hist(hb, ref) and pb.tobytes() == p.tobytes()
    e.set_tuning("sample_bytes", -1)
    # two cell windows added on the host (the vn sums are multiples of q below 2^53 q: their double sum is exact)
    e.set_cell_window(0, 120)
    w0, s0 = e.sample_binned(5, nev, y_cut, fast, plasma)
    e.set_cell_window(120, N_CELLS)
    w1, s1 = e.sample_binned(5, nev, y_cut, fast, plasma)
    e.set_cell_window(-1, -1)
    assert same_hist(add_hist(w0, w1), ref) and s0["kept"] + s1["kept"] == st["kept"]
    e.close()
    # two shards on one device
    g = build_engine(spec, s, T_avg=plasma[0], devices=[0, 0])
    g.set_sample_bins(**BINS)
    hg, st_g = g.sample_binned(5, nev, y_cut, fast, plasma)
    hl, st_gl, pg, _ = g.sample_binned(5, nev, y_cut, fast, plasma, keep_list=True)
    g.close()
    assert same_hist(hg, ref) and same_hist(hl, ref) and pg.tobytes() == p.tobytes()
    assert st_g["kept"] == st["kept"] and st_g["candidates"] == st["candidates"]


def test_a_binned_only_call_needs_no_memory_per_candidate():
    """Cells 40 times synth's volume draw tens of candidates per (cell, event).  Bound: the 12 bytes of every
    (event, cell) pair of one event plus 64 -- the list path cannot fit one cell's candidates (204 bytes each) in it,
    the binned-only path needs nothing more."""
    dimension, mode, nev = 2, 1, 4
    spec = make_spec(chosen="pikp", df_mode=mode, dimension=dimension)
    s = surface(dimension, volume=40.0)
    plasma = O.averages(s, 0)
    e = build_engine(spec, s, T_avg=plasma[0])
    e.set_sample_bins(**BINS)
    ref, st = e.sample_binned(9, nev, 0.5, 0, plasma)
    assert st["batches"] == 1 and st["candidates"] > 20 * N_CELLS * nev
    e.set_tuning("sample_bytes", 12 * N_CELLS + 64)
    with pytest.raises(IS3DError) as ei:
        e.sample(9, nev, 0.5, 0, plasma)
    assert ei.value.code == _lib.IS3D_ERR_ARG and "sample_bytes" in str(ei.value)
    with pytest.raises(IS3DError) as ei:
        e.sample_binned(9, nev, 0.5, 0, plasma, keep_list=True)
    assert ei.value.code == _lib.IS3D_ERR_ARG
    hist, st_b = e.sample_binned(9, nev, 0.5, 0, plasma)
    e.close()
    assert same_hist(hist, ref) and st_b["batches"] == nev
    assert {k: st_b[k] for k in st if k != "batches"} == {k: st[k] for k in st if k != "batches"}


def test_errors_and_the_empty_surface():
    s = surface(2, n=100, seed=3)
    spec = make_spec(chosen="pikp", df_mode=1, dimension=2)
    plasma = O.averages(s, 0)
    e = build_engine(spec, s, T_avg=plasma[0])
    with pytest.raises(IS3DError) as ei:
        e.sample_binned(1, 2, 0.5, 0, plasma)
    assert ei.value.code == _lib.IS3D_ERR_STATE
    with pytest.raises(IS3DError) as ei:
        e.sample_hist()
    assert ei.value.code == _lib.IS3D_ERR_STATE
    for kw in (dict(pT_bins=0), dict(tau_max=BINS["tau_min"]), dict(tau_max=BINS["tau_min"] - 1.0), dict(eta_cut=0.0),
               dict(eta_cut=-1.0), dict(y_cut=0.0), dict(r_bins=-3), dict(pT_max=BINS["pT_min"]), dict(phip_bins=0)):
        b = dict(BINS)
        b.update(kw)
        with pytest.raises(IS3DError) as ei:
            e.set_sample_bins(**b)
        assert ei.value.code == _lib.IS3D_ERR_ARG, kw
    with pytest.raises(IS3DError) as ei:          # a refused setter sets nothing
        e.sample_binned(1, 2, 0.5, 0, plasma)
    assert ei.value.code == _lib.IS3D_ERR_STATE
    e.set_sample_bins(**BINS)
    for kw, code in [(dict(n_events=0), _lib.IS3D_ERR_ARG), (dict(y_cut=0.0), _lib.IS3D_ERR_ARG), (dict(seed=-1), _lib.IS3D_ERR_ARG)]:
        a = dict(seed=1, n_events=2, y_cut=0.5, fast=0, plasma=plasma)
        a.update(kw)
        with pytest.raises(IS3DError) as ei:
            e.sample_binned(**a)
        assert ei.value.code == code
    hist, st = e.sample_binned(1, 2, 0.5, 0, plasma)
    assert st["kept"] > 0 and hist["dN_dphipdy"].sum() == st["kept"]
    # a list call in between: the histograms of the binned call are gone
    e.sample(1, 2, 0.5, 0, plasma)
    with pytest.raises(IS3DError) as ei:
        e.sample_hist()
    assert ei.value.code == _lib.IS3D_ERR_STATE
    e.set_surface({k: v[:0] for k, v in s.items()})
    for keep in (False, True):
        out = e.sample_binned(1, 5, 0.5, 0, plasma, keep_list=keep)
        assert all((out[0][k] == 0).all() for k in out[0]) and out[1]["candidates"] == 0 and out[1]["kept"] == 0
        assert out[0]["pT_count"].shape == (3, BINS["pT_bins"]) and out[0]["vn_imag"].shape == (7, 3, BINS["pT_bins"])
    e.close()
    spec5 = make_spec(chosen="pikp", df_mode=5, dimension=2)
    e5 = build_engine(spec5, s, T_avg=plasma[0])
    e5.set_sample_bins(**BINS)
    with pytest.raises(IS3DError) as ei:
        e5.sample_binned(1, 2, 0.5, 0, plasma)
    assert ei.value.code == _lib.IS3D_ERR_UNSUPPORTED
    e5.close()


def test_dropin_run_directory_writes_the_sampled_tree_and_no_list(tmp_path):
    """test_sampler = 1: results/sampled/* as the reference's writers format Engine.sample_binned's histograms, no
    particle list; test_sampler = 0 in the same directory: lists as before and no results/sampled."""
    from is3d2_amd import host, rundir
    s = synth.surface(200, seed=43)
    params = dict(operation=2, dimension=2, df_mode=1, include_baryon=0, include_bulk_deltaf=1, include_shear_deltaf=1,
                  include_baryondiff_deltaf=0, regulate_deltaf=0, outflow=0, deta_min=1e-5, mass_pion0=0.138, oversample=1,
                  min_num_hadrons=2000.0, max_num_samples=100.0, sampler_seed=77, fast=0, test_sampler=1)
    bins = dict(BINS)
    bins["y_cut"] = 0.75                   # the run directory has one y_cut: the sampler's window and the binning's
    params.update(bins)
    d = rundir.write_run_dir(str(tmp_path / "binned"), s, params, hrg_eos=2, chosen="pikp", surface_format=1)
    lists = lambda d: sorted(glob.glob(os.path.join(d, "results", "particle_list*")))
    got = host.sample(d, write_files=True, write_csv=True)
    nev = got["n_events"]
    assert len(got["particles"]) == 0 and len(got["mcid"]) == 0 and (got["offsets"] == 0).all() and len(got["offsets"]) == nev + 1
    assert nev > 1 and got["seed"] == 77 and lists(d) == []
    spec = make_spec(hrg_eos=2, chosen="pikp", **{k: v for k, v in params.items() if k != "operation"})
    fields, avg = host.read_surface(d, 1, 2, 0)
    surf = {k: fields[i] for i, k in enumerate(synth.FIELDS)}
    e = build_engine(spec, surf, T_avg=avg[0])
    e.set_sample_bins(**bins)
    hist, st = e.sample_binned(77, nev, 0.75, 0, avg)
    e.close()
    assert st["kept"] > 500 and same_hist(got["hist"], hist) and got["stats"] == st
    mcids = [int(m) for m in spec["species"]["mcid"]]
    want = B.expected_files(hist, bins, nev, mcids)
    tree = B.read_tree(os.path.join(d, "results", "sampled"))
    assert sorted(tree) == sorted(want) and len(tree) == 9 * len(mcids)
    for name in sorted(want):
        assert tree[name] == want[name], name
    # the same directory with test_sampler = 0
    params0 = dict(params, test_sampler=0)
    d0 = rundir.write_run_dir(str(tmp_path / "lists"), s, params0, hrg_eos=2, chosen="pikp", surface_format=1)
    got0 = host.sample(d0, write_files=True, write_csv=False)
    assert got0["hist"] is None and got0["n_events"] == nev and len(got0["particles"]) == st["kept"]
    assert [os.path.basename(f) for f in lists(d0)] == sorted("particle_list_osc_%d.dat" % (k + 1) for k in range(nev))
    assert not os.path.exists(os.path.join(d0, "results", "sampled"))


def test_the_eta_histogram_accounts_for_every_kept_particle():
    """3+1D SMASH, eta_cut beyond the surface's |eta| < 4 and pT_max = 50 GeV: the dN_deta counts sum to kept minus the
    list's out-of-range particles (none in eta: the particle's eta is its cell's), species by species."""
    e, spec, s, plasma, nev, y_cut = setup(3, 2)
    bins = dict(BINS, eta_cut=5.0, eta_bins=9, pT_min=0.0, pT_max=50.0)
    e.set_sample_bins(**bins)
    hist, st, p, off = e.sample_binned(13, nev, y_cut, 0, plasma, keep_list=True)
    only, st_o = e.sample_binned(13, nev, y_cut, 0, plasma)
    e.close()
    npart = len(spec["species"]["mass"])
    out_eta = int((B.np_index(p["eta"], -bins["eta_cut"], B.widths(bins)["eta"], bins["eta_bins"]) < 0).sum())
    pT = np.sqrt(p["px"] * p["px"] + p["py"] * p["py"])
    out_pT = int((B.np_index(pT, 0.0, B.widths(bins)["pT"], bins["pT_bins"]) < 0).sum())
    assert out_eta == 0 and np.abs(s["eta"]).max() < bins["eta_cut"]
    for h, stats in ((hist, st), (only, st_o)):
        assert h["dN_deta"].sum() == stats["kept"] - out_eta == len(p)
        assert h["pT_count"].sum() == stats["kept"] - out_pT
        np.testing.assert_array_equal(h["dN_deta"].sum(axis=1), np.bincount(p["species"], minlength=npart))
