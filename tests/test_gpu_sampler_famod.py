"""GPU tier of the df_mode 5 (PTMA) particle sampler (is3d_sample_famod: the Newton prepass under the sampler's chain
rule -- k_prep<PTMA>, k_chain_pass / _finish / _count or k_aniso -- then the famod variants of k_cells and k_sample in
is3d2_amd/csrc/sampler.hip).

The list and the histograms are a pure function of (seed, inputs): the same bytes whatever the batches, the cell windows
or the devices.  Statistical bars are derived (tests/sampler_ref.py): 5 sqrt(mu) for a count, 5 standard errors for a
mean; none is tuned.  U(dim) and Q are the surfaces of tests/sampler_famod_ref.py."""
import glob
import os

import numpy as np
import pytest

from is3d2_amd import IS3DError, build_engine, make_spec, synth
from is3d2_amd import _lib
from oracle import oracle as O

import sampler_bins_ref as B
import sampler_famod_ref as F
import sampler_ref as R

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
BINS = B.TEST_BINS
COUNT_PARTS = [name for name, _ in B.PARTS]
_cache = {}


def q_chain(chains):
    """The restatement of the sampler's chain rule on Q (tests/test_sampler_famod_cpu.py checks it), once per C."""
    if chains not in _cache:
        spec = make_spec(chosen="pikp", df_mode=5, dimension=3)
        _cache[chains] = F.sampler_chain(spec, F.surface_q(), chains)
    return _cache[chains]


def same_hist(a, b):
    return all(a[k].tobytes() == b[k].tobytes() and a[k].shape == b[k].shape for k in COUNT_PARTS + ["vn_real", "vn_imag"])


def add_hist(a, b):
    return {k: a[k] + b[k] for k in a}


def merge_windows(lists, n_events):
    out = []
    for ev in range(n_events):
        for parts, off in lists:
            out.append(parts[off[ev]:off[ev + 1]])
    return np.concatenate(out)


def seed_case(name):
    if name == "Qb":         # Q with a chemical potential: the exp(Ebar + chem) weights and chem in sample_momentum
        return make_spec(chosen="pikp", df_mode=5, dimension=3, include_baryon=1), F.surface_q(baryon=True), 301
    dim = int(name[1])
    return make_spec(chosen="pikp", df_mode=5, dimension=dim), F.uniform_surface(300, dim), 120


@pytest.mark.parametrize("name", ["U2", "U3", "Qb"])
def test_the_list_and_the_histograms_depend_on_the_seed_and_nothing_else(name):
    nev = 16
    spec, s, cut = seed_case(name)
    n = len(s["tau"])
    npart = len(spec["species"]["mass"])
    e = build_engine(spec, s)
    e.set_sample_bins(**BINS)
    a, off_a, st = e.sample_famod(11, nev)
    fst = e.sample_famod_stats()
    b, off_b, _ = e.sample_famod(11, nev)
    assert len(a) > 1000 and st["capped"] == 0 and st["batches"] == 1 and st["kept"] == len(a) and st["cells"] == n
    assert a.tobytes() == b.tobytes() and (off_a == off_b).all() and e.sample_famod_stats() == fst
    # the histograms: binned with the list = the list + the numpy binning of it; binned only = the same bits
    ref, st_l, p, off = e.sample_famod_binned(11, nev, keep_list=True)
    assert p.tobytes() == a.tobytes() and (off == off_a).all() and st_l == st
    rap = B.rapidity_from_momentum(p)
    assert B.ambiguous(p, rap, BINS) == 0
    want = B.np_hist(p, rap, BINS, npart)
    for part in COUNT_PARTS:
        np.testing.assert_array_equal(ref[part], want[part], err_msg=part)
    hist, st_h = e.sample_famod_binned(11, nev)
    assert same_hist(hist, ref) and e.lib.is3d_sample_count(e._e) == 0
    assert {k: st_h[k] for k in st if k != "batches"} == {k: st[k] for k in st if k != "batches"}
    # several event batches
    e.set_tuning("sample_bytes", 200000)
    c, off_c, st_c = e.sample_famod(11, nev)
    assert st_c["batches"] > 3 and c.tobytes() == a.tobytes() and (off_c == off_a).all()
    hb, st_b, pb, _ = e.sample_famod_binned(11, nev, keep_list=True)
    assert st_b["batches"] > 3 and same_hist(hb, ref) and pb.tobytes() == a.tobytes()
    # one event in several batches of cells
    e.set_tuning("sample_bytes", 20000)
    c1, _, st_c1 = e.sample_famod(11, 3)
    assert st_c1["batches"] > 3 and c1.tobytes() == a[:off_a[3]].tobytes()
    e.set_tuning("sample_bytes", 1200)                 # binned only: 100 (event, cell) pairs a batch
    hb, st_b = e.sample_famod_binned(11, nev)
    assert st_b["batches"] == -(-n // 100) * nev and same_hist(hb, ref) and st_b["kept"] == st["kept"]
    e.set_tuning("sample_bytes", -1)
    # two cell windows (Q: cut in the middle of a chain segment): the chain walks every cell whatever window is sampled
    e.set_cell_window(0, cut)
    w0 = e.sample_famod(11, nev)
    f0 = e.sample_famod_stats()
    h0, _ = e.sample_famod_binned(11, nev)
    e.set_cell_window(cut, n)
    w1 = e.sample_famod(11, nev)
    h1, _ = e.sample_famod_binned(11, nev)
    e.set_cell_window(-1, -1)
    assert merge_windows([w0[:2], w1[:2]], nev).tobytes() == a.tobytes()
    assert (w0[1] + w1[1] == off_a).all() and w0[2]["breakdown"] + w1[2]["breakdown"] == st["breakdown"]
    assert same_hist(add_hist(h0, h1), ref) and f0 == fst == e.sample_famod_stats()
    # another seed
    d, _, _ = e.sample_famod(12, nev)
    assert d.tobytes() != a.tobytes()
    e.close()
    # two shards on one device: each solves the whole chain and samples its window
    g = build_engine(spec, s, devices=[0, 0])
    g.set_sample_bins(**BINS)
    h, off_h, st_h = g.sample_famod(11, nev)
    fg = g.sample_famod_stats()
    hg, st_g = g.sample_famod_binned(11, nev)
    hl, _, pg, _ = g.sample_famod_binned(11, nev, keep_list=True)
    g.close()
    assert h.tobytes() == a.tobytes() and (off_h == off_a).all() and pg.tobytes() == a.tobytes()
    assert st_h["candidates"] == st["candidates"] and st_h["kept"] == len(a) and st_h["breakdown"] == st["breakdown"]
    assert fg == fst and same_hist(hg, ref) and same_hist(hl, ref) and st_g["kept"] == st["kept"]


def test_cold_cells_on_a_device_list():
    """famod_chains = 0: the shards hold their windows and solve them cold; the list, the histogram and the summed
    counters are the one-device ones."""
    nev = 8
    spec = make_spec(chosen="pikp", df_mode=5, dimension=3, famod_chains=0)
    s = F.surface_q()
    e = build_engine(spec, s)
    e.set_sample_bins(**BINS)
    a, off_a, st = e.sample_famod(11, nev)
    fst = e.sample_famod_stats()
    ref, _ = e.sample_famod_binned(11, nev)
    e.close()
    g = build_engine(spec, s, devices=[0, 0])
    g.set_sample_bins(**BINS)
    h, off_h, st_h = g.sample_famod(11, nev)
    fg = g.sample_famod_stats()
    hg, _ = g.sample_famod_binned(11, nev)
    g.close()
    assert len(a) > 1000 and h.tobytes() == a.tobytes() and (off_h == off_a).all() and same_hist(hg, ref)
    assert fg == fst and st_h["breakdown"] == st["breakdown"] and st_h["kept"] == st["kept"]


@pytest.mark.parametrize("dimension", [2, 3])
def test_invariants_of_every_particle(dimension):
    """Q with the SMASH species.  Tolerances as tests/test_gpu_sampler.py: 8 ulp of E^2 for the mass shell, 16 ulp for
    t = tau cosh(eta) and z = tau sinh(eta)."""
    nev, y_cut = 20, 0.8
    spec = make_spec(chosen="smash", df_mode=5, dimension=dimension)
    s = F.surface_q()
    n = len(s["tau"])
    e = build_engine(spec, s)
    p, off, st = e.sample_famod(3, nev, y_cut)
    e.close()
    assert len(p) > 1000 and st["capped"] == 0 and st["kept"] == len(p) and st["cells"] == n and st["breakdown"] > 10
    assert off[0] == 0 and off[-1] == len(p) and (np.diff(off) >= 0).all()
    npart = len(spec["species"]["mass"])
    assert (p["species"] >= 0).all() and (p["species"] < npart).all()
    assert (p["cell"] >= 0).all() and (p["cell"] < n).all()
    for ev in range(nev):
        q = p[off[ev]:off[ev + 1]]
        assert (q["event"] == ev).all()
        assert (np.diff(q["cell"]) >= 0).all()           # ordered by cell inside an event
    c = p["cell"]
    m = spec["species"]["mass"][p["species"]]
    E2 = p["E"] ** 2
    shell = np.abs(E2 - p["px"] ** 2 - p["py"] ** 2 - p["pz"] ** 2 - m * m)
    print("%dD: %d particles, max |E^2 - p^2 - m^2| / (ulp E^2) = %.2f" % (dimension, len(p), float(np.max(shell / (EPS * E2)))))
    assert (shell <= 8 * EPS * E2).all()
    for k in ("tau", "x", "y"):
        np.testing.assert_array_equal(p[k], s[k][c])
    tau = p["tau"]
    assert (np.abs(p["t"] - tau * np.cosh(p["eta"])) <= 16 * EPS * p["t"]).all()
    assert (np.abs(p["z"] - tau * np.sinh(p["eta"])) <= 16 * EPS * (np.abs(p["z"]) + tau)).all()
    rap = 0.5 * np.log((p["E"] + p["pz"]) / (p["E"] - p["pz"]))
    if dimension == 3:
        np.testing.assert_array_equal(p["eta"], s["eta"][c])
    else:
        assert (np.abs(rap) <= y_cut * (1 + 1e-12)).all()
    mT = np.sqrt(m * m + p["px"] ** 2 + p["py"] ** 2)
    ptau, pn = mT * np.cosh(rap - p["eta"]), mT * np.sinh(rap - p["eta"]) / tau
    pds = ptau * s["dat"][c] + p["px"] * s["dax"][c] + p["py"] * s["day"][c] + pn * s["dan"][c]
    assert (pds > 0).all()
    uds = F.lrf(spec, s)["uds"]
    assert (uds <= 0).sum() > 5 and (uds[c] > 0).all()


def exact_mu(spec, s, nev, y_max=0.5):
    """mu and mu per species at the oracle chain's (lambda, aT, aL): f_a,mod is even in p, so of p.dsigma only
    E dsigma_t = E (u.dsigma) survives the momentum integral and a cell emits 2 y_max (u.dsigma) n_a.  Conditions on the
    input, asserted: no pl / pt < 0, no failure, no det B breakdown."""
    n = len(s["tau"])
    L = F.lrf(spec, s)
    assert (L["uds"] > 0).all()
    states, _, _ = O.FamodChain(spec, s).walk(np.arange(n), np.zeros(4))
    assert (states[:, 0] == 1).all() and (L["pl"] >= 0).all() and (L["pt"] >= 0).all()
    ref = F.sampler_chain(spec, s)
    assert ref["counters"]["plpt_negative"] == 0 and ref["counters"]["reconstruction_fail"] == 0 and not ref["broken"].any()
    emu = F.emu_chain(spec, s)
    assert not F.prologue(dict(spec, params=dict(spec["params"], deta_min=1e-5)), s, emu["sol"])["breaks"].any()
    na = F.densities(spec, states[:, 1], states[:, 2] ** 2 * states[:, 3])
    per = nev * 2 * y_max * (L["uds"][:, None] * na).sum(axis=0)
    return per.sum(), per


@pytest.mark.parametrize("dimension,deta_min", [(2, 1e-5), (3, 1e-5), (3, 1e9)])
def test_exact_yield(dimension, deta_min):
    """mu ~ 1.16e6.  deta_min = 1e9: every cell breaks down on det B (B = 1) at its solved (lambda, aT, aL), and the
    density does not depend on B: the same mu."""
    nev = 4000
    spec = make_spec(chosen="pikp", df_mode=5, dimension=dimension, deta_min=deta_min, include_baryon=0)
    s = F.uniform_surface(300, dimension)
    mu, per = exact_mu(spec, s, nev)
    e = build_engine(spec, s)
    p, off, st = e.sample_famod(7, nev)
    fst = e.sample_famod_stats()
    e.close()
    print("%dD deta_min %g: kept %d, mu %.1f (%.2f sigma), candidates %d, efficiency %.3f, %s" %
          (dimension, deta_min, len(p), mu, (len(p) - mu) / np.sqrt(mu), st["candidates"], st["acceptances"] / st["proposals"], fst))
    assert mu > 9e5 and st["capped"] == 0
    assert st["breakdown"] == (0 if deta_min < 1 else 300) and st["cells"] == 300
    assert fst["plpt_negative"] == 0 and fst["reconstruction_fail"] == 0
    assert abs(len(p) - mu) <= 5 * np.sqrt(mu)
    counts = np.bincount(p["species"], minlength=len(per))
    for i, mcid in enumerate(spec["species"]["mcid"]):
        assert abs(counts[i] - per[i]) <= 5 * np.sqrt(per[i]), (int(mcid), counts[i], per[i])


@pytest.mark.parametrize("chains", [1, 3, 0])
def test_counters_on_q(chains):
    spec = make_spec(chosen="pikp", df_mode=5, dimension=3, famod_chains=chains)
    s = F.surface_q()
    ref = q_chain(chains)
    e = build_engine(spec, s)
    _, _, st = e.sample_famod(5, 2)
    fst = e.sample_famod_stats()
    e.calculate_spectra()
    sp = e.stats()
    e.close()
    print("famod_chains %d: sampler %s, spectra failures %d, restatement %s" % (chains, fst, sp["recon_fail"], ref["counters"]))
    assert fst == ref["counters"]
    assert fst["plpt_negative"] == sp["pl_negative"] > 10
    if chains == 1:      # cell 37, the copy of cell 36: the one failure the spectra's rule does not count
        assert ref["quirk"] == [37] and fst["reconstruction_fail"] == sp["recon_fail"] + 1
    # every broken-down live cell: the chain's causes and det B <= deta_min
    emu = F.emu_cells(spec, s, chains)
    assert st["breakdown"] == int(((emu["live"] != 0) & (emu["breaks"] != 0)).sum()) >= int(ref["broken"].sum())


def test_momentum_distribution_against_the_continuous_spectra():
    """2+1D, synth normals (spacelike ones included), outflow = 1: the oracle's famod integrand is the sampler's density,
    so per species N = 2 y_cut dN/dy, <pT> and v2 of the continuous spectra are the sampled ones' expectations.  The
    quadrature difference (48x32 against 24x24 momentum tables) must stay below a fifth of the statistical sigma, which
    holds at 300 events (the tightest entry, the proton <pT>, measured 0.204 at 400).  No cell of this surface breaks
    down (asserted), so the spectra's and the sampler's chain rules coincide."""
    nev, y_cut = 300, 0.5
    s = synth.as_read(synth.surface(300, seed=37))
    flags = dict(chosen="pikp", df_mode=5, dimension=2, outflow=1)
    spec = make_spec(pT="pT48", phi="phi32", **flags)
    ref = F.sampler_chain(spec, s)
    assert not ref["broken"].any() and ref["quirk"] == []
    fine = R.spectra_moments(spec, s, y_cut)
    coarse = R.spectra_moments(make_spec(pT="pT24", phi="phi24", **flags), s, y_cut)
    e = build_engine(spec, s)
    p, off, st = e.sample_famod(41, nev, y_cut)
    e.close()
    assert st["capped"] == 0 and st["breakdown"] == 0
    pT = np.hypot(p["px"], p["py"])
    c2 = np.cos(2.0 * np.arctan2(p["py"], p["px"]))
    for i, mcid in enumerate(spec["species"]["mcid"]):
        k = p["species"] == i
        mu = nev * fine[0][i]
        sig = (np.sqrt(mu), fine[3][i] / np.sqrt(mu), c2[k].std() / np.sqrt(mu))
        got = (int(k.sum()), pT[k].mean(), c2[k].mean())
        want = (mu, fine[1][i], fine[2][i])
        quad = (nev * abs(fine[0][i] - coarse[0][i]), abs(fine[1][i] - coarse[1][i]), abs(fine[2][i] - coarse[2][i]))
        for name, g, w, sg, q in zip(("N", "<pT>", "v2"), got, want, sig, quad):
            print("mcid %d %s: sampled %.6g, spectra %.6g (%.2f sigma), quadrature / sigma %.3f" % (mcid, name, g, w, (g - w) / sg, q / sg))
            assert q < sg / 5
            assert abs(g - w) <= 5 * sg


def test_errors_and_the_empty_surface():
    s = synth.as_read(synth.surface(100, seed=3))
    plasma = O.averages(s, 0)
    e2 = build_engine(make_spec(chosen="pikp", df_mode=2, dimension=2), s)
    with pytest.raises(IS3DError) as ei:
        e2.sample_famod(1, 2)
    assert ei.value.code == _lib.IS3D_ERR_STATE
    e2.close()
    e = build_engine(make_spec(chosen="pikp", df_mode=5, dimension=2), s)
    for kw in (dict(n_events=0), dict(seed=-1)):
        a = dict(seed=1, n_events=2)
        a.update(kw)
        with pytest.raises(IS3DError) as ei:
            e.sample_famod(**a)
        assert ei.value.code == _lib.IS3D_ERR_ARG
    with pytest.raises(IS3DError) as ei:
        e.sample_famod_binned(1, 2)
    assert ei.value.code == _lib.IS3D_ERR_STATE
    with pytest.raises(IS3DError) as ei:              # the df_mode 1-4 entry still refuses df_mode 5
        e.sample(1, 2, 0.5, 0, plasma)
    assert ei.value.code == _lib.IS3D_ERR_UNSUPPORTED and "is3d_sample_famod" in str(ei.value)
    with pytest.raises(IS3DError) as ei:              # no famod call succeeded yet
        e.sample_famod_stats()
    assert ei.value.code == _lib.IS3D_ERR_STATE
    p, off, st = e.sample_famod(1, 2)
    assert len(p) > 0 and st["kept"] == len(p)
    e.set_surface({k: v[:0] for k, v in s.items()})
    p, off, st = e.sample_famod(1, 5)
    assert len(p) == 0 and (off == 0).all() and len(off) == 6 and st["candidates"] == 0
    assert e.sample_famod_stats() == dict(plpt_negative=0, reconstruction_fail=0, iterations=0)
    e.close()


def test_dropin_run_directory(tmp_path):
    """host.sample on a df_mode 5 run directory goes to the famod entry: the list is Engine.sample_famod's with the same
    seed and Nevents and the OSCAR files hold it; with test_sampler = 1 the histograms are Engine.sample_famod_binned's
    and no list is written."""
    from is3d2_amd import host, rundir
    s = synth.surface(200, seed=43)
    params = dict(operation=2, dimension=2, df_mode=5, include_baryon=0, include_bulk_deltaf=1, include_shear_deltaf=1,
                  include_baryondiff_deltaf=0, regulate_deltaf=0, outflow=0, deta_min=1e-5, mass_pion0=0.138, oversample=1,
                  min_num_hadrons=2000.0, max_num_samples=100.0, y_cut=0.75, sampler_seed=77, fast=0, test_sampler=0)
    d = rundir.write_run_dir(str(tmp_path / "lists"), s, params, hrg_eos=2, chosen="pikp", surface_format=1)
    lists = lambda d: sorted(glob.glob(os.path.join(d, "results", "particle_list*")))
    got = host.sample(d, write_files=True, write_csv=False)
    nev = got["n_events"]
    assert nev > 1 and got["seed"] == 77
    spec = make_spec(hrg_eos=2, chosen="pikp", **{k: v for k, v in params.items() if k != "operation"})
    fields, avg = host.read_surface(d, 1, 2, 0)
    surf = {k: fields[i] for i, k in enumerate(synth.FIELDS)}
    e = build_engine(spec, surf, T_avg=avg[0])
    p, off, st = e.sample_famod(77, nev, 0.75)
    assert got["particles"].tobytes() == p.tobytes() and (got["offsets"] == off).all() and len(p) > 500
    mcids = spec["species"]["mcid"]
    assert (got["mcid"] == mcids[p["species"]]).all()
    assert [os.path.basename(f) for f in lists(d)] == sorted("particle_list_osc_%d.dat" % (k + 1) for k in range(nev))
    for ev in (0, nev - 1):
        with open(os.path.join(d, "results", "particle_list_osc_%d.dat" % (ev + 1))) as f:
            assert f.readline() == "n pid px py pz E m x y z t\n"
            rows = np.array([[float(v) for v in ln.split()] for ln in f]).reshape(-1, 11)
        q = p[off[ev]:off[ev + 1]]
        want = np.stack([q["px"], q["py"], q["pz"], q["E"], spec["species"]["mass"][q["species"]], q["x"], q["y"], q["z"], q["t"]], axis=1)
        assert len(rows) == len(q) and (rows[:, 1] == mcids[q["species"]]).all()
        np.testing.assert_array_equal(rows[:, 2:], want)
    # test_sampler = 1
    bins = dict(BINS, y_cut=0.75)
    params1 = dict(params, test_sampler=1)
    params1.update(bins)
    d1 = rundir.write_run_dir(str(tmp_path / "binned"), s, params1, hrg_eos=2, chosen="pikp", surface_format=1)
    got1 = host.sample(d1, write_files=True, write_csv=True)
    e.set_sample_bins(**bins)
    hist, st1 = e.sample_famod_binned(77, nev, 0.75)
    e.close()
    assert got1["n_events"] == nev and len(got1["particles"]) == 0 and lists(d1) == []
    assert same_hist(got1["hist"], hist) and got1["stats"] == st1 and st1["kept"] == len(p)
    assert os.path.isdir(os.path.join(d1, "results", "sampled"))
