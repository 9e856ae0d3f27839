"""GPU tier of the operation = 2 particle sampler (is3d_sample: k_cells, k_count, k_sample, k_compact in
is3d2_amd/csrc/sampler.hip).

The list is a pure function of (seed, inputs): same seed -> the same bytes, whatever the event batches, the cell
windows or the devices.  Statistical bars are derived (tests/sampler_ref.py): 5 sqrt(mu) for a count with expectation
mu; seeds are fixed."""
import numpy as np
import pytest

from is3d2_amd import IS3DError, build_engine, make_spec, synth
from is3d2_amd import _lib
from oracle import oracle as O

import sampler_ref as R

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


def engine(spec, s, plasma=None, **kw):
    plasma = O.averages(s, spec["params"]["include_baryon"]) if plasma is None else plasma
    return build_engine(spec, s, T_avg=plasma[0], **kw), plasma


def test_device_uniforms_equal_the_host_header_bit_for_bit():
    spec = make_spec(chosen="pikp", df_mode=1, dimension=2)
    e, _ = engine(spec, synth.as_read(synth.surface(8, seed=1)))
    for args in [(0, 0, 0, 0, 0), (12345, 2, 7, 3, 1), (2 ** 62 + 5, 3, 299, 49, 17), (9, 1, 2 ** 33 + 11, 2 ** 31 - 1, 2 ** 31 + 3)]:
        got = e.sample_uniforms(*args, 33)
        np.testing.assert_array_equal(got, R.uniforms(*args, 33))
    e.close()


def merge_windows(lists, n_events):
    out = []
    for ev in range(n_events):
        for parts, off in lists:
            out.append(parts[off[ev]:off[ev + 1]])
    return np.concatenate(out)


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("mode", [1, 4])
@pytest.mark.parametrize("dimension", [2, 3])
def test_the_list_depends_on_the_seed_and_nothing_else(dimension, mode, fast):
    nev, n = 50, 300
    spec = make_spec(chosen="pikp", df_mode=mode, dimension=dimension)
    s = synth.as_read(synth.surface(n, seed=23, dimension=dimension, full3d=(dimension == 3)))
    e, plasma = engine(spec, s)
    a, off_a, st = e.sample(11, nev, 0.5, fast, plasma)
    b, off_b, _ = e.sample(11, nev, 0.5, fast, plasma)
    assert len(a) > 1000 and st["capped"] == 0 and st["batches"] == 1
    assert a.tobytes() == b.tobytes() and (off_a == off_b).all()
    # several event batches
    e.set_tuning("sample_bytes", 200000)
    c, off_c, st_c = e.sample(11, nev, 0.5, fast, plasma)
    assert st_c["batches"] > 3
    assert c.tobytes() == a.tobytes() and (off_c == off_a).all()
    # ... and one event in several batches of cells
    e.set_tuning("sample_bytes", 20000)
    c1, off_c1, st_c1 = e.sample(11, 3, 0.5, fast, plasma)
    assert st_c1["batches"] > 3
    assert c1.tobytes() == a[:off_a[3]].tobytes()
    e.set_tuning("sample_bytes", -1)
    # cell windows merged per event
    e.set_cell_window(0, 120)
    w0 = e.sample(11, nev, 0.5, fast, plasma)
    e.set_cell_window(120, n)
    w1 = e.sample(11, nev, 0.5, fast, plasma)
    e.set_cell_window(-1, -1)
    assert merge_windows([w0[:2], w1[:2]], nev).tobytes() == a.tobytes()
    assert (w0[1] + w1[1] == off_a).all()
    # another seed
    d, _, _ = e.sample(12, nev, 0.5, fast, plasma)
    assert d.tobytes() != a.tobytes()
    e.close()
    # two shards on one device
    g, _ = engine(spec, s, plasma, devices=[0, 0])
    h, off_h, st_h = g.sample(11, nev, 0.5, fast, plasma)
    g.close()
    assert h.tobytes() == a.tobytes() and (off_h == off_a).all()
    assert st_h["candidates"] == st["candidates"] and st_h["kept"] == st["kept"] == len(a)


@pytest.mark.parametrize("dimension", [2, 3])
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_invariants_of_every_particle(dimension, mode):
    """SMASH species.  Tolerances: E and t, z are a handful of rounded operations from their inputs -- 8 ulp of E^2
    for the mass shell (E^2, p^2 are each rounded, E itself is a rounded square root), 16 ulp for t = tau cosh(eta)
    and z = tau sinh(eta) (the sampler forms cosh as sqrt(1 + sinh^2); in 2+1D eta = asinh(sinh eta))."""
    nev, n, y_cut = 20, 300, 0.8
    spec = make_spec(chosen="smash", df_mode=mode, dimension=dimension)
    s = synth.as_read(synth.surface(n, seed=29, dimension=dimension, full3d=(dimension == 3)))
    s["dat"] = s["dat"].copy()
    s["dat"][::7] *= -1.0          # cells with u.dsigma <= 0
    e, plasma = engine(spec, s)
    p, off, st = e.sample(3, nev, y_cut, 0, plasma)
    e.close()
    assert len(p) > 1000 and st["capped"] == 0 and st["kept"] == len(p) and st["cells"] == n
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
    print("mode %d %dD: %d particles, max |E^2 - p^2 - m^2| / (ulp E^2) = %.2f" % (mode, dimension, len(p), float(np.max(shell / (EPS * E2)))))
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
    # p.dsigma > 0 in the lab (Milne) components
    mT = np.sqrt(m * m + p["px"] ** 2 + p["py"] ** 2)
    ptau, pn = mT * np.cosh(rap - p["eta"]), mT * np.sinh(rap - p["eta"]) / tau
    pds = ptau * s["dat"][c] + p["px"] * s["dax"][c] + p["py"] * s["day"][c] + pn * s["dan"][c]
    assert (pds > 0).all()
    # no particle from a cell with u.dsigma <= 0
    ut = np.sqrt(1 + s["ux"] ** 2 + s["uy"] ** 2 + (s["tau"] * s["un"]) ** 2)
    uds = ut * s["dat"] + s["ux"] * s["dax"] + s["uy"] * s["day"] + s["un"] * s["dan"]
    assert (uds <= 0).sum() > 10 and (uds[c] > 0).all()


PI_SCALE = 0.125


def uniform_surface(n, dimension, seed=17):
    """Uniform (T, E, P), normals dsigma = (dat > 0, 0, 0, 0) (timelike in every LRF) and synth's pi and Pi scaled by
    1/8: at synth's own size the linear delta-f of Grad / RTA-CE is clamped for 1-2 % of the candidates and the yield
    is no longer the oracle's (+4 sigma already at mu = 5e5, measured with the CPU emulator); at 1/8 the emulator
    clamps 8 of 3.6e6 candidates (Grad) and none (RTA-CE), below the 1e-5 this test allows."""
    s = synth.surface(n, seed=seed, dimension=dimension, full3d=(dimension == 3))
    for k in ("dax", "day", "dan"):
        s[k][:] = 0.0
    for k in ("pixx", "pixy", "pixn", "piyy", "piyn", "bulkPi"):
        s[k] *= PI_SCALE
    s["T"][:] = 0.150
    s["E"][:] = 0.28
    s["P"][:] = 0.045
    return synth.as_read(s)


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("mode,dimension", [(1, 2), (2, 3), (3, 3), (4, 2)])
def test_exact_yield(mode, dimension, fast):
    """mu ~ 1e6: with uniform thermodynamics the oracle's Plasma-average densities are the cells' own, so
    Nevents x total_yield is the exact mean of the kept count (thinning a Poisson draw leaves a Poisson)."""
    nev, y_cut = 4000, 0.5
    spec = make_spec(chosen="pikp", df_mode=mode, dimension=dimension)
    s = uniform_surface(300, dimension)
    e, plasma = engine(spec, s)
    p, off, st = e.sample(7, nev, y_cut, fast, plasma)
    e.close()
    mu = nev * O.total_yield(spec, s, plasma, y_cut=y_cut)[0]
    print("mode %d %dD fast %d: kept %d, mu %.1f (%.2f sigma), candidates %d, clamped %d, efficiency %.3f" %
          (mode, dimension, fast, len(p), mu, (len(p) - mu) / np.sqrt(mu), st["candidates"], st["clamped"],
           st["acceptances"] / st["proposals"]))
    assert mu > 9e5
    assert st["capped"] == 0 and st["breakdown"] == 0
    assert st["clamped"] <= 1e-5 * st["candidates"]
    assert abs(len(p) - mu) <= 5 * np.sqrt(mu)
    counts = np.bincount(p["species"], minlength=len(spec["species"]["mass"]))
    for i, mcid in enumerate(spec["species"]["mcid"]):
        spec1 = make_spec(chosen=[int(mcid)], df_mode=mode, dimension=dimension)
        mus = nev * O.total_yield(spec1, s, plasma, y_cut=y_cut)[0]
        assert abs(counts[i] - mus) <= 5 * np.sqrt(mus), (int(mcid), counts[i], mus)


def test_ptm_yield_equals_rta_ce_and_its_breakdown_reproduces_the_list():
    nev = 1000
    s = uniform_surface(300, 3)
    lists = {}
    for mode, deta_min in [(2, 1e-5), (3, 1e-5), (2, 1e9), (3, 1e9)]:
        spec = make_spec(chosen="pikp", df_mode=mode, dimension=3, deta_min=deta_min)
        e, plasma = engine(spec, s)
        lists[mode, deta_min] = e.sample(21, nev, 0.5, 0, plasma)
        e.close()
    p2, _, st2 = lists[2, 1e-5]
    p3, _, st3 = lists[3, 1e-5]
    assert st3["breakdown"] == 0 and st3["capped"] == 0 and st2["capped"] == 0
    for i, mcid in enumerate(spec["species"]["mcid"]):
        spec1 = make_spec(chosen=[int(mcid)], df_mode=2, dimension=3)
        mus = nev * O.total_yield(spec1, s, plasma)[0]          # both means are neq + Pi dn_bulk
        n2, n3 = int((p2["species"] == i).sum()), int((p3["species"] == i).sum())
        assert abs(n3 - n2) <= 5 * np.sqrt(2 * mus), (int(mcid), n2, n3, mus)
    # det A <= deta_min everywhere: the reference's goto chapman_enskog, with the same streams
    b2, off2, _ = lists[2, 1e9]
    b3, off3, st = lists[3, 1e9]
    assert st["breakdown"] == st["cells"] == 300
    assert b3.tobytes() == b2.tobytes() and (off2 == off3).all()
    assert b2.tobytes() == p2.tobytes()              # deta_min plays no part in RTA-CE


def test_errors_and_the_empty_surface():
    s = synth.as_read(synth.surface(100, seed=3))
    spec = make_spec(chosen="pikp", df_mode=1, dimension=2)
    e, plasma = engine(spec, s)
    for kw, code in [(dict(n_events=0), _lib.IS3D_ERR_ARG), (dict(y_cut=0.0), _lib.IS3D_ERR_ARG), (dict(seed=-1), _lib.IS3D_ERR_ARG)]:
        a = dict(seed=1, n_events=2, y_cut=0.5, fast=0, plasma=plasma)
        a.update(kw)
        with pytest.raises(IS3DError) as ei:
            e.sample(**a)
        assert ei.value.code == code
    # a (cell, event) that cannot fit the memory bound is an error, not a truncation
    e.set_tuning("sample_bytes", 100)
    with pytest.raises(IS3DError) as ei:
        e.sample(1, 2, 0.5, 0, plasma)
    assert ei.value.code == _lib.IS3D_ERR_ARG and "sample_bytes" in str(ei.value)
    e.set_tuning("sample_bytes", -1)
    hot = dict(s)
    hot["T"] = s["T"].copy()
    hot["T"][17] = 0.5                      # outside the 0.1..0.2 GeV coefficient spline
    e.set_surface(hot)
    with pytest.raises(IS3DError) as ei:
        e.sample(1, 2, 0.5, 0, plasma)
    assert ei.value.code == _lib.IS3D_ERR_DF_RANGE
    e.set_surface({k: v[:0] for k, v in s.items()})
    p, off, st = e.sample(1, 5, 0.5, 0, plasma)
    assert len(p) == 0 and (off == 0).all() and len(off) == 6 and st["candidates"] == 0
    e.close()
    spec5 = make_spec(chosen="pikp", df_mode=5, dimension=2)
    e5, _ = engine(spec5, s, plasma)
    with pytest.raises(IS3DError) as ei:
        e5.sample(1, 2, 0.5, 0, plasma)
    assert ei.value.code == _lib.IS3D_ERR_UNSUPPORTED
    e5.close()


def test_dropin_run_directory(tmp_path):
    """is3d_host_sample on an operation = 2 run directory: the list is Engine.sample's with the same seed and Nevents,
    the OSCAR files hold it to the printed precision, and the estimate-only entry points still write no list."""
    import glob
    import os
    from is3d2_amd import host, rundir
    s = synth.surface(200, seed=43)
    params = dict(operation=2, dimension=2, df_mode=1, include_baryon=0, include_bulk_deltaf=1, include_shear_deltaf=1,
                  include_baryondiff_deltaf=0, regulate_deltaf=0, outflow=0, deta_min=1e-5, mass_pion0=0.138, oversample=1,
                  min_num_hadrons=2000.0, max_num_samples=100.0, y_cut=0.75, sampler_seed=77, fast=0, test_sampler=0)
    d = rundir.write_run_dir(str(tmp_path), s, params, hrg_eos=2, chosen="pikp", surface_format=1)
    lists = lambda: sorted(glob.glob(os.path.join(d, "results", "particle_list*")))
    ntot, nev = host.total_yield(d)
    host.run_particlization(d, 0)
    assert lists() == [] and nev > 1
    got = host.sample(d, write_files=True, write_csv=False)
    assert got["n_events"] == nev and got["seed"] == 77 and got["n_total"] == ntot
    spec = make_spec(hrg_eos=2, chosen="pikp", **{k: v for k, v in params.items() if k != "operation"})
    fields, avg = host.read_surface(d, 1, 2, 0)
    surf = {k: fields[i] for i, k in enumerate(synth.FIELDS)}
    e = build_engine(spec, surf, T_avg=avg[0])
    p, off, st = e.sample(77, nev, 0.75, 0, avg)
    e.close()
    assert got["particles"].tobytes() == p.tobytes() and (got["offsets"] == off).all() and len(p) > 500
    mcids = spec["species"]["mcid"]
    assert (got["mcid"] == mcids[p["species"]]).all()
    assert [os.path.basename(f) for f in lists()] == sorted("particle_list_osc_%d.dat" % (k + 1) for k in range(nev))
    for ev in range(nev):
        with open(os.path.join(d, "results", "particle_list_osc_%d.dat" % (ev + 1))) as f:
            assert f.readline() == "n pid px py pz E m x y z t\n"
            rows = np.array([[float(v) for v in ln.split()] for ln in f]).reshape(-1, 11)
        q = p[off[ev]:off[ev + 1]]
        assert len(rows) == len(q)
        assert (rows[:, 0] == np.arange(len(q))).all() and (rows[:, 1] == mcids[q["species"]]).all()
        want = np.stack([q["px"], q["py"], q["pz"], q["E"], spec["species"]["mass"][q["species"]], q["x"], q["y"], q["z"], q["t"]], axis=1)
        # 17 significant digits round-trip a double exactly
        np.testing.assert_array_equal(rows[:, 2:], want)


@pytest.mark.parametrize("mode", [1, 2])
def test_momentum_distribution_against_the_continuous_spectra(mode):
    """2+1D, fast = 0, synth normals (spacelike ones included), outflow = 1 and regulate_deltaf = 1: the oracle's
    integrand is then the sampler's density term by term, so per species N = 2 y_cut dN/dy, <pT> and v2 of the
    continuous spectra are the sampled ones' expectations.  The quadrature uncertainty (48x32 against 24x24 momentum
    tables) must stay below a fifth of the statistical sigma: measured on the oracle, the tightest case (RTA-CE pion
    <pT>: 2.9e-4 GeV between the tables, std 0.489 GeV, 184 pions per event) allows 617 events; 400 are drawn."""
    nev, y_cut = 400, 0.5
    s = synth.as_read(synth.surface(300, seed=37))
    flags = dict(chosen="pikp", df_mode=mode, dimension=2, outflow=1, regulate_deltaf=1)
    spec = make_spec(pT="pT48", phi="phi32", **flags)
    fine = R.spectra_moments(spec, s, y_cut)
    coarse = R.spectra_moments(make_spec(pT="pT24", phi="phi24", **flags), s, y_cut)
    e, plasma = engine(spec, s)
    p, off, st = e.sample(41, nev, y_cut, 0, plasma)
    e.close()
    assert st["capped"] == 0
    pT = np.hypot(p["px"], p["py"])
    c2 = np.cos(2.0 * np.arctan2(p["py"], p["px"]))
    for i, mcid in enumerate(spec["species"]["mcid"]):
        k = p["species"] == i
        n = int(k.sum())
        mu = nev * fine[0][i]
        sig = (np.sqrt(mu), fine[3][i] / np.sqrt(mu), c2[k].std() / np.sqrt(mu))
        got = (n, pT[k].mean(), c2[k].mean())
        want = (mu, fine[1][i], fine[2][i])
        quad = (nev * abs(fine[0][i] - coarse[0][i]), abs(fine[1][i] - coarse[1][i]), abs(fine[2][i] - coarse[2][i]))
        for name, g, w, sg, q in zip(("N", "<pT>", "v2"), got, want, sig, quad):
            print("mode %d mcid %d %s: sampled %.6g, spectra %.6g (%.2f sigma), quadrature / sigma %.3f" %
                  (mode, mcid, name, g, w, (g - w) / sg, q / sg))
            assert q < sg / 5
            assert abs(g - w) <= 5 * sg
