"""GPU tier of the resonance-decay feed-down (decay.hip through the C ABI and the Python binding): the kernels against
the CPU emulator (the same decay_math.h on the host, tests/native/decay_emulator.cpp), the whole SMASH decay table,
the device-list engine and the errors.

Parity is |got - emulator| / sum |terms|, bar 1e-8.  Measured on MI355X: see DESIGN.md 7.6.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import decay_ref as R
from is3d2_amd import Engine, IS3DError, _lib, build_engine, hrg, make_spec, synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MASS, CHANNELS = R.CASE_MASS, R.CASE_CHANNELS      # decay_ref's small case: the awkward parents sit on unfed species


def decay_engine(mass, pT, phi, y, dimension, channels=None, devices=None):
    """An engine with only what the feed-down needs: params (the dimension), species, grid, channels."""
    e = Engine(devices=devices)
    e.set_params(dimension=dimension)
    n = len(mass)
    e.set_species(mass, -np.ones(n), np.ones(n), np.zeros(n))
    e.set_momentum_grid(pT, phi, y, np.zeros(1), np.ones(1))
    if channels is not None:
        e.set_decays(channels)
    return e


@functools.lru_cache(maxsize=None)
def small_case(npT, nphi, ny):
    rng = np.random.default_rng(npT + nphi + ny)
    pT = np.linspace(0.1, 3.0, npT) ** 1.3
    phi = np.sort(rng.uniform(0, 2 * np.pi, nphi))
    y = np.linspace(-2.5, 2.5, ny) if ny > 1 else np.zeros(1)
    S = R.case_spectra(pT, phi, y)
    ref, ab, st, _ = R.emulate(S, MASS, pT, phi, y, CHANNELS)
    for a in (pT, phi, y, S, ref, ab):
        a.setflags(write=False)
    return pT, phi, y, S, ref, ab, st


@pytest.mark.parametrize("shape", [(10, 8, 1), (10, 8, 5), (6, 32, 21)], ids=lambda s: "%dx%dx%d" % s)
def test_gpu_against_emulator(shape):
    """2-body and 3-body channels, a daughter twice, a chain, the four awkward parents; 6 x 32 x 21: a 3+1D slab of
    the production phi and y sizes (the parent slab is read through L2; 72 of the 144 nodes per LDS batch)."""
    import torch
    pT, phi, y, S, ref, ab, st = small_case(*shape)
    e = decay_engine(MASS, pT, phi, y, 3 if shape[2] > 1 else 2, CHANNELS)
    got = e.feeddown(S)
    err = R.parity(got, ref, ab)
    print("%s: GPU vs emulator %.3e of sum |terms|" % (shape, err))
    assert err < R.BAR
    # the zero, the negative value, the top-node zeros and the rising last interval reach the kernel's interpolation
    R.check_awkward_parents(S, got, e.feeddown)
    gst = e.decay_stats()
    assert {k: gst[k] for k in st if k != "ms_total"} == {k: st[k] for k in st if k != "ms_total"}
    assert gst["ms_total"] > 0
    again = e.feeddown(S)
    assert again.tobytes() == got.tobytes()
    dev = torch.from_numpy(S.copy()).to("cuda:0")
    e.launch_feeddown(dev.data_ptr(), torch.cuda.current_stream(0).cuda_stream)
    e.finish()
    assert dev.cpu().numpy().tobytes() == got.tobytes()
    # the order the channels are listed in does not matter
    e.set_decays(CHANNELS[::-1])
    assert e.feeddown(S).tobytes() == got.tobytes()
    e.close()


def test_device_list_engine_gives_the_same_bytes():
    pT, phi, y, S, ref, ab, st = small_case(10, 8, 5)
    one = decay_engine(MASS, pT, phi, y, 3, CHANNELS)
    want = one.feeddown(S)
    one.close()
    e = decay_engine(MASS, pT, phi, y, 3, CHANNELS, devices=[0, 0])
    got = e.feeddown(S)
    assert e.decay_stats()["kept"] == st["kept"]
    e.close()
    assert got.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------
# the whole SMASH table on a tiny grid
# ------------------------------------------------------------------------------------------
def test_whole_smash_table():
    """444 species x 8 pT x 8 phi x 1 y, thermal spectra of a 64-cell surface: against the emulator; the stats equal
    the emulator's counts; pi+ grows and no stable species loses anywhere its input is > 0."""
    d = dict(np.load(os.path.join(HERE, "golden", "decays_smash.npz")))
    spec = make_spec(hrg_eos=2, chosen="smash", df_mode=2, dimension=2)
    spec["pT"] = np.linspace(0.15, 2.6, 8)
    spec["phi"] = (np.arange(8) + 0.5) * (2 * np.pi / 8)
    spec["pT_w"], spec["phi_w"] = np.ones(8), np.ones(8)
    mcids = spec["species"]["mcid"]
    ch = hrg.decay_channels(d, d, mcids)
    e = build_engine(spec, synth.as_read(synth.surface(64, seed=7)))
    S = e.calculate_spectra().reshape(len(mcids), 8, 8, 1)
    e.set_decays(ch)
    got = e.feeddown(S)
    gst = e.decay_stats()
    e.close()
    ref, ab, st, slots = R.emulate(S, spec["species"]["mass"], spec["pT"], spec["phi"], np.zeros(1), ch)
    err = R.parity(got, ref, ab)
    print("SMASH: %d channels, %d slots, stats %s, GPU vs emulator %.3e" % (len(ch), slots, gst, err))
    assert err < R.BAR
    assert {k: gst[k] for k in st if k != "ms_total"} == {k: st[k] for k in st if k != "ms_total"}
    assert st["kept"] > 2000 and st["skipped_many_body"] == 0 and st["levels"] > 3
    pip = int(np.nonzero(mcids == 211)[0][0])
    assert np.all(got[pip] > S[pip])
    stable = np.unique(ch["parent"][ch["n_body"] == 1])
    assert len(stable) > 10 and pip in stable
    for s in stable:
        m = S[s] > 0
        assert np.all(got[s][m] >= S[s][m])


# ------------------------------------------------------------------------------------------
# errors
# ------------------------------------------------------------------------------------------
def expect(code, f, *a):
    with pytest.raises(IS3DError) as ei:
        f(*a)
    assert ei.value.code == code, str(ei.value)


def test_errors():
    pT, phi, y, S, ref, ab, st = small_case(10, 8, 1)
    ok = [R.channel(2, [0, 1], 1.0, 0.776, [0.138, 0.138])]
    # state: decays before the species / the grid; a feed-down without decays, or without params
    e = Engine()
    expect(_lib.IS3D_ERR_STATE, e.set_decays, ok)
    n = len(MASS)
    e.set_species(MASS, -np.ones(n), np.ones(n), np.zeros(n))
    expect(_lib.IS3D_ERR_STATE, e.set_decays, ok)
    e.set_momentum_grid(pT, phi, y, np.zeros(1), np.ones(1))
    e.set_decays(ok)
    buf = S.copy()
    rc = e.lib.is3d_decay_feeddown(e._e, buf.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == _lib.IS3D_ERR_STATE                       # no params: the dimension is unknown
    e.close()
    e = decay_engine(MASS, pT, phi, y, 2)
    expect(_lib.IS3D_ERR_STATE, e.feeddown, S)
    expect(_lib.IS3D_ERR_STATE, e.decay_stats)
    # arguments
    expect(_lib.IS3D_ERR_ARG, e.set_decays, [R.channel(2, [0, 1], 1.0, 0.776, [0.138, 0.138], n_body=0)])
    expect(_lib.IS3D_ERR_ARG, e.set_decays, [R.channel(n, [0, 1], 1.0, 0.776, [0.138, 0.138])])
    expect(_lib.IS3D_ERR_ARG, e.set_decays, [R.channel(-1, [0, 1], 1.0, 0.776, [0.138, 0.138])])
    expect(_lib.IS3D_ERR_ARG, e.set_decays, [R.channel(2, [0, n], 1.0, 0.776, [0.138, 0.138])])
    expect(_lib.IS3D_ERR_ARG, e.set_decays, [R.channel(2, [0, -2], 1.0, 0.776, [0.138, 0.138])])
    expect(_lib.IS3D_ERR_ARG, e.set_decays, ok + [R.channel(0, [2, -1], 1.0, 3.0, [0.776, 0.1])])      # a cycle
    expect(_lib.IS3D_ERR_ARG, e.set_decays, [R.channel(2, [2, 1], 1.0, 0.776, [0.138, 0.138])])        # ... of one
    expect(_lib.IS3D_ERR_STATE, e.feeddown, S)             # a refused table leaves none behind
    for bad_pT in (np.concatenate([[0.0], pT[1:]]), np.concatenate([[-0.1], pT[1:]]), pT[::-1].copy()):
        e.set_momentum_grid(bad_pT, phi, y, np.zeros(1), np.ones(1))
        expect(_lib.IS3D_ERR_ARG, e.set_decays, ok)
    for bad_phi in (phi[::-1].copy(), np.concatenate([phi[:-1], [2 * np.pi]]), np.concatenate([[-0.1], phi[1:]]),
                    np.concatenate([phi[:1], phi[:-1]])):
        e.set_momentum_grid(pT, bad_phi, y, np.zeros(1), np.ones(1))
        expect(_lib.IS3D_ERR_ARG, e.set_decays, ok)
    # a new species list or grid clears the table
    e.set_momentum_grid(pT, phi, y, np.zeros(1), np.ones(1))
    e.set_decays(ok)
    e.feeddown(S)
    e.set_momentum_grid(pT, phi, y, np.zeros(1), np.ones(1))
    expect(_lib.IS3D_ERR_STATE, e.feeddown, S)
    e.set_decays(ok)
    e.set_species(MASS, -np.ones(n), np.ones(n), np.zeros(n))
    expect(_lib.IS3D_ERR_STATE, e.feeddown, S)
    e.set_decays([])                                       # an empty table is a table: nothing changes
    assert np.array_equal(e.feeddown(S), S)
    e.close()


# ------------------------------------------------------------------------------------------
# drop-in: do_resonance_decays in iS3D_parameters.dat
# ------------------------------------------------------------------------------------------
DROPIN_CHOSEN = [211, -211, 111, 2212, -2212, 2112, 113, 213, 223, 2224, -2224, 2214, 321, 313]


def read_results(d):
    out = {}
    for fn in sorted(os.listdir(os.path.join(d, "results", "continuous"))):
        out[fn] = open(os.path.join(d, "results", "continuous", fn), "rb").read()
    return out


def test_dropin_run_directory(tmp_path):
    """operation = 1 with do_resonance_decays = 1: the returned spectra are Engine.feeddown(calculate_spectra()) bit
    for bit and the files hold them at the writer's precision; with the key 0 the files are the files without it."""
    from is3d2_amd import host, rundir
    dec = dict(np.load(os.path.join(HERE, "golden", "decays_smash.npz")))
    s = synth.surface(64, seed=31)
    params = dict(dimension=2, df_mode=2, include_baryon=0, include_bulk_deltaf=1, include_shear_deltaf=1,
                  include_baryondiff_deltaf=0, regulate_deltaf=0, outflow=0, deta_min=1e-5, mass_pion0=0.138)
    spec = make_spec(hrg_eos=2, chosen=DROPIN_CHOSEN, pT="pT24", phi="phi24", **params)
    n = len(DROPIN_CHOSEN) * 24 * 24
    runs = {}
    for name, extra in (("on", dict(do_resonance_decays=1, lightest_particle=111)), ("off", dict(do_resonance_decays=0)),
                        ("absent", {})):
        d = rundir.write_run_dir(str(tmp_path / name), s, dict(params, **extra), hrg_eos=2, chosen=DROPIN_CHOSEN,
                                 decays=dec)
        runs[name] = (d, host.run_particlization(d, n))
    assert read_results(runs["off"][0]) == read_results(runs["absent"][0])
    assert runs["off"][1].tobytes() == runs["absent"][1].tobytes()
    d, got = runs["on"]
    fields, avg = host.read_surface(d, 1, 2, 0)
    e = build_engine(spec, {k: fields[i] for i, k in enumerate(synth.FIELDS)}, T_avg=avg[0])
    thermal = e.calculate_spectra()
    assert thermal.tobytes() == runs["off"][1].tobytes()
    e.set_decays(hrg.decay_channels(dec, dec, DROPIN_CHOSEN))
    want = e.feeddown(thermal)
    st = e.decay_stats()
    e.close()
    assert st["kept"] > 10 and got.tobytes() == want.tobytes()
    assert np.all(want[:12 * 24] > thermal[:12 * 24])      # pi+ gained (lower half of pT24; the far tail is delta-f noise)
    on, off = read_results(d), read_results(runs["off"][0])
    assert sorted(on) == sorted(off) and on != off
    for k, mc in enumerate(DROPIN_CHOSEN):
        lines = on["dN_pTdpTdphidy_%d.dat" % mc].decode().split("\n")
        vals = np.array([float(ln.split("\t")[3]) for ln in lines[1:] if ln])
        arr = want.reshape(len(DROPIN_CHOSEN), 24, 24, 1)[k]             # file order: y, phi, pT
        np.testing.assert_allclose(vals, np.transpose(arr, (2, 1, 0)).ravel(), rtol=5e-9)


def test_key_changes_nothing_under_another_operation(tmp_path):
    """do_resonance_decays = 1 with operation = 0: the decay rows are not even resolved (a row naming a particle the
    PDG list lacks fails an operation = 1 run only) and the output is the output without the key."""
    from is3d2_amd import host, rundir
    dec = dict(np.load(os.path.join(HERE, "golden", "decays_smash.npz")))
    bad = dict(dec)
    bad["row_mcid"] = np.array([211]); bad["row_n_body"] = np.array([2]); bad["row_branching"] = np.array([1.0])
    bad["row_daughters"] = np.array([[999999, 111, 0, 0, 0]])
    s = synth.surface(24, seed=3)
    params = dict(dimension=2, df_mode=1, include_baryon=0, include_bulk_deltaf=1, include_shear_deltaf=1,
                  include_baryondiff_deltaf=0, regulate_deltaf=0, outflow=0, deta_min=1e-5, mass_pion0=0.138)
    n0 = 3 * (120 + 60 + 100)
    with_key = rundir.write_run_dir(str(tmp_path / "a"), s, dict(params, operation=0, do_resonance_decays=1), decays=bad)
    without = rundir.write_run_dir(str(tmp_path / "b"), s, dict(params, operation=0), decays=bad)
    assert host.run_particlization(with_key, n0).tobytes() == host.run_particlization(without, n0).tobytes()
    assert read_results(with_key) == read_results(without)
    op1 = rundir.write_run_dir(str(tmp_path / "c"), s, dict(params, operation=1, do_resonance_decays=1), decays=bad)
    with pytest.raises(host.HostError, match="999999"):
        host.run_particlization(op1, 3 * 24 * 24)
