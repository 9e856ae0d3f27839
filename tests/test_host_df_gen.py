"""Host layer: generate_df_coefficients in iS3D_parameters.dat (include/is3d_host.h) -- a run directory without
deltaf_coefficients/ against the Python path with generated tables, the written files against the shipped ones, and the
key off against the Python path with the shipped tables."""
import os
import shutil

import numpy as np
import pytest

import df_gen_ref as R
from helpers import parity
from is3d2_amd import build_engine, data, host, make_spec, rundir, synth

pytestmark = pytest.mark.gpu
PARAMS = dict(dimension=2, df_mode=1, include_baryon=0, include_bulk_deltaf=1, include_shear_deltaf=1,
              include_baryondiff_deltaf=0, regulate_deltaf=0, outflow=0, deta_min=1e-5, mass_pion0=0.138)
ENGINE_KEYS = {k: v for k, v in PARAMS.items()}


def run_dir(tmp_path, name, extra, mode=1):
    s = synth.surface(150, seed=31)
    params = dict(PARAMS, df_mode=mode, **extra)
    d = rundir.write_run_dir(str(tmp_path / name), s, params, hrg_eos=2, chosen="pikp", surface_format=1)
    fields, avg = host.read_surface(d, 1, 2, 0)
    return d, {k: fields[i] for i, k in enumerate(synth.FIELDS)}, avg


def python_path(surf, avg, mode=1, **spec_kw):
    spec = make_spec(hrg_eos=2, chosen="pikp", pT="pT24", phi="phi24", **dict(ENGINE_KEYS, df_mode=mode), **spec_kw)
    e = build_engine(spec, surf, T_avg=avg[0])
    out = e.calculate_spectra()
    e.close()
    return out, spec


@pytest.mark.parametrize("mode", [1, 2])
def test_generate_key_replaces_the_deltaf_directory(tmp_path, mode):
    keys = dict(generate_df_coefficients=1, df_T_min=0.14, df_T_max=0.16, df_T_points=11, df_muB_min=0.0, df_muB_max=0.1,
                df_muB_points=3)
    d, surf, avg = run_dir(tmp_path, "gen", keys, mode)
    shutil.rmtree(os.path.join(d, "deltaf_coefficients"))
    got = host.run_particlization(d, 3 * 24 * 24)
    T = np.array([0.14 + i * ((0.16 - 0.14) / 10.0) for i in range(11)]); T[0] = 0.14      # the driver's grid
    muB = np.array([0.0, 0.05, 0.1])
    ref, spec = python_path(surf, avg, mode, df_tables="generate", df_grid=(T, muB))
    assert parity(got, ref)[0] < 1e-8            # the bar of tests/test_host_layer.py between the two paths
    assert not os.path.exists(os.path.join(d, "results", "deltaf_coefficients"))       # only the key 2 writes them
    mc = spec["species"]["mcid"][2]
    lines = open(os.path.join(d, "results/continuous/dN_pTdpTdphidy_%d.dat" % mc)).read().split("\n")
    vals = np.array([float(ln.split("\t")[3]) for ln in lines[1:] if ln])
    last = ref.reshape(3, 24, 24, 1)[2]          # file order: y, phi, pT
    np.testing.assert_allclose(vals, np.transpose(last, (2, 1, 0)).ravel(), rtol=5e-9)
    # ... and they are not the shipped-table spectra
    base, _ = python_path(surf, avg, mode)
    assert not np.array_equal(got, base)


def test_key_two_writes_the_ten_files(tmp_path):
    d, surf, avg = run_dir(tmp_path, "write", dict(generate_df_coefficients=2))
    shutil.rmtree(os.path.join(d, "deltaf_coefficients"))
    host.run_particlization(d, 3 * 24 * 24)
    out = os.path.join(d, "results", "deltaf_coefficients")
    assert sorted(os.listdir(out)) == sorted(n + ".dat" for n in R.NAMES)
    T, muB, tab = host.read_df_tables(out)
    Ts, muBs, shipped = data.df_tables(2)
    np.testing.assert_allclose(T, Ts, rtol=0, atol=1e-12)
    np.testing.assert_allclose(muB, muBs, rtol=0, atol=1e-12)
    R.assert_shipped(tab, shipped, "results/deltaf_coefficients")
    lines = open(os.path.join(out, "c0.dat")).read().split("\n")
    assert lines[:4] == ["101", "81", "T [GeV]\t\tmuB [GeV]\t\tc0_T4 [fm^3/GeV^3 * GeV^4]", "0.100000\t\t0.000000\t\t-0.545933"]


def test_key_off_or_absent_reads_the_directory_as_before(tmp_path):
    d0, surf, avg = run_dir(tmp_path, "absent", {})
    d1, _, _ = run_dir(tmp_path, "zero", dict(generate_df_coefficients=0))
    a = host.run_particlization(d0, 3 * 24 * 24)
    b = host.run_particlization(d1, 3 * 24 * 24)
    ref, _ = python_path(surf, avg)
    assert a.tobytes() == b.tobytes() == ref.tobytes()
    assert not os.path.exists(os.path.join(d0, "results", "deltaf_coefficients"))
    shutil.rmtree(os.path.join(d1, "deltaf_coefficients"))          # off: the directory is needed, as before
    with pytest.raises(host.HostError, match="Couldn't open"):
        host.run_particlization(d1, 3 * 24 * 24)
