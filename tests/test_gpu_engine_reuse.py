"""GPU tier: one engine used again and again.  Every device buffer of the engine has one owner (csrc/devbuf.h) that
grows it on demand and keeps it otherwise, and the entry points share their host sequences (the launch prologue, the
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
