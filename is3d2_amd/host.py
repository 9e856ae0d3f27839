"""ctypes binding of the C++ host layer (libis3d_host.so, include/is3d_host.h)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libis3d_host.so")
_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libis3d_host.so not built (make -C is3d2_amd/csrc/host)")
        lib = C.CDLL(LIB_PATH)
        PD, PL, PI = C.POINTER(C.c_double), C.POINTER(C.c_long), C.POINTER(C.c_int)
        lib.is3d_host_run_particlization.argtypes = [C.c_char_p, C.c_int, C.c_int, PD, C.c_long, C.c_char_p, C.c_int]
        lib.is3d_host_run_particlization_devices.argtypes = [C.c_char_p, PI, C.c_int, PD, C.c_long, C.c_char_p,
                                                             C.c_int]
        lib.is3d_host_read_surface.restype = C.c_long
        lib.is3d_host_read_surface.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, PD, PD]
        lib.is3d_host_read_pdg.argtypes = [C.c_char_p, C.c_int, C.c_int, PL, PD, PI, PI, PI]
        lib.is3d_host_read_decays.restype = C.c_long
        lib.is3d_host_read_decays.argtypes = [C.c_char_p, C.c_int, C.c_long, PL, PI, PD, PL]
        lib.is3d_host_param.argtypes = [C.c_char_p, C.c_char_p, PD]
        lib.is3d_host_read_df_tables.argtypes = [C.c_char_p, PI, PI, C.c_long, PD, PD, PD]
        lib.is3d_host_total_yield.argtypes = [C.c_char_p, C.c_int, C.c_int, PD, PL, C.c_char_p, C.c_int]
        lib.is3d_host_read_vorticity.restype = C.c_long
        lib.is3d_host_read_vorticity.argtypes = [C.c_char_p, C.c_int, C.c_int, PD]
        lib.is3d_host_polarization.argtypes = [C.c_char_p, PI, C.c_int, PD, C.c_long, C.c_char_p, C.c_int]
        lib.is3d_host_sample.argtypes = [C.c_char_p, PI, C.c_int, C.c_int, C.c_int, C.c_void_p, PL, C.c_long, PL, C.c_long,
                                         PL, PL, PD, PL, C.c_char_p, C.c_int]
        lib.is3d_host_write_particle_lists.argtypes = [C.c_char_p, C.c_long, PL, C.c_void_p, PL, PD, C.c_int, C.c_char_p,
                                                       C.c_int]
        from ._lib import DecayListStats, SampleBins, SampleStats
        lib.is3d_host_sample_binned_decays.argtypes = [C.c_char_p, PI, C.c_int, C.c_int, PL, C.c_long, PD, C.c_long, PL, PD, PL,
                                                       C.POINTER(SampleStats), C.POINTER(DecayListStats), C.c_char_p, C.c_int]
        lib.is3d_host_sample_decays.argtypes = [C.c_char_p, PI, C.c_int, C.c_int, C.c_int, C.c_void_p, PL, C.c_long, PL,
                                                C.c_long, PL, PL, PD, PL, PL, C.POINTER(DecayListStats), C.c_char_p, C.c_int]
        lib.is3d_host_sample_hist_size.argtypes = [C.c_char_p, C.POINTER(SampleBins), PI, PL, PL]
        lib.is3d_host_sample_binned.argtypes = [C.c_char_p, PI, C.c_int, C.c_int, PL, C.c_long, PD, C.c_long, PL, PD, PL,
                                                C.POINTER(SampleStats), C.c_char_p, C.c_int]
        _lib = lib
    return _lib


def read_surface(workdir, mode, dimension, include_baryon):
    lib = load()
    n = lib.is3d_host_read_surface(workdir.encode(), mode, dimension, include_baryon, None, None)
    if n < 0:
        raise RuntimeError("surface read failed")
    f = np.zeros(25 * n)
    avg = np.zeros(5)
    lib.is3d_host_read_surface(workdir.encode(), mode, dimension, include_baryon,
                               f.ctypes.data_as(C.POINTER(C.c_double)), avg.ctypes.data_as(C.POINTER(C.c_double)))
    return f.reshape(25, n), avg


def read_vorticity(workdir, dimension, include_baryon):
    """The six thermal-vorticity columns (wtx wty wtn wxy wxn wyn) of a mode-5 input/surface.dat, shape (6, n)."""
    lib = load()
    n = lib.is3d_host_read_vorticity(workdir.encode(), dimension, include_baryon, None)
    if n < 0:
        raise RuntimeError("surface read failed")
    w = np.zeros(6 * n)
    lib.is3d_host_read_vorticity(workdir.encode(), dimension, include_baryon, w.ctypes.data_as(C.POINTER(C.c_double)))
    return w.reshape(6, n)


def read_pdg(workdir, hrg_eos):
    lib = load()
    n = lib.is3d_host_read_pdg(workdir.encode(), hrg_eos, 0, None, None, None, None, None)
    if n < 0:
        raise RuntimeError("pdg read failed")
    mc = np.zeros(n, dtype=np.int64); m = np.zeros(n); g = np.zeros(n, dtype=np.int32)
    b = np.zeros(n, dtype=np.int32); s = np.zeros(n, dtype=np.int32)
    lib.is3d_host_read_pdg(workdir.encode(), hrg_eos, n, mc.ctypes.data_as(C.POINTER(C.c_long)),
                           m.ctypes.data_as(C.POINTER(C.c_double)), g.ctypes.data_as(C.POINTER(C.c_int)),
                           b.ctypes.data_as(C.POINTER(C.c_int)), s.ctypes.data_as(C.POINTER(C.c_int)))
    return dict(mcid=mc, mass=m, gspin=g, baryon=b, sign=s)


def read_decays(workdir, hrg_eos):
    """The decay rows of the run directory's PDG file, antibaryon rows generated, in hrg.decay_channels' form:
    row_mcid, row_n_body, row_branching, row_daughters[n][5]."""
    lib = load()
    n = lib.is3d_host_read_decays(workdir.encode(), hrg_eos, 0, None, None, None, None)
    if n < 0:
        raise RuntimeError("pdg read failed")
    mc = np.zeros(n, dtype=np.int64); nb = np.zeros(n, dtype=np.int32); br = np.zeros(n)
    ds = np.zeros((n, 5), dtype=np.int64)
    lib.is3d_host_read_decays(workdir.encode(), hrg_eos, n, mc.ctypes.data_as(C.POINTER(C.c_long)),
                              nb.ctypes.data_as(C.POINTER(C.c_int)), br.ctypes.data_as(C.POINTER(C.c_double)),
                              ds.ctypes.data_as(C.POINTER(C.c_long)))
    return dict(row_mcid=mc, row_n_body=nb.astype(np.int64), row_branching=br, row_daughters=ds)


def read_df_tables(table_dir):
    """(T[nT], muB[nmuB], tab[10][nmuB][nT]) of the ten files c0.dat .. betapi.dat in table_dir (the driver's reader)."""
    lib = load()
    nT, nB = C.c_int(), C.c_int()
    if lib.is3d_host_read_df_tables(table_dir.encode(), C.byref(nT), C.byref(nB), 0, None, None, None):
        raise RuntimeError("df table read failed")
    T, muB, tab = np.zeros(nT.value), np.zeros(nB.value), np.zeros((10, nB.value, nT.value))
    PD = C.POINTER(C.c_double)
    lib.is3d_host_read_df_tables(table_dir.encode(), C.byref(nT), C.byref(nB), tab.size, T.ctypes.data_as(PD),
                                 muB.ctypes.data_as(PD), tab.ctypes.data_as(PD))
    return T, muB, tab


def param(path, key):
    v = C.c_double()
    if load().is3d_host_param(path.encode(), key.encode(), C.byref(v)):
        raise KeyError(key)
    return v.value


class HostError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def run_particlization(workdir, out_size, device=0, num_devices=1):
    """IS3D::run_particlization on devices [device, device + num_devices); returns the spectra (operation = 1) or,
    per species, [tau bins | r bins | phip bins] of the spacetime distributions (operation = 0: df_mode 1-4 through
    is3d_calculate_dN_dX, df_mode 5 through is3d_calculate_dN_dX_famod)."""
    lib = load()
    out = np.zeros(out_size)
    err = C.create_string_buffer(512)
    rc = lib.is3d_host_run_particlization(workdir.encode(), device, num_devices,
                                          out.ctypes.data_as(C.POINTER(C.c_double)), out_size, err, 512)
    if rc:
        raise HostError(rc, err.value.decode())
    return out


def run_particlization_devices(workdir, out_size, devices):
    """The same with cell shard k on devices[k] (indices may repeat)."""
    lib = load()
    out = np.zeros(out_size)
    err = C.create_string_buffer(512)
    dv = np.ascontiguousarray(devices, dtype=np.int32)
    rc = lib.is3d_host_run_particlization_devices(workdir.encode(), dv.ctypes.data_as(C.POINTER(C.c_int)), len(dv),
                                                  out.ctypes.data_as(C.POINTER(C.c_double)), out_size, err, 512)
    if rc:
        raise HostError(rc, err.value.decode())
    return out


def polarization(workdir, out_size, devices=(0,)):
    """mode = 5 run directory: calculate_spin_polzn alone (Polarization.cpp:25-263).  Writes results/S{t,x,y,n}.dat
    and returns the raw sums (S_t, S_x, S_y, S_n, Snorm), flat [5][species][pT][phi][y]; out_size = 5 x spectra size."""
    lib = load()
    out = np.zeros(out_size)
    err = C.create_string_buffer(512)
    dv = np.ascontiguousarray(devices, dtype=np.int32)
    rc = lib.is3d_host_polarization(workdir.encode(), dv.ctypes.data_as(C.POINTER(C.c_int)), len(dv),
                                    out.ctypes.data_as(C.POINTER(C.c_double)), out_size, err, 512)
    if rc:
        raise HostError(rc, err.value.decode())
    return out


def total_yield(workdir, device=0, num_devices=1):
    """operation = 2 in the run directory: (Ntotal, Nevents) of the oversampling estimate."""
    lib = load()
    nt, ne = C.c_double(), C.c_long()
    err = C.create_string_buffer(512)
    rc = lib.is3d_host_total_yield(workdir.encode(), device, num_devices, C.byref(nt), C.byref(ne), err, 512)
    if rc:
        raise RuntimeError(err.value.decode())
    return nt.value, ne.value


def sample(workdir, devices=(0,), write_files=True, write_csv=False):
    """operation = 2 run directory (df_mode 1-4; df_mode 5 through is3d_sample_famod): the estimate, then the GPU
    sampler over Nevents events.  Writes
    results/particle_list_osc_<event>.dat (and particle_list_<event>.dat with write_csv).  Returns a dict: particles
    (structured array, _lib.PARTICLE_DTYPE), mcid (per particle), offsets (Nevents + 1), n_total, n_events, seed.
    The list is sized by a first call that writes nothing, so a clock seed (sampler_seed < 0) is refused here:
    the second call would sample another list.

    test_sampler = 1 in the run directory: the particles are binned on the device and never listed, as in the
    reference -- write_files writes the results/sampled/* tree and no particle list, the returned list is empty and
    "hist" holds the histograms (Engine.sample_hist's dict) and "stats" the sampler's counters; "hist" is None for
    test_sampler = 0.

    do_resonance_decays = 1: the sampled list is decayed down its chains on the GPU (Engine.decay_sampled with the
    sampler's seed) before anything is returned or written -- particles, mcid, offsets and the files are the final
    hadrons', and the dict gains "origins" (index of each record's primary in the sampled list) and "decay_stats";
    with test_sampler = 1 the final hadrons are binned."""
    from ._lib import PARTICLE_DTYPE, DecayListStats, SampleBins, SampleStats
    from .engine import split_sample_hist
    lib = load()
    pfile = os.path.join(workdir, "iS3D_parameters.dat")
    if param(pfile, "sampler_seed") < 0:
        raise HostError(1, "host.sample needs a fixed sampler_seed >= 0 in iS3D_parameters.dat")
    dv = np.ascontiguousarray(devices, dtype=np.int32)
    pdv = dv.ctypes.data_as(C.POINTER(C.c_int))
    n, nev, nt, seed = C.c_long(), C.c_long(), C.c_double(), C.c_long()
    err = C.create_string_buffer(512)
    try:
        binned = param(pfile, "test_sampler") != 0
    except KeyError:
        binned = False
    try:
        decays = param(pfile, "do_resonance_decays") == 1
    except KeyError:
        decays = False
    if binned:
        PL = C.POINTER(C.c_long)
        bins, npart, nc, nv = SampleBins(), C.c_int(), C.c_long(), C.c_long()
        if lib.is3d_host_sample_hist_size(workdir.encode(), C.byref(bins), C.byref(npart), C.byref(nc), C.byref(nv)):
            raise HostError(1, "cannot read iS3D_parameters.dat / PDG/chosen_particles.dat")
        counts = np.zeros(nc.value, dtype=np.int64)
        vn = np.zeros(nv.value)
        st, dst = SampleStats(), DecayListStats()
        rc = lib.is3d_host_sample_binned_decays(workdir.encode(), pdv, len(dv), int(write_files), counts.ctypes.data_as(PL),
                                                len(counts), vn.ctypes.data_as(C.POINTER(C.c_double)), len(vn), C.byref(nev),
                                                C.byref(nt), C.byref(seed), C.byref(st), C.byref(dst), err, 512)
        if rc:
            raise HostError(rc, err.value.decode())
        hist = split_sample_hist(counts, vn, {k: getattr(bins, k) for k, _ in bins._fields_})
        extra = dict(origins=np.zeros(0, dtype=np.int64), decay_stats={k: getattr(dst, k) for k, _ in dst._fields_}) if decays else {}
        return dict(extra, particles=np.zeros(0, dtype=PARTICLE_DTYPE), mcid=np.zeros(0, dtype=np.int64),
                    offsets=np.zeros(nev.value + 1, dtype=np.int64), n_total=nt.value, n_events=nev.value, seed=seed.value,
                    hist=hist, stats={k: getattr(st, k) for k, _ in st._fields_})
    rc = lib.is3d_host_sample(workdir.encode(), pdv, len(dv), 0, 0, None, None, 0, None, 0, C.byref(n), C.byref(nev),
                              C.byref(nt), C.byref(seed), err, 512)
    if rc:
        raise HostError(rc, err.value.decode())
    parts = np.zeros(n.value, dtype=PARTICLE_DTYPE)
    mcid = np.zeros(n.value, dtype=np.int64)
    off = np.zeros(nev.value + 1, dtype=np.int64)
    PL = C.POINTER(C.c_long)
    origins = np.zeros(n.value if decays else 0, dtype=np.int64)
    dst = DecayListStats()
    rc = lib.is3d_host_sample_decays(workdir.encode(), pdv, len(dv), int(write_files), int(write_csv),
                                     C.c_void_p(parts.ctypes.data), mcid.ctypes.data_as(PL), n.value, off.ctypes.data_as(PL),
                                     len(off), C.byref(n), C.byref(nev), C.byref(nt), C.byref(seed),
                                     origins.ctypes.data_as(PL) if decays else None, C.byref(dst), err, 512)
    if rc:
        raise HostError(rc, err.value.decode())
    out = dict(particles=parts, mcid=mcid, offsets=off, n_total=nt.value, n_events=nev.value, seed=seed.value, hist=None)
    if decays:        # do_resonance_decays = 1: the list is the decayed one
        out.update(origins=origins, decay_stats={k: getattr(dst, k) for k, _ in dst._fields_})
    return out


def write_particle_lists(workdir, particles, offsets, mcid, mass, write_csv=True):
    """The reference's two particle-list writers for a list the caller holds (host_io.cpp write_particle_list_*)."""
    lib = load()
    p = np.ascontiguousarray(particles)
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    mc = np.ascontiguousarray(mcid, dtype=np.int64)
    m = np.ascontiguousarray(mass, dtype=np.float64)
    err = C.create_string_buffer(512)
    rc = lib.is3d_host_write_particle_lists(workdir.encode(), len(off) - 1, off.ctypes.data_as(C.POINTER(C.c_long)),
                                            C.c_void_p(p.ctypes.data), mc.ctypes.data_as(C.POINTER(C.c_long)),
                                            m.ctypes.data_as(C.POINTER(C.c_double)), int(write_csv), err, 512)
    if rc:
        raise HostError(rc, err.value.decode())
