"""Python host binding of the MI355X engine, shaped like the reference's plug-in
surface for operation = 1:

  EmissionFunctionArray(params, chosen species, pT/phi/y/eta tables, PDG, FO surface, Deltaf_Data)
      -> calculate_spectra()  ->  dN/(pT dpT dphi dy)[species][pT][phi][y]

(EmissionFunction.h:135-140, EmissionFunction.cpp:114-391, 981-1231).  Every call goes
through libis3d_amd.so; there is no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _lib
from . import data as _data
from . import hrg as _hrg

# famod_chains = 1: PTMA's Newton solves warm-start along one chain over every cell, as the reference does as
# shipped (serial: CORES = 1, EmissionFunction.cpp:131-135; MomentumSpectra.cpp:1308-1364); C > 1 reproduces
# a reference run with OMP_NUM_THREADS = C, 0 solves every cell from (T, 1, 1) -- differently converged
# solutions, measured 3.6e-6 from the one-chain spectra (tests/test_gpu_chains.py)
_DEFAULTS = dict(operation=1, dimension=2, df_mode=1, include_baryon=0, include_bulk_deltaf=1,
                 include_shear_deltaf=1, include_baryondiff_deltaf=0, regulate_deltaf=0, outflow=0,
                 famod_chains=1, deta_min=1.e-5, mass_pion0=0.138)


# operation = 0 binning (iS3D_parameters.dat defaults; EmissionFunction.cpp:232-247).  `threads` is the
# reference's CORES: 0 bins every species from zero; C >= 1 reproduces a reference run with
# OMP_NUM_THREADS = C, including its per-species byte-count memset carry (SpacetimeDistribution.cpp:165-167)
SPACETIME_BINS = dict(tau_min=0.0, tau_max=12.0, tau_bins=120, r_min=0.0, r_max=12.0, r_bins=60, phip_bins=100,
                      threads=0)


# test_sampler = 1 binning of the sampled particles (iS3D_parameters.dat defaults; EmissionFunction.cpp:223-247)
SAMPLE_BINS = dict(pT_min=0.0, pT_max=3.0, pT_bins=100, y_cut=5.0, y_bins=100, phip_bins=100, eta_cut=7.0, eta_bins=140,
                   tau_min=0.0, tau_max=12.0, tau_bins=120, r_min=0.0, r_max=12.0, r_bins=60)


def split_sample_hist(counts, vn, bins):
    """The flat (counts, vn) of is3d_get_sample_hist as Engine.sample_hist's dict of arrays."""
    sizes = [int(bins[key]) for _, key in _lib.SAMPLE_BIN_PARTS]
    npart = len(counts) // sum(sizes)
    hist, at = {}, 0
    for (name, _), nb in zip(_lib.SAMPLE_BIN_PARTS, sizes):
        hist[name] = counts[at:at + npart * nb].reshape(npart, nb)
        at += npart * nb
    v = np.asarray(vn).reshape(2, 7, npart, int(bins["pT_bins"]))
    hist["vn_real"], hist["vn_imag"] = v[0], v[1]
    return hist


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _arr(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _decay_table(channels):
    """(n, pointer, array) of a channel table given as a DECAY_DTYPE or DECAY4_DTYPE array or a list of dicts; a
    dict with four daughters makes it a DECAY4_DTYPE table (the array's dtype tells the caller which call to use)."""
    if isinstance(channels, np.ndarray) and channels.dtype in (_lib.DECAY_DTYPE, _lib.DECAY4_DTYPE):
        a = np.ascontiguousarray(channels)
    else:
        four = any(len(c.get("daughter", ())) > 3 for c in channels)
        a = np.zeros(len(channels), dtype=_lib.DECAY4_DTYPE if four else _lib.DECAY_DTYPE)
        a["daughter"] = -1
        for i, c in enumerate(channels):
            for k, v in c.items():
                if k in ("daughter", "mass", "width"):
                    a[k][i, :len(v)] = v
                else:
                    a[k][i] = v
    return len(a), C.c_void_p(a.ctypes.data), a


class IS3DError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("is3d error %d: %s" % (code, msg))
        self.code = code


class Engine:
    """One engine per GPU (device index in the current process's visible devices), or -- devices = [d0, d1,
    ...] -- one engine over several GPUs of this process (is3d_create_devices: cells sharded by estimated cost,
    spectra summed with one RCCL all-reduce inside the compute call)."""

    def __init__(self, device=0, devices=None):
        self.lib = _lib.load()
        if devices is not None:
            dv = (C.c_int * len(devices))(*[int(d) for d in devices])
            self._e = self.lib.is3d_create_devices(len(devices), dv)
            if not self._e:
                raise IS3DError(_lib.IS3D_ERR_DEVICE, "is3d_create_devices(%s) failed" % list(devices))
        else:
            self._e = self.lib.is3d_create(int(device))
        if not self._e:
            raise IS3DError(_lib.IS3D_ERR_DEVICE, "is3d_create(%d) failed (no HIP device?)" % device)
        self._keep = []
        self._list_events = 0      # events of the particle list the engine holds

    def close(self):
        if getattr(self, "_e", None):
            self.lib.is3d_destroy(self._e)
            self._e = None

    def __del__(self):
        self.close()

    def _chk(self, rc):
        if rc != 0:
            raise IS3DError(rc, self.lib.is3d_last_error(self._e).decode())
        return rc

    # --- setup, mirroring the reference services --------------------------------------
    def set_params(self, **kw):
        p = dict(_DEFAULTS)
        p.update({k: v for k, v in kw.items() if k in _DEFAULTS})
        self.params = p
        self._chk(self.lib.is3d_set_params(self._e, C.byref(_lib.Params(**p))))

    def set_tuning(self, key, value):
        """Engine knob (is3d_set_tuning): "phitab_one_bytes" / "phitab_chunk_bytes" (F_TS table chunking),
        "max_splits" / "slab_bytes" / "split_bytes" (k_spectra's cell splits), "sample_bytes" (the sampler's batch
        memory bound); a negative value restores the default."""
        self._chk(self.lib.is3d_set_tuning(self._e, key.encode(), int(value)))

    def get_tuning(self, key):
        """is3d_get_tuning: the knobs above, "phitab_chunks" (F_TS chunks of the last launch) or "splits" (cell splits
        of the last launch); -1 = unknown."""
        return self.lib.is3d_get_tuning(self._e, key.encode())

    def set_species(self, mass, sign, degen, baryon):
        a = [_arr(x) for x in (mass, sign, degen, baryon)]
        self._chk(self.lib.is3d_set_species(self._e, len(a[0]), *[_dp(x) for x in a]))
        self.npart = len(a[0])

    def set_species_classes(self, on=True):
        """Integrate species with identical (mass, sign, baryon [, degeneracy for PTM]) once (default on);
        the spectra equal the per-species integration (bit for bit at the BASELINE sizes, include/is3d_amd.h)."""
        self._chk(self.lib.is3d_set_species_classes(self._e, int(bool(on))))

    def species_integrated(self):
        """The integrand classes under the documented key (include/is3d_amd.h); see lanes_integrated."""
        n = self.lib.is3d_species_integrated(self._e)
        if n < 0:
            self._chk(-n)     # an error comes back as minus its IS3D_ERR_* code
        return n

    def lanes_integrated(self):
        """The lane classes the kernels integrate: the integrand classes, or fewer when the run is baryon-blind
        (is3d_lanes_integrated: SMASH 193 -> 135 without baryon terms)."""
        n = self.lib.is3d_lanes_integrated(self._e)
        if n < 0:
            self._chk(-n)
        return n

    def set_pdg(self, mass, sign, degen, baryon):
        a = [_arr(x) for x in (mass, sign, degen, baryon)]
        self._chk(self.lib.is3d_set_pdg(self._e, len(a[0]), *[_dp(x) for x in a]))

    def set_momentum_grid(self, pT, phi, y, eta, eta_w):
        a = [_arr(x) for x in (pT, phi, y, eta, eta_w)]
        self._chk(self.lib.is3d_set_momentum_grid(self._e, len(a[0]), _dp(a[0]), len(a[1]), _dp(a[1]),
                                                  len(a[2]), _dp(a[2]), len(a[3]), _dp(a[3]), _dp(a[4])))
        self.npT, self.nphi = len(a[0]), len(a[1])

    def set_momentum_weights(self, pT_w, phi_w):
        a, b = _arr(pT_w), _arr(phi_w)
        self._chk(self.lib.is3d_set_momentum_weights(self._e, _dp(a), _dp(b)))

    def set_spacetime_bins(self, **kw):
        b = dict(SPACETIME_BINS)
        b.update({k: v for k, v in kw.items() if k in SPACETIME_BINS})
        self.bins = b
        self._chk(self.lib.is3d_set_spacetime_bins(self._e, C.byref(_lib.SpacetimeBins(**b))))

    def set_gauss_laguerre(self, roots, weights):
        r, w = _arr(roots), _arr(weights)
        self._chk(self.lib.is3d_set_gauss_laguerre(self._e, r.shape[0], r.shape[1], _dp(r), _dp(w)))

    def set_df_tables(self, T, muB, tab, T_avg):
        T, muB, tab = _arr(T), _arr(muB), _arr(tab)
        self._chk(self.lib.is3d_set_df_tables(self._e, len(T), len(muB), _dp(T), _dp(muB), _dp(tab), float(T_avg)))

    def set_surface(self, surf):
        cols = [_arr(surf[k]) if surf.get(k) is not None else None for k in _lib.SURFACE_FIELDS]
        n = len(cols[0])
        self._keep = cols
        s = _lib.Surface(*[(_dp(c) if c is not None else C.POINTER(C.c_double)()) for c in cols])
        self._chk(self.lib.is3d_set_surface(self._e, n, C.byref(s)))
        self.ncell = n
        self._window = None

    def set_surface_device(self, ptr, n):
        self._chk(self.lib.is3d_set_surface_device(self._e, int(n), C.c_void_p(ptr)))
        self.ncell = n
        self._window = None

    def set_cell_window(self, lo, hi):
        """Integrate only cells [lo, hi) of the surface (-1, -1: all); PTMA chains still walk every cell."""
        self._chk(self.lib.is3d_set_cell_window(self._e, int(lo), int(hi)))
        self._window = None if lo < 0 or hi < 0 else (int(lo), int(hi))

    # --- compute -----------------------------------------------------------------------
    def cell_costs(self):
        """Per-cell shard cost estimate of the surface set last (is3d_cell_costs: 0.02 skipped, PTM / PTB
        separable-fallback cells 1.4 / 1.8, else 1)."""
        n = self.ncell
        out = np.zeros(max(n, 1))
        self._chk(self.lib.is3d_cell_costs(self._e, _dp(out)))
        return out[:n]

    def output_size(self):
        return self.lib.is3d_output_size(self._e)

    def calculate_spectra(self):
        out = np.zeros(self.output_size(), dtype=np.float64)
        self._chk(self.lib.is3d_calculate_spectra(self._e, _dp(out)))
        return out

    def calculate_dN_dX(self):
        """operation = 0: (dN_taudtaudy, dN_2pirdrdy, dN_dphidy), each [species][bins]."""
        b = self.bins
        t = np.zeros((self.npart, b["tau_bins"])); r = np.zeros((self.npart, b["r_bins"]))
        ph = np.zeros((self.npart, b["phip_bins"]))
        self._chk(self.lib.is3d_calculate_dN_dX(self._e, _dp(t), _dp(r), _dp(ph)))
        self._yield_cells = self.ncell
        return t, r, ph

    def calculate_dN_dX_famod(self):
        """operation = 0 for df_mode 5 (is3d_calculate_dN_dX_famod): the same three arrays from the per-cell
        decomposition of the PTMA spectra (the reference has no routine); cell_yields() holds the decomposition and
        stats() the breakdown cells and Newton iterations."""
        b = getattr(self, "bins", None)
        if b is None:       # the output shapes come from the bins: the library's own check, before the buffers exist
            raise IS3DError(_lib.IS3D_ERR_STATE, "is3d_set_spacetime_bins not called")
        t = np.zeros((self.npart, b["tau_bins"])); r = np.zeros((self.npart, b["r_bins"]))
        ph = np.zeros((self.npart, b["phip_bins"]))
        self._chk(self.lib.is3d_calculate_dN_dX_famod(self._e, _dp(t), _dp(r), _dp(ph)))
        w = getattr(self, "_window", None)       # a cell window (set_cell_window) is honoured: its cells only
        self._yield_cells = self.ncell if w is None else w[1] - w[0]
        return t, r, ph

    def cell_yields(self):
        """dN_dy_cell [species][cell] of the last calculate_dN_dX / calculate_dN_dX_famod (the latter under a cell
        window: the window's cells)."""
        out = np.zeros((self.npart, getattr(self, "_yield_cells", self.ncell)))
        self._chk(self.lib.is3d_get_cell_yields(self._e, _dp(out)))
        return out

    # --- mode 5: spin polarization from thermal vorticity (Polarization.cpp:25-263) ------------------------
    def set_vorticity(self, w):
        """Thermal vorticity of the surface set last: an array (6, n) in the order wtx wty wtn wxy wxn wyn (the
        last six columns of a mode-5 surface.dat) or a dict with those keys.  A new surface clears it."""
        if isinstance(w, dict):
            cols = [_arr(w[k]) for k in _lib.VORTICITY_FIELDS]
        else:
            w = _arr(w)
            if w.ndim != 2 or w.shape[0] != 6:
                raise ValueError("vorticity must have shape (6, n)")
            cols = [_arr(w[k]) for k in range(6)]
        v = _lib.Vorticity(*[_dp(c) for c in cols])
        self._chk(self.lib.is3d_set_vorticity(self._e, len(cols[0]), C.byref(v)))

    def calculate_polarization(self, T_avg):
        """Raw cell sums (S_t, S_x, S_y, S_n, Snorm)[species][pT][phi][y] at T_avg = Plasma::temperature; the
        reference's results/S*.dat hold S_c / Snorm.  Returns an array (5, npart, npT, nphi, ny)."""
        n = self.lib.is3d_polarization_size(self._e)
        if n < 0:
            raise IS3DError(_lib.IS3D_ERR_STATE, "params / species / momentum grid not set")
        out = np.zeros(n, dtype=np.float64)
        self._chk(self.lib.is3d_calculate_polarization(self._e, float(T_avg), _dp(out)))
        return out.reshape(5, self.npart, self.npT, self.nphi, -1)

    def launch_polarization(self, T_avg, dev_out_ptr, stream_ptr=None):
        """Resident form: writes 5 x output_size doubles into the device buffer; finish() synchronises."""
        self._chk(self.lib.is3d_launch_polarization(self._e, float(T_avg), C.c_void_p(dev_out_ptr),
                                                    C.c_void_p(stream_ptr or 0)))

    # --- do_resonance_decays: feed-down of the continuous spectra (csrc/decay_math.h) -------
    def set_decays(self, channels):
        """The decay channel table over the chosen species (after set_species and set_momentum_grid, which clear it):
        a numpy array of _lib.DECAY_DTYPE (hrg.decay_channels builds it from PDG rows) or a list of dicts with its
        field names.  A _lib.DECAY4_DTYPE array (hrg.decay_channels(..., four_body=True)), or a list in which any dict
        has four daughters, goes through is3d_set_decays4: open 4-body channels are then kept, not skipped."""
        n, ptr, keep = _decay_table(channels)      # keep: the array behind ptr, alive over the call
        call = self.lib.is3d_set_decays4 if keep.dtype == _lib.DECAY4_DTYPE else self.lib.is3d_set_decays
        self._chk(call(self._e, n, ptr))
        del keep

    def feeddown(self, dN):
        """A new array: dN (spectra layout, any shape of output_size elements) with the decay feed-down added;
        every species then holds thermal + feed-down, a decaying parent keeps its own spectrum."""
        out = np.array(dN, dtype=np.float64, order="C", copy=True)
        if out.size != self.output_size():
            raise ValueError("feeddown: the array must hold output_size() = %d values" % self.output_size())
        self._chk(self.lib.is3d_decay_feeddown(self._e, _dp(out)))
        return out

    def launch_feeddown(self, dev_inout_ptr, stream_ptr=None):
        """Resident form: updates output_size doubles in device memory in place; finish() synchronises."""
        self._chk(self.lib.is3d_launch_feeddown(self._e, C.c_void_p(dev_inout_ptr), C.c_void_p(stream_ptr or 0)))

    def decay_stats(self):
        """The channel bookkeeping of set_decays (channels, kept, skipped_many_body, skipped_closed, adjusted,
        levels, branching_skipped) and the device time of the last feed-down (ms_total)."""
        s = _lib.DecayStats()
        self._chk(self.lib.is3d_get_decay_stats(self._e, C.byref(s)))
        return {k: getattr(s, k) for k, _ in s._fields_}

    def launch(self, dev_out_ptr, stream_ptr=None):
        self._chk(self.lib.is3d_launch(self._e, C.c_void_p(dev_out_ptr), C.c_void_p(stream_ptr or 0)))

    def finish(self):
        self._chk(self.lib.is3d_finish(self._e))

    # --- staged launch: PTMA warm-start chains split over processes (include/is3d_amd.h, dist.launch_chained) ---
    def set_chain_range(self, q0, q1):
        """Solve chain positions [q0, q1) of every PTMA warm-start chain and integrate cells [q0 C, q1 C)
        (-1, -1: off).  Needs the staged launch (dist.launch_chained)."""
        self._chk(self.lib.is3d_set_chain_range(self._e, int(q0), int(q1)))

    def launch_begin(self, dev_out_ptr, stream_ptr=None):
        self._chk(self.lib.is3d_launch_begin(self._e, C.c_void_p(dev_out_ptr), C.c_void_p(stream_ptr or 0)))

    def chain_passes(self):
        return self.lib.is3d_chain_passes(self._e)

    def chain_pass(self, j):
        self._chk(self.lib.is3d_chain_pass(self._e, int(j)))

    def chain_end(self):
        self._chk(self.lib.is3d_chain_end(self._e))

    def launch_end(self):
        self._chk(self.lib.is3d_launch_end(self._e))

    def chain_boundary_size(self):
        return self.lib.is3d_chain_boundary_size(self._e)

    def chain_boundary_get(self, slot, buf):
        """Copy this range's boundary slot (0, 1: pass parity, 2: final) into the device tensor buf (launch stream)."""
        self._chk(self.lib.is3d_chain_boundary_get(self._e, int(slot), C.c_void_p(buf.data_ptr())))

    def chain_boundary_put(self, slot, buf):
        """Copy the device tensor buf (the previous range's end states) into this range's incoming slot."""
        self._chk(self.lib.is3d_chain_boundary_put(self._e, int(slot), C.c_void_p(buf.data_ptr())))

    def stats(self):
        s = _lib.Stats()
        self._chk(self.lib.is3d_get_stats(self._e, C.byref(s)))
        out = {k: getattr(s, k) for k, _ in s._fields_}
        # the lane classes of the tables as they stand (is3d_stats itself is fixed by the ABI); 0 before a full setup
        out["lanes_integrated"] = max(0, self.lib.is3d_lanes_integrated(self._e))
        return out

    def evaluate_df_coefficients(self, T, muB, E, P, bulkPi):
        out = np.zeros(15)
        self._chk(self.lib.is3d_evaluate_df_coefficients(self._e, T, muB, E, P, bulkPi, _dp(out)))
        return out

    def generate_df_tables(self, T, muB):
        """The ten delta-f coefficient tables [10][nmuB][nT] (order of set_df_tables) of the PDG list set with set_pdg
        on the grid T x muB, computed on the GPU with rows 1-4 of the Gauss-Laguerre table set with
        set_gauss_laguerre (is3d_generate_df_tables, DESIGN.md 7.9: the reference's offline generator).  Installs
        nothing: pass the result to set_df_tables."""
        T, muB = _arr(T), _arr(muB)
        out = np.zeros((10, len(muB), len(T)))
        self._chk(self.lib.is3d_generate_df_tables(self._e, len(T), len(muB), _dp(T), _dp(muB), _dp(out)))
        return out

    def total_yield(self, plasma, y_cut=0.5):
        """operation = 2 oversampling estimate (ParticleSampler.cpp:447-636): (Ntotal, densities[3][npart]).
        plasma = (T, E, P, muB, nB) averages; the engine's Gauss-Laguerre table must be the 32-point one."""
        pl = _arr(plasma)
        nt = np.zeros(1)
        dens = np.zeros(3 * self.npart)
        self._chk(self.lib.is3d_total_yield(self._e, _dp(pl), float(y_cut), _dp(nt), _dp(dens)))
        return float(nt[0]), dens.reshape(3, self.npart)

    # --- operation = 2: the particle sampler (ParticleSampler.cpp:638-1134) -------------------------------
    def sample(self, seed, n_events, y_cut=0.5, fast=0, plasma=None):
        """Sample n_events events (df_mode 1-4).  plasma = (T, E, P, muB, nB) averages (surface_averages).
        Returns (particles, offsets, stats): a numpy structured array (_lib.PARTICLE_DTYPE: species index, event,
        global cell, tau x y eta t z E px py pz), events contiguous and ordered by (cell, candidate) inside an
        event; offsets[n_events + 1]; and the is3d_sample_stats fields as a dict.  The list is a pure function
        of the seed and the inputs: it does not depend on "sample_bytes" batches, cell windows or devices."""
        pl = _arr(plasma)
        sp = _lib.SampleParams(int(seed), int(n_events), int(fast), float(y_cut))
        self._chk(self.lib.is3d_sample(self._e, C.byref(sp), _dp(pl)))
        self._list_events = int(n_events)
        n = self.lib.is3d_sample_count(self._e)
        parts = np.zeros(max(n, 0), dtype=_lib.PARTICLE_DTYPE)
        offsets = np.zeros(int(n_events) + 1, dtype=np.int64)
        self._chk(self.lib.is3d_sample_offsets(self._e, offsets.ctypes.data_as(C.POINTER(C.c_long))))
        if n > 0:
            self._chk(self.lib.is3d_get_particles(self._e, 0, n, C.c_void_p(parts.ctypes.data)))
        return parts, offsets, self.sample_stats()

    # --- test_sampler = 1: the binned distributions of the kept particles (BinSampledParticle.cpp:9-133) ---
    def set_sample_bins(self, **bins):
        """The reference's bin parameters (is3d_sample_bins): pT_min pT_max pT_bins, y_cut y_bins, phip_bins,
        eta_cut eta_bins, tau_min tau_max tau_bins, r_min r_max r_bins; defaults SAMPLE_BINS."""
        b = dict(SAMPLE_BINS)
        b.update({k: v for k, v in bins.items() if k in SAMPLE_BINS})
        self.sample_bins = b
        self._chk(self.lib.is3d_set_sample_bins(self._e, C.byref(_lib.SampleBins(**b))))

    def sample_hist(self):
        """The histograms of the last sample_binned as a dict: the count parts (int64 [npart][bins]) dN_dy, dN_deta,
        dN_dphipdy, pT_count, dN_taudtaudy, dN_2pirdrdy, dN_dphisdy, and the raw sums vn_real, vn_imag
        ([7][npart][pT_bins]) of cos(k phi), sin(k phi), k = 1..7."""
        nc, nv = C.c_long(0), C.c_long(0)
        if self.lib.is3d_sample_hist_size(self._e, C.byref(nc), C.byref(nv)) < 0:
            raise IS3DError(_lib.IS3D_ERR_STATE, "sample bins / species not set")
        counts = np.zeros(nc.value, dtype=np.int64)
        vn = np.zeros(nv.value, dtype=np.float64)
        self._chk(self.lib.is3d_get_sample_hist(self._e, counts.ctypes.data_as(C.POINTER(C.c_long)), _dp(vn)))
        return split_sample_hist(counts, vn, self.sample_bins)

    def sample_binned(self, seed, n_events, y_cut=0.5, fast=0, plasma=None, keep_list=False):
        """sample() with every kept particle binned on the device (set_sample_bins first).  keep_list = False:
        (hist, stats) -- no list is built, a batch needs only its (event, cell) counts; keep_list = True:
        (hist, stats, particles, offsets) with sample()'s list.  hist: see sample_hist(); it is bit-identical for
        every "sample_bytes" batch, cell window split and device list."""
        pl = _arr(plasma)
        sp = _lib.SampleParams(int(seed), int(n_events), int(fast), float(y_cut))
        self._chk(self.lib.is3d_sample_binned(self._e, C.byref(sp), _dp(pl), int(bool(keep_list))))
        self._list_events = int(n_events)
        hist, stats = self.sample_hist(), self.sample_stats()
        if not keep_list:
            return hist, stats
        n = self.lib.is3d_sample_count(self._e)
        parts = np.zeros(max(n, 0), dtype=_lib.PARTICLE_DTYPE)
        offsets = np.zeros(int(n_events) + 1, dtype=np.int64)
        self._chk(self.lib.is3d_sample_offsets(self._e, offsets.ctypes.data_as(C.POINTER(C.c_long))))
        if n > 0:
            self._chk(self.lib.is3d_get_particles(self._e, 0, n, C.c_void_p(parts.ctypes.data)))
        return hist, stats, parts, offsets

    # --- df_mode 5: sample_dN_pTdpTdphidy_famod (ParticleSampler.cpp:1138-1627) -----------------------------
    def _sampled_list(self, n_events):
        n = self.lib.is3d_sample_count(self._e)
        parts = np.zeros(max(n, 0), dtype=_lib.PARTICLE_DTYPE)
        offsets = np.zeros(int(n_events) + 1, dtype=np.int64)
        self._chk(self.lib.is3d_sample_offsets(self._e, offsets.ctypes.data_as(C.POINTER(C.c_long))))
        if n > 0:
            self._chk(self.lib.is3d_get_particles(self._e, 0, n, C.c_void_p(parts.ctypes.data)))
        return parts, offsets

    def sample_famod(self, seed, n_events, y_cut=0.5):
        """sample() for df_mode 5 (PTMA): (particles, offsets, stats) in sample()'s shapes.  The method takes no
        plasma averages and has no fast branch; each call first reconstructs (lambda, aT, aL) along the reference's
        chain (famod_chains as for the spectra, the sampler's rule); sample_famod_stats() has its counters."""
        sp = _lib.SampleParams(int(seed), int(n_events), 0, float(y_cut))
        self._chk(self.lib.is3d_sample_famod(self._e, C.byref(sp), 0))
        self._list_events = int(n_events)
        parts, offsets = self._sampled_list(n_events)
        return parts, offsets, self.sample_stats()

    def sample_famod_binned(self, seed, n_events, y_cut=0.5, keep_list=False):
        """sample_binned() for df_mode 5: (hist, stats), or (hist, stats, particles, offsets) with keep_list."""
        sp = _lib.SampleParams(int(seed), int(n_events), 0, float(y_cut))
        self._chk(self.lib.is3d_sample_famod(self._e, C.byref(sp), 2 if keep_list else 1))
        self._list_events = int(n_events)
        hist, stats = self.sample_hist(), self.sample_stats()
        if not keep_list:
            return hist, stats
        return (hist, stats) + self._sampled_list(n_events)

    def sample_famod_stats(self):
        """The last sample_famod's reconstruction counters: plpt_negative, reconstruction_fail, iterations."""
        s = _lib.SampleFamodStats()
        self._chk(self.lib.is3d_get_sample_famod_stats(self._e, C.byref(s)))
        return {k: getattr(s, k) for k, _ in s._fields_}

    def sample_stats(self):
        s = _lib.SampleStats()
        self._chk(self.lib.is3d_get_sample_stats(self._e, C.byref(s)))
        return {k: getattr(s, k) for k, _ in s._fields_}

    # --- do_resonance_decays for the sampler: Monte Carlo decays of a particle list ----------
    def _decayed_list(self):
        n = self.lib.is3d_sample_count(self._e)
        parts = np.zeros(max(n, 0), dtype=_lib.PARTICLE_DTYPE)
        origins = np.zeros(max(n, 0), dtype=np.int64)
        if n > 0:
            self._chk(self.lib.is3d_get_particles(self._e, 0, n, C.c_void_p(parts.ctypes.data)))
            self._chk(self.lib.is3d_get_particle_origins(self._e, 0, n, origins.ctypes.data_as(C.POINTER(C.c_long))))
        return parts, origins

    def decay_sampled(self, seed, binned=False):
        """Decay the last sampled list down the chains of set_decays' channels, in place of it.  Returns (particles,
        offsets, origins, stats): the final hadrons in sample()'s shapes (primaries in their order, each replaced by
        its leaves), origins[i] = index in the sampled list of the primary record i descends from, and the
        is3d_decay_list_stats fields.  binned = True (set_sample_bins first): sample_hist() then holds the
        histograms of the decayed list.  The list is a pure function of (seed, sampled list)."""
        self._chk(self.lib.is3d_decay_sampled(self._e, int(seed), int(bool(binned))))
        parts, origins = self._decayed_list()
        offsets = np.zeros(self._list_events + 1, dtype=np.int64)     # the events of the list the engine holds
        self._chk(self.lib.is3d_sample_offsets(self._e, offsets.ctypes.data_as(C.POINTER(C.c_long))))
        return parts, offsets, origins, self.decay_list_stats()

    def sample_decayed(self, seed, n_events, decay_seed, y_cut=0.5, fast=0, plasma=None, keep_list=True, binned=False):
        """sample() (df_mode 5: sample_famod(); plasma and fast are then unused) and decay_sampled(decay_seed, binned)
        in one device-resident pass (is3d_sample_decayed): the sampler's batches are decayed where
        they lie and no primary crosses to the host.  Returns (particles, offsets, origins, stats) with the bytes of
        the two calls.  keep_list = False (with binned = True): only sample_hist() is filled; particles and origins
        are empty and the offsets zero.  sample_stats() holds the sampler's stats."""
        pl = None if plasma is None else _arr(plasma)
        sp = _lib.SampleParams(int(seed), int(n_events), int(fast), float(y_cut))
        self._chk(self.lib.is3d_sample_decayed(self._e, C.byref(sp), None if pl is None else _dp(pl), int(decay_seed),
                                               int(bool(keep_list)), int(bool(binned))))
        self._list_events = int(n_events)
        parts, origins = self._decayed_list()
        offsets = np.zeros(self._list_events + 1, dtype=np.int64)
        self._chk(self.lib.is3d_sample_offsets(self._e, offsets.ctypes.data_as(C.POINTER(C.c_long))))
        return parts, offsets, origins, self.decay_list_stats()

    def list_transfer_bytes(self):
        """(host-to-device, device-to-host) bytes of particle records, stream keys and origins that the last sampling or
        list-decay call copied: the "list_h2d_bytes" / "list_d2h_bytes" tuning keys."""
        return self.get_tuning("list_h2d_bytes"), self.get_tuning("list_d2h_bytes")

    def decay_particles(self, particles, offsets, seed, binned=False):
        """decay_sampled() for a caller's list: particles (PARTICLE_DTYPE) with events contiguous, offsets[n_events
        + 1] into it (offsets[0] may be > 0: a sub-range of events), the records' event field non-decreasing.
        Returns (particles, offsets, origins, stats); origins index the array given."""
        parts = np.ascontiguousarray(particles, dtype=_lib.PARTICLE_DTYPE)
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        self._list_events = len(off) - 1
        self._chk(self.lib.is3d_decay_particles(self._e, int(seed), len(off) - 1, off.ctypes.data_as(C.POINTER(C.c_long)),
                                                C.c_void_p(parts.ctypes.data), int(bool(binned))))
        out, origins = self._decayed_list()
        new_off = np.zeros(len(off), dtype=np.int64)
        self._chk(self.lib.is3d_sample_offsets(self._e, new_off.ctypes.data_as(C.POINTER(C.c_long))))
        return out, new_off, origins, self.decay_list_stats()

    def decay_list_stats(self):
        """The last decay_sampled / decay_particles: primaries, decays, undecayed, dropped_daughters, capped,
        final_particles, passes, batches, ms_total (device time)."""
        s = _lib.DecayListStats()
        self._chk(self.lib.is3d_get_decay_list_stats(self._e, C.byref(s)))
        return {k: getattr(s, k) for k, _ in s._fields_}

    def sample_uniforms(self, seed, purpose, cell, event, candidate, n):
        """Test hook: the first n uniforms of one stream, generated on the device."""
        out = np.zeros(int(n))
        self._chk(self.lib.is3d_sample_uniforms(self._e, int(seed), int(purpose), int(cell), int(event),
                                                int(candidate), int(n), _dp(out)))
        return out

    def jonah_table(self):
        l2, z, bp, mx = np.zeros(301), np.zeros(301), np.zeros(301), np.zeros(1)
        self._chk(self.lib.is3d_get_jonah_table(self._e, _dp(l2), _dp(z), _dp(bp), _dp(mx)))
        return l2, z, bp, mx[0]


def surface_averages(surf, include_baryon=0):
    """Plasma averages (T, E, P, muB, nB) after the reference's setprecision(15) file round trip."""
    lib = _lib.load()
    cols = [_arr(surf[k]) if surf.get(k) is not None else None for k in _lib.SURFACE_FIELDS]
    s = _lib.Surface(*[(_dp(c) if c is not None else C.POINTER(C.c_double)()) for c in cols])
    out = np.zeros(5)
    rc = lib.is3d_surface_averages(len(cols[0]), C.byref(s), int(include_baryon), _dp(out))
    if rc:
        raise IS3DError(rc, "surface averages")
    return out


# ------------------------------------------------------------------------------------------
# run specifications (inputs shared by the engine, the oracle and the bench)
# ------------------------------------------------------------------------------------------
def make_spec(hrg_eos=2, chosen="pikp", pT="pT24", phi="phi24", y="y21", eta="eta24", dimension=2, df_mode=1,
              gla_points=32, df_tables="shipped", df_grid=None, **flags):
    """Everything calculate_spectra needs except the surface: parameters, species, grids,
    Gauss-Laguerre table, delta-f tables.  `chosen` is a key of PDG/chosen_particles_*.dat
    ('pikp', 'smash', 'urqmd', 'box', 'default') or an explicit MCID list.
    df_tables = "generate": build_engine generates the delta-f tables from the spec's PDG list on df_grid = (T, muB)
    (default: the shipped 101 x 81 grid) with the 64-point Gauss-Laguerre table, installs them and stores them as
    spec["df"], so that whatever else reads the spec afterwards (the oracle) sees the same tables."""
    if df_tables not in ("shipped", "generate"):
        raise ValueError('df_tables must be "shipped" or "generate"')
    if df_grid is not None and df_tables != "generate":
        raise ValueError('df_grid needs df_tables="generate"')
    parts = _hrg.pdg_particles(hrg_eos)
    mcids = _hrg.chosen_mcids(chosen) if isinstance(chosen, str) else np.asarray(chosen, dtype=np.int64)
    sp = _hrg.chosen_species(parts, mcids)
    pTv, pTw = _data.grid(pT)
    phiv, phiw = _data.grid(phi)
    yv, _ = _data.grid(y)
    etav, etaw = _data.grid(eta)
    roots, weights = _data.gauss_laguerre(gla_points)
    T, muB, tab = _data.df_tables(hrg_eos)
    params = dict(_DEFAULTS)
    params.update(dimension=dimension, df_mode=df_mode)
    params.update({k: v for k, v in flags.items() if k in _DEFAULTS})
    bins = dict(SPACETIME_BINS)
    bins.update({k: v for k, v in flags.items() if k in SPACETIME_BINS})
    spec = dict(params=params, species=sp, pdg=parts, pT=pTv, phi=phiv, y=yv, eta=etav, eta_w=etaw,
                pT_w=pTw, phi_w=phiw, bins=bins, gla=(roots, weights), df=(T, muB, tab), hrg_eos=hrg_eos)
    if df_tables == "generate":
        gT, gB = (T, muB) if df_grid is None else (_arr(df_grid[0]), _arr(df_grid[1]))
        spec["df"] = None                   # filled by the first build_engine
        spec["df_generate"] = (gT, gB)
    return spec


def build_engine(spec, surf, T_avg=None, device=0, devices=None, species_classes=True):
    e = Engine(device, devices)
    p = spec["params"]
    e.set_params(**p)
    sp = spec["species"]
    e.set_species(sp["mass"], sp["sign"], sp["degen"], sp["baryon"])
    if not species_classes:
        e.set_species_classes(False)
    pdg = spec["pdg"]
    e.set_pdg(pdg["mass"], pdg["sign"], pdg["gspin"], pdg["baryon"])
    e.set_momentum_grid(spec["pT"], spec["phi"], spec["y"], spec["eta"], spec["eta_w"])
    if "pT_w" in spec:
        e.set_momentum_weights(spec["pT_w"], spec["phi_w"])
    e.set_spacetime_bins(**spec.get("bins", {}))
    if spec.get("df") is None:             # make_spec(df_tables="generate"): from the PDG list, with 64 points
        gT, gB = spec["df_generate"]
        e.set_gauss_laguerre(*_data.gauss_laguerre(64))
        spec["df"] = (gT, gB, e.generate_df_tables(gT, gB))
    e.set_gauss_laguerre(*spec["gla"])
    if T_avg is None:
        T_avg = surface_averages(surf, p["include_baryon"])[0]
    e.set_df_tables(*spec["df"], T_avg)
    if surf is not None:
        e.set_surface(surf)
        if all(surf.get(k) is not None for k in _lib.VORTICITY_FIELDS):   # mode 5: thermal vorticity
            e.set_vorticity({k: surf[k] for k in _lib.VORTICITY_FIELDS})
    return e


def output_shape(spec):
    ny = len(spec["y"]) if spec["params"]["dimension"] == 3 else 1
    return (len(spec["species"]["mass"]), len(spec["pT"]), len(spec["phi"]), ny)
