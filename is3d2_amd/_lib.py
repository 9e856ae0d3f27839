"""ctypes binding of libis3d_amd.so (include/is3d_amd.h).

The library is built in-tree by is3d2_amd/csrc/Makefile (or __graft_entry__.build()).
There is no fallback: if the HIP library is missing, importing the engine fails.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IS3D_LIB") or os.path.join(_HERE, "libis3d_amd.so")   # IS3D_LIB: A/B builds only

SURFACE_FIELDS = ["tau", "x", "y", "eta", "dat", "dax", "day", "dan", "ux", "uy", "un", "E", "T", "P",
                  "pixx", "pixy", "pixn", "piyy", "piyn", "bulkPi", "muB", "nB", "Vx", "Vy", "Vn"]

IS3D_OK, IS3D_ERR_ARG, IS3D_ERR_STATE, IS3D_ERR_DEVICE, IS3D_ERR_DF_RANGE, IS3D_ERR_UNSUPPORTED = range(6)

# every symbol include/is3d_amd.h declares
EXPORTS = ["is3d_abi_version", "is3d_build_id", "is3d_create", "is3d_create_devices", "is3d_destroy", "is3d_last_error", "is3d_set_params", "is3d_set_tuning", "is3d_get_tuning",
           "is3d_set_species", "is3d_set_species_classes", "is3d_species_integrated", "is3d_lanes_integrated", "is3d_set_pdg", "is3d_set_momentum_grid", "is3d_set_gauss_laguerre",
           "is3d_set_df_tables", "is3d_set_surface", "is3d_set_surface_device", "is3d_set_cell_window", "is3d_cell_costs", "is3d_calculate_spectra",
           "is3d_launch", "is3d_finish", "is3d_get_stats", "is3d_output_size", "is3d_evaluate_df_coefficients",
           "is3d_surface_averages", "is3d_get_jonah_table", "is3d_set_momentum_weights", "is3d_set_spacetime_bins",
           "is3d_calculate_dN_dX", "is3d_get_cell_yields", "is3d_total_yield", "is3d_set_chain_range",
           "is3d_launch_begin", "is3d_chain_passes", "is3d_chain_pass", "is3d_chain_end", "is3d_launch_end",
           "is3d_chain_boundary_size", "is3d_chain_boundary_get", "is3d_chain_boundary_put",
           "is3d_set_vorticity", "is3d_polarization_size", "is3d_calculate_polarization", "is3d_launch_polarization",
           "is3d_sample", "is3d_sample_count", "is3d_sample_offsets", "is3d_get_particles", "is3d_get_sample_stats",
           "is3d_sample_uniforms", "is3d_set_sample_bins", "is3d_sample_binned", "is3d_sample_hist_size",
           "is3d_get_sample_hist", "is3d_sample_famod", "is3d_get_sample_famod_stats",
           "is3d_calculate_dN_dX_famod",
           "is3d_set_decays", "is3d_set_decays4", "is3d_decay_feeddown", "is3d_launch_feeddown", "is3d_get_decay_stats",
           "is3d_decay_particles", "is3d_decay_sampled", "is3d_get_particle_origins", "is3d_get_decay_list_stats",
           "is3d_sample_decayed", "is3d_generate_df_tables"]

VORTICITY_FIELDS = ["wtx", "wty", "wtn", "wxy", "wxn", "wyn"]


class Params(C.Structure):
    _fields_ = [("operation", C.c_int), ("dimension", C.c_int), ("df_mode", C.c_int), ("include_baryon", C.c_int),
                ("include_bulk_deltaf", C.c_int), ("include_shear_deltaf", C.c_int),
                ("include_baryondiff_deltaf", C.c_int), ("regulate_deltaf", C.c_int), ("outflow", C.c_int),
                ("famod_chains", C.c_int), ("deta_min", C.c_double), ("mass_pion0", C.c_double)]


class SpacetimeBins(C.Structure):
    _fields_ = [("tau_min", C.c_double), ("tau_max", C.c_double), ("tau_bins", C.c_int),
                ("r_min", C.c_double), ("r_max", C.c_double), ("r_bins", C.c_int), ("phip_bins", C.c_int),
                ("threads", C.c_int)]


class Surface(C.Structure):
    _fields_ = [(k, C.POINTER(C.c_double)) for k in SURFACE_FIELDS]


class Vorticity(C.Structure):
    _fields_ = [(k, C.POINTER(C.c_double)) for k in VORTICITY_FIELDS]


class Stats(C.Structure):
    _fields_ = [("cells", C.c_long), ("breakdown", C.c_long), ("pl_negative", C.c_long), ("recon_fail", C.c_long),
                ("iterations", C.c_long), ("ms_prepass", C.c_double), ("ms_spectra", C.c_double),
                ("ms_total", C.c_double)]


class SampleParams(C.Structure):
    _fields_ = [("seed", C.c_long), ("n_events", C.c_int), ("fast", C.c_int), ("y_cut", C.c_double)]


class Particle(C.Structure):
    """is3d_particle: the sampler's plain 96-byte record (PARTICLE_DTYPE is its numpy form)."""
    _fields_ = [("species", C.c_int), ("event", C.c_int), ("cell", C.c_long)] + \
               [(k, C.c_double) for k in ("tau", "x", "y", "eta", "t", "z", "E", "px", "py", "pz")]


PARTICLE_DTYPE = [("species", "<i4"), ("event", "<i4"), ("cell", "<i8")] + \
                 [(k, "<f8") for k in ("tau", "x", "y", "eta", "t", "z", "E", "px", "py", "pz")]


class SampleStats(C.Structure):
    _fields_ = [(k, C.c_long) for k in ("cells", "breakdown", "candidates", "kept", "proposals", "acceptances",
                                        "capped", "clamped", "batches")]


class SampleFamodStats(C.Structure):
    """is3d_sample_famod_stats: the reconstruction counters of the last is3d_sample_famod."""
    _fields_ = [(k, C.c_long) for k in ("plpt_negative", "reconstruction_fail", "iterations")]


class SampleBins(C.Structure):
    """is3d_sample_bins: the test_sampler = 1 bin parameters (SAMPLE_BIN_PARTS: the count parts in layout order)."""
    _fields_ = [("pT_min", C.c_double), ("pT_max", C.c_double), ("pT_bins", C.c_int), ("y_cut", C.c_double),
                ("y_bins", C.c_int), ("phip_bins", C.c_int), ("eta_cut", C.c_double), ("eta_bins", C.c_int),
                ("tau_min", C.c_double), ("tau_max", C.c_double), ("tau_bins", C.c_int),
                ("r_min", C.c_double), ("r_max", C.c_double), ("r_bins", C.c_int)]


class DecayChannel(C.Structure):
    """is3d_decay_channel: one decay row over the chosen species (DECAY_DTYPE is its numpy form)."""
    _fields_ = [("parent", C.c_int), ("n_body", C.c_int), ("daughter", C.c_int * 3), ("branching", C.c_double),
                ("mass_parent", C.c_double), ("width_parent", C.c_double), ("mass", C.c_double * 3),
                ("width", C.c_double * 3)]


DECAY_DTYPE = np.dtype([("parent", "<i4"), ("n_body", "<i4"), ("daughter", "<i4", (3,)), ("branching", "<f8"),
                        ("mass_parent", "<f8"), ("width_parent", "<f8"), ("mass", "<f8", (3,)), ("width", "<f8", (3,))],
                       align=True)


class DecayChannel4(C.Structure):
    """is3d_decay_channel4: a decay row with four daughter slots (DECAY4_DTYPE is its numpy form)."""
    _fields_ = [("parent", C.c_int), ("n_body", C.c_int), ("daughter", C.c_int * 4), ("branching", C.c_double),
                ("mass_parent", C.c_double), ("width_parent", C.c_double), ("mass", C.c_double * 4),
                ("width", C.c_double * 4)]


DECAY4_DTYPE = np.dtype([("parent", "<i4"), ("n_body", "<i4"), ("daughter", "<i4", (4,)), ("branching", "<f8"),
                         ("mass_parent", "<f8"), ("width_parent", "<f8"), ("mass", "<f8", (4,)), ("width", "<f8", (4,))],
                        align=True)


class DecayStats(C.Structure):
    _fields_ = [(k, C.c_long) for k in ("channels", "kept", "skipped_many_body", "skipped_closed", "adjusted",
                                        "levels")] + [("branching_skipped", C.c_double), ("ms_total", C.c_double)]


class DecayListStats(C.Structure):
    """is3d_decay_list_stats: the counters of the last Monte Carlo decay of a particle list."""
    _fields_ = [(k, C.c_long) for k in ("primaries", "decays", "undecayed", "dropped_daughters", "capped",
                                        "final_particles", "passes", "batches")] + [("ms_total", C.c_double)]


# (name in Engine.sample_binned's dict, the bins field that sizes it)
SAMPLE_BIN_PARTS = [("dN_dy", "y_bins"), ("dN_deta", "eta_bins"), ("dN_dphipdy", "phip_bins"), ("pT_count", "pT_bins"),
                    ("dN_taudtaudy", "tau_bins"), ("dN_2pirdrdy", "r_bins"), ("dN_dphisdy", "phip_bins")]


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libis3d_amd.so not built (run `make -C is3d2_amd/csrc` or __graft_entry__.build())")
    lib = C.CDLL(LIB_PATH)
    P = C.POINTER
    d = C.c_double
    pd = P(C.c_double)
    lib.is3d_abi_version.restype = C.c_int
    lib.is3d_build_id.restype = C.c_char_p
    lib.is3d_create.restype = C.c_void_p
    lib.is3d_create.argtypes = [C.c_int]
    lib.is3d_create_devices.restype = C.c_void_p
    lib.is3d_create_devices.argtypes = [C.c_int, P(C.c_int)]
    lib.is3d_destroy.argtypes = [C.c_void_p]
    lib.is3d_last_error.restype = C.c_char_p
    lib.is3d_last_error.argtypes = [C.c_void_p]
    lib.is3d_set_params.argtypes = [C.c_void_p, P(Params)]
    lib.is3d_set_tuning.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
    lib.is3d_get_tuning.restype = C.c_long
    lib.is3d_get_tuning.argtypes = [C.c_void_p, C.c_char_p]
    lib.is3d_set_species.argtypes = [C.c_void_p, C.c_int, pd, pd, pd, pd]
    lib.is3d_set_species_classes.argtypes = [C.c_void_p, C.c_int]
    lib.is3d_species_integrated.argtypes = [C.c_void_p]
    lib.is3d_lanes_integrated.argtypes = [C.c_void_p]
    lib.is3d_set_pdg.argtypes = [C.c_void_p, C.c_int, pd, pd, pd, pd]
    lib.is3d_set_momentum_grid.argtypes = [C.c_void_p, C.c_int, pd, C.c_int, pd, C.c_int, pd, C.c_int, pd, pd]
    lib.is3d_set_gauss_laguerre.argtypes = [C.c_void_p, C.c_int, C.c_int, pd, pd]
    lib.is3d_set_df_tables.argtypes = [C.c_void_p, C.c_int, C.c_int, pd, pd, pd, d]
    lib.is3d_set_surface.argtypes = [C.c_void_p, C.c_long, P(Surface)]
    lib.is3d_set_surface_device.argtypes = [C.c_void_p, C.c_long, C.c_void_p]
    lib.is3d_set_cell_window.argtypes = [C.c_void_p, C.c_long, C.c_long]
    lib.is3d_cell_costs.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    lib.is3d_calculate_spectra.argtypes = [C.c_void_p, pd]
    lib.is3d_launch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.is3d_finish.argtypes = [C.c_void_p]
    lib.is3d_get_stats.argtypes = [C.c_void_p, P(Stats)]
    lib.is3d_output_size.restype = C.c_long
    lib.is3d_output_size.argtypes = [C.c_void_p]
    lib.is3d_evaluate_df_coefficients.argtypes = [C.c_void_p, d, d, d, d, d, pd]
    lib.is3d_generate_df_tables.argtypes = [C.c_void_p, C.c_int, C.c_int, pd, pd, pd]
    lib.is3d_surface_averages.argtypes = [C.c_long, P(Surface), C.c_int, pd]
    lib.is3d_get_jonah_table.argtypes = [C.c_void_p, pd, pd, pd, pd]
    lib.is3d_set_momentum_weights.argtypes = [C.c_void_p, pd, pd]
    lib.is3d_set_spacetime_bins.argtypes = [C.c_void_p, P(SpacetimeBins)]
    lib.is3d_calculate_dN_dX.argtypes = [C.c_void_p, pd, pd, pd]
    lib.is3d_calculate_dN_dX_famod.argtypes = [C.c_void_p, pd, pd, pd]
    lib.is3d_get_cell_yields.argtypes = [C.c_void_p, pd]
    lib.is3d_total_yield.argtypes = [C.c_void_p, pd, d, pd, pd]
    lib.is3d_set_chain_range.argtypes = [C.c_void_p, C.c_long, C.c_long]
    lib.is3d_launch_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.is3d_chain_passes.argtypes = [C.c_void_p]
    lib.is3d_chain_pass.argtypes = [C.c_void_p, C.c_int]
    lib.is3d_chain_end.argtypes = [C.c_void_p]
    lib.is3d_launch_end.argtypes = [C.c_void_p]
    lib.is3d_chain_boundary_size.restype = C.c_long
    lib.is3d_chain_boundary_size.argtypes = [C.c_void_p]
    lib.is3d_chain_boundary_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.is3d_chain_boundary_put.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.is3d_set_vorticity.argtypes = [C.c_void_p, C.c_long, P(Vorticity)]
    lib.is3d_polarization_size.restype = C.c_long
    lib.is3d_polarization_size.argtypes = [C.c_void_p]
    lib.is3d_calculate_polarization.argtypes = [C.c_void_p, d, pd]
    lib.is3d_launch_polarization.argtypes = [C.c_void_p, d, C.c_void_p, C.c_void_p]
    lib.is3d_sample.argtypes = [C.c_void_p, P(SampleParams), pd]
    lib.is3d_sample_count.restype = C.c_long
    lib.is3d_sample_count.argtypes = [C.c_void_p]
    lib.is3d_sample_offsets.argtypes = [C.c_void_p, P(C.c_long)]
    lib.is3d_get_particles.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_void_p]
    lib.is3d_get_sample_stats.argtypes = [C.c_void_p, P(SampleStats)]
    lib.is3d_sample_uniforms.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_long, C.c_long, C.c_long, C.c_int, pd]
    lib.is3d_set_sample_bins.argtypes = [C.c_void_p, P(SampleBins)]
    lib.is3d_sample_binned.argtypes = [C.c_void_p, P(SampleParams), pd, C.c_int]
    lib.is3d_sample_famod.argtypes = [C.c_void_p, P(SampleParams), C.c_int]
    lib.is3d_get_sample_famod_stats.argtypes = [C.c_void_p, P(SampleFamodStats)]
    lib.is3d_sample_hist_size.restype = C.c_long
    lib.is3d_sample_hist_size.argtypes = [C.c_void_p, P(C.c_long), P(C.c_long)]
    lib.is3d_get_sample_hist.argtypes = [C.c_void_p, P(C.c_long), pd]
    lib.is3d_set_decays.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.is3d_set_decays4.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.is3d_decay_feeddown.argtypes = [C.c_void_p, pd]
    lib.is3d_launch_feeddown.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.is3d_get_decay_stats.argtypes = [C.c_void_p, P(DecayStats)]
    lib.is3d_decay_particles.argtypes = [C.c_void_p, C.c_long, C.c_int, P(C.c_long), C.c_void_p, C.c_int]
    lib.is3d_decay_sampled.argtypes = [C.c_void_p, C.c_long, C.c_int]
    lib.is3d_get_particle_origins.argtypes = [C.c_void_p, C.c_long, C.c_long, P(C.c_long)]
    lib.is3d_get_decay_list_stats.argtypes = [C.c_void_p, P(DecayListStats)]
    lib.is3d_sample_decayed.argtypes = [C.c_void_p, P(SampleParams), pd, C.c_long, C.c_int, C.c_int]
    _lib = lib
    return lib


def build_id():
    """Identity of the loaded libis3d_amd.so (hash of its sources and flags, is3d_build_id())."""
    return load().is3d_build_id().decode()
