"""ctypes binding of libsph_mi355x.so (include/sph_mi355x.h).

The library is the product: there is no CPU fallback and nothing here imports oracle/.
If the shared object is missing it is built with hipcc (cfd_taichi_amd/build.py); if that is
impossible, or no gfx950 device is visible when a simulation is created, a RuntimeError is raised.
"""
import ctypes
import os

import numpy as np

from . import build as _build

SPH_OK = 0
ARITH_EXACT, ARITH_RELAXED = 0, 1      # SphConfig.arith
SPH_E_INVALID, SPH_E_HIP, SPH_E_NO_DEVICE, SPH_E_OVERFLOW, SPH_E_STATE = -1, -2, -3, -4, -5
SOLVER_WCSPH, SOLVER_DFSPH, SOLVER_PCISPH, SOLVER_IISPH, SOLVER_PBF = 0, 1, 2, 3, 4
SOLVER_IDS = {"wcsph": SOLVER_WCSPH, "dfsph": SOLVER_DFSPH, "pcisph": SOLVER_PCISPH, "iisph": SOLVER_IISPH, "pbf": SOLVER_PBF}
SPECIES_FLUID, SPECIES_WALL, SPECIES_RIGID = 0, 1, 2
F_POS, F_VEL, F_ACC, F_RHO, F_PRESSURE, F_ALPHA, F_WARM_K, F_RHO_ADV, F_RHO_DER, F_VEL_ADV = range(10)
F_NBR_COUNT = 14
F_PRESS_ITER, F_PRESS_FORCE, F_POS_PREDICT, F_D_II, F_A_II, F_D_IJ = range(16, 22)
F_PBF_LAMBDA, F_PBF_DELTA_POS = 22, 23
F_WALL_POS, F_WALL_VOL = 32, 33
F_RIGID_POS, F_RIGID_VOL, F_RIGID_FORCE, F_RIGID_MASS, F_RIGID_VERT = 48, 49, 50, 51, 52
S_RIGID_CENTROID, S_RIGID_OMEGA, S_RIGID_VEL, S_RIGID_MASS, S_RIGID_INERTIA_INV = 10, 13, 16, 19, 20
S_DELTA_TIME, S_SIMULATE_CNT, S_PARTICLE_M, S_SUPPORT_RADIUS, S_PS_DELTA_TIME, S_GRAPH_LAUNCHES = range(6)
S_PCISPH_DELTA, S_PCISPH_BETA, S_PCISPH_MAX_INDEX, S_PCISPH_MAX_COUNT = range(6, 10)
S_ARITH_RELAXED = 30
S_VERLET_BUILDS = 31
S_RIGID_ACTIVE = 32
S_RIGID_ACC, S_RIGID_ALPHA, S_RIGID_MODE = 33, 36, 39
S_TIME, S_ACCEL, S_GRAVITY_VEC = 40, 41, 44                  # the handle's clock (f64), its acceleration vector (+0, 1, 2) and the base vector g
S_PAIR_BITS = 48                                              # diagnostics: 1 if the last dfsph step's solver-loop sweeps read the pair-bit cache
S_FLUID_CAPACITY = 47                                         # fluid particles the handle can hold (SphConfig.fluid_capacity, or the lattice's count)
RIGID_DYNAMIC, RIGID_SCRIPTED, RIGID_FIXED = 0, 1, 2          # sph_rigid_set_mode
RIGID_MODES = {"dynamic": RIGID_DYNAMIC, "scripted": RIGID_SCRIPTED, "fixed": RIGID_FIXED}
# `solver.<attribute> = value` (include/sph_mi355x.h SPH_P_*): name of the reference's attribute -> id
SOLVER_PARAMS = {"density_threshold": 64, "min_iteration_density": 65, "min_iteration_density_divergence": 66, "max_iteration_density_divergence": 67,
                 "density_divergence_threshold": 68, "warm_start": 69, "adaptive_dt": 70, "max_dt": 71, "min_dt": 72,
                 "viscosity_c_s": 73, "viscosity_alpha": 74, "viscosity_epsilon": 75, "tension_k": 76,
                 # the adaptive time step of wcsph / pcisph / iisph / pbf handles (this library's own; dfsph has 70-72)
                 "step_adaptive_dt": 77, "step_max_dt": 78, "step_min_dt": 79}
VECTOR_FIELDS = {F_POS, F_VEL, F_ACC, F_VEL_ADV, F_WALL_POS, F_RIGID_POS, F_RIGID_FORCE, F_RIGID_VERT, F_PRESS_FORCE, F_POS_PREDICT, F_D_II, F_D_IJ,
                 F_PBF_DELTA_POS}

EXPORTS = [
    "sph_abi_version", "sph_set_comm_sized", "sph_create", "sph_destroy", "sph_get_sizes", "sph_last_error", "sph_upload", "sph_download",
    "sph_step_wcsph", "sph_step_dfsph", "sph_step_pcisph", "sph_step_iisph", "sph_step_pbf", "sph_build_neighbors", "sph_compute_density", "sph_compute_alpha",
    "sph_get_scalar", "sph_set_scalar", "sph_synchronize", "sph_overrides", "sph_profile_enable", "sph_profile_reset", "sph_profile_kernel_count",
    "sph_profile_kernel_name", "sph_profile_get", "sph_selftest_math", "sph_selftest_wave", "sph_selftest_stage", "sph_selftest_walk", "sph_selftest_walk_bits", "sph_tune_time",
    "sph_set_comm", "sph_rccl_unique_id", "sph_rccl_attach", "sph_rccl_selftest", "sph_get_stream", "sph_plan_slabs", "sph_replan_slabs", "sph_slab_set_overlap", "sph_slab_info", "sph_comm_stats", "sph_download_local", "sph_download_ids",
    "sph_create_rigid", "sph_rigid_step", "sph_rigid_set_active", "sph_rigid_init_data", "sph_slab_set_state",
    "sph_rigid_set_mode", "sph_rigid_set_motion", "sph_rigid_get_load", "sph_set_gravity", "sph_set_forcing",
    "sph_add_particles", "sph_remove_in_box", "sph_diagnostics", "sph_diag_record", "sph_diag_read", "sph_derived",
    "sph_scalar_enable", "sph_scalar_disable", "sph_scalar_upload", "sph_scalar_download", "sph_scalar_set_inflow", "sph_scalar_rate",
    "sph_geometry_add", "sph_geometry_remove", "sph_geometry_info", "sph_geometry_carve", "sph_geometry_wall_counts",
    "sph_wall_load_select", "sph_wall_load_get", "sph_wall_load_impulse", "sph_wall_load_forces",
]
# the 32 slots of an SphDiagnostics row (include/sph_mi355x.h), in order: the members' names, _x / _y / _z for the vectors
DIAG_SLOTS = ("time", "dt", "step", "n", "mass", "momentum_x", "momentum_y", "momentum_z",
              "angular_momentum_x", "angular_momentum_y", "angular_momentum_z", "kinetic", "potential", "com_x", "com_y", "com_z",
              "vmax", "vmax_id", "pos_min_x", "pos_min_y", "pos_min_z", "pos_max_x", "pos_max_y", "pos_max_z", "rho_min", "rho_max", "rho_mean",
              "reserved_0", "reserved_1", "reserved_2", "reserved_3", "reserved_4")
DIAG_DTYPE = np.dtype([(name, np.float64) for name in DIAG_SLOTS])
# the derived per-particle fields (include/sph_mi355x.h SPH_D_*): name -> id, and id -> the shape of one particle's entry
D_VELGRAD, D_VORTICITY, D_DIVERGENCE, D_NORMAL, D_COVER = 0, 1, 2, 3, 4
DERIVED = {"velgrad": D_VELGRAD, "vorticity": D_VORTICITY, "divergence": D_DIVERGENCE, "normal": D_NORMAL, "cover": D_COVER}
DERIVED_SHAPE = {D_VELGRAD: (3, 3), D_VORTICITY: (3,), D_DIVERGENCE: (), D_NORMAL: (3,), D_COVER: ()}


class SphConfig(ctypes.Structure):
    _fields_ = [
        ("box_min", ctypes.c_double * 3),
        ("box_max", ctypes.c_double * 3),
        ("particle_radius", ctypes.c_double),
        ("gravity", ctypes.c_double),
        ("delta_time", ctypes.c_double),
        ("start_pos", ctypes.c_double * 3),
        ("water_size", ctypes.c_double * 3),
        ("boundary_handle", ctypes.c_int32),
        ("fs_couple", ctypes.c_int32),
        ("solver", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("max_neighbors", ctypes.c_int32),
        ("max_wall_neighbors", ctypes.c_int32),
        ("max_density_iters", ctypes.c_int32),
        ("slab_rank", ctypes.c_int32),
        ("slab_count", ctypes.c_int32),
        ("slab_capacity", ctypes.c_int32),
        ("slab_rebalance_every", ctypes.c_int32),
        ("arith", ctypes.c_int32),
        ("slab_ghost_layers", ctypes.c_int32),
        ("slab_overlap", ctypes.c_int32),
        ("fluid_capacity", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 1),
    ]


class SphRigid(ctypes.Structure):
    _fields_ = [
        ("n_particles", ctypes.c_int32),
        ("n_vertices", ctypes.c_int32),
        ("points", ctypes.c_void_p),
        ("vertices", ctypes.c_void_p),
        ("rho_0", ctypes.c_double),
        ("pos_offset", ctypes.c_double * 3),
        ("attitude_offset", ctypes.c_double * 3),
        ("active", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class SphSizes(ctypes.Structure):
    _fields_ = [
        ("n_fluid", ctypes.c_int32),
        ("n_wall", ctypes.c_int32),
        ("n_rigid", ctypes.c_int32),
        ("grid", ctypes.c_int32 * 3),
        ("n_cells", ctypes.c_int32),
        ("max_neighbors", ctypes.c_int32),
        ("max_wall_neighbors", ctypes.c_int32),
    ]


class SphStepStats(ctypes.Structure):
    _fields_ = [
        ("n_div", ctypes.c_int32),
        ("n_dens", ctypes.c_int32),
        ("n_div_evals", ctypes.c_int32),
        ("capped", ctypes.c_int32),
        ("div_first_err", ctypes.c_float),
        ("div_err", ctypes.c_float),
        ("dens_err", ctypes.c_float),
        ("dt", ctypes.c_float),
        ("max_nbrs", ctypes.c_int32),
        ("max_wall_nbrs", ctypes.c_int32),
        ("lost", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


EXCHANGE_COUNTS_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                      ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32))
EXCHANGE_BUFFERS_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t)
ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int32, ctypes.c_int32)
ALLREDUCE_STREAM_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32)
EXCHANGE_COUNTS_N_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                        ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32))


class SphComm(ctypes.Structure):
    _fields_ = [
        ("user", ctypes.c_void_p),
        ("exchange_counts", EXCHANGE_COUNTS_FN),
        ("exchange_buffers", EXCHANGE_BUFFERS_FN),
        ("allreduce", ALLREDUCE_FN),
        ("send_left", ctypes.c_void_p),
        ("send_right", ctypes.c_void_p),
        ("recv_left", ctypes.c_void_p),
        ("recv_right", ctypes.c_void_p),
        ("capacity", ctypes.c_size_t),
        ("on_host", ctypes.c_int32),
        ("stream_ordered", ctypes.c_int32),
        ("allreduce_stream", ALLREDUCE_STREAM_FN),
        ("reduce_buf", ctypes.c_void_p),
        ("exchange_counts_n", EXCHANGE_COUNTS_N_FN),
        ("reduce_capacity", ctypes.c_size_t),
    ]


_lib = None


def dev_mode():
    """Development overrides (SPH_LIB here, the SPH_* knobs inside the library) take effect only with SPH_DEV=1."""
    return os.environ.get("SPH_DEV") == "1"


def library_path():
    # SPH_LIB selects an alternative build of the same library (A/B experiments, tools); default is the in-tree build.
    # It is a development override: without SPH_DEV=1 a set SPH_LIB is refused, never silently honoured or silently dropped.
    alt = os.environ.get("SPH_LIB")
    if alt and not dev_mode():
        raise RuntimeError("SPH_LIB=%s is set but development overrides need SPH_DEV=1; the product loads %s only" % (alt, _build.LIB))
    return alt or _build.LIB


# the per-step path of include/sph_mi355x.h: what any implementation of the ABI exports (the device-specific entry points --
# slabs / RCCL, profiling, tuning, self-tests -- are bound by load() for libsph_mi355x.so only)
ABI_VERSION = 5          # include/sph_mi355x.h SPH_ABI_VERSION: checked when a library is bound
CORE_EXPORTS = [
    "sph_abi_version", "sph_create", "sph_create_rigid", "sph_destroy", "sph_get_sizes", "sph_last_error", "sph_upload", "sph_download",
    "sph_step_wcsph", "sph_step_dfsph", "sph_step_pcisph", "sph_step_iisph", "sph_step_pbf", "sph_rigid_step",
    "sph_build_neighbors", "sph_compute_density", "sph_compute_alpha", "sph_get_scalar", "sph_set_scalar", "sph_synchronize",
]
# entry points added without a change of SPH_ABI_VERSION (no struct grew, no signature changed): bound where the library has them, and a call on a
# library without them raises SphError(SPH_E_STATE)
OPTIONAL_EXPORTS = ["sph_rigid_set_active", "sph_rigid_init_data", "sph_selftest_stage", "sph_selftest_walk", "sph_selftest_walk_bits", "sph_slab_set_state",
                    "sph_rigid_set_mode", "sph_rigid_set_motion", "sph_rigid_get_load", "sph_set_gravity", "sph_set_forcing",
                    "sph_add_particles", "sph_remove_in_box", "sph_diagnostics", "sph_diag_record", "sph_diag_read", "sph_derived",
                    "sph_scalar_enable", "sph_scalar_disable", "sph_scalar_upload", "sph_scalar_download", "sph_scalar_set_inflow", "sph_scalar_rate",
                    "sph_geometry_add", "sph_geometry_remove", "sph_geometry_info", "sph_geometry_carve", "sph_geometry_wall_counts",
                    "sph_wall_load_select", "sph_wall_load_get", "sph_wall_load_impulse", "sph_wall_load_forces"]


def _bind_core(lib):
    vp, ci = ctypes.c_void_p, ctypes.c_int
    try:
        lib.sph_abi_version.argtypes = []
    except AttributeError:          # a build from before the symbol existed: the very case the check is for
        raise RuntimeError("%s predates SPH_ABI_VERSION (include/sph_mi355x.h is at version %d): rebuild (python -m cfd_taichi_amd.build)"
                           % (getattr(lib, "_name", "library"), ABI_VERSION))
    lib.sph_abi_version.restype = ctypes.c_int32
    if lib.sph_abi_version() != ABI_VERSION:
        raise RuntimeError("%s implements version %d of include/sph_mi355x.h, this binding version %d: rebuild (python -m cfd_taichi_amd.build)"
                           % (getattr(lib, "_name", "library"), lib.sph_abi_version(), ABI_VERSION))
    lib.sph_create.argtypes = [ctypes.POINTER(SphConfig), ctypes.POINTER(vp)]
    lib.sph_create.restype = ci
    lib.sph_create_rigid.argtypes = [ctypes.POINTER(SphConfig), ctypes.POINTER(SphRigid), ctypes.POINTER(vp)]
    lib.sph_rigid_step.argtypes = [vp]
    lib.sph_destroy.argtypes = [vp]
    lib.sph_destroy.restype = None
    lib.sph_get_sizes.argtypes = [vp, ctypes.POINTER(SphSizes)]
    lib.sph_last_error.argtypes = [vp]
    lib.sph_last_error.restype = ctypes.c_char_p
    lib.sph_upload.argtypes = [vp, ci, ci, vp, ctypes.c_size_t]
    lib.sph_download.argtypes = [vp, ci, ci, vp, ctypes.c_size_t]
    lib.sph_step_wcsph.argtypes = [vp, ci]
    lib.sph_step_pbf.argtypes = [vp, ci]
    lib.sph_step_dfsph.argtypes = [vp, ci, ctypes.POINTER(SphStepStats)]
    lib.sph_step_pcisph.argtypes = [vp, ci, ctypes.POINTER(SphStepStats)]
    lib.sph_step_iisph.argtypes = [vp, ci, ctypes.POINTER(SphStepStats)]
    for name in ("sph_build_neighbors", "sph_compute_density", "sph_compute_alpha", "sph_synchronize"):
        getattr(lib, name).argtypes = [vp]
    lib.sph_get_scalar.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_double)]
    lib.sph_set_scalar.argtypes = [vp, ci, ctypes.c_double]
    if hasattr(lib, "sph_rigid_set_active"):
        lib.sph_rigid_set_active.argtypes = [vp, ci]
    if hasattr(lib, "sph_rigid_init_data"):
        lib.sph_rigid_init_data.argtypes = [vp]
    if hasattr(lib, "sph_rigid_set_mode"):
        lib.sph_rigid_set_mode.argtypes = [vp, ci]
    if hasattr(lib, "sph_rigid_set_motion"):
        lib.sph_rigid_set_motion.argtypes = [vp, vp, vp, vp, vp]
    if hasattr(lib, "sph_rigid_get_load"):
        lib.sph_rigid_get_load.argtypes = [vp, vp, vp]
    if hasattr(lib, "sph_set_gravity"):
        lib.sph_set_gravity.argtypes = [vp, vp]
    if hasattr(lib, "sph_set_forcing"):
        lib.sph_set_forcing.argtypes = [vp, vp, vp, vp]
    if hasattr(lib, "sph_add_particles"):
        lib.sph_add_particles.argtypes = [vp, vp, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32)]
    if hasattr(lib, "sph_remove_in_box"):
        lib.sph_remove_in_box.argtypes = [vp, vp, vp, ctypes.POINTER(ctypes.c_int32)]
    if hasattr(lib, "sph_diagnostics"):
        lib.sph_diagnostics.argtypes = [vp, vp]
    if hasattr(lib, "sph_diag_record"):
        lib.sph_diag_record.argtypes = [vp, ci, ci]
    if hasattr(lib, "sph_diag_read"):
        lib.sph_diag_read.argtypes = [vp, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int64)]
    if hasattr(lib, "sph_derived"):
        lib.sph_derived.argtypes = [vp, ci, vp, ctypes.c_size_t]
    if hasattr(lib, "sph_scalar_enable"):
        lib.sph_scalar_enable.argtypes = [vp, ctypes.c_double, ctypes.c_double, ctypes.c_double]
        lib.sph_scalar_disable.argtypes = [vp]
        lib.sph_scalar_upload.argtypes = [vp, vp, ctypes.c_size_t]
        lib.sph_scalar_download.argtypes = [vp, vp, ctypes.c_size_t]
        lib.sph_scalar_set_inflow.argtypes = [vp, ctypes.c_double]
        lib.sph_scalar_rate.argtypes = [vp, vp, ctypes.c_size_t]
    if hasattr(lib, "sph_geometry_add"):
        lib.sph_geometry_add.argtypes = [vp, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32)]
        lib.sph_geometry_remove.argtypes = [vp, ctypes.c_int32]
        lib.sph_geometry_info.argtypes = [vp, vp, vp, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
        lib.sph_geometry_carve.argtypes = [vp, ctypes.c_int32, ctypes.c_float, ctypes.POINTER(ctypes.c_int32)]
    if hasattr(lib, "sph_geometry_wall_counts"):
        lib.sph_geometry_wall_counts.argtypes = [vp, vp, ctypes.c_size_t]
    if hasattr(lib, "sph_wall_load_select"):
        lib.sph_wall_load_select.argtypes = [vp, vp, ctypes.c_size_t]
        lib.sph_wall_load_get.argtypes = [vp, ctypes.c_int32, vp, vp, vp]
        lib.sph_wall_load_impulse.argtypes = [vp, ctypes.c_int32, vp, vp, vp, ctypes.POINTER(ctypes.c_double), ci]
        lib.sph_wall_load_forces.argtypes = [vp, ctypes.c_int32, vp, ctypes.c_size_t]
    return lib


def bind_core(path):
    """Any shared library that implements the per-step path of include/sph_mi355x.h (CORE_EXPORTS), ready for Simulation(cfg, lib=...):
    a test written against the ABI runs unchanged on another implementation of it."""
    lib = ctypes.CDLL(path)
    missing = [n for n in CORE_EXPORTS if not hasattr(lib, n)]
    if missing:
        raise RuntimeError("%s does not export %s" % (path, missing))
    return _bind_core(lib)


def load(build_if_missing=True):
    """Load libsph_mi355x.so; raises RuntimeError if it cannot be found or built."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path) and os.environ.get("SPH_LIB"):
        raise RuntimeError("SPH_LIB=%s does not exist" % path)
    if not os.path.exists(path):
        if not build_if_missing:
            raise RuntimeError("%s is missing; run `python -m cfd_taichi_amd.build`" % path)
        _build.build()
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:
        raise RuntimeError("cannot load %s (%s); the HIP extension is required, there is no CPU fallback" % (path, e))
    vp, ci = ctypes.c_void_p, ctypes.c_int
    _bind_core(lib)
    lib.sph_profile_reset.argtypes = [vp]
    lib.sph_overrides.argtypes = [vp]
    lib.sph_overrides.restype = ctypes.c_char_p
    lib.sph_profile_enable.argtypes = [vp, ci]
    lib.sph_profile_kernel_count.argtypes = []
    lib.sph_profile_kernel_name.argtypes = [ci]
    lib.sph_profile_kernel_name.restype = ctypes.c_char_p
    lib.sph_profile_get.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)]
    lib.sph_selftest_math.argtypes = [ci, ci, vp, vp, vp, ctypes.c_size_t]
    lib.sph_selftest_wave.argtypes = [ci, ci, vp, vp, ctypes.c_size_t]
    if hasattr(lib, "sph_selftest_walk"):
        lib.sph_selftest_walk.argtypes = [vp, ci, ci, ci, vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp]
    if hasattr(lib, "sph_selftest_walk_bits"):
        lib.sph_selftest_walk_bits.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "sph_selftest_stage"):
        lib.sph_selftest_stage.argtypes = [vp, ci, ci, ci, ci, ci, vp, ci, vp, vp, vp, vp, ctypes.c_size_t, vp, ctypes.POINTER(ci)]
    lib.sph_tune_time.argtypes = [vp, ci, ctypes.c_uint, ci, ctypes.POINTER(ctypes.c_double)]
    lib.sph_set_comm.argtypes = [vp, ctypes.POINTER(SphComm)]
    lib.sph_set_comm_sized.argtypes = [vp, ctypes.POINTER(SphComm), ctypes.c_size_t]
    lib.sph_get_stream.argtypes = [vp, ctypes.POINTER(vp)]
    lib.sph_rccl_unique_id.argtypes = [vp]
    lib.sph_rccl_attach.argtypes = [vp, vp, ctypes.c_size_t]
    lib.sph_rccl_selftest.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.c_int32, ctypes.c_int32]
    lib.sph_plan_slabs.argtypes = [ctypes.POINTER(SphConfig), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
    lib.sph_slab_info.argtypes = [vp, ctypes.POINTER(ctypes.c_int32)]
    lib.sph_slab_set_overlap.argtypes = [vp, ctypes.c_int32]
    lib.sph_comm_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_int64), ci]
    lib.sph_replan_slabs.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]
    lib.sph_download_local.argtypes = [vp, ci, vp, ctypes.c_size_t]
    lib.sph_download_ids.argtypes = [vp, vp, ctypes.c_size_t]
    if hasattr(lib, "sph_slab_set_state"):
        lib.sph_slab_set_state.argtypes = [vp, vp, vp, vp, ctypes.c_size_t, ctypes.c_double]
    _lib = lib
    return lib


class SphError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("libsph_mi355x error %d: %s" % (code, message))
        self.code = code


def config_from_dict(config, solver_name=None, device=0, max_neighbors=0, max_wall_neighbors=0, max_density_iters=0,
                     slab_rank=0, slab_count=0, slab_capacity=0, slab_rebalance_every=0, arith=0, slab_ghost_layers=0, slab_overlap=0):
    """Flatten a reference-style config dict (config/*.json schema) into SphConfig.  `fluid.capacity` (optional, an integer): the fluid
    particles the handle can ever hold (SphConfig.fluid_capacity: add_particles, emitters); absent or 0: the lattice's own count."""
    scene, sol, fluid = config["scene"], config["solver"], config["fluid"]
    name = solver_name or sol["name"]
    c = SphConfig()
    c.box_min[:] = [float(v) for v in scene["box_min"]]
    c.box_max[:] = [float(v) for v in scene["box_max"]]
    c.particle_radius = float(scene["particle_radius"])
    c.gravity = gravity_scalar(scene["gravity"])
    c.delta_time = float(sol["delta_time"])
    c.start_pos[:] = [float(v) for v in fluid["start_pos"]]
    c.water_size[:] = [float(v) for v in fluid["water_size"]]
    c.boundary_handle = 1 if sol.get("boundary_handle", True) else 0   # solver_base.py:31
    c.fs_couple = 1 if sol.get("fs_couple", True) else 0              # solver_base.py:32
    if name not in SOLVER_IDS:
        raise NotImplementedError("solver %r: this library covers %s" % (name, sorted(SOLVER_IDS)))
    c.solver = SOLVER_IDS[name]
    c.device = int(device)
    c.max_neighbors = int(max_neighbors)
    c.max_wall_neighbors = int(max_wall_neighbors)
    c.max_density_iters = int(max_density_iters)
    c.slab_rank, c.slab_count, c.slab_capacity = int(slab_rank), int(slab_count), int(slab_capacity)
    c.slab_rebalance_every = int(slab_rebalance_every)
    c.arith = int(arith)
    c.slab_ghost_layers = int(slab_ghost_layers)
    c.slab_overlap = int(slab_overlap)
    capacity = fluid.get("capacity", 0)
    if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or capacity < 0:
        raise ValueError("fluid.capacity must be an integer >= 0, got %r" % (capacity,))
    c.fluid_capacity = int(capacity)
    return c


def _vec3(value, what):
    """three finite numbers -> a list of three floats; anything else is refused"""
    import math
    if isinstance(value, (str, bytes)) or not hasattr(value, "__len__") or len(value) != 3:
        raise ValueError("%s must be a list of three numbers, got %r" % (what, value))
    out = []
    for v in value:
        if isinstance(v, (bool, str, bytes)) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)):
            raise ValueError("%s must be a list of three finite numbers, got %r" % (what, value))
        out.append(float(v))
    return out


def gravity_scalar(gravity):
    """SphConfig.gravity of `scene.gravity`: the number itself, or for a list of three (the vector g) its downward part -g[1], so that
    [0, -G, 0] creates the handle G creates; the vector is then applied by gravity_calls()."""
    return float(gravity) if not hasattr(gravity, "__len__") else -_vec3(gravity, "scene.gravity")[1]


def gravity_calls(config):
    """What a config asks of a new handle, as the calls that will be made: [("set_gravity", [gx, gy, gz])] for a `scene.gravity` that is a list of
    three, [("set_forcing", amplitude, omega, phase)] for a block `scene.forcing` = {"amplitude": [...], "omega": [...], "phase": [...]}
    (omega / phase optional: None).  A plain number and no block: no call, the handle keeps gravity * (0, -1, 0).  Pure Python; a malformed
    list raises ValueError."""
    scene = config["scene"]
    calls = []
    g = scene.get("gravity")
    if hasattr(g, "__len__"):
        calls.append(("set_gravity", _vec3(g, "scene.gravity")))
    frc = scene.get("forcing")
    if frc is not None:
        if not isinstance(frc, dict) or "amplitude" not in frc or set(frc) - {"amplitude", "omega", "phase"}:
            raise ValueError("scene.forcing must be {\"amplitude\": [...], \"omega\": [...], \"phase\": [...]}, got %r" % (frc,))
        calls.append(("set_forcing", _vec3(frc["amplitude"], "scene.forcing.amplitude"),
                      None if frc.get("omega") is None else _vec3(frc["omega"], "scene.forcing.omega"),
                      None if frc.get("phase") is None else _vec3(frc["phase"], "scene.forcing.phase")))
    return calls


def adaptive_dt_calls(config, solver_name=None):
    """What `solver.adaptive_dt` / `solver.max_dt` / `solver.min_dt` of a config ask of a new wcsph, pcisph, iisph or pbf handle, as the
    set_param calls that will be made, the bounds before the switch: [("step_max_dt", v), ("step_min_dt", v), ("step_adaptive_dt", 1.0)].
    All three keys are optional; a bound that is absent keeps the library's default (max_dt: the configured delta_time, min_dt: 1e-5).
    Under dfsph (solver_name, default `solver.name`) the keys are the reference's own attributes and nothing is asked here.  Pure Python; a bound that is not a finite number
    > 0, or a flag that is not a truth value, raises ValueError."""
    solver = config["solver"]
    if (solver_name or solver.get("name")) == "dfsph":
        return []
    calls = []
    for key in ("max_dt", "min_dt"):
        v = solver.get(key)
        if v is None:
            continue
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not (v > 0 and v < float("inf")):
            raise ValueError("solver.%s must be a finite number > 0, got %r" % (key, v))
        calls.append(("step_" + key, float(v)))
    flag = solver.get("adaptive_dt", False)
    if flag not in (True, False, 0, 1):
        raise ValueError("solver.adaptive_dt must be true or false, got %r" % (flag,))
    if flag:
        calls.append(("step_adaptive_dt", 1.0))
    return calls


def scalar_init_values(pos, init, default=0.0):
    """T of the initial lattice from `scene.scalar.init` = {"value": v, "boxes": [{"min": [...], "max": [...], "value": v}, ...]}: v (absent:
    `default`, the reference value) everywhere, then every box in turn (later boxes win), a particle being inside when lo <= x < hi on all three
    axes in f32.  Pure numpy; returns (n,) f32."""
    pos = np.asarray(pos, dtype=np.float32)
    init = init or {}
    if not isinstance(init, dict) or set(init) - {"value", "boxes"}:
        raise ValueError("scene.scalar.init must be {\"value\": v, \"boxes\": [...]}, got %r" % (init,))
    out = np.full(len(pos), np.float32(init.get("value", default)), dtype=np.float32)
    for box in init.get("boxes", []) or []:
        if not isinstance(box, dict) or set(box) != {"min", "max", "value"}:
            raise ValueError("scene.scalar.init.boxes: each entry needs min, max and value, got %r" % (box,))
        lo = np.float32(_vec3(box["min"], "scene.scalar.init.boxes.min"))
        hi = np.float32(_vec3(box["max"], "scene.scalar.init.boxes.max"))
        inside = ((lo <= pos) & (pos < hi)).all(axis=1)
        out[inside] = np.float32(box["value"])
    return out


def scalar_call(config):
    """What `scene.scalar` = {"diffusivity", "beta", "ref", "init"} of a config asks of a new handle: None without the block, else the keyword
    arguments of Simulation.enable_scalar but for `values` (diffusivity, beta, ref: 0 where absent) and the init block (or None).  Pure Python; an
    unknown key or a value that is not a finite number raises ValueError."""
    block = config["scene"].get("scalar")
    if block is None:
        return None
    if not isinstance(block, dict) or set(block) - {"diffusivity", "beta", "ref", "init"}:
        raise ValueError("scene.scalar must be {\"diffusivity\", \"beta\", \"ref\", \"init\"}, got %r" % (block,))
    kw = {}
    for key in ("diffusivity", "beta", "ref"):
        v = block.get(key, 0.0)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v in (float("inf"), -float("inf")) or (key == "diffusivity" and v < 0):
            raise ValueError("scene.scalar.%s must be a finite number%s, got %r" % (key, " >= 0" if key == "diffusivity" else "", v))
        kw[key] = float(v)
    return kw, block.get("init")


def apply_gravity_calls(target, config):
    """make gravity_calls(config) on a Simulation, a SlabSimulation or a solver mirror, right after creation"""
    for name, *args in gravity_calls(config):
        getattr(target, name)(*args)


def arith_id(arith):
    """"exact" / "relaxed" / 0 / 1 / None -> SphConfig.arith"""
    if arith in (None, 0, "0", "exact", ARITH_EXACT):
        return ARITH_EXACT
    if arith in (1, "1", "relaxed"):
        return ARITH_RELAXED
    raise ValueError("arith must be 'exact' or 'relaxed', got %r" % (arith,))


def plan_slabs(cfg, slab_count):
    """Host-only: (cuts, counts) of the equal-count x-slab decomposition of the scene's initial lattice."""
    lib = load()
    c = SphConfig.from_buffer_copy(cfg)
    c.slab_count = int(slab_count)
    cuts = (ctypes.c_int32 * (slab_count + 1))()
    counts = (ctypes.c_int32 * slab_count)()
    rc = lib.sph_plan_slabs(ctypes.byref(c), cuts, counts)
    if rc != SPH_OK:
        raise SphError(rc, (lib.sph_last_error(None) or b"").decode())
    return list(cuts), list(counts)


def rccl_unique_id():
    """128 opaque bytes from ncclGetUniqueId (rank 0 calls this and broadcasts them)."""
    lib = load()
    buf = ctypes.create_string_buffer(128)
    rc = lib.sph_rccl_unique_id(buf)
    if rc != SPH_OK:
        raise SphError(rc, (lib.sph_last_error(None) or b"").decode())
    return buf.raw


def replan_slabs(column_histogram, old_cuts, ghost_layers=0):
    """Host-only: the re-balancing rule of a slab run (new cuts from a per-column particle histogram; ghost_layers > 0 weighs in the ghosts of every cut)."""
    lib = load()
    gx, nslab = len(column_histogram), len(old_cuts) - 1
    hist = (ctypes.c_int64 * gx)(*[int(v) for v in column_histogram])
    old = (ctypes.c_int32 * (nslab + 1))(*[int(v) for v in old_cuts])
    new = (ctypes.c_int32 * (nslab + 1))()
    rc = lib.sph_replan_slabs(hist, gx, nslab, old, int(ghost_layers), new)
    if rc != SPH_OK:
        raise SphError(rc, (lib.sph_last_error(None) or b"").decode())
    return list(new)


class Simulation:
    """Owns one SphHandle: device buffers of one ParticleSystem + one fluid solver."""

    def __init__(self, cfg, rigid=None, lib=None, config=None):
        """rigid: dict(points, vertices, rho_0, pos_offset, attitude_offset (degrees), active) from mesh.rigid_from_config;
        lib: another implementation of the ABI's per-step path (bind_core), default libsph_mi355x.so;
        config: the config dict cfg was flattened from: its `scene.gravity` list and `scene.forcing` block (gravity_calls) and its
        `solver.adaptive_dt` / `max_dt` / `min_dt` (adaptive_dt_calls) are applied right after creation"""
        self._lib = lib or load()
        self.cfg = cfg
        handle = ctypes.c_void_p()
        self.n_vertices = 0
        if rigid is None:
            rc = self._lib.sph_create(ctypes.byref(cfg), ctypes.byref(handle))
        else:
            pts = np.ascontiguousarray(rigid["points"], dtype=np.float32)
            vts = np.ascontiguousarray(rigid["vertices"], dtype=np.float32)
            rg = SphRigid()
            rg.n_particles, rg.n_vertices = len(pts), len(vts)
            rg.points, rg.vertices = pts.ctypes.data, vts.ctypes.data
            rg.rho_0 = float(rigid["rho_0"])
            rg.pos_offset[:] = [float(v) for v in rigid["pos_offset"]]
            rg.attitude_offset[:] = [float(v) for v in rigid["attitude_offset"]]
            rg.active = 1 if rigid.get("active", False) else 0
            rc = self._lib.sph_create_rigid(ctypes.byref(cfg), ctypes.byref(rg), ctypes.byref(handle))
            self.n_vertices = len(vts)
        if rc != SPH_OK:
            raise SphError(rc, (self._lib.sph_last_error(None) or b"").decode())
        self._h = handle
        sizes = SphSizes()
        self._check(self._lib.sph_get_sizes(self._h, ctypes.byref(sizes)))
        self._n_fluid, self.n_wall, self.n_rigid = sizes.n_fluid, sizes.n_wall, sizes.n_rigid
        self.grid = tuple(sizes.grid)
        self.n_cells = sizes.n_cells
        self.max_neighbors, self.max_wall_neighbors = sizes.max_neighbors, sizes.max_wall_neighbors
        self.last_stats = SphStepStats()
        self.geometry_groups = {}
        self.measured_groups = []            # the wall groups whose load is measured (measure_loads), by id
        if config is not None:
            apply_gravity_calls(self, config)
            for name, value in adaptive_dt_calls(config, "dfsph" if cfg.solver == SOLVER_DFSPH else "other"):
                self.set_param(name, value)
            sc = scalar_call(config)
            if sc is not None:
                self.enable_scalar(**sc[0])                  # (a slab handle refuses here)
                if sc[1] is not None:
                    self.set_scalar(scalar_init_values(self.download(F_POS), sc[1], default=sc[0]["ref"]))
            from . import geometry as _geometry
            self.geometry_groups = _geometry.apply_config(self, config)      # `scene.geometry`: name -> group
            try:                              # `scene.loads`: the wall groups whose load is measured, on a handle that can measure (apply_loads)
                _geometry.apply_loads(self, config)
            except Exception:
                self.close()                  # the handle exists by now: a config that names an unknown group must not leak it
                raise

    def _check(self, rc):
        if rc != SPH_OK:
            raise SphError(rc, (self._lib.sph_last_error(self._h) or b"").decode())

    @property
    def n_fluid(self):
        """the live particle count: the lattice's until add_particles / remove_in_box change it"""
        return self._n_fluid

    @property
    def capacity(self):
        """fluid particles the handle can hold (SphConfig.fluid_capacity, or the lattice's count)"""
        try:
            return int(self.scalar(S_FLUID_CAPACITY))
        except SphError:              # an implementation of the ABI without the scalar: a handle of a fixed count
            return self._n_fluid

    def _refresh_count(self):
        sizes = SphSizes()
        self._check(self._lib.sph_get_sizes(self._h, ctypes.byref(sizes)))
        self._n_fluid = sizes.n_fluid

    def add_particles(self, pos, vel=None, scalar=None):
        """Append len(pos) fluid particles between steps (sph_add_particles): pos (n, 3), vel (n, 3) or None (at rest).  Returns the original id
        of the first one; the others follow it.  No overlap test is made against the fluid already there.  scalar: the carried scalar of the new
        particles (the handle's inflow value is set for this call and restored); None: the inflow value as it stands."""
        if scalar is not None:
            keep = getattr(self, "_scalar_inflow", 0.0)
            self.set_scalar_inflow(scalar)
            try:
                return self.add_particles(pos, vel)
            finally:
                self.set_scalar_inflow(keep)
        pos = np.ascontiguousarray(pos, dtype=np.float32)
        if pos.ndim != 2 or pos.shape[1] != 3:
            raise ValueError("pos must be (n, 3), got %s" % (pos.shape,))
        if vel is not None:
            vel = np.ascontiguousarray(vel, dtype=np.float32)
            if vel.shape != pos.shape:
                raise ValueError("expected vel of shape %s, got %s" % (pos.shape, vel.shape))
        first = ctypes.c_int32(-1)
        self._check(self._optional("sph_add_particles")(self._h, pos.ctypes.data if len(pos) else None, vel.ctypes.data if vel is not None and len(pos) else None,
                                                        len(pos), ctypes.byref(first)))
        self._refresh_count()
        return int(first.value)

    def remove_in_box(self, lo, hi):
        """Remove every fluid particle with lo <= x < hi on all three axes, between steps (sph_remove_in_box); the survivors are renumbered
        densely in the order of their ids.  Returns the number removed."""
        lo = np.ascontiguousarray(lo, dtype=np.float32).reshape(3)
        hi = np.ascontiguousarray(hi, dtype=np.float32).reshape(3)
        removed = ctypes.c_int32(0)
        self._check(self._optional("sph_remove_in_box")(self._h, lo.ctypes.data, hi.ctypes.data, ctypes.byref(removed)))
        self._refresh_count()
        return int(removed.value)

    def _refresh_walls(self):
        sizes = SphSizes()
        self._check(self._lib.sph_get_sizes(self._h, ctypes.byref(sizes)))
        self.n_wall = sizes.n_wall

    def add_geometry(self, points):
        """Append static geometry between steps (sph_geometry_add): points (n, 3) f32 in world coordinates become wall
        samples of a new group, felt by every sweep as the box is.  Returns the group's id (1, 2, ...: never reused).  The volumes of all wall
        samples are recomputed; n_wall and the wall downloads report the new set.  cfd_taichi_amd.geometry has samplers."""
        pts = np.ascontiguousarray(points, dtype=np.float32)
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise ValueError("points must be (n, 3), got %s" % (pts.shape,))
        group = ctypes.c_int32(0)
        self._check(self._optional("sph_geometry_add")(self._h, pts.ctypes.data if len(pts) else None, len(pts), ctypes.byref(group)))
        self._refresh_walls()
        return int(group.value)

    def remove_geometry(self, group):
        """Take a group out of the wall set between steps (sph_geometry_remove): later groups move down in the wall arrays and keep their ids"""
        self._check(self._optional("sph_geometry_remove")(self._h, int(group)))
        self._refresh_walls()
        self.measured_groups = [g for g in self.measured_groups if g != int(group)]      # a removed group leaves the selection

    def geometry(self):
        """the live groups in order of addition: a list of (group, first, count), [first, first + count) being the group's rows of the wall downloads"""
        info = self._optional("sph_geometry_info")
        n = ctypes.c_size_t(0)
        self._check(info(self._h, None, None, None, 0, ctypes.byref(n)))
        cap = max(int(n.value), 1)
        g, f, c = (np.zeros(cap, dtype=np.int32) for _ in range(3))
        self._check(info(self._h, g.ctypes.data, f.ctypes.data, c.ctypes.data, cap, ctypes.byref(n)))
        return [(int(g[k]), int(f[k]), int(c[k])) for k in range(int(n.value))]

    def carve(self, group=-1, clearance=None):
        """Remove every fluid particle nearer than `clearance` (default: the particle diameter; at most h) to a sample of `group` (-1: of any added
        group; the box never carves) -- sph_geometry_carve.  Survivors are renumbered as by remove_in_box.  Returns the number removed."""
        if clearance is None:
            clearance = np.float32(2.0 * self.cfg.particle_radius)
        removed = ctypes.c_int32(0)
        self._check(self._optional("sph_geometry_carve")(self._h, int(group), float(np.float32(clearance)), ctypes.byref(removed)))
        self._refresh_count()
        return int(removed.value)

    def wall_neighbor_counts(self):
        """(n,) int32 in original particle order: the wall samples, box and geometry, in each particle's list as the last list build left it
        (sph_geometry_wall_counts)"""
        out = np.zeros(self._n_fluid, dtype=np.int32)
        self._check(self._optional("sph_geometry_wall_counts")(self._h, out.ctypes.data, out.size))
        return out

    # ---- loads on walls and geometry ----
    def _load_group(self, group, all_allowed=False):
        """a group as the load calls take it: "box" (0), a name of geometry_groups, or an id; None / "all": every measured group (-1)"""
        if all_allowed and (group is None or group == "all"):
            return -1
        if group == "box":
            return 0
        if isinstance(group, str):
            if group not in self.geometry_groups:
                raise ValueError("no geometry named '%s' (the handle knows %s)" % (group, ", ".join(["box"] + sorted(self.geometry_groups))))
            return int(self.geometry_groups[group])
        return int(group)

    def measure_loads(self, groups):
        """Measure the load of the fluid on the wall groups named (sph_wall_load_select): "box", names of geometry_groups, or ids; an empty list
        switches measuring off.  Impulses and seconds start at zero.  Invisible to the fluid; a step costs a few small launches more."""
        ids = np.ascontiguousarray([self._load_group(g) for g in groups], dtype=np.int32)
        self._check(self._optional("sph_wall_load_select")(self._h, ids.ctypes.data if len(ids) else None, len(ids)))
        self.measured_groups = [int(g) for g in ids]

    def wall_load(self, group=None, about=None):
        """(force, torque) of the last step on a measured group (None: on all of them), f64 (3,) each; the torque about `about` (None: the origin)
        -- sph_wall_load_get"""
        c = None if about is None else np.ascontiguousarray(about, dtype=np.float64).reshape(3)
        f, t = np.zeros(3), np.zeros(3)
        self._check(self._optional("sph_wall_load_get")(self._h, self._load_group(group, True), None if c is None else c.ctypes.data, f.ctypes.data, t.ctypes.data))
        return f, t

    def wall_impulse(self, group=None, about=None, reset=True):
        """(impulse, angular impulse, seconds) a measured group has collected since it was selected or last reset: the sums of dt F, dt torque and
        dt over the steps; the mean force of the window is impulse / seconds (sph_wall_load_impulse).  reset: start the next window"""
        c = None if about is None else np.ascontiguousarray(about, dtype=np.float64).reshape(3)
        j, l, sec = np.zeros(3), np.zeros(3), ctypes.c_double(0.0)
        self._check(self._optional("sph_wall_load_impulse")(self._h, self._load_group(group, True), None if c is None else c.ctypes.data, j.ctypes.data, l.ctypes.data,
                                                            ctypes.byref(sec), 1 if reset else 0))
        return j, l, float(sec.value)

    def wall_forces(self, group):
        """(count, 3) f32: the last step's force on every sample of a measured group, in the group's own sample order -- for "box" the first rows
        of download(F_WALL_POS, SPECIES_WALL), for a geometry group the points it was added with (sph_wall_load_forces)"""
        gid = self._load_group(group)
        count = {g: c for g, _, c in self.geometry()}
        n = self.n_wall - sum(count.values()) if gid == 0 else count.get(gid, 0)
        out = np.zeros((n, 3), dtype=np.float32)
        self._check(self._optional("sph_wall_load_forces")(self._h, gid, out.ctypes.data, out.size))
        return out

    def diagnostics(self):
        """The run diagnostics of the fluid as it stands, between steps (sph_diagnostics): a dict keyed by the names of DIAG_SLOTS, f64.  The
        rho_* entries are NaN unless compute_density ran since the positions last changed.  Changes nothing on the handle."""
        row = np.zeros(1, dtype=DIAG_DTYPE)
        self._check(self._optional("sph_diagnostics")(self._h, row.ctypes.data))
        return {name: float(row[name][0]) for name in DIAG_SLOTS}

    def record_diagnostics(self, every, rows=4096):
        """Record one diagnostics row at the end of every `every`-th solver step into a ring of `rows` rows on the device (sph_diag_record);
        every = 0 stops.  No host wait is added to a step; diagnostics_log() reads the rows when the caller likes."""
        self._check(self._optional("sph_diag_record")(self._h, int(every), int(rows)))
        if every:
            self._diag_rows, self._diag_seen = int(rows), 0

    def diagnostics_log(self):
        """The recorded rows not read yet, oldest first, as a structured array of DIAG_DTYPE, and the number of rows that were overwritten in the
        ring before any read could return them (since recording was switched on).  The read consumes the rows."""
        cap = getattr(self, "_diag_rows", 0)
        out = np.zeros(max(cap, 1), dtype=DIAG_DTYPE)
        n, total = ctypes.c_size_t(0), ctypes.c_int64(0)
        self._check(self._optional("sph_diag_read")(self._h, out.ctypes.data, cap, ctypes.byref(n), ctypes.byref(total)))
        self._diag_seen = getattr(self, "_diag_seen", 0) + int(n.value)
        return out[:int(n.value)].copy(), int(total.value) - self._diag_seen

    def derived(self, which):
        """A derived per-particle field of the fluid as it stands (sph_derived): `which` is a name of DERIVED or an SPH_D_* id.  Returns f32 in
        original particle order: (n, 3, 3) velgrad (row a, column b: d v_a / d x_b), (n, 3) vorticity / normal, (n,) divergence / cover.  Runs
        compute_density first (its caveat applies); changes no trajectory.  All five come from one sweep, kept until the state changes."""
        wid = DERIVED[which] if isinstance(which, str) else int(which)
        shape = DERIVED_SHAPE.get(wid, ())
        out = np.empty((self._n_fluid,) + shape, dtype=np.float32)
        self._check(self._optional("sph_derived")(self._h, wid, out.ctypes.data, out.size))
        return out

    def enable_scalar(self, diffusivity=0.0, beta=0.0, ref=0.0, values=None):
        """Switch the carried scalar on (sph_scalar_enable), or change its parameters: diffusivity D in m^2/s, the buoyancy
        coefficient beta (0: passive) and the reference value.  A first call sets T = ref everywhere and the inflow value to ref; values: (n,) to
        upload behind it."""
        fresh = not getattr(self, "_scalar_on", False)
        self._check(self._optional("sph_scalar_enable")(self._h, float(diffusivity), float(beta), float(ref)))
        self._scalar_on = True
        if fresh:
            self._scalar_inflow = float(ref)
        if values is not None:
            self.set_scalar(values)

    def disable_scalar(self):
        """sph_scalar_disable: the memory is freed, the handle steps as if the scalar had never been enabled"""
        self._check(self._optional("sph_scalar_disable")(self._h))
        self._scalar_on = False

    def set_scalar(self, values):
        """upload the carried scalar, (n,) in original particle order (sph_scalar_upload)"""
        arr = np.ascontiguousarray(values, dtype=np.float32)
        if arr.shape != (self._n_fluid,):
            raise ValueError("expected shape %s, got %s" % ((self._n_fluid,), arr.shape))
        self._check(self._optional("sph_scalar_upload")(self._h, arr.ctypes.data, arr.size))

    def set_scalar_inflow(self, value):
        """the carried scalar of the particles add_particles brings from now on (sph_scalar_set_inflow)"""
        self._check(self._optional("sph_scalar_set_inflow")(self._h, float(value)))
        self._scalar_inflow = float(value)

    def scalar_rate(self):
        """dT/dt of the state as it stands, (n,) f32 in original particle order (sph_scalar_rate): builds the lists first if positions changed
        (build_neighbors' caveat applies); changes neither T nor any trajectory"""
        out = np.empty(self._n_fluid, dtype=np.float32)
        self._check(self._optional("sph_scalar_rate")(self._h, out.ctypes.data, out.size))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sph_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _shape(self, species, field):
        if species == SPECIES_RIGID:
            n = self.n_vertices if field == F_RIGID_VERT else self.n_rigid
            return (n, 3) if field in VECTOR_FIELDS else (n,)
        n = self.n_wall if species == SPECIES_WALL else self.n_fluid
        return (n, 3) if field in VECTOR_FIELDS else (n,)

    def download(self, field, species=SPECIES_FLUID):
        out = np.empty(self._shape(species, field), dtype=np.float32)
        self._check(self._lib.sph_download(self._h, species, field, out.ctypes.data, out.size))
        return out

    def upload(self, field, values, species=SPECIES_FLUID):
        arr = np.ascontiguousarray(values, dtype=np.float32)
        if arr.shape != self._shape(species, field):
            raise ValueError("expected shape %s, got %s" % (self._shape(species, field), arr.shape))
        self._check(self._lib.sph_upload(self._h, species, field, arr.ctypes.data, arr.size))

    def step_wcsph(self, nsteps=1):
        self._check(self._lib.sph_step_wcsph(self._h, nsteps))

    def step_dfsph(self, nsteps=1):
        self._check(self._lib.sph_step_dfsph(self._h, nsteps, ctypes.byref(self.last_stats)))
        return self.last_stats

    def step_pcisph(self, nsteps=1):
        self._check(self._lib.sph_step_pcisph(self._h, nsteps, ctypes.byref(self.last_stats)))
        return self.last_stats

    def step_iisph(self, nsteps=1):
        self._check(self._lib.sph_step_iisph(self._h, nsteps, ctypes.byref(self.last_stats)))
        return self.last_stats

    def step_pbf(self, nsteps=1):
        self._check(self._lib.sph_step_pbf(self._h, nsteps))

    def step(self, nsteps=1):
        """One call for any solver; returns the last step's SphStepStats (None for wcsph)."""
        sid = self.cfg.solver
        if sid == SOLVER_WCSPH:
            return self.step_wcsph(nsteps)
        if sid == SOLVER_PBF:
            return self.step_pbf(nsteps)
        return {SOLVER_DFSPH: self.step_dfsph, SOLVER_PCISPH: self.step_pcisph, SOLVER_IISPH: self.step_iisph}[sid](nsteps)

    def rigid_step(self):
        self._check(self._lib.sph_rigid_step(self._h))

    def _optional(self, name):
        fn = getattr(self._lib, name, None)
        if fn is None:
            raise SphError(SPH_E_STATE, "%s does not export %s" % (getattr(self._lib, "_name", "this library"), name))
        return fn

    def rigid_set_active(self, active):
        """ps.active_rigid[None] = active: the flag alone; an active body is binned (and, with fs_couple, coupled) from the next grid build."""
        self._check(self._optional("sph_rigid_set_active")(self._h, 1 if active else 0))

    def rigid_init_data(self):
        """ps.init_rigid_particles_data(): sample volumes, masses, centroid and inertia from the body's current sample positions."""
        self._check(self._optional("sph_rigid_init_data")(self._h))

    def rigid_set_mode(self, mode):
        """what rigid_step does with the body: "dynamic" (rigid_solver.step, the default), "scripted" (moved by rigid_set_motion's motion) or
        "fixed" (never moves); a name of RIGID_MODES or its number."""
        self._check(self._optional("sph_rigid_set_mode")(self._h, RIGID_MODES.get(mode, mode)))

    def rigid_set_motion(self, vel, omega, acc=None, alpha=None):
        """the motion a scripted body follows from the next rigid_step on, until it is replaced (acc, alpha: None = zeros)"""
        arrs = [None if v is None else np.ascontiguousarray(v, dtype=np.float32).reshape(3) for v in (vel, omega, acc, alpha)]
        self._check(self._optional("sph_rigid_set_motion")(self._h, *[None if a is None else a.ctypes.data for a in arrs]))

    def rigid_load(self):
        """(force, torque) of the fluid on the body as the last rigid_step summed them, f64; the torque about the centroid before that step's move"""
        force, torque = np.zeros(3, dtype=np.float64), np.zeros(3, dtype=np.float64)
        self._check(self._optional("sph_rigid_get_load")(self._h, force.ctypes.data, torque.ctypes.data))
        return force, torque

    def rigid_scalars(self, motion=False):
        """the body's scalars; motion=True adds acc, alpha (what the sweeps extrapolate vel and omega with) and mode (RIGID_*), which a library
        from before the body modes does not have"""
        g = self.scalar
        out = {"centroid": [g(S_RIGID_CENTROID + k) for k in range(3)], "omega": [g(S_RIGID_OMEGA + k) for k in range(3)],
               "vel": [g(S_RIGID_VEL + k) for k in range(3)], "mass": g(S_RIGID_MASS),
               "inertia_inv": [g(S_RIGID_INERTIA_INV + k) for k in range(9)]}
        if motion:
            out.update(acc=[g(S_RIGID_ACC + k) for k in range(3)], alpha=[g(S_RIGID_ALPHA + k) for k in range(3)], mode=int(g(S_RIGID_MODE)))
        return out

    def build_neighbors(self):
        self._check(self._lib.sph_build_neighbors(self._h))

    def compute_density(self):
        self._check(self._lib.sph_compute_density(self._h))

    def compute_alpha(self):
        self._check(self._lib.sph_compute_alpha(self._h))

    def scalar(self, which=None):
        """scalar(S_*): a scalar of the handle (sph_get_scalar).  scalar(): the carried scalar, (n,) f32 in original particle order
        (sph_scalar_download)"""
        if which is None:
            out = np.empty(self._n_fluid, dtype=np.float32)
            self._check(self._optional("sph_scalar_download")(self._h, out.ctypes.data, out.size))
            return out
        out = ctypes.c_double()
        self._check(self._lib.sph_get_scalar(self._h, which, ctypes.byref(out)))
        return out.value

    def set_dt(self, value):
        """solver.delta_time[None] = value"""
        self._check(self._lib.sph_set_scalar(self._h, S_DELTA_TIME, float(value)))

    def set_gravity(self, vec):
        """the base vector g of the handle's acceleration (sph_set_gravity), between steps: three finite numbers, rounded to f32"""
        g = np.ascontiguousarray(vec, dtype=np.float32).reshape(3)
        self._check(self._optional("sph_set_gravity")(self._h, g.ctypes.data))

    def set_forcing(self, amp, omega=None, phase=None):
        """harmonic forcing per axis, a_k = f32(g_k + amp_k sin(omega_k t + phase_k)) in f64 (sph_set_forcing), between steps; amp None switches it
        off, omega / phase None are zeros"""
        arrs = [None if v is None else np.ascontiguousarray(v, dtype=np.float64).reshape(3) for v in (amp, omega, phase)]
        self._check(self._optional("sph_set_forcing")(self._h, *[None if a is None else a.ctypes.data for a in arrs]))

    def time(self):
        """the handle's simulated time: the f64 sum of the delta_time of every solver step so far"""
        return self.scalar(S_TIME)

    def set_time(self, value):
        self._check(self._lib.sph_set_scalar(self._h, S_TIME, float(value)))

    def accel(self):
        """the acceleration vector (three f32) as the last solver step used it, or as the next will if none has run since a set call"""
        return np.array([self.scalar(S_ACCEL + k) for k in range(3)], dtype=np.float32)

    def gravity_vec(self):
        return np.array([self.scalar(S_GRAVITY_VEC + k) for k in range(3)], dtype=np.float32)

    def set_param(self, name, value):
        """solver.<name> = value for the attributes of SOLVER_PARAMS (dfsph_solver.py:21-29, solver_base.py:23-26, wcsph_solver.py:17-20)."""
        self._check(self._lib.sph_set_scalar(self._h, SOLVER_PARAMS[name], float(value)))

    def param(self, name):
        return self.scalar(SOLVER_PARAMS[name])

    def synchronize(self):
        self._check(self._lib.sph_synchronize(self._h))

    def overrides(self):
        """Development overrides in force on this handle, e.g. ['SPH_CELL_ORDER=morton'] (needs SPH_DEV=1 to take effect at all)."""
        if not hasattr(self._lib, "sph_overrides"):
            return []
        txt = (self._lib.sph_overrides(self._h) or b"").decode()
        out = [t for t in txt.split(";") if t]
        if os.environ.get("SPH_LIB"):
            out.append("SPH_LIB=" + os.environ["SPH_LIB"])
        return out

    # ---- multi-GPU slab handles ----
    def set_comm(self, comm, struct_size=None):
        """struct_size: what a caller built against an older, shorter SphComm would pass as sizeof(SphComm) (sph_set_comm_sized): the fields
        beyond it read as 0 / NULL whatever this structure holds there."""
        self._comm = comm            # keep the callbacks and buffers alive
        if struct_size is None:
            self._check(self._lib.sph_set_comm(self._h, ctypes.byref(comm)))
        else:
            self._check(self._lib.sph_set_comm_sized(self._h, ctypes.byref(comm), int(struct_size)))

    def rccl_attach(self, unique_id, capacity_bytes=64 << 20):
        """Collective over all slabs: the library opens its own RCCL communicator (native transport, no callbacks)."""
        buf = ctypes.create_string_buffer(bytes(unique_id), 128)
        self._check(self._lib.sph_rccl_attach(self._h, buf, capacity_bytes))

    def rccl_selftest(self, values, op=0):
        arr = (ctypes.c_double * len(values))(*values)
        self._check(self._lib.sph_rccl_selftest(self._h, arr, len(values), op))
        return list(arr)

    def stream_ptr(self):
        """The handle's hipStream_t as an integer (for torch.cuda.ExternalStream in stream-ordered transports)."""
        out = ctypes.c_void_p()
        self._check(self._lib.sph_get_stream(self._h, ctypes.byref(out)))
        return out.value or 0

    def slab_info(self):
        out = (ctypes.c_int32 * 8)()
        self._check(self._lib.sph_slab_info(self._h, out))
        return {"owned": out[0], "ghosts": out[1], "x_lo": out[2], "x_hi": out[3], "capacity": out[4], "recuts": out[5],
                "rebalance_every": out[6], "ghost_columns": out[7] & 15, "halo_overlapped": bool(out[7] & 16), "allreduce_hidden": bool(out[7] & 32)}

    def set_slab_overlap(self, on):
        """Between steps, on every slab alike: halo and reductions of the dfsph loops on their own streams (True) or in order (False); same bits."""
        self._check(self._lib.sph_slab_set_overlap(self._h, 1 if on else 0))

    def comm_stats(self, reset=False):
        """Transport requests since the last reset: {p2p_groups, bytes_sent, bytes_received, count_exchanges, allreduce_stream, allreduce_host, steps}."""
        out = (ctypes.c_int64 * 8)()
        self._check(self._lib.sph_comm_stats(self._h, out, 1 if reset else 0))
        keys = ("p2p_groups", "bytes_sent", "bytes_received", "count_exchanges", "allreduce_stream", "allreduce_host", "steps")
        return {k: int(out[i]) for i, k in enumerate(keys)}

    def slab_set_state(self, pos, vel=None, scalar=None, delta_time=0.0):
        """Collective over all slabs: this handle's share of one full state in original particle order (sph_slab_set_state); vel / scalar None = zeros,
        delta_time 0 keeps the handle's.  A refusal raises the same SphError on every rank and changes no handle."""
        def flat(a, shape):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != shape:
                raise ValueError("expected shape %s, got %s" % (shape, a.shape))
            return a
        pos = np.ascontiguousarray(pos, dtype=np.float32)
        if pos.ndim != 2 or pos.shape[1] != 3:
            raise ValueError("pos must be (n, 3), got %s" % (pos.shape,))
        n = len(pos)
        vel, scalar = flat(vel, (n, 3)), flat(scalar, (n,))
        self._check(self._optional("sph_slab_set_state")(self._h, pos.ctypes.data, vel.ctypes.data if vel is not None else None,
                                                         scalar.ctypes.data if scalar is not None else None, n, float(delta_time or 0.0)))

    def download_local(self, field):
        """(ids, values) of every resident particle in device order; ids < 0 are ghosts (~id)."""
        info = self.slab_info()
        n = info["owned"] + info["ghosts"]
        ids = np.empty(n, dtype=np.int32)
        self._check(self._lib.sph_download_ids(self._h, ids.ctypes.data, n))
        out = np.empty((n, 3) if field in VECTOR_FIELDS else (n,), dtype=np.float32)
        self._check(self._lib.sph_download_local(self._h, field, out.ctypes.data, out.size))
        return ids, out

    def download_owned(self, field):
        ids, vals = self.download_local(field)
        keep = ids >= 0
        return ids[keep], vals[keep]

    # ---- profiling (HIP events on the handle's stream) ----
    def tune_time(self, which, lds_bytes=0, reps=10):
        out = ctypes.c_double()
        self._check(self._lib.sph_tune_time(self._h, which, lds_bytes, reps, ctypes.byref(out)))
        return out.value

    def profile_enable(self, on=True):
        self._check(self._lib.sph_profile_enable(self._h, 1 if on else 0))

    def profile_reset(self):
        self._check(self._lib.sph_profile_reset(self._h))

    def profile(self):
        """{kernel name: (total_ms, launches)} for kernels launched while profiling was on."""
        res = {}
        for k in range(self._lib.sph_profile_kernel_count()):
            ms, n = ctypes.c_double(), ctypes.c_int64()
            self._check(self._lib.sph_profile_get(self._h, k, ctypes.byref(ms), ctypes.byref(n)))
            if n.value:
                res[self._lib.sph_profile_kernel_name(k).decode()] = (ms.value, n.value)
        return res


MATH_RECIP, MATH_DIV_SHARED, MATH_DIV_SHARED_TWO_STEP, MATH_DIV_SHARED_FLOORED = 7, 8, 9, 10    # sph_selftest_math ops (include/sph_mi355x.h)
MATH_SQRT_BY_FIELD, MATH_SQRT_VERDICT = 11, 12


def selftest_math(op, a, b, device=0):
    """out[i] = op(a[i], b[i]) in f32 on the device (see sph_selftest_math): 0 a/b, 1 sqrt(a), 2 W(a; h=b), 3-5 grad W, 6 sqrt_rn(a),
    MATH_RECIP recip_prepare(b).y, MATH_DIV_SHARED / MATH_DIV_SHARED_TWO_STEP the sweeps' quotient a/b with one / two residual corrections,
    MATH_DIV_SHARED_FLOORED the first of them with the divisor raised to kDenFloor, MATH_SQRT_BY_FIELD the root of a taken as the hardware root plus
    the verdict of sqrt_rn's rounding step through a 2-bit field of the pair-bit cache, MATH_SQRT_VERDICT that verdict (-1, 0, +1)."""
    lib = load()
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    out = np.empty_like(a)
    rc = lib.sph_selftest_math(device, op, a.ctypes.data, b.ctypes.data, out.ctypes.data, a.size)
    if rc != SPH_OK:
        raise SphError(rc, (lib.sph_last_error(None) or b"").decode())
    return out


def selftest_wave(op, values, device=0):
    """Per-lane results of one wave primitive (see sph_selftest_wave); len(values) must be a multiple of 256."""
    lib = load()
    a = np.ascontiguousarray(values, dtype=np.float64)
    out = np.empty_like(a)
    rc = lib.sph_selftest_wave(device, op, a.ctypes.data, out.ctypes.data, a.size)
    if rc != SPH_OK:
        raise SphError(rc, (lib.sph_last_error(None) or b"").decode())
    return out


STAGE_CAP_MAX = 2560          # csrc/sph_kernels.h kStageCapMax
STAGE_LAYOUTS = {"f4": 0, "f4_scaled": 1, "ps": 2, "ps_scaled": 3, "pv": 4, "pv_scaled": 5, "f4s": 6, "f4src": 7}
STAGE_CHECKS = {"none": 0, "with": 1, "first": 2}


def selftest_stage(layout, check, runs, A, B, S, changed, use_pre=False, not_staged=False, empty_idle=False, handle=None):
    """(image, verdict) of the LDS staging routine on one workgroup's plan (see sph_selftest_stage): image[e] = the six floats of staged
    element e, for all STAGE_CAP_MAX slots.  empty_idle: the verdict the call site names for a staged set of no particles is "idle"; handle: the raw
    handle whose device runs it (None: device 0)."""
    lib = load()
    if not hasattr(lib, "sph_selftest_stage"):
        raise SphError(SPH_E_STATE, "this library has no sph_selftest_stage")
    runs = np.ascontiguousarray(runs, dtype=np.uint32).reshape(-1, 2)
    A = np.ascontiguousarray(A, dtype=np.float32).reshape(-1, 4)
    B = np.ascontiguousarray(B, dtype=np.float32).reshape(-1, 4)
    S = np.ascontiguousarray(S, dtype=np.float32)
    changed = np.ascontiguousarray(changed, dtype=np.uint8)
    assert len(A) == len(B) == len(S) == len(changed)
    out = np.zeros((STAGE_CAP_MAX, 6), dtype=np.float32)
    verdict = ctypes.c_int(-1)
    rc = lib.sph_selftest_stage(handle, STAGE_LAYOUTS[layout], STAGE_CHECKS[check], int(empty_idle), int(use_pre), int(not_staged), runs.ctypes.data, len(runs),
                                A.ctypes.data, B.ctypes.data, S.ctypes.data, changed.ctypes.data, len(A), out.ctypes.data, ctypes.byref(verdict))
    if rc != SPH_OK:
        raise SphError(rc, (lib.sph_last_error(handle) or b"").decode())
    return out, verdict.value


WALKS = {"list": 0, "quad": 1, "staged": 2, "list16": 3}
WALK_SOURCES_MEM = {"p": 0, "a": 1, "ab": 2, "as": 3, "abc": 4}
WALK_SOURCES_LDS = {"f4": 0, "f4_scaled": 1, "ps": 2, "ps_scaled": 3, "pv": 4, "pv_scaled": 5, "f4s": 6, "f4src_b": 7, "update_p": 8}
WALK_ROWS, WALK_PITCH, WALK_PARTICLES = 24, 28, 256


def selftest_walk_bits(lists, counts, words=None, verdicts=None, handle=None):
    """walk_list16 with the pair-bit stream on one workgroup (see sph_selftest_walk_bits).  With `words` (256 x 3) the bodies read their fields from
    them; with `verdicts` (256 x 24) body k records verdicts[i, k] and the words the walk stored are returned.  -> (seen 256 x 24, calls 256, words)"""
    lib = load()
    if not hasattr(lib, "sph_selftest_walk_bits"):
        raise SphError(SPH_E_STATE, "this library has no sph_selftest_walk_bits")
    write = verdicts is not None
    lists = np.ascontiguousarray(lists, dtype=np.uint32).reshape(WALK_PARTICLES, WALK_ROWS)
    counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(WALK_PARTICLES)
    words = np.zeros((WALK_PARTICLES, WALK_ROWS // 8), dtype=np.uint32) if write else np.array(words, dtype=np.uint32).reshape(WALK_PARTICLES, WALK_ROWS // 8)
    verdicts = np.ascontiguousarray(verdicts if write else np.zeros((WALK_PARTICLES, WALK_ROWS)), dtype=np.int32).reshape(WALK_PARTICLES, WALK_ROWS)
    seen = np.zeros((WALK_PARTICLES, WALK_ROWS), dtype=np.uint32)
    calls = np.zeros(WALK_PARTICLES, dtype=np.int32)
    rc = lib.sph_selftest_walk_bits(handle, int(write), lists.ctypes.data, counts.ctypes.data, words.ctypes.data, verdicts.ctypes.data, seen.ctypes.data,
                                    calls.ctypes.data)
    if rc != SPH_OK:
        raise SphError(rc, (lib.sph_last_error(None) or b"").decode())
    return seen, calls, words


def selftest_walk(walk, src, rigid, lists, counts, run, A, B, C, S, RP, handle=None):
    """What the pair bodies of one list walk saw (see sph_selftest_walk): a (threads, 4) uint32 array of body calls, hash and, for the quad walk, the
    bits of the two sums; threads = 256, or 1024 for the quad walk (four per particle)."""
    lib = load()
    if not hasattr(lib, "sph_selftest_walk"):
        raise SphError(SPH_E_STATE, "this library has no sph_selftest_walk")
    lists = np.ascontiguousarray(lists, dtype=np.uint32).reshape(WALK_PARTICLES, WALK_PITCH)
    counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(WALK_PARTICLES)
    A, B, C, RP = (np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 4) for x in (A, B, C, RP))
    S = np.ascontiguousarray(S, dtype=np.float32)
    assert len(A) == len(B) == len(C) == len(S)
    out = np.zeros((WALK_PARTICLES * (4 if walk == "quad" else 1), 4), dtype=np.uint32)
    table = WALK_SOURCES_LDS if WALKS[walk] >= 2 else WALK_SOURCES_MEM
    rc = lib.sph_selftest_walk(handle, WALKS[walk], table[src], int(rigid), lists.ctypes.data, counts.ctypes.data, int(run[0]), int(run[1]),
                               A.ctypes.data, B.ctypes.data, C.ctypes.data, S.ctypes.data, len(A), RP.ctypes.data, len(RP), out.ctypes.data)
    if rc != SPH_OK:
        raise SphError(rc, (lib.sph_last_error(handle) or b"").decode())
    return out
